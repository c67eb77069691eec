// grid.cpp — svo_chunk_from_grid: the tree of a dense voxel grid on the host.  grow() (src/Octree.cpp:74-176) with "all cells of the
// node are equal" in the place of the height bounds; grid.hip is its device twin, as builder.hip is terrain.cpp's.
//
//   grid      N^3 uint16 materials, N = 2^depth, x fastest: cell (x, y, z) at (z*N + y)*N + x; 0 = empty
//   summary   one uint32 per node of the levels 0 .. depth-2 (level L: (2^L)^3 nodes, x fastest): the node's one value, or MIXED.
//             The base level (one entry per 4^3 block) reads the grid once; each level above folds eight entries into one
//   tree      the FIFO walk of grow(): root at slot 0, a node that is MIXED becomes a TWIG at level depth-2 (its 64 cells copied,
//             brick index z*16 + y*4 + x) and a BRANCH above it (its 8 children at the pool's tail, slot x + 2y + 4z)
// Integer arithmetic only; no HIP include: plain g++ compiles this file (host/grid_check.cpp runs it under the sanitizers).
#include <cmath>
#include <new>

#include "chunk_pools.h"

namespace svo {

namespace {

constexpr uint32_t MIXED = 0xFFFFFFFFu;
inline uint32_t fold(uint32_t a, uint32_t b) { return a == b ? a : MIXED; }

struct GridNode { uint32_t x, y, z, slot; };        // node coordinates at its level (corner = coordinate * edge), slot in tree[]

void chunk_from_grid(const uint16_t *grid, uint32_t depth, std::vector<uint32_t> &tree, std::vector<uint16_t> &twig)
{
    const uint64_t N = 1ull << depth;
    const uint32_t maxlevel = depth - TWIG_LEVELS;
    // summary pyramid, level L at sum[L]
    std::vector<std::vector<uint32_t>> sum(maxlevel + 1);
    {
        const uint64_t nb = N / TWIG_SIZE;
        std::vector<uint32_t> &base = sum[maxlevel];
        base.resize(nb * nb * nb);
        for (uint64_t bz = 0; bz < nb; ++bz)
            for (uint64_t by = 0; by < nb; ++by)
                for (uint64_t bx = 0; bx < nb; ++bx) {
                    const uint16_t *p = grid + ((bz * 4) * N + by * 4) * N + bx * 4;
                    uint32_t v = p[0];
                    for (uint64_t z = 0; z < 4; ++z)
                        for (uint64_t y = 0; y < 4; ++y)
                            for (uint64_t x = 0; x < 4; ++x) v = fold(v, p[(z * N + y) * N + x]);
                    base[(bz * nb + by) * nb + bx] = v;
                }
    }
    for (uint32_t L = maxlevel; L > 0; --L) {
        const uint64_t n = 1ull << (L - 1), f = 2 * n;
        const std::vector<uint32_t> &fine = sum[L];
        std::vector<uint32_t> &up = sum[L - 1];
        up.resize(n * n * n);
        for (uint64_t z = 0; z < n; ++z)
            for (uint64_t y = 0; y < n; ++y)
                for (uint64_t x = 0; x < n; ++x) {
                    uint32_t v = fine[((2 * z) * f + 2 * y) * f + 2 * x];
                    for (uint64_t c = 1; c < 8; ++c) v = fold(v, fine[((2 * z + (c >> 2)) * f + 2 * y + ((c >> 1) & 1)) * f + 2 * x + (c & 1)]);
                    up[(z * n + y) * n + x] = v;
                }
    }
    // the FIFO walk: `queue` holds one level at a time, in visiting order
    tree.assign(1, node_make(EMPTY, 0));
    twig.clear();
    std::vector<GridNode> queue(1, GridNode{ 0, 0, 0, 0 }), next;
    for (uint32_t L = 0; !queue.empty(); ++L) {
        const uint64_t n = 1ull << L;
        next.clear();
        for (const GridNode &e : queue) {
            const uint32_t v = sum[L][((uint64_t)e.z * n + e.y) * n + e.x];
            if (v != MIXED) { tree[e.slot] = v ? node_make(LEAF, v) : node_make(EMPTY, 0); continue; }
            if (L == maxlevel) {
                const uint64_t k = twig.size() / TWIG_WORDS;
                tree[e.slot] = node_make(TWIG, (uint32_t)k);
                const uint16_t *p = grid + (((uint64_t)e.z * 4) * N + (uint64_t)e.y * 4) * N + (uint64_t)e.x * 4;
                for (uint64_t z = 0; z < 4; ++z)
                    for (uint64_t y = 0; y < 4; ++y)
                        for (uint64_t x = 0; x < 4; ++x) twig.push_back(p[(z * N + y) * N + x]);
                continue;
            }
            const uint32_t first = (uint32_t)tree.size();
            tree[e.slot] = node_make(BRANCH, first);
            tree.resize(tree.size() + 8, node_make(EMPTY, 0));
            for (uint32_t c = 0; c < 8; ++c) next.push_back(GridNode{ 2 * e.x + (c & 1), 2 * e.y + ((c >> 1) & 1), 2 * e.z + (c >> 2), first + c });
        }
        queue.swap(next);
    }
}

} // namespace

} // namespace svo

extern "C" {

int svo_chunk_from_grid(const uint16_t *grid, uint32_t depth, const float position[3], float size, svo_chunk_desc *out)
{
    using namespace svo;
    if (!grid || !position || !out || depth < SVO_GRID_MIN_DEPTH || depth > SVO_GRID_MAX_DEPTH || !(size > 0.0f) || !std::isfinite(size)) {
        set_error("svo_chunk_from_grid: bad argument (depth must be in [2, 10], size positive and finite)");
        return SVO_ERR_INVALID_ARG;
    }
    try {
        std::vector<uint32_t> tree;
        std::vector<uint16_t> twig;
        chunk_from_grid(grid, depth, tree, twig);
        // (trees <= 1 + 8 * (8^8 - 1) / 7 and twigs <= 8^8 at depth 10: the 30-bit node offset is never reached)
        return chunk_desc_take(out, position, size, depth, tree, twig, "svo_chunk_from_grid");
    } catch (const std::bad_alloc &) {
        set_error("svo_chunk_from_grid: out of host memory");
        return SVO_ERR_OUT_OF_MEMORY;
    }
}

} // extern "C"
