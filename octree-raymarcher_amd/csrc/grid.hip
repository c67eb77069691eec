// grid.hip — svo_world_chunk_from_grid / svo_world_chunk_to_grid: a chunk of an uploaded world built from a dense voxel grid in
// device memory, and read back into one.  grid.cpp states the tree of a grid as the host walk; here it is grow()
// (src/Octree.cpp:74-176) as builder.hip runs it - a level-synchronous BFS - with a summary pyramid of the grid in the place of the
// height pyramid:
//   k_grid_summary   the pyramid's base, one uint32 per 4^3 block (its one value, or MIXED).  One thread per brick x-row: an 8-byte
//                    load of its 4 cells, neighbouring lanes neighbouring rows along x (a wave reads up to 512 contiguous bytes); the
//                    16 rows of a block (4 y x 4 z) sit in one workgroup and are folded through LDS.  Every cell is read once
//   k_grid_mip       one level up: eight equal, non-MIXED entries give that value
//   hipcub reduce    MIXED entries above the base = BRANCHes, in the base = TWIGs: the pools' sizes before anything is written
//   per level        k_grid_classify (the frontier node's entry of the pyramid -> EMPTY / LEAF / BRANCH / TWIG), bfs_grow's steps
//                    (bfs.hip.h: the scan that ranks the flags, k_level_totals, k_emit - node words, children in FIFO order, brick
//                    jobs), k_grid_bricks (one thread per brick z-row: four 8-byte loads, one 32-byte store - MIXED blocks are the only
//                    cells read a second time)
// The pools are written to the edits' resident scratch (edit_scratch), the pyramid to the world's GridScratch, the level arrays are the
// BfsArrays the terrain grower uses too, and the install is svo_world_coarsen's (install_rebuilt).  No float arithmetic anywhere.
//   k_to_grid        the inverse: one thread per run of 8 output cells along x, one descent from the root per EMPTY / LEAF node or
//                    brick cell the run crosses (a run inside one node: one descent), one 16-byte store.  Every index read from the
//                    pools is checked against the chunk's counts.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "bfs.hip.h"
#include "hip_own.h"

namespace svo {

namespace {

constexpr uint32_t MIXED = 0xFFFFFFFFu;
constexpr unsigned SUMMARY_BLOCK = 1024;            // 16 waves: the 16 rows of up to 64 blocks along x
__host__ __device__ __forceinline__ uint32_t fold(uint32_t a, uint32_t b) { return a == b ? a : MIXED; }
// Level L of the pyramid ((2^L)^3 entries, x fastest) starts at this word: level 0 at 0, level 1 at 8, the others straight behind
// ((8^L - 1) / 7 is 1 mod 8) - every level from 1 on is 32-byte aligned, k_grid_mip reads pairs.  Words 1 .. 7 are cleared.
inline uint64_t pyramid_offset(uint32_t L) { return L == 0 ? 0 : ((1ull << (3 * L)) - 1) / 7 + 7; }

using GridCell = BfsCell<uint32_t>;                 // frontier entry: the node's integer corner in cells and its slot

// base[(bz * nb + by) * nb + bx] of the 4^3 block (bx, by, bz), nb = N / 4.  Thread g: lx = g % TX its block along x within the tile,
// yz = (g / TX) % 16 its row (y = yz & 3, z = yz >> 2), g / (16 * TX) the tile (TX = 2^tx_log2 <= 64 blocks along x; tiles x fastest).
__global__ __launch_bounds__(SUMMARY_BLOCK) void k_grid_summary(const uint16_t *grid, uint32_t depth, uint32_t tx_log2, uint32_t *base)
{
    __shared__ uint32_t sh[SUMMARY_BLOCK];
    const uint32_t nb_log2 = depth - TWIG_LEVELS;
    const uint64_t g = (uint64_t)blockIdx.x * SUMMARY_BLOCK + threadIdx.x;
    const bool live = g < (16ull << (3 * nb_log2));
    const uint32_t lx = (uint32_t)g & ((1u << tx_log2) - 1u), yz = (uint32_t)(g >> tx_log2) & 15u;
    const uint64_t tile = g >> (tx_log2 + 4);
    const uint32_t tiles_log2 = nb_log2 - tx_log2;
    const uint32_t bx = (((uint32_t)tile & ((1u << tiles_log2) - 1u)) << tx_log2) + lx;
    const uint32_t by = (uint32_t)(tile >> tiles_log2) & ((1u << nb_log2) - 1u);
    const uint32_t bz = (uint32_t)(tile >> (tiles_log2 + nb_log2));
    uint32_t v = MIXED;
    if (live) {
        const uint64_t z = (uint64_t)bz * 4 + (yz >> 2), y = by * 4 + (yz & 3u);
        const uint64_t cell = (((z << depth) + y) << depth) + bx * 4;
        const uint2 q = *reinterpret_cast<const uint2 *>(grid + cell);
        const uint32_t c = q.x & 0xFFFFu;
        v = (q.x == (c | c << 16) && q.y == q.x) ? c : MIXED;
    }
    sh[threadIdx.x] = v;
    __syncthreads();
    if (live && yz == 0u) {
#pragma unroll
        for (uint32_t k = 1; k < 16; ++k) v = fold(v, sh[threadIdx.x + (k << tx_log2)]);
        base[((((uint64_t)bz << nb_log2) + by) << nb_log2) + bx] = v;
    }
}

// level L (n = 2^L per axis) from level L + 1
__global__ __launch_bounds__(256) void k_grid_mip(const uint32_t *fine, uint32_t *up, uint32_t L)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (1ull << (3 * L))) return;
    const uint32_t m = (1u << L) - 1u, x = (uint32_t)i & m, y = (uint32_t)(i >> L) & m, z = (uint32_t)(i >> (2 * L));
    uint32_t v = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint64_t at = ((((uint64_t)(2 * z + (r >> 1)) << (L + 1)) + 2 * y + (r & 1u)) << (L + 1)) + 2 * x;
        const uint2 q = *reinterpret_cast<const uint2 *>(fine + at);
        const uint32_t p = fold(q.x, q.y);
        v = r ? fold(v, p) : p;
    }
    up[i] = v;
}

struct IsMixed { __host__ __device__ __forceinline__ uint32_t operator()(const uint32_t &v) const { return v == MIXED ? 1u : 0u; } };
using MixedIterator = hipcub::TransformInputIterator<uint32_t, IsMixed, const uint32_t *>;

// type of every frontier node and its flags for the scan (BRANCH in the low half, TWIG in the high half, as builder.hip's k_classify):
// `level` is the pyramid's level L, shift = depth - L turns a cell corner into the node's coordinate, `last` = (L == depth - 2)
__global__ __launch_bounds__(256) void k_grid_classify(const GridCell *frontier, uint32_t n, const uint32_t *level, uint32_t L, uint32_t shift,
                                                       uint32_t last, uint32_t *word, unsigned long long *flags)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const GridCell e = frontier[i];
    const uint32_t v = level[((((uint64_t)(e.z >> shift) << L) + (e.y >> shift)) << L) + (e.x >> shift)];
    uint32_t w, br = 0, tw = 0;
    if (v != MIXED) w = v ? node_make(LEAF, v) : node_make(EMPTY, 0);
    else if (last) { w = node_make(TWIG, 0); tw = 1; }
    else { w = node_make(BRANCH, 0); br = 1; }
    word[i] = w;
    flags[i] = (unsigned long long)br | ((unsigned long long)tw << 32);
}

// one thread per (brick, z-row): the row's 16 cells (index z*16 + y*4 + x) are four x-rows of the grid, out as one 32-byte store
__global__ __launch_bounds__(256) void k_grid_bricks(const GridCell *jobs, uint32_t n, const uint16_t *grid, uint32_t depth, uint16_t *twig)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n * 4u) return;
    const uint32_t j = i >> 2, z = i & 3u;
    const GridCell e = jobs[j];
    const uint16_t *src = grid + ((((((uint64_t)e.z + z) << depth) + e.y) << depth) + e.x);
    const uint64_t row = 1ull << depth;
    const uint2 r0 = *reinterpret_cast<const uint2 *>(src), r1 = *reinterpret_cast<const uint2 *>(src + row);
    const uint2 r2 = *reinterpret_cast<const uint2 *>(src + 2 * row), r3 = *reinterpret_cast<const uint2 *>(src + 3 * row);
    uint4 *dst = reinterpret_cast<uint4 *>(twig + (uint64_t)e.slot * TWIG_WORDS + z * 16);
    dst[0] = make_uint4(r0.x, r0.y, r1.x, r1.y);
    dst[1] = make_uint4(r2.x, r2.y, r3.x, r3.y);
}

struct ToGridArgs {
    const uint32_t *tree;       // the chunk's node words (in the world's tree pool)
    const uint16_t *twig;       // its bricks
    uint32_t trees, twigs;      // how many of each: nothing beyond them is read
    uint32_t chunk_depth, depth;
    uint16_t *out;
};

// Output cells [8r, 8r + 8) of the grid (x fastest: one row, or two rows of a 4^3 grid).  Output cell x reports the finest voxel
// X = x << (D - d) (d <= D: its min corner) or x >> (d - D) (replication).  A descent ends in an EMPTY / LEAF node of edge 2^lg voxels
// or a brick cell of edge 2^(lg - 2): every output cell of the row whose voxel lies below X | (2^lg - 1) + 1 shares the value.
__global__ __launch_bounds__(256) void k_to_grid(ToGridArgs A)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (1ull << (3 * A.depth - 3))) return;
    const uint32_t d = A.depth, D = A.chunk_depth, m = (1u << d) - 1u;
    const uint32_t up = d <= D ? D - d : 0u, down = d <= D ? 0u : d - D;
    uint64_t lo = 0, hi = 0;
    for (uint32_t k = 0; k < 8;) {
        const uint64_t lin = 8 * r + k;
        const uint32_t x = (uint32_t)lin & m, y = (uint32_t)(lin >> d) & m, z = (uint32_t)(lin >> (2 * d));
        const uint32_t X = (x << up) >> down, Y = (y << up) >> down, Z = (z << up) >> down;
        uint32_t node = 0, lg = D, material = 0, span_lg = 0;
        while (node < A.trees) {
            const uint32_t w = A.tree[node], type = node_type(w), off = node_offset(w);
            if (type == BRANCH) {
                if (lg <= TWIG_LEVELS) break;                                   // (a BRANCH below level depth-2: no pool validate_chunk admits)
                --lg;
                node = off + (((X >> lg) & 1u) | ((Y >> lg) & 1u) << 1 | ((Z >> lg) & 1u) << 2);
                continue;
            }
            if (type == TWIG) {
                if (off >= A.twigs) break;
                const uint32_t c = lg - TWIG_LEVELS;                            // a brick cell's edge is 2^c voxels
                material = A.twig[(uint64_t)off * TWIG_WORDS + ((Z >> c) & 3u) * 16 + ((Y >> c) & 3u) * 4 + ((X >> c) & 3u)];
                span_lg = c;
            } else {
                material = type == LEAF ? off & 0xFFFFu : 0u;
                span_lg = lg;
            }
            break;
        }
        const uint32_t end_voxel = (X | ((1u << span_lg) - 1u)) + 1u;           // first voxel along x beyond the node / cell
        const uint32_t end_cell = ((end_voxel + (1u << up) - 1u) >> up) << down;    // first output cell of the row that is not in it
        const uint32_t count = min(end_cell - x, 8u - k);
        for (uint32_t j = 0; j < count; ++j, ++k) {
            if (k < 4) lo |= (uint64_t)material << (16 * k);
            else hi |= (uint64_t)material << (16 * (k - 4));
        }
    }
    *reinterpret_cast<uint4 *>(A.out + 8 * r) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}

// the summary pyramid of `grid` at `pyr` (pyramid_offset); with SVO_BUILD_TIMING the base kernel's device time goes to stderr
int build_summary(const uint16_t *grid, uint32_t depth, uint32_t *pyr, hipStream_t s)
{
    const uint32_t maxlevel = depth - TWIG_LEVELS;
    const bool timing = std::getenv("SVO_BUILD_TIMING") != nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (timing) { HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1)); HIP_TRY(hipEventRecord(e0, s)); }
    const uint32_t tx_log2 = std::min(maxlevel, 6u);
    hipLaunchKernelGGL(k_grid_summary, dim3(blocks_for(16ull << (3 * maxlevel), SUMMARY_BLOCK)), dim3(SUMMARY_BLOCK), 0, s,
                       grid, depth, tx_log2, pyr + pyramid_offset(maxlevel));
    if (timing) HIP_TRY(hipEventRecord(e1, s));
    if (maxlevel > 0) HIP_TRY(hipMemsetAsync(pyr, 0, 8 * sizeof(uint32_t), s));
    for (uint32_t L = maxlevel; L > 0; --L)
        hipLaunchKernelGGL(k_grid_mip, dim3(blocks_for(1ull << (3 * (L - 1)), 256)), dim3(256), 0, s, pyr + pyramid_offset(L), pyr + pyramid_offset(L - 1), L - 1);
    HIP_TRY(hipGetLastError());
    if (timing) {
        float ms = 0.0f;
        HIP_TRY(hipEventSynchronize(e1));
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        std::fprintf(stderr, "[svo grid] summary base, depth %u: %.4f ms\n", depth, ms);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    return SVO_OK;
}

int chunk_from_grid_resident(svo_world &w, int chunk, const uint16_t *grid, uint32_t depth)
{
    HIP_TRY(hipSetDevice(w.device));
    HIP_TRY(hipDeviceSynchronize());                    // ordered behind every launch issued before it, like svo_world_edit_box
    hipStream_t s = nullptr;
    const uint32_t maxlevel = depth - TWIG_LEVELS;
    int rc;
    GridScratch &S = grid_scratch(w);
    BfsArrays &B = bfs_arrays(w);
    // the pyramid, and from it the pools' sizes
    const uint64_t above = pyramid_offset(maxlevel), base = 1ull << (3 * maxlevel);
    if ((rc = S.pyramid.reserve(above + base, false, s)) != SVO_OK || (rc = S.counts.reserve(2, false, s)) != SVO_OK || (rc = B.h_totals.alloc(2)) != SVO_OK) return rc;
    uint32_t *const pyr = S.pyramid.p, *const counts = S.counts.p, *const h = B.h_totals.p;
    if ((rc = build_summary(grid, depth, pyr, s)) != SVO_OK) return rc;
    HIP_TRY(hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), s));
    {
        size_t need_above = 0, need_base = 0;
        if (above) HIP_TRY(hipcub::DeviceReduce::Sum(nullptr, need_above, MixedIterator(pyr, IsMixed()), counts, (int)above, s));
        HIP_TRY(hipcub::DeviceReduce::Sum(nullptr, need_base, MixedIterator(pyr + above, IsMixed()), counts + 1, (int)base, s));
        if ((rc = S.reduce_tmp.reserve(std::max(need_above, need_base) + 16, false, s)) != SVO_OK) return rc;
        unsigned char *const tmp = S.reduce_tmp.p;
        if (above) HIP_TRY(hipcub::DeviceReduce::Sum(tmp, need_above, MixedIterator(pyr, IsMixed()), counts, (int)above, s));
        HIP_TRY(hipcub::DeviceReduce::Sum(tmp, need_base, MixedIterator(pyr + above, IsMixed()), counts + 1, (int)base, s));
    }
    HIP_TRY(hipMemcpyAsync(h, counts, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t trees = 1 + 8ull * h[0], twigs = h[1];
    if (trees >= (1ull << 30) || twigs >= (1ull << 30)) { set_error("svo_world_chunk_from_grid: chunk exceeds the 30-bit node offset"); return SVO_ERR_UNSUPPORTED; }
    uint32_t *tree = nullptr;
    uint16_t *twig = nullptr;
    if ((rc = edit_scratch(w, trees, twigs, &tree, &twig)) != SVO_OK) return rc;
    // grow(): the corners are in cells, a node's coordinate in level L of the pyramid is its corner >> (depth - L)
    const char *const disagree = "svo_world_chunk_from_grid: the walk disagrees with the summary's counts";
    uint64_t trees_done = 1, twigs_done = 0;
    rc = bfs_grow<uint32_t>(B, GridCell{ 0u, 0u, 0u, 0u }, 1u << depth, trees_done, twigs_done, tree, s,
        [&](uint32_t level, uint32_t, const GridCell *frontier, uint32_t n, uint32_t *word, unsigned long long *flags) -> int {
            hipLaunchKernelGGL(k_grid_classify, dim3(blocks_for(n, 256)), dim3(256), 0, s, frontier, n, pyr + pyramid_offset(level), level, depth - level,
                               level == maxlevel ? 1u : 0u, word, flags);
            return SVO_OK;
        },
        [&](uint64_t nb, uint64_t nt) -> int {      // (the walk numbers exactly what the reduce counted: anything else would write beyond the pools)
            if (trees_done + 8 * nb > trees || twigs_done + nt > twigs) { set_error(disagree); return SVO_ERR_HIP; }
            return SVO_OK;
        },
        [&](const GridCell *jobs, uint32_t nt) { hipLaunchKernelGGL(k_grid_bricks, dim3(blocks_for((uint64_t)nt * 4, 256)), dim3(256), 0, s, jobs, nt, grid, depth, twig); });
    if (rc != SVO_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    if (trees_done != trees || twigs_done != twigs) { set_error(disagree); return SVO_ERR_HIP; }
    return install_rebuilt(w, chunk, depth, nullptr, trees, twigs, tree, twig);
}

bool grid_args_ok(const svo_world *w, int chunk, const void *grid_dev, uint32_t depth)
{
    return w && grid_dev && chunk >= 0 && chunk < (int)w->chunks.size() && depth >= SVO_GRID_MIN_DEPTH && depth <= SVO_GRID_MAX_DEPTH &&
           ((uintptr_t)grid_dev & 15u) == 0;
}

} // namespace

} // namespace svo

using namespace svo;

extern "C" {

int svo_world_chunk_from_grid(svo_world *w, int chunk, const uint16_t *grid_dev, uint32_t depth)
{
    if (!grid_args_ok(w, chunk, grid_dev, depth)) { set_error("svo_world_chunk_from_grid: bad argument (chunk in range, depth in [2, 10], a 16-byte aligned grid)"); return SVO_ERR_INVALID_ARG; }
    if (w->device < 0) { set_error("svo_world_chunk_from_grid: the world is not uploaded (svo_chunk_from_grid builds host pools)"); return SVO_ERR_NOT_UPLOADED; }
    return fenced("svo_world_chunk_from_grid", [&] { return chunk_from_grid_resident(*w, chunk, grid_dev, depth); });
}

int svo_world_chunk_to_grid(svo_world *w, int chunk, uint32_t depth, uint16_t *grid_dev, void *stream)
{
    if (!grid_args_ok(w, chunk, grid_dev, depth)) { set_error("svo_world_chunk_to_grid: bad argument (chunk in range, depth in [2, 10], a 16-byte aligned grid)"); return SVO_ERR_INVALID_ARG; }
    if (w->device < 0) { set_error("svo_world_chunk_to_grid: world is not uploaded"); return SVO_ERR_NOT_UPLOADED; }
    HIP_TRY(hipSetDevice(w->device));
    const ChunkPools &c = w->chunks[(size_t)chunk];
    const DevChunk &e = w->table[(size_t)chunk];
    ToGridArgs A;
    A.tree = w->hbm->tree.p + e.tree_off;
    A.twig = w->hbm->twig.p + e.twig_off * TWIG_WORDS;
    A.trees = (uint32_t)c.tree_count(); A.twigs = (uint32_t)c.twig_count();     // (< 2^30: offsets are 30-bit)
    A.chunk_depth = c.depth; A.depth = depth;
    A.out = grid_dev;
    hipLaunchKernelGGL(k_to_grid, dim3(blocks_for(1ull << (3 * depth - 3), 256)), dim3(256), 0, (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError());
    return SVO_OK;
}

} // extern "C"
