// sparse_fill.cpp — svo_chunk_fill_enclosed: svo_grid_fill_enclosed's rule applied to the chunk's conceptual grid of finest voxels, on
// the tree, on the host.  The readable statement of the sparse interior fill and the twin of sparse_fill.hip; depth 2 .. 16.
//   elements   the walk from the root collects what the flood moves through: the EMPTY nodes it reaches (EMPTY, or LEAF | 0: a cube of
//              edge 2^(depth - level) cells that is connected inside) and the empty cells of the bricks (one 64-bit mask per TWIG node,
//              bit cz * 16 + cy * 4 + cx).  Two face-adjacent cubes share a pair of face-adjacent cells, so the flood over the elements
//              is the flood over the cells
//   flood      a queue.  An EMPTY node that touches a face of the chunk and a brick cell with a coordinate of 0 or N - 1 are OUTSIDE.
//              An element that turns OUTSIDE hands that on across its six faces: the neighbour is found by the integer descent from
//              the root towards the adjacent cell, stopped at the element's own level; a BRANCH found there is enumerated by a
//              recursive descent restricted to the children on that face.  A brick floods inside its own mask by shifts of 1, 4, 16
//   fold       bottom-up, a result word per reached node: an EMPTY node that is not outside is LEAF | material; a brick that holds one
//              value after the fill is that LEAF (EMPTY for 0); a BRANCH whose eight results are one EMPTY / LEAF word is that word
//   emit       the FIFO walk over the results (chunk_pools.h: emit_fifo, which also holds the validation pass and the desc's producer)
// Working memory is proportional to the node words and the bricks; nothing has N^3 entries.  No HIP include: plain g++ compiles this
// file (host/sparse_fill_check.cpp runs it under the sanitizers).
#include <cmath>
#include <new>

#include "chunk_pools.h"
#include "sparse_fill_rule.h"

namespace svo {

namespace {

struct Item { uint32_t node, x, y, z, level; };             // an element in the queue: its node word's index, its corner in cells, its level

struct Fill {
    const uint32_t *tree; const uint16_t *twig;
    uint32_t depth, maxlevel, N;
    std::vector<uint8_t> outside;                           // per node word: the EMPTY node there is OUTSIDE
    std::vector<uint32_t> slot;                             // per node word: a TWIG's entry in `empty` / `out`
    std::vector<uint64_t> empty, out;                       // per TWIG node: its cells that are 0 / that are OUTSIDE
    std::vector<Item> queue;

    bool hollow(uint32_t w) const { return fill_is_empty(w); }

    void node_out(uint32_t node, uint32_t x, uint32_t y, uint32_t z, uint32_t level)
    {
        if (outside[node]) return;
        outside[node] = 1;
        queue.push_back(Item{ node, x, y, z, level });
    }
    void brick_out(uint32_t node, uint32_t x, uint32_t y, uint32_t z, uint64_t bits)
    {
        const uint32_t k = slot[node];
        const uint64_t now = fill_flood_brick(out[k] | (bits & empty[k]), empty[k]);
        if (now == out[k]) return;
        out[k] = now;
        queue.push_back(Item{ node, x, y, z, maxlevel });
    }

    // the walk: elements, the bricks' masks and the seeds
    void collect(uint32_t node, uint32_t x, uint32_t y, uint32_t z, uint32_t level)
    {
        const uint32_t w = tree[node], e = N >> level;
        if (node_type(w) == BRANCH) {
            for (uint32_t c = 0; c < 8; ++c) collect(node_offset(w) + c, x + (c & 1u) * (e / 2), y + ((c >> 1) & 1u) * (e / 2), z + (c >> 2) * (e / 2), level + 1);
        } else if (node_type(w) == TWIG) {
            const uint16_t *cells = twig + (size_t)node_offset(w) * TWIG_WORDS;
            uint64_t m = 0;
            for (uint32_t i = 0; i < TWIG_WORDS; ++i) m |= (uint64_t)(cells[i] == 0) << i;
            slot[node] = (uint32_t)empty.size();
            empty.push_back(m); out.push_back(0);
            brick_out(node, x, y, z, fill_border_cells(x, y, z, N));
        } else if (hollow(w) && (x == 0 || y == 0 || z == 0 || x + e == N || y + e == N || z + e == N)) node_out(node, x, y, z, level);
    }

    // what lies behind face `f` (axis f >> 1, side f & 1) of the cube (x, y, z) of level `level`, itself OUTSIDE, turns OUTSIDE.
    // `bits`: a brick's OUTSIDE cells (level == maxlevel and the element is a brick), ~0 for an EMPTY node
    void across(const Item &it, uint32_t f, uint64_t bits)
    {
        const uint32_t e = N >> it.level, axis = f >> 1, side = f & 1u;
        uint32_t p[3] = { it.x, it.y, it.z };
        if (side ? p[axis] + e == N : p[axis] == 0) return; // the chunk's own faces are the outside: nothing beyond them is consulted
        p[axis] = side ? p[axis] + e : p[axis] - 1;
        uint32_t node = 0, level = 0;
        while (node_type(tree[node]) == BRANCH && level < it.level) {
            ++level;
            const uint32_t lg = depth - level;
            node = node_offset(tree[node]) + (((p[0] >> lg) & 1u) | ((p[1] >> lg) & 1u) << 1 | ((p[2] >> lg) & 1u) << 2);
        }
        const uint32_t mask = ~((N >> level) - 1u);
        spread(node, p[0] & mask, p[1] & mask, p[2] & mask, level, f, bits);
    }
    // the part of node (corner, level) that touches the face: everything for an EMPTY node, the facing cells of a brick, the four
    // children of a BRANCH that lie on the side the face came from
    void spread(uint32_t node, uint32_t x, uint32_t y, uint32_t z, uint32_t level, uint32_t f, uint64_t bits)
    {
        const uint32_t w = tree[node];
        if (node_type(w) == BRANCH) {
            const uint32_t axis = f >> 1, near = (f & 1u) ? 0u : 1u, h = N >> (level + 1);      // leaving through +axis enters at the child's low side
            for (uint32_t c = 0; c < 8; ++c)
                if (((c >> axis) & 1u) == near) spread(node_offset(w) + c, x + (c & 1u) * h, y + ((c >> 1) & 1u) * h, z + (c >> 2) * h, level + 1, f, bits);
        } else if (node_type(w) == TWIG) brick_out(node, x, y, z, fill_face_pull(bits, f));
        else if (hollow(w) && fill_face_pull(bits, f) != 0) node_out(node, x, y, z, level);
    }

    void flood()
    {
        while (!queue.empty()) {
            const Item it = queue.back();
            queue.pop_back();
            const bool brick = node_type(tree[it.node]) == TWIG;
            const uint64_t bits = brick ? out[slot[it.node]] : ~0ull;
            for (uint32_t f = 0; f < 6; ++f) across(it, f, bits);
        }
    }

    // ---- fold and emit ----
    std::vector<uint32_t> res;                              // per reached node word: its result (BRANCH / TWIG without an offset)
    uint64_t filled = 0;
    uint32_t material = 0;

    uint32_t fold(uint32_t node, uint32_t level)
    {
        const uint32_t w = tree[node];
        uint32_t r;
        if (node_type(w) == BRANCH) {
            uint32_t first = 0;
            bool one = true;
            for (uint32_t c = 0; c < 8; ++c) {
                const uint32_t k = fold(node_offset(w) + c, level + 1);
                if (c == 0) first = k;
                one = one && k == first;
            }
            r = one && node_type(first) != BRANCH && node_type(first) != TWIG ? first : node_make(BRANCH, 0);
        } else if (node_type(w) == TWIG) {
            const uint64_t in = empty[slot[node]] & ~out[slot[node]];
            filled += (uint64_t)__builtin_popcountll(in);
            r = fill_brick_result(twig + (size_t)node_offset(w) * TWIG_WORDS, in, material);
        } else if (hollow(w)) {
            const uint64_t e = N >> level;
            if (!outside[node]) filled += e * e * e;
            r = outside[node] ? node_make(EMPTY, 0) : node_make(LEAF, material);
        } else r = node_make(LEAF, node_offset(w) & 0xFFFFu);
        return res[node] = r;
    }

    void emit(std::vector<uint32_t> &otree, std::vector<uint16_t> &otwig) const
    {
        emit_fifo(0u, [&](uint32_t node) { return res[node]; }, [&](uint32_t node, uint32_t c) { return node_offset(tree[node]) + c; },
                  [&](uint32_t node, std::vector<uint16_t> &to) {
                      const uint64_t in = empty[slot[node]] & ~out[slot[node]];
                      const uint16_t *cells = twig + (size_t)node_offset(tree[node]) * TWIG_WORDS;
                      for (uint32_t i = 0; i < TWIG_WORDS; ++i) to.push_back((in >> i) & 1ull ? (uint16_t)material : cells[i]);
                  }, otree, otwig);
    }
};

} // namespace

} // namespace svo

extern "C" {

int svo_chunk_fill_enclosed(const svo_chunk_desc *in, uint16_t material, svo_chunk_desc *out, uint64_t *filled_out)
{
    using namespace svo;
    const char *who = "svo_chunk_fill_enclosed";
    if (!in || !out || in == out || material == 0 || !in->tree || in->trees == 0 || (in->twigs && !in->twig) || !(in->size > 0.0f) || !std::isfinite(in->size)) {
        set_error(std::string(who) + ": bad argument (in and out, not the same; a material other than 0; pools; a positive finite size)");
        return SVO_ERR_INVALID_ARG;
    }
    try {
        // a depth the fill reaches, then what a world asks of the pools (chunk_pools.h: pools_walk); a shallow TWIG met before the
        // first malformed word is the answer
        if (in->depth < SVO_FILL_MIN_DEPTH || in->depth > SVO_FILL_MAX_DEPTH) { set_error(std::string(who) + ": the chunk's depth is outside [2, 16]"); return SVO_ERR_UNSUPPORTED; }
        bool shallow = false;
        const char *why = (in->trees - 1) % 8 != 0 || in->trees > (1ull << 30) || in->twigs > (1ull << 30) ? "the tree pool is not 1 + 8k node words"
                                                                                                            : pools_walk(in->tree, in->trees, in->twigs, in->depth, &shallow);
        if (shallow) { set_error(std::string(who) + ": " + SHALLOW_TWIG_WHY); return SVO_ERR_UNSUPPORTED; }
        if (why) { set_error(std::string(who) + ": " + why); return SVO_ERR_INVALID_ARG; }
        Fill F;
        F.tree = in->tree; F.twig = in->twig;
        F.depth = in->depth; F.maxlevel = in->depth - TWIG_LEVELS; F.N = 1u << in->depth;
        F.material = material;
        F.outside.assign(in->trees, 0);
        F.slot.assign(in->trees, 0);
        F.res.assign(in->trees, 0);
        F.collect(0, 0, 0, 0, 0);
        F.flood();
        F.fold(0, 0);
        std::vector<uint32_t> tree;
        std::vector<uint16_t> twig;
        F.emit(tree, twig);
        if (const int rc = chunk_desc_take(out, in->position, in->size, in->depth, tree, twig, who)) return rc;
        if (filled_out) *filled_out = F.filled;
        return SVO_OK;
    } catch (const std::bad_alloc &) {
        set_error(std::string(who) + ": out of host memory");
        return SVO_ERR_OUT_OF_MEMORY;
    }
}

} // extern "C"
