// compact.cpp — Ocroot::defragcopy and Ocroot::lodmm (src/Octree.cpp:445-614, 626-765) on a chunk's host pools: the host half
// of svo_world_compact / svo_world_coarsen.  An uploaded world takes the device half (compact.hip) instead.
//
// Both rebuild a chunk from its root into fresh pools, depth-first in child-slot order, so that a block's index is 1 + 8 x (kept
// BRANCHes before it in preorder) and a brick's is the number of kept bricks before it:
//   compact   only what the root reaches is copied (a brick two TWIGs share is copied twice); a brick of one value becomes
//             EMPTY / LEAF; a BRANCH whose children all come back as one node of one type and value becomes that node; a BRANCH
//             whose subtree is at most two levels of EMPTY / LEAF nodes becomes one brick sampled at its 4x4x4 cell centres (and
//             then goes through the one-value test).  A folded subtree's blocks and bricks are taken back.
//   coarsen   depth -> depth - 1: BRANCHes above level depth-3 are copied as they are, a BRANCH at depth-3 becomes a brick whose
//             cells are the majority (density + MisraGriesCounter<8>) of the 8 cells under each; every other node is compacted.
// In a tree that passes validate_chunk each coarsened cell sees one child (weight 64) or one 2x2x2 block of brick cells (weight
// 1 each); with at most 8 values in 8 counter slots the counter never evicts, so the majority is the most frequent value with
// ties to the one seen first in z, y, x order.  That short form is what is computed here and in compact.hip; tests/lod_model.py
// states the counter in full and its CPU tests check that the two agree.
#include "world.h"

#include <algorithm>
#include <cstring>

namespace svo {

namespace {

uint16_t leaf_value(uint32_t word) { return node_type(word) == LEAF ? (uint16_t)node_offset(word) : (uint16_t)0; }

// most frequent of n values, ties to the first seen
uint16_t majority(const uint16_t *v, int n)
{
    int best = 0, best_count = 0;
    for (int i = 0; i < n; ++i) {
        int c = 0;
        for (int j = 0; j < n; ++j) c += v[j] == v[i];
        if (c > best_count) { best = i; best_count = c; }
    }
    return v[best];
}

struct Rebuild {
    const ChunkPools &from;
    std::vector<uint32_t> tree;         // may hold more than `trees` words: a taken-back subtree's words stay readable
    std::vector<uint16_t> twig;
    uint64_t trees = 1, twigs = 0;
    uint32_t coarse_level = UINT32_MAX; // coarsen: the level whose BRANCHes become bricks

    explicit Rebuild(const ChunkPools &c) : from(c), tree(16), twig(16 * TWIG_WORDS) {}

    // a brick to be written at node t: one value -> EMPTY / LEAF (returns 1), otherwise appended (returns 3)
    int brick(uint64_t t, const uint16_t *cells, bool fold = true)
    {
        bool mono = true;
        for (uint32_t i = 1; i < TWIG_WORDS && mono; ++i) mono = cells[i] == cells[0];
        if (fold && mono) { tree[t] = cells[0] ? node_make(LEAF, cells[0]) : node_make(EMPTY, 0); return 1; }
        const uint64_t i = twigs++;
        if (twig.size() < twigs * TWIG_WORDS) twig.resize(twig.size() * 2);
        std::memcpy(&twig[i * TWIG_WORDS], cells, TWIG_WORDS * sizeof(uint16_t));
        tree[t] = node_make(TWIG, (uint32_t)i);
        return (int)TWIG_LEVELS + 1;
    }

    uint64_t open_block(uint64_t t)
    {
        const uint64_t first = trees;
        trees += 8;
        if (tree.size() < trees) tree.resize(std::max<size_t>(tree.size() * 2, trees));
        tree[t] = node_make(BRANCH, (uint32_t)first);
        return first;
    }

    // defragcopy: node f of `from` -> node t; returns the depth of what was written
    int compact(uint64_t f, uint64_t t)
    {
        const uint32_t word = from.tree[f];
        switch (node_type(word)) {
        case EMPTY: tree[t] = node_make(EMPTY, 0); return 1;
        case LEAF: tree[t] = word; return 1;
        case TWIG: return brick(t, &from.twig[(size_t)node_offset(word) * TWIG_WORDS]);
        default: break;
        }
        const uint64_t trees0 = trees, twigs0 = twigs;
        const uint64_t first = open_block(t);
        int maxd = 0;
        for (uint32_t c = 0; c < 8; ++c) maxd = std::max(maxd, compact(node_offset(word) + c, first + c));
        if (maxd == 1) {
            bool mono = true;
            for (uint32_t c = 1; c < 8 && mono; ++c) mono = tree[first + c] == tree[first];
            if (mono) {
                trees = trees0; twigs = twigs0;
                const uint32_t x = node_offset(tree[first]);
                tree[t] = x ? node_make(LEAF, x) : node_make(EMPTY, 0);
                return 1;
            }
        }
        if (maxd == (int)TWIG_LEVELS) {
            // two levels of EMPTY / LEAF under t: one brick, sampled at its cell centres from the children just written
            trees = trees0; twigs = twigs0;
            uint16_t cells[TWIG_WORDS];
            for (uint32_t w = 0; w < TWIG_WORDS; ++w) {
                const uint32_t x = w & 3, y = (w >> 2) & 3, z = w >> 4;
                uint32_t node = tree[first + ((x >> 1) | (y >> 1) << 1 | (z >> 1) << 2)];
                if (node_type(node) == BRANCH) node = tree[node_offset(node) + ((x & 1) | (y & 1) << 1 | (z & 1) << 2)];
                cells[w] = leaf_value(node);
            }
            return brick(t, cells);
        }
        return maxd + 1;
    }

    // lodmm: node f at `level` of `from` -> node t
    void coarsen(uint64_t f, uint64_t t, uint32_t level)
    {
        const uint32_t word = from.tree[f];
        if (node_type(word) != BRANCH) { (void)compact(f, t); return; }
        if (level == coarse_level) {
            uint16_t cells[TWIG_WORDS];
            for (uint32_t w = 0; w < TWIG_WORDS; ++w) {
                const uint32_t x = w & 3, y = (w >> 2) & 3, z = w >> 4;
                const uint32_t child = from.tree[node_offset(word) + ((x >> 1) | (y >> 1) << 1 | (z >> 1) << 2)];
                if (node_type(child) != TWIG) { cells[w] = node_type(child) == LEAF ? (uint16_t)node_offset(child) : 0; continue; }
                const uint16_t *b = &from.twig[(size_t)node_offset(child) * TWIG_WORDS];
                const uint32_t x0 = (x & 1) * 2, y0 = (y & 1) * 2, z0 = (z & 1) * 2;
                uint16_t v[8];
                for (uint32_t k = 0; k < 8; ++k)
                    v[k] = b[(z0 + (k >> 2)) * 16 + (y0 + ((k >> 1) & 1)) * 4 + x0 + (k & 1)];
                cells[w] = majority(v, 8);
            }
            (void)brick(t, cells, false);       // (written even when every cell is 0: lodmm does not fold these)
            return;
        }
        const uint64_t first = open_block(t);
        for (uint32_t c = 0; c < 8; ++c) coarsen(node_offset(word) + c, first + c, level + 1);
    }
};

int rebuild_host(svo_world &w, int chunk, bool lod, const char *who)
{
    ChunkPools &cur = w.chunks[(size_t)chunk];
    Rebuild r(cur);
    if (lod) { r.coarse_level = cur.depth - 1 - TWIG_LEVELS; r.coarsen(0, 0, 0); }
    else (void)r.compact(0, 0);
    ChunkPools next;
    std::memcpy(next.position, cur.position, sizeof next.position);
    next.size = cur.size; next.depth = lod ? cur.depth - 1 : cur.depth;
    r.tree.resize(r.trees); r.twig.resize(r.twigs * TWIG_WORDS);
    next.tree.swap(r.tree); next.twig.swap(r.twig);
    next.tree_capacity = cur.tree_capacity; next.twig_capacity = cur.twig_capacity;     // (svo_world_update's floor)
    next.fit_capacity(next.tree.size(), next.twig_count());
    std::string why;
    const int rc = validate_chunk(next, why);
    if (rc != SVO_OK) { set_error(std::string(who) + ": " + why); return rc; }
    cur.tree.swap(next.tree); cur.twig.swap(next.twig);
    cur.depth = next.depth;
    cur.tree_capacity = next.tree_capacity; cur.twig_capacity = next.twig_capacity;
    classify_world(w);
    return SVO_OK;
}

int rebuild_chunk(svo_world *w, int chunk, bool lod, const char *who)
{
    if (!w || chunk < 0 || chunk >= (int)w->chunks.size()) { set_error(std::string(who) + ": bad argument"); return SVO_ERR_INVALID_ARG; }
    if (lod && w->chunks[(size_t)chunk].depth <= TWIG_LEVELS) {
        set_error(std::string(who) + ": a chunk of depth 2 has no coarser level (depth 1 cannot hold a brick)");
        return SVO_ERR_UNSUPPORTED;
    }
    return fenced(who, [&] { return w->device >= 0 ? rebuild_resident(*w, chunk, lod) : rebuild_host(*w, chunk, lod, who); });
}

} // namespace

} // namespace svo

extern "C" {

int svo_world_compact(svo_world *w, int chunk) { return svo::rebuild_chunk(w, chunk, false, "svo_world_compact"); }
int svo_world_coarsen(svo_world *w, int chunk) { return svo::rebuild_chunk(w, chunk, true, "svo_world_coarsen"); }

} // extern "C"
