// locate.hip.h — svo_world_locate: the voxel under each point of a device list, one thread per point.
//
//   World::index_float + World::index   src/World.cpp:288-293,323-332   (march.hip.h: chunk_index)
//   traverse                            src/Traverse.cpp:34-48
//   the cell lookup of twigmarch        src/Traverse.cpp:58-67 / shaders/Chunkmarch.glsl:201,212
//
// A query is one chain of dependent loads - chunk table entry, one node word per level (k_locate_literal) or one wide entry per
// two levels (k_locate_wide: wide_tree.hip.h), the brick cell - and a handful of compares: occupancy is what hides it, so both
// kernels stay free of LDS and far below the register budget of a full SIMD.  Both write the same record for every point:
// k_locate_wide keeps the reference's comparisons p >= mid against the accumulated midpoints (two per axis per wide node) and
// only takes the WORDS from the wide pool; a cell coordinate rounded from (p - bmin) / size could cross a face.
// The record (include/svo.h svo_voxel) is laid out like svo_hit: store_hit writes it, bmin in the place of t and the first two
// normal components, size in the place of the third.
// The walks are device functions - walk_literal / walk_wide: point -> terminal node; terminal_solid: its brick cell and solid bit -
// because svo_hit_ao (ao.hip.h) asks the same question of eight points per pixel and keeps only the solid bit.
#pragma once
#include <stddef.h>

#include "march.hip.h"
#include "wide_tree.hip.h"

namespace svo {

static_assert(sizeof(svo_voxel) == sizeof(svo_hit) && offsetof(svo_voxel, size) == offsetof(svo_hit, normal) + 8 &&
              offsetof(svo_voxel, material) == offsetof(svo_hit, material) && offsetof(svo_voxel, cell) == offsetof(svo_hit, cell),
              "svo_voxel is written by store_hit");

// The node traverse() ends in for a point: its box (lo, size), its type, the low 16 bits of its word (a LEAF's material), its brick
// (a TWIG's), its chunk and - where asked for - its index in the chunk's tree[].
struct Terminal { V3 lo; float size; uint32_t type, leaf_material, chunk, node; const uint16_t *cells; };

// Steps 4-7 of svo_world_locate on T: false for EMPTY, true for a LEAF, a TWIG narrowed to its brick cell (box, material and cell
// index; the node's own box and SVO_CELL_NONE on the chunk's max face).  `see`: svo_trace_params.see_through (0 = off).
__device__ __forceinline__ bool terminal_solid(V3 p, Terminal &T, bool glsl, uint32_t see, uint32_t &material, uint32_t &cell)
{
    material = 0u; cell = SVO_CELL_NONE;
    bool solid = false;
    if (T.type == LEAF) {
        material = T.leaf_material;
        solid = true;
    } else if (T.type == TWIG) {
        const float voxel = T.size / 4.0f;
        const V3 f = glsl ? (p - T.lo) * (1.0f / voxel) : (p - T.lo) / voxel;   // shaders/Chunkmarch.glsl:201,212 / src/Traverse.cpp:58
        const int ox = (int)f.x, oy = (int)f.y, oz = (int)f.z;
        const V3 off = mk((float)ox, (float)oy, (float)oz);
        if (inside(off, mk(0.0f, 0.0f, 0.0f), mk(3.0f, 3.0f, 3.0f))) {          // :59 - fails on the chunk's max face (the node's own box then)
            cell = (uint32_t)(oz * 16 + oy * 4 + ox);
            T.lo = T.lo + off * voxel;
            T.size = voxel;
            material = T.cells[cell];
            solid = material != 0u;
        }
    }
    if (see != 0u && solid && material == see) { material = 0u; solid = false; }
    return solid;
}

__device__ __forceinline__ void locate_store(void *out, int64_t k, V3 p, Terminal T, bool glsl, uint32_t see)
{
    uint32_t material, cell;
    const bool solid = terminal_solid(p, T, glsl, see, material, cell);
    store_hit(out, k, T.lo.x, mk(T.lo.y, T.lo.z, T.size), material, SVO_LOCATE_INSIDE | (solid ? (uint32_t)SVO_LOCATE_SOLID : 0u), T.chunk, T.node, cell);
}

// The tree pool, one load per level: steps 1-3 as they read.  Any geometry.  false: the point has no node (the all-zero record).
__device__ __forceinline__ bool walk_literal(const TraceArgs &A, V3 p, Terminal &T)
{
    if (!inside(p, ld3(A.worldmin), ld3(A.worldmax))) return false;
    const int ci = chunk_index(A, p);
    const DevChunk ch = A.chunks[ci];
    V3 lo = ld3(ch.bmin);
    float size = A.chunksize;
    if (!inside(p, lo, lo + size)) return false;                                // src/Traverse.cpp:154
    const uint32_t *tree = A.tree + ch.tree_off;
    uint32_t node = 0u, word;
    for (int lv = 0;; ++lv) {
        word = tree[node];
        if (node_type(word) != BRANCH || lv >= 32) break;
        const float half = size * 0.5f;
        const V3 mid = lo + half;
        const bool gx = p.x >= mid.x, gy = p.y >= mid.y, gz = p.z >= mid.z;
        lo = lo + mk(gx ? 1.0f : 0.0f, gy ? 1.0f : 0.0f, gz ? 1.0f : 0.0f) * half;
        node = node_offset(word) + (uint32_t)gx + 2u * (uint32_t)gy + 4u * (uint32_t)gz;
        size = half;
    }
    T.type = node_type(word);
    if (T.type == BRANCH) return false;                                         // deeper than 32 levels: malformed (refused on create)
    T.lo = lo; T.size = size; T.leaf_material = node_offset(word) & 0xFFFFu; T.chunk = (uint32_t)ci; T.node = node;
    T.cells = A.twig + (ch.twig_off + node_offset(word)) * TWIG_WORDS;
    return true;
}

// The wide pool, two levels per load.  The wide node of wide level kk expands the reference node of level r = 2 kk - pad (pad: the
// virtual levels above the chunk root when the branch levels are odd or none, wide_tree.hip.h); its entry is selected by the two
// comparisons per axis the reference makes at levels r and r + 1 - virtual levels make none: the chunk root is their child 0.  The
// entry names the node traverse() ends in: its level (hence which of the two boxes on the way is its box), its type and material /
// brick, and - through wbase, as in the stack kernel's hit block; only where NODE asks for it - its index in tree[].  Pool indices
// are 64-bit throughout.
template <bool NODE>
__device__ __forceinline__ bool walk_wide(const TraceArgs &A, V3 p, Terminal &T)
{
    if (!inside(p, ld3(A.worldmin), ld3(A.worldmax))) return false;
    const int ci = chunk_index(A, p);
    const DevWide ch = A.wchunks[ci];
    const V3 clo = ld3(ch.bmin);
    if (!inside(p, clo, clo + A.chunksize)) return false;
    const int levels = (int)ch.levels;
    const int nw = wide_levels(levels);
    V3 lo = clo, lo1 = clo;                         // box after both comparisons of a wide node / after the first one
    float size = A.chunksize, size1 = size;
    uint64_t wn = ch.wide_off;                      // the wide node's index in the pool
    int r = levels - 2 * nw;                        // -pad
    uint32_t word, slot;
    for (int kk = 0;; ++kk) {
        uint32_t sx = 0u, sy = 0u, sz = 0u;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (r + j >= 0) {
                const float half = size * 0.5f;
                const V3 mid = lo + half;
                const bool gx = p.x >= mid.x, gy = p.y >= mid.y, gz = p.z >= mid.z;
                lo = lo + mk(gx ? 1.0f : 0.0f, gy ? 1.0f : 0.0f, gz ? 1.0f : 0.0f) * half;
                size = half;
                sx |= (uint32_t)gx << (1 - j); sy |= (uint32_t)gy << (1 - j); sz |= (uint32_t)gz << (1 - j);
            }
            if (j == 0) { lo1 = lo; size1 = size; }
        }
        slot = sx | (sy << 2) | (sz << 4);
        word = A.wide[wn * 64u + slot];
        if (node_type(word) != BRANCH || kk + 1 >= nw) break;
        wn = (uint64_t)ch.wide_off + (word & WIDE_PAYLOAD_MASK);    // (entries count wide nodes from the chunk's top one)
        r += 2;
    }
    T.type = node_type(word);
    if (T.type == BRANCH) return false;                             // a BRANCH below the last wide level: malformed (never built)
    const int plev = (int)wide_entry_level(word);     // the reference node's level
    uint32_t node = 0u;                                             // level 0 is the chunk's root
    if (plev == 0) { lo = clo; size = A.chunksize; }
    else {
        const uint32_t cidx = ((slot >> 1) & 1u) | ((slot >> 2) & 2u) | ((slot >> 3) & 4u);
        const uint32_t gidx = (slot & 1u) | ((slot >> 1) & 2u) | ((slot >> 2) & 4u);
        const bool child = plev == r + 1;                           // a child of the expanded node: the box after one comparison
        if (child) { lo = lo1; size = size1; }
        if (NODE) {
            const uint32_t *wb = A.wbase + wn * WIDE_BASE_WORDS;
            node = child ? wb[0] + cidx : wb[1 + cidx] + gidx;
        }
    }
    T.lo = lo; T.size = size; T.leaf_material = word & 0xFFFFu; T.chunk = (uint32_t)ci; T.node = node;
    T.cells = A.twig + (ch.twig_off + (word & WIDE_PAYLOAD_MASK)) * TWIG_WORDS;
    return true;
}

// One thread per point.  A.origins = the points, A.out = the records.
__global__ __launch_bounds__(256) void k_locate_literal(TraceArgs A, uint32_t see)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= A.n) return;
    const V3 p = ld3(A.origins + 3 * k);
    Terminal T;
    if (!walk_literal(A, p, T)) { store_miss(A.out, k, 0u); return; }
    locate_store(A.out, k, p, T, A.glsl != 0, see);
}

__global__ __launch_bounds__(256) void k_locate_wide(TraceArgs A, uint32_t see)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= A.n) return;
    const V3 p = ld3(A.origins + 3 * k);
    Terminal T;
    if (!walk_wide<true>(A, p, T)) { store_miss(A.out, k, 0u); return; }
    locate_store(A.out, k, p, T, A.glsl != 0, see);
}

} // namespace svo
