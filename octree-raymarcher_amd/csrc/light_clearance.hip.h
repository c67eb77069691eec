// light_clearance.hip.h — the "clear way to the light" bit of EMPTY wide entries (svo_world_prepare_light).
//
// A shadow ray carries one bit into its record: whether some later sample lands in an occupied cell.  An EMPTY reference node C
// is CLEAR for a light direction when no sample the reference's march can take after one located in C can be located in a LEAF or
// TWIG node; a shadow ray of the stack kernel that locates a clear cell retires at once (step_asm_body.inc, label 4).  Whether C is
// clear depends only on the world and the direction, so it is decided once per world and light, by two sweeps per EMPTY node:
//     R1  C's own chunk, the samples of the treemarch invocation that located C: the exact octant of C (q >= lo where s > 0,
//         q < hi where s < 0, lo <= q < hi where s == 0; cells are half open, so every test is strict) intersected with the prism
//         C + {lambda s, lambda >= 0} grown by d1;
//     R2  every chunk, the samples of all later invocations: octant and prism grown by d2, boxes closed, minus the part of C's own
//         chunk that lies deeper than d2 inside it (a later invocation re-enters that chunk only at the face it left by).
// d1, d2 and the premises under which the rule holds are the host's (device.hip prepare_light; the proof is in DESIGN.md 6t).  A
// brick counts as occupied whatever its cells hold.  tests/clearance_model.py is the same predicate in Python.
//
// Three kernels over the wide pool: k_clear_seed and k_clear_boxes give every reachable wide node its place (cell coordinates of
// its low corner, wide level, chunk) level by level - a wide node's index says nothing about where it sits -, k_clear_sweep decides
// every EMPTY terminal entry and writes WIDE_CLEAR_BIT.  All slots of one reference node get the same answer: a child-level
// terminal fills 8 slots, its first slot decides for all of them.
#pragma once
#include <hip/hip_runtime.h>

#include "wide_tree.hip.h"

namespace svo {

struct ClearArgs {
    const DevWide *wchunks;
    uint32_t *wide;
    uint4 *place;               // per wide node of the pool: x, y, z = low corner in the chunk's finest cells, w = chunk << 4 | wide level; w = ~0: not reachable
    uint64_t pool_nodes;
    int32_t n_chunks;
    double chunksize;
    double s[3];                // the shadow direction, float32 values
    double d1, d2;
    unsigned long long *clear_nodes;    // count of reference nodes found clear
};

constexpr uint32_t CLEAR_NO_PLACE = 0xFFFFFFFFu;
constexpr int CLEAR_MAX_WIDE_LEVELS = (WIDE_MAX_LEVELS + 1) / 2;

__global__ __launch_bounds__(256) void k_clear_seed(ClearArgs K)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K.n_chunks) return;
    const uint32_t top = K.wchunks[i].wide_off;
    if (top < K.pool_nodes) K.place[top] = make_uint4(0u, 0u, 0u, (uint32_t)i << 4);
}

// round r: every wide node of wide level r places the wide nodes its BRANCH entries point at
__global__ __launch_bounds__(256) void k_clear_boxes(ClearArgs K, uint32_t r)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= K.pool_nodes * 64u) return;
    const uint4 b = K.place[i >> 6];
    if (b.w == CLEAR_NO_PLACE || (b.w & 15u) != r) return;
    const uint32_t word = K.wide[i];
    if (node_type(word) != BRANCH) return;
    const DevWide ch = K.wchunks[b.w >> 4];
    const int levels = (int)ch.levels, nw = levels ? (levels + 1) >> 1 : 1;
    if ((int)r + 1 >= nw) return;
    const int sh = 2 * (nw - 1 - (int)r);
    const uint32_t slot = (uint32_t)i & 63u;
    const uint64_t child = (uint64_t)ch.wide_off + (word & WIDE_PAYLOAD_MASK);
    if (child >= K.pool_nodes) return;
    K.place[child] = make_uint4(b.x | ((slot & 3u) << sh), b.y | (((slot >> 2) & 3u) << sh), b.z | ((slot >> 4) << sh), (b.w & ~15u) | (r + 1u));
}

struct ClearCell { double lo[3], hi[3]; };

// does the closed box [lo, hi] meet C + {lambda s, lambda >= 0} grown by d?  One slab test of the ray {lambda s} against
// [lo - C.hi - d, hi - C.lo + d]; `slack` covers the quotients' rounding
__device__ __forceinline__ bool clear_prism(const ClearArgs &K, const ClearCell &C, const double lo[3], const double hi[3], double d)
{
    double l0 = 0.0, l1 = __builtin_huge_val();
    const double slack = 1e-9;
    for (int a = 0; a < 3; ++a) {
        const double blo = lo[a] - C.hi[a] - d, bhi = hi[a] - C.lo[a] + d, s = K.s[a];
        if (s == 0.0) { if (blo > 0.0 || bhi < 0.0) return false; }
        else {
            double t0 = blo / s, t1 = bhi / s;
            if (t0 > t1) { const double t = t0; t0 = t1; t1 = t; }
            l0 = fmax(l0, t0 - slack); l1 = fmin(l1, t1 + slack);
        }
    }
    return l0 <= l1;
}

__device__ __forceinline__ bool clear_meets(const ClearArgs &K, const ClearCell &C, bool own, const double inner_lo[3], const double inner_hi[3],
                                            const double lo[3], const double hi[3])
{
    if (own) {                                              // R1
        bool oct = true;
        for (int a = 0; a < 3; ++a) {
            if (K.s[a] >= 0.0 && !(hi[a] > C.lo[a])) oct = false;
            if (K.s[a] <= 0.0 && !(lo[a] < C.hi[a])) oct = false;
        }
        if (oct && clear_prism(K, C, lo, hi, K.d1)) return true;
        bool inner = true;                                  // R2 leaves out what lies deep inside C's chunk
        for (int a = 0; a < 3; ++a) inner &= lo[a] >= inner_lo[a] && hi[a] <= inner_hi[a];
        if (inner) return false;
    }
    for (int a = 0; a < 3; ++a) {                           // R2 (a zero component never moves the sample: no drift on that axis)
        const double g = K.s[a] == 0.0 ? 0.0 : K.d2;
        if (K.s[a] >= 0.0 && !(hi[a] >= C.lo[a] - g)) return false;
        if (K.s[a] <= 0.0 && !(lo[a] <= C.hi[a] + g)) return false;
    }
    return clear_prism(K, C, lo, hi, K.d2);
}

// depth-first walk of chunk j's wide tree: does a LEAF or TWIG entry's box meet the region of C?
__device__ bool clear_occupied(const ClearArgs &K, const ClearCell &C, int j, bool own)
{
    const DevWide ch = K.wchunks[j];
    const int levels = (int)ch.levels, nw = levels ? (levels + 1) >> 1 : 1;
    const double res = K.chunksize / (double)(1u << levels);
    const double base[3] = { (double)ch.bmin[0], (double)ch.bmin[1], (double)ch.bmin[2] };
    double inner_lo[3], inner_hi[3], lo[3], hi[3];
    for (int a = 0; a < 3; ++a) { inner_lo[a] = base[a] + K.d2; inner_hi[a] = base[a] + K.chunksize - K.d2; lo[a] = base[a]; hi[a] = base[a] + K.chunksize; }
    if (!clear_meets(K, C, own, inner_lo, inner_hi, lo, hi)) return false;
    uint32_t node[CLEAR_MAX_WIDE_LEVELS + 1], cur[CLEAR_MAX_WIDE_LEVELS + 1], bx[CLEAR_MAX_WIDE_LEVELS + 1], by[CLEAR_MAX_WIDE_LEVELS + 1], bz[CLEAR_MAX_WIDE_LEVELS + 1];
    int k = 0;
    node[0] = 0u; cur[0] = 0u; bx[0] = by[0] = bz[0] = 0u;
    while (k >= 0) {
        if (cur[k] >= 64u) { --k; continue; }
        const uint32_t s = cur[k]++;
        const int sh = 2 * (nw - 1 - k);
        const uint32_t c[3] = { bx[k] | ((s & 3u) << sh), by[k] | (((s >> 2) & 3u) << sh), bz[k] | ((s >> 4) << sh) };
        if (((c[0] | c[1] | c[2]) >> levels) != 0u) continue;           // a position of the virtual levels above the chunk root
        const uint64_t wn = (uint64_t)ch.wide_off + node[k];
        if (wn >= K.pool_nodes) return true;                            // (never built; counted as occupied)
        const uint32_t word = K.wide[wn * 64u + s];
        const uint32_t type = node_type(word);
        if (type == EMPTY) continue;
        // a BRANCH entry: the slot's box.  A terminal: the box of its reference node, which may span 8 slots (or all 64), tested whole in
        // each of them - the region tests are stated, and proven, for node boxes (the part of a node inside R2's shell is not split off)
        uint32_t span = 1u << sh;
        if (type != BRANCH) { const uint32_t lv = (word >> WIDE_LEVEL_SHIFT) & ((1u << WIDE_LEVEL_BITS) - 1u); span = lv <= (uint32_t)levels ? 1u << (levels - lv) : span; }
        const double edge = res * (double)span;
        for (int a = 0; a < 3; ++a) { lo[a] = base[a] + (double)(c[a] & ~(span - 1u)) * res; hi[a] = lo[a] + edge; }
        if (!clear_meets(K, C, own, inner_lo, inner_hi, lo, hi)) continue;
        if (type != BRANCH || k + 1 >= nw) return true;
        ++k;
        node[k] = word & WIDE_PAYLOAD_MASK; cur[k] = 0u; bx[k] = c[0]; by[k] = c[1]; bz[k] = c[2];
    }
    return false;
}

// one thread per wide entry of the pool
__global__ __launch_bounds__(256) void k_clear_sweep(ClearArgs K)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= K.pool_nodes * 64u) return;
    const uint4 b = K.place[i >> 6];
    if (b.w == CLEAR_NO_PLACE) return;
    const uint32_t word = K.wide[i];
    if (node_type(word) != EMPTY) return;
    const int own = (int)(b.w >> 4), k = (int)(b.w & 15u);
    const DevWide ch = K.wchunks[own];
    const int levels = (int)ch.levels, nw = levels ? (levels + 1) >> 1 : 1;
    const int sh = 2 * (nw - 1 - k);
    const uint32_t slot = (uint32_t)i & 63u;
    const uint32_t c[3] = { b.x | ((slot & 3u) << sh), b.y | (((slot >> 2) & 3u) << sh), b.z | ((slot >> 4) << sh) };
    if (((c[0] | c[1] | c[2]) >> levels) != 0u) return;                 // not reachable: stays 0
    const int level = (int)((word >> WIDE_LEVEL_SHIFT) & ((1u << WIDE_LEVEL_BITS) - 1u));
    if (level > levels) return;
    const bool child = level == 2 * k + 1 - (2 * nw - levels);          // a child of the expanded node: 8 slots, the first decides
    if (child && (slot & 0x15u) != 0u) return;
    const uint32_t span = 1u << (levels - level);
    const double res = K.chunksize / (double)(1u << levels);
    ClearCell C;
    for (int a = 0; a < 3; ++a) { C.lo[a] = (double)ch.bmin[a] + (double)(c[a] & ~(span - 1u)) * res; C.hi[a] = C.lo[a] + (double)span * res; }
    bool clear = !clear_occupied(K, C, own, true);
    for (int j = 0; clear && j < K.n_chunks; ++j)
        if (j != own) clear = !clear_occupied(K, C, j, false);
    const uint32_t out = clear ? (word | WIDE_CLEAR_BIT) : (word & ~WIDE_CLEAR_BIT);
    if (!child) K.wide[i] = out;
    else {
        uint32_t *node = K.wide + (i & ~(uint64_t)63u);
        for (uint32_t g = 0; g < 8u; ++g) node[slot | (g & 1u) | ((g & 2u) << 1) | ((g & 4u) << 2)] = out;
    }
    if (level == 0 && !child && slot != 0u) clear = false;              // (a chunk that is one EMPTY node fills all 64 slots: counted once)
    const unsigned long long voted = __ballot(clear);                   // (one atomic per wave)
    if (clear && (int)(threadIdx.x & 63u) == __ffsll((long long)voted) - 1) atomicAdd(K.clear_nodes, (unsigned long long)__popcll(voted));
}

} // namespace svo
