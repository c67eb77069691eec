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
// d1, d2 and the premises under which the rule holds are the host's (prepare_light below; the proof is in DESIGN.md 6t).  A
// brick counts as occupied whatever its cells hold.  tests/clearance_model.py is the same predicate in Python.
//
// Three kernels over the wide pool: k_clear_seed and k_clear_boxes give every reachable wide node its place (cell coordinates of
// its low corner, wide level, chunk) level by level - a wide node's index says nothing about where it sits -, k_clear_sweep decides
// every EMPTY terminal entry and writes WIDE_CLEAR_BIT.  All slots of one reference node get the same answer: a child-level
// terminal fills 8 slots, its first slot decides for all of them.
//
// Behind the sweep, k_clear_bricks decides one flag per brick (bit 15 of its bmat word, BMAT_CLEAR_BIT): every EMPTY
// cell of the brick is clear under the same rule with the cell in the place of C and with bricks seen cell by cell - occupied is
// every LEAF node and every occupied cell of every brick, the brick's own among them.  The stack kernel's hit block settles a
// shadow ray whose origin lies in an empty cell of such a brick without a step.  tests/brick_clearance_model.py is its model.
//
// Below the kernels, the host half: the pass (prepare_light), what drops it, the gate that lets a launch use it and the read-back of
// its counts.  DESIGN.md 6w has what the bits, the flags and "dark at birth" share.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "hip_own.h"
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
    // k_clear_bricks
    const uint64_t *mask;               // the mask pool: bit w of mask[b] = cell w of brick b is occupied
    uint16_t *bmat;                     // per brick: material | BMAT_CLEAR_BIT (0xFFFF carries no flag)
    unsigned long long *clear_bricks;   // count of bricks flagged (clear_nodes + 1)
    int32_t brick_premises;             // the premises of 6u hold: otherwise every flag is written 0
};

constexpr uint32_t CLEAR_NO_PLACE = 0xFFFFFFFFu;
constexpr int CLEAR_MAX_WIDE_LEVELS = (WIDE_MAX_LEVELS + 1) / 2;

// Slot `slot` of the wide node placed at `place` (ClearArgs::place) in chunk `ch`: c = the slot's low corner in the chunk's finest
// cells, sh = log2 of the slot's edge in those cells, above_root = a position of the virtual levels above the chunk root (not reachable)
struct ClearSlot { uint32_t c[3]; int sh; bool above_root; };
__device__ __forceinline__ ClearSlot clear_slot(const uint4 &place, const DevWide &ch, uint32_t slot)
{
    const int sh = 2 * (wide_levels((int)ch.levels) - 1 - (int)(place.w & 15u));
    const uint32_t x = place.x | ((slot & 3u) << sh), y = place.y | (((slot >> 2) & 3u) << sh), z = place.z | ((slot >> 4) << sh);
    return { { x, y, z }, sh, ((x | y | z) >> ch.levels) != 0u };
}

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
    if ((int)r + 1 >= wide_levels((int)ch.levels)) return;
    const uint64_t child = (uint64_t)ch.wide_off + (word & WIDE_PAYLOAD_MASK);
    if (child >= K.pool_nodes) return;
    const ClearSlot S = clear_slot(b, ch, (uint32_t)i & 63u);
    K.place[child] = make_uint4(S.c[0], S.c[1], S.c[2], b.w + 1u);      // (one wide level down, the same chunk)
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

// depth-first walk of chunk j's wide tree: does a LEAF or TWIG entry's box meet the region of C?  CELLS: a TWIG entry counts by its
// occupied cells, each a box of its own
template <bool CELLS>
__device__ bool clear_occupied(const ClearArgs &K, const ClearCell &C, int j, bool own)
{
    const DevWide ch = K.wchunks[j];
    const int levels = (int)ch.levels, nw = wide_levels(levels);
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
        const ClearSlot S = clear_slot(make_uint4(bx[k], by[k], bz[k], (uint32_t)k), ch, s);     // (word arrays, not a uint4 one: they stay in registers)
        if (S.above_root) continue;
        const uint64_t wn = (uint64_t)ch.wide_off + node[k];
        if (wn >= K.pool_nodes) return true;                            // (never built; counted as occupied)
        const uint32_t word = K.wide[wn * 64u + s];
        const uint32_t type = node_type(word);
        if (type == EMPTY) continue;
        // a BRANCH entry: the slot's box.  A terminal: the box of its reference node, which may span 8 slots (or all 64), tested whole in
        // each of them - the region tests are stated, and proven, for node boxes (the part of a node inside R2's shell is not split off)
        uint32_t span = 1u << S.sh;
        if (type != BRANCH) { const uint32_t lv = wide_entry_level(word); span = lv <= (uint32_t)levels ? 1u << (levels - lv) : span; }
        const double edge = res * (double)span;
        for (int a = 0; a < 3; ++a) { lo[a] = base[a] + (double)(S.c[a] & ~(span - 1u)) * res; hi[a] = lo[a] + edge; }
        if (!clear_meets(K, C, own, inner_lo, inner_hi, lo, hi)) continue;
        if constexpr (CELLS) {
            if (type == TWIG) {
                if (((S.c[0] | S.c[1] | S.c[2]) & (span - 1u)) != 0u) continue;   // (a node that fills several slots: its first one looks at the cells)
                unsigned long long m = K.mask[ch.twig_off + (word & WIDE_PAYLOAD_MASK)];
                const double leaf = edge * 0.25, blo[3] = { lo[0], lo[1], lo[2] };
                bool met = false;
                while (m != 0ull && !met) {
                    const uint32_t w = (uint32_t)__ffsll((long long)m) - 1u;
                    m &= m - 1ull;
                    lo[0] = blo[0] + leaf * (double)(w & 3u); lo[1] = blo[1] + leaf * (double)((w >> 2) & 3u); lo[2] = blo[2] + leaf * (double)(w >> 4);
                    for (int a = 0; a < 3; ++a) hi[a] = lo[a] + leaf;
                    met = clear_meets(K, C, own, inner_lo, inner_hi, lo, hi);
                }
                if (met) return true;
                continue;
            }
        }
        if (type != BRANCH || k + 1 >= nw) return true;
        ++k;
        node[k] = word & WIDE_PAYLOAD_MASK; cur[k] = 0u; bx[k] = S.c[0]; by[k] = S.c[1]; bz[k] = S.c[2];
    }
    return false;
}

// ... in any chunk: C's own first (R1 and R2), then every other one (R2)
template <bool CELLS>
__device__ bool clear_anywhere_occupied(const ClearArgs &K, const ClearCell &C, int own)
{
    bool met = clear_occupied<CELLS>(K, C, own, true);
    for (int j = 0; !met && j < K.n_chunks; ++j)
        if (j != own) met = clear_occupied<CELLS>(K, C, j, false);
    return met;
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
    const int own = (int)(b.w >> 4);
    const DevWide ch = K.wchunks[own];
    const int levels = (int)ch.levels;
    const uint32_t slot = (uint32_t)i & 63u;
    const ClearSlot S = clear_slot(b, ch, slot);
    if (S.above_root) return;                                           // not reachable: stays 0
    const int level = (int)wide_entry_level(word);
    if (level > levels) return;
    const bool child = levels - level == S.sh + 1;                      // a child of the expanded node (twice a slot's edge): 8 slots, the first decides
    if (child && (slot & 0x15u) != 0u) return;
    const uint32_t span = 1u << (levels - level);
    const double res = K.chunksize / (double)(1u << levels);
    ClearCell C;
    for (int a = 0; a < 3; ++a) { C.lo[a] = (double)ch.bmin[a] + (double)(S.c[a] & ~(span - 1u)) * res; C.hi[a] = C.lo[a] + (double)span * res; }
    bool clear = !clear_anywhere_occupied<false>(K, C, own);
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

// one wave per wide node: its TWIG entries one after the other, one lane per cell of the brick, a vote at the end
__global__ __launch_bounds__(256) void k_clear_bricks(ClearArgs K)
{
    const uint64_t wn = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (wn >= K.pool_nodes) return;
    const uint4 b = K.place[wn];
    if (b.w == CLEAR_NO_PLACE) return;
    const uint32_t lane = threadIdx.x & 63u;
    const int own = (int)(b.w >> 4);
    const DevWide ch = K.wchunks[own];
    const int levels = (int)ch.levels;
    const double res = K.chunksize / (double)(1u << levels);
    unsigned long long twigs = __ballot(node_type(K.wide[wn * 64u + lane]) == TWIG);
    unsigned flagged = 0;
    while (twigs != 0ull) {
        const uint32_t slot = (uint32_t)__ffsll((long long)twigs) - 1u;
        twigs &= twigs - 1ull;
        const uint32_t word = K.wide[wn * 64u + slot];
        const ClearSlot S = clear_slot(b, ch, slot);
        if (S.above_root) continue;
        const int level = (int)wide_entry_level(word);
        if (level > levels) continue;
        const uint32_t span = 1u << (levels - level);
        if (((S.c[0] | S.c[1] | S.c[2]) & (span - 1u)) != 0u) continue;    // a node that fills 8 (or all 64) slots: decided in its first
        const uint64_t brick = ch.twig_off + (word & WIDE_PAYLOAD_MASK);
        bool clear = K.brick_premises != 0;
        if (clear && ((K.mask[brick] >> lane) & 1ull) == 0ull) {            // an EMPTY cell: the rule of the sweep, the cell in the place of C
            const double leaf = res * (double)span * 0.25;
            ClearCell C;
            const uint32_t w3[3] = { lane & 3u, (lane >> 2) & 3u, lane >> 4 };
            for (int a = 0; a < 3; ++a) { C.lo[a] = (double)ch.bmin[a] + (double)S.c[a] * res + leaf * (double)w3[a]; C.hi[a] = C.lo[a] + leaf; }
            clear = !clear_anywhere_occupied<true>(K, C, own);
        }
        const bool all_clear = __ballot(!clear) == 0ull;
        if (lane == 0u) {
            const uint32_t m = K.bmat[brick];
            if (m != BMAT_SEVERAL) {
                K.bmat[brick] = (uint16_t)((m & ~BMAT_CLEAR_BIT) | (all_clear ? BMAT_CLEAR_BIT : 0u));
                flagged += all_clear;
            }
        }
    }
    if (flagged) atomicAdd(K.clear_bricks, (unsigned long long)flagged);
}

// ---- the host half ------------------------------------------------------------------------------------------------------------------

// The rule's premises: every component of the shadow direction is 0 or at least CLEAR_S_MIN in magnitude (a smaller one
// lets a ray graze a chunk face for a long way: the chunk march then resumes far behind the tree march's last sample), the world's
// largest coordinate has a float spacing u of at most eps / 2, and eps is a power of two.
constexpr double CLEAR_S_MIN = 1.0 / 64.0;
// The sweep looks at every chunk's root per EMPTY entry: its cost grows with entries x chunks.  The 4x1x4 depth-12 world (163 M entries,
// 16 chunks: 2.6e9) takes 0.86 s (profiles/light_clearance_ab.txt); a launch prepares a world on its own up to four times that product,
// a few seconds by proportion - and seventeen times that with the brick flags behind it (k_clear_bricks: 14.9 s on that world, 0.8 s at
// depth 10; DESIGN.md 6u "Not done").  Larger worlds - the 10x1x10 one of scripts/bigworld_check.py is at 1.3e11 - are prepared on request only.
constexpr double CLEAR_AUTO_WORK = 1.0e10;

// u: the float spacing at the world's largest coordinate
inline float clear_spacing(const svo_world &w)
{
    const int dims[3] = { w.width, w.height, w.depth };
    float m = 1.0f;
    for (int a = 0; a < 3; ++a)
        for (int k = 0; k < 2; ++k) m = std::max(m, std::fabs((float)(w.chunkcoordmin[a] + k * dims[a]) * (float)w.chunksize));
    return std::nextafter(m, INFINITY) - m;
}
inline bool eps_is_pow2(float eps)
{
    uint32_t b;
    std::memcpy(&b, &eps, sizeof b);
    return (b & 0x807FFFFFu) == 0u && b >= 0x00800000u && b < 0x7F800000u;
}

// Every change to the pools drops the bits - a rebuilt chunk has none, and those of the other chunks were decided against matter that
// may have changed - until svo_world_prepare_light is called again
inline void drop_clearance(svo_world &w)
{
    LightClearance &c = w.hbm->clear;
    if (c.place.p) { (void)hipDeviceSynchronize(); c.place = Pooled<uint4>(); }
    c.state = ClearState::DROPPED;                                      // (the flags in bmat stay and are ignored)
}

// The bits for shadow direction `sdir`, issued on `s` behind every launch of the world in flight (one of them may be reading the
// bits of another light); launches that use them wait for `built`.  light_gate.h says where each way out leaves the state.
inline int prepare_light(svo_world &w, const float sdir[3], hipStream_t s)
{
    Hbm &d = *w.hbm;
    LightClearance &c = d.clear;
    if (c.state == ClearState::NODES || c.state == ClearState::BRICKS) c.state = ClearState::UNUSED;
    if (!w.wide_ok || w.wide_pool_len == 0) return SVO_OK;              // the literal kernel marches this world: nothing reads the bits
    HIP_TRY(hipSetDevice(w.device));
    bool premises = true;
    for (int a = 0; a < 3; ++a) premises &= std::isfinite(sdir[a]) && (sdir[a] == 0.0f || std::fabs((double)sdir[a]) >= CLEAR_S_MIN);
    std::memcpy(c.sdir, sdir, sizeof c.sdir);
    c.state = ClearState::UNUSED;
    if (!premises || !w.exact_geometry) return SVO_OK;                  // prepared, and never used
    c.state = ClearState::DROPPED;                                      // (until everything below is issued)
    const uint64_t nodes = w.wide_pool_len;
    if (c.place.bytes < nodes * sizeof(uint4)) {
        if (c.place.p) HIP_TRY(hipDeviceSynchronize());
        if (c.place.alloc(nodes, w.device) != hipSuccess) { set_error("svo_world_prepare_light: hipMalloc failed"); return SVO_ERR_OUT_OF_MEMORY; }
    }
    if (const int rc = c.count.reserve(2, false, nullptr)) return rc;
    for (Event &e : d.work_done) if (e.e) if (const int rc = e.wait(s)) return rc;
    if (c.built.e) if (const int rc = c.built.wait(s)) return rc;
    const double u = (double)clear_spacing(w);
    // the brick flags ask more of the world: no negative coordinate and no voxel below u, so that a sample's cell
    // contains it exactly (exact_geometry has the power-of-two chunk size); where that fails every flag is written 0
    bool bricks = true;
    for (int a = 0; a < 3; ++a) bricks &= w.chunkcoordmin[a] >= 0;
    for (const ChunkPools &p : w.chunks) bricks &= std::ldexp((double)w.chunksize, -(int)p.depth) >= u;
    const ClearArgs K = {
        d.wchunks.p, d.wide.p, c.place.p, nodes, (int32_t)w.chunks.size(), (double)w.chunksize,
        { (double)sdir[0], (double)sdir[1], (double)sdir[2] },
        4.0 * u, (8.0 / CLEAR_S_MIN + 6.0 + 4.0 * (double)(w.width + w.height + w.depth + 2)) * u,      // d1, d2
        c.count.p, d.mask.p, d.bmat.p, c.count.p + 1, bricks ? 1 : 0,
    };
    HIP_TRY(hipMemsetAsync(c.place.p, 0xFF, nodes * sizeof(uint4), s));
    HIP_TRY(hipMemsetAsync(c.count.p, 0, 2 * sizeof(unsigned long long), s));
    const char *who = "svo_world_prepare_light";
    const int64_t entries = (int64_t)nodes * 64;
    int rc = launch_per_element(who, K.n_chunks, s, k_clear_seed, K);
    for (int r = 0; rc == SVO_OK && r + 1 < wide_levels(w.max_levels); ++r) rc = launch_per_element(who, entries, s, k_clear_boxes, K, (uint32_t)r);
    if (rc == SVO_OK) rc = launch_per_element(who, entries, s, k_clear_sweep, K);
    if (rc == SVO_OK) rc = launch_per_element(who, entries, s, k_clear_bricks, K);
    if (rc == SVO_OK) rc = c.built.record(s);
    if (rc == SVO_OK) c.state = bricks ? ClearState::BRICKS : ClearState::NODES;
    return rc;
}

// TraceArgs::light_clear of a stack-kernel launch (light_gate.h decides): the world's first eligible launch after its
// upload prepares the bits for its own light, a launch that uses prepared bits waits for the pass
inline int gate_light_clearance(svo_world &w, const svo_trace_params *prm, TraceArgs &A, uint32_t see, hipStream_t s)
{
    A.light_clear = 0;
    LightClearance &c = w.hbm->clear;
    // camera frames of the CPU march with shadow rays and nothing that looks at a ray's later steps (tile costs), ends it (segments) or
    // marches another world (the see-through view)
    const bool eligible = A.shadow && A.from_camera && !A.tmax && !see && !A.glsl && !A.tile_cost;
    // dark at birth's own premises.  Exact geometry has the power-of-two chunk and voxel size (the stack kernel demands it anyway); a finite
    // direction: fl(s * 0) = 0, the march's first sample is the origin; no negative corner: World::index puts a point at or just above a
    // negative multiple of the chunk size in the chunk below, and the reference's march then misses the brick
    bool dark = w.exact_geometry;
    for (int a = 0; a < 3; ++a) dark &= std::isfinite(A.sdir[a]) && w.chunkcoordmin[a] >= 0;
    LightGateIn g = { eligible, prm ? prm->shadow : 0, c.state, (double)w.wide_pool_len * 64.0 * (double)w.chunks.size() <= CLEAR_AUTO_WORK,
                      std::memcmp(c.sdir, A.sdir, sizeof c.sdir) == 0, eps_is_pow2(A.eps), A.eps >= 2.0f * clear_spacing(w), dark };
    LightGateOut o = light_gate(g);
    if (o.prepare) {
        if (const int rc = prepare_light(w, A.sdir, s)) return rc;
        g.state = c.state; g.same_dir = std::memcmp(c.sdir, A.sdir, sizeof c.sdir) == 0;
        o = light_gate(g);
    }
    if (o.bits & (LIGHT_CLEAR_NODES | LIGHT_CLEAR_BRICKS)) if (const int rc = c.built.wait(s)) return rc;
    A.light_clear = o.bits;
    return SVO_OK;
}

// count[which] of the last pass, once `s` and the pass - which may have been issued on another stream - are through
inline int read_clear_count(const svo_world &w, hipStream_t s, int which, uint64_t *out)
{
    const LightClearance &c = w.hbm->clear;
    HIP_TRY(hipSetDevice(w.device));
    HIP_TRY(hipStreamSynchronize(s));
    if (c.built.e) HIP_TRY(hipEventSynchronize(c.built.e));
    unsigned long long v = 0;
    HIP_TRY(hipMemcpy(&v, c.count.p + which, sizeof v, hipMemcpyDeviceToHost));
    *out = v;
    return SVO_OK;
}

} // namespace svo
