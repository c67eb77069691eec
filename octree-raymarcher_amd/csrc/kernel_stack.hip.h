// kernel_stack.hip.h — SVO_KERNEL_STACK: the CDNA4 fast path of the SVO march.
//
// Same results as kernel_literal.hip.h / src/Traverse.cpp, bit for bit, on worlds whose voxel
// corners are exact floats (svo_world_info.exact_geometry: power-of-two chunk edge, positions on
// the voxel lattice), reached differently:
//
//  * Persistent single-wave workgroups pull 8x8-pixel tiles (64 rays) from atomic cursors, one per screen region;
//    a wave starts in the region of its XCD (HW_REG_XCC_ID), so each XCD's L2 serves one part of the world, and
//    moves on to the other regions when its own is used up.  One launch may carry several frames (cameras): a
//    region's cursor then runs through its tiles frame after frame, and the waves drain once per launch.
//    When >= REFILL lanes of the wave have retired (64-bit __ballot), the dead lanes are handed
//    the next ray ids by prefix rank (mbcnt) — the wave re-compacts instead of idling on its
//    slowest ray.  A primary hit turns its lane into the shadow ray in place.
//  * The three nested loops of chunkmarch/treemarch/twigmarch are flattened into one loop whose
//    body every lane runs in one of three modes, sharing one escape-distance evaluation.
//  * Descent: the position inside the chunk is reduced to integer cell coordinates at level
//    depth-2 (one exact compare-and-fix per axis reproduces the reference's float `p >= mid`
//    tests) and looked up in the chunk's WIDE tree (wide_tree.hip.h: built on upload from tree[], 64 entries per node
//    = two reference levels per dependent load).  The wide node of every wide level of the current path is cached in
//    a per-lane LDS column ([level][lane]: bank = lane, conflict-free); the next step restarts at the deepest level
//    whose coordinate prefix is unchanged - and keeps the cache across rays of the same chunk (a shadow ray starts
//    where its primary ray ended).  ONE dependent load per lane and step: a lane whose entry is a BRANCH pushes the child
//    onto its cache and sits the step out (step_asm.hip.h) - the wave never waits for a second level, unless a quarter of
//    its tree lanes need one.
//  * Bricks are tested against a 64-bit occupancy mask held in registers (one 8-byte load per
//    brick visit); the 128-byte brick line is touched only to fetch the hit material.
//  * Ray generation (camera ray, 1/dir, world-entry distance: ~10 IEEE divisions) is done once per
//    tile by all 64 lanes together and parked in LDS; a refill is then 11 LDS reads per lane, so
//    waves can refill after only a few retirements.
//  * The rare, expensive blocks (chunk step, G-buffer resolve of a primary hit) run only when a
//    ballot shows enough lanes waiting for them (or nothing else is runnable).
//  * Creeping rays - pinned on a lattice plane, advancing by EPS alone for thousands of steps, alone or nested over a
//    brick whose marches are bound to miss - are taken in closed form by a vote-gated block (same t, same counters).
//  * The step runs four times per pass of the outer loop while >= 8 lanes are marching (decided before the loop: nothing
//    is voted on between the steps, the loop control is scalar), and keeps repeating once the tile cursors are dry and
//    every live lane is marching: the refill / vote / block checks around it are a quarter of an iteration, and a
//    launch's last waves are alone on their SIMD, bound by their own instruction stream.  Scalar instructions and
//    branches cost a SIMD what vector instructions do (scripts/microbench/valu_issue.hip): the step avoids them
//    where a select or an unconditional LDS read does the same.
//  * The step itself is one hand-scheduled asm statement that runs the steps of a pass (step_asm.hip.h; the C++ step of
//    step_cxx.hip.h is the readable statement of the same algorithm, built with -DSVO_CXX_STEP): what a wave-step costs is its chain of
//    dependent loads and the instructions between them, and that chain is what the statement is arranged around.
//  * The chunk step is a second hand-scheduled statement (chunk_step_asm.hip.h; its C++ twin, chunk_step_cxx.hip.h, is built with -DSVO_CXX_STEP as well).
//  * Lane state is kept small (re-basing points pw/pt and the node box are recomputed with the
//    reference's own expressions instead of being held): 80 VGPRs, 6 waves per SIMD, no spill inside the pass loop.
//  * The chunk table of worlds of up to 64 chunks sits in LDS: the chunk step waits for no global load.
//  * Instantiations (round 4): BIG - 64-bit wide-tree and mask addresses for worlds beyond 4 GiB of wide nodes / 2^29 bricks, a
//    126-chunk LDS table; GLSL - the march of shaders/Chunkmarch.glsl (svo_trace_params.semantics): guarded escape distance, LEAF
//    hits at t, tnear > 0 at the world entry, no containment re-check.  The asm statement (step_asm_body.inc) and the creep block
//    (creep_block.inc) are shared text.
//
// All float arithmetic that decides t is evaluated exactly as in the reference; only loads and
// integer bookkeeping differ.  Divisions by powers of two (chunk edge, node edge) are written as
// multiplications by the exact reciprocal, which is bit-identical.
#pragma once
#include "march.hip.h"
#include "step_asm.hip.h"
#include "chunk_step_asm.hip.h"

namespace svo {

constexpr int CW_ESCAPE_PENDING = (int)0x80000000;    // bit of the lane's chunk-step counter: tw still lacks the escape out of the chunk just left
enum : int { M_DONE = 0, M_WORLD = 1, M_HIT = 2, M_TREE = 3, M_TWIG = 4 };     // (step_asm.hip.h: marching = mode > 2)

// Vote thresholds of the rare blocks (DESIGN.md §6 swept them)
constexpr int VOTE_WORLD = 8;           // lanes waiting for a chunk step that make the wave run it
constexpr int VOTE_HIT = 16;            // primary hits waiting for their G-buffer record
constexpr int VOTE_BUSY = 24;           // fewer marching lanes than this: serve the waiting ones regardless
// Creeping rays (see the creep block in the kernel): a lane whose last CREEP_SERIOUS steps all advanced by ~EPS makes
// the wave run the creep block; CREEP_LANES creeping lanes do so at once.
constexpr int CREEP_SERIOUS = 6;
constexpr int CREEP_LANES = 8;
// Block placement: a taken branch costs a shared SIMD about three vector instructions' time, a not-taken one about one
// (scripts/microbench/valu_issue.hip) - rare blocks go out of line so that the common path falls through.
#define SVO_LIKELY(x) __builtin_expect(!!(x), 1)
#define SVO_UNLIKELY(x) __builtin_expect(!!(x), 0)
// the step runs up to 1 + STEP_EXTRA times per pass of the outer loop while at least STEP_LANES lanes are marching
constexpr int STEP_EXTRA = 4;
constexpr int STEP_LANES = 8;
// steps per statement while the inner repeat lasts (the drain of a launch: the wave is alone on its SIMD, every instruction of the
// loop control around the statement costs it ~5 cycles)
constexpr int DRAIN_STEPS = 8;          // (round 4: 8 instead of 4 - one frame 1.62 - 1.63 ms against 1.655 - 1.659, the serialized 16-frame launch 8.79 against 8.91 - 8.99 ms; 16: the same as 8, 2: as 4)
// when a wave skips the bricks whose march is bound to miss (step_asm_body.inc, "sure"): the test is ~95 instructions for every wave-step
// in which some lane enters a brick, so a wave of the bulk would pay more than its lanes win; a draining wave's instructions are its
// critical path and the test runs while the brick's mask is on its way
#ifndef SVO_SURE_MISS_WHEN
#define SVO_SURE_MISS_WHEN __builtin_amdgcn_readfirstlane(more ? 0 : 1)
#endif

// 1/x for x an exact power of two (normal range): exponent negation, no division sequence.
__device__ __forceinline__ float recip_pow2(float x) { return __uint_as_float(0x7F000000u - __float_as_uint(x)); }

// A wave vote.  HIP's __ballot(int) takes a lane value: a bool goes through v_cndmask 0/1 and a second compare wherever the
// optimiser does not see through it; the builtin takes the compare's own mask.
__device__ __forceinline__ unsigned long long vote(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// ... and the number of its lanes as a 32-bit scalar.  __popcll is 64 bits wide and the optimiser, knowing that, widens every
// comparison of the count back to 64 bits - a v_cmp_*_u64 on an SGPR pair with moves around it, the SALU has no ordered 64-bit
// compare.  Behind the (empty) statement the count is an int in an SGPR and a comparison of it one s_cmp.
__device__ __forceinline__ int vote_count(unsigned long long m)
{
    int n = (int)__popcll(m);
    asm("" : "+s"(n));
    return n;
}

// What the chunk step needs of the chunk grid, eight words that k_trace_stack stages in LDS once per wave beside the chunk
// table: read there, the block waits for an LDS read where it waited for scalar loads of ten kernel arguments (a trip to the
// scalar cache in six of ten passes; holding them in SGPRs across the march loop is what the kernel has no room for).
struct ChunkGrid {
    float inv;                  // 1 / chunksize, exact: the edge is a power of two
    int32_t off[3];             // cbase - ccm: grid cell of a chunk coordinate = coordinate + off, within one period of the grid
    int32_t dimw, dimh, dimd;
    uint32_t table_in_lds;      // the chunk table lies in LDS as well (at most CHUNK_TAB chunks)
};
static_assert(sizeof(ChunkGrid) == 32, "two 16-byte LDS reads");

// m mod dim for -dim <= m < 2 dim (cbase - 1 <= m <= cbase + dim with 0 <= cbase < dim, below): of m, m + dim and m - dim the one
// in [0, dim) is the smallest as an unsigned number, the others are negative (huge) or larger by dim - add, subtract, v_min3_u32
// where "subtract dim if >= dim, then add dim if negative" took six instructions per axis.
__device__ __forceinline__ int wrap_once(int m, int dim)
{
    const uint32_t a = (uint32_t)m, b = (uint32_t)(m + dim), c = (uint32_t)(m - dim);
    return (int)min(min(a, b), c);
}

// World::index_float(p) for a power-of-two chunk edge (src/World.cpp:288-293,323-332), as the grid cell (mx, my, mz):
// p / chunksize == p * inv (exact), and positive_mod() of a coordinate that lies within one grid
// period of the grid's first chunk is a conditional add/subtract.  Only for p inside the world box.
__device__ __forceinline__ void chunk_cell_pow2(const ChunkGrid &G, V3 p, int &mx, int &my, int &mz)
{
    float qx = p.x * G.inv, qy = p.y * G.inv, qz = p.z * G.inv;
    if (qx < 0.0f) qx -= 1.0f;
    if (qy < 0.0f) qy -= 1.0f;
    if (qz < 0.0f) qz -= 1.0f;
    const int ix = (int)qx, iy = (int)qy, iz = (int)qz;
    // p lies inside the world box (the caller's isInsideCube test, src/Traverse.cpp:145): wlo <= p <= whi with
    // wlo = ccm * chunksize and whi = (ccm + dims) * chunksize exactly, so ccm - 1 <= i <= ccm + dims per axis (the - 1:
    // index_float sends an exact negative multiple one chunk down) - within one grid period, no general modulo needed
    // (cbase + (i - ccm) == i + (cbase - ccm) in 32-bit arithmetic)
    mx = wrap_once(ix + G.off[0], G.dimw); my = wrap_once(iy + G.off[1], G.dimh); mz = wrap_once(iz + G.off[2], G.dimd);
}
// World::index (src/World.cpp:288-293) of the grid cell, (my * dimd + mz) * dimw + mx.  The stack kernel marches worlds of fewer
// than 2^24 chunks (device.hip, pick_kernel: larger ones go to the literal kernel): 0 <= mx < dimw, my < dimh, mz < dimd, every
// dimension and the partial sum my * dimd + mz < dimh * dimd are then below 2^24 and both products exact as 24-bit ones
// (v_mul_u32_u24 / v_mad_u32_u24, full rate, where v_mul_lo_u32 runs at a quarter).
// (as a statement: the optimiser turns the inner __umul24, of which the outer one needs 24 bits only, back into a 32-bit multiply)
__device__ __forceinline__ uint32_t mad_u24(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ int chunk_index_u24(const ChunkGrid &G, int mx, int my, int mz)
{
    return (int)mad_u24(mad_u24((uint32_t)my, (uint32_t)G.dimd, (uint32_t)mz), (uint32_t)G.dimw, (uint32_t)mx);
}

// cubeNormal (shaders/Chunkmarch.glsl:128-136) for a cube whose half edge is a power of two:
// p / d == p * (1/d) exactly, and normalize() of a vector of small integers multiplies by
// 1/sqrt(1|2|3), whose correctly rounded values are constants.
__device__ __forceinline__ V3 cube_normal_pow2(V3 s, V3 lo, float size, float eps)
{
    const V3 hi = lo + size;
    const V3 c = (lo + hi) * 0.5f;
    const V3 p = s - c;
    const float d = fabsf(lo.x - hi.x) * 0.5f;                 // same on every axis: a cube
    const float invd = recip_pow2(d);                           // power of two: exact
    const float b = 1.0f + eps;
    const float ix = (float)(int)((p.x * invd) * b), iy = (float)(int)((p.y * invd) * b), iz = (float)(int)((p.z * invd) * b);
    const float dot = ix * ix + iy * iy + iz * iz;
    float inv;
    if (dot == 1.0f) inv = 1.0f;
    else if (dot == 2.0f) inv = __uint_as_float(0x3F3504F3u);  // 1.0f / sqrtf(2.0f)
    else if (dot == 3.0f) inv = __uint_as_float(0x3F13CD3Au);  // 1.0f / sqrtf(3.0f)
    else inv = 1.0f / sqrtf(dot);                               // 0 -> inf -> NaN normal, as in the reference
    return mk(ix * inv, iy * inv, iz * inv);
}

// Octree::branch (src/Octree.cpp:55-58) of the cell (ux, uy, uz) at the level whose selector bit is `sh`.
__device__ __forceinline__ uint32_t child_slot(int ux, int uy, int uz, int sh)
{
    const uint32_t bx = __builtin_amdgcn_ubfe((uint32_t)ux, (uint32_t)sh, 1u);
    const uint32_t by = __builtin_amdgcn_ubfe((uint32_t)uy, (uint32_t)sh, 1u);
    const uint32_t bz = __builtin_amdgcn_ubfe((uint32_t)uz, (uint32_t)sh, 1u);
    return ((bz << 1) + by) * 2u + bx;
}
// node word at byte offset `boff` of the tree pool: scalar base + zero-extended 32-bit vector offset (one VGPR of address
// instead of a 64-bit pointer per lane; pools of 4 GiB and more are marched by the BIG instantiation, which addresses with 64 bits)
__device__ __forceinline__ uint32_t ld_node(const uint32_t *pool, uint32_t boff)
{
    return *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(pool) + (size_t)boff);
}
// entry of a wide node (wide_tree.hip.h) for the cell (ux, uy, uz): its two coordinate bits at `sh` per axis, x lowest
constexpr uint32_t WIDE_PAYLOAD = (1u << 25) - 1u;
__device__ __forceinline__ uint32_t wide_slot(int ux, int uy, int uz, int sh)
{
    const uint32_t bx = __builtin_amdgcn_ubfe((uint32_t)ux, (uint32_t)sh, 2u);
    const uint32_t by = __builtin_amdgcn_ubfe((uint32_t)uy, (uint32_t)sh, 2u);
    const uint32_t bz = __builtin_amdgcn_ubfe((uint32_t)uz, (uint32_t)sh, 2u);
    return (bz << 4) | (by << 2) | bx;
}
// type == BRANCH (binary 10 in the top bits) as one signed comparison
__device__ __forceinline__ bool is_branch(uint32_t word) { return (int32_t)word < (int32_t)0xC0000000; }

// The launch arguments as they lie in the kernarg segment, behind a barrier the optimiser cannot see through: a rare
// block that reads its arguments through this re-loads them where it runs, instead of pinning ~60 SGPRs (camera, world
// grid) across the march loop, which spilled into VGPR lanes (v_readlane in the hot path).  What the loads compile to, at every
// call site of this kernel (the refill's tile order pointer, tile generation, note_tile_cost): VECTOR loads of the uniform address,
// scalar base plus a zero lane offset (global_load_dword(x2/x4) v, vzero, s[..] offset:field), not s_load - the copy through memcpy
// loses the constant address space - each group waited for (s_waitcnt vmcnt) before the next is issued, and whatever is derived
// from the values is computed per lane.  A few hundred cycles per tile of 64 rays; tile generation is 2.8 % of the kernel's
// instructions.  Reading the fields through an address_space(4) pointer gives s_load and costs the march loop ten more spilled
// VGPRs, some inside the chunk step (profiles/blocks_diet_ab.txt): left as it is.
__device__ __forceinline__ TraceArgs args_reloaded()
{
    auto p = __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    TraceArgs T;
    __builtin_memcpy(&T, p, sizeof T);              // only the fields the caller uses survive
    return T;
}
// camera f of the launch, read where it is needed at a uniform offset (vector loads in tile generation, see above)
__device__ __forceinline__ FrameCam camera_reloaded(int f)
{
    auto p = __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    FrameCam c;
    __builtin_memcpy(&c, (decltype(p))((const char __attribute__((address_space(4))) *)p + __builtin_offsetof(TraceArgs, cams) + (size_t)f * sizeof(FrameCam)), sizeof c);
    return c;
}

// How far along the ray a + b*s (s >= 0) can brick marches go before one of them might see an occupied cell?
// Asked for a run of tree steps over one TWIG node whose start points p_j = a + b*s_j all lie ON the brick's lower
// face of axis k (p_j.k == bmin.k) with b.k < 0; every twigmarch(p_j, b, brick) (src/Traverse.cpp:50-72) then
//  * only sees cells with coordinate 0 on axis k: p.k = p_j.k + b.k*t <= bmin.k for t >= 0, so p is in that layer or
//    outside the brick (the march returns false);
//  * takes pinned steps only, t += EPS (see the creep block), and ends once |b.k|*t exceeds half an ulp of bmin.k;
//  * moves forward along the ray: on the other two axes the brick's corner is at least a brick edge away from 0
//    (checked), so p - bmin is exact (Sterbenz), the truncated cell index is the cell p really lies in and no escape
//    distance is negative.
// Returns the smallest s at which the ray, widened by r/16 (>> the rounding of p, checked), touches an occupied cell of
// that layer: +inf if it never does, -1 if a precondition fails.  Marches that stay below that parameter are misses,
// however they end (leaving the brick, step cap, NaN).  r = voxel edge.
__device__ __noinline__ float brick_layer_first_touch(int k, V3 a, V3 b, V3 g, V3 bmin, float r, unsigned long long mask)
{
    // axis k is the pinned one; u, v = the other two (component selection by k, no indexed arrays)
    const float ak = k == 0 ? a.x : k == 1 ? a.y : a.z, bk = k == 0 ? b.x : k == 1 ? b.y : b.z, mk_ = k == 0 ? bmin.x : k == 1 ? bmin.y : bmin.z;
    const float au = k == 0 ? a.y : k == 1 ? a.z : a.x, av = k == 0 ? a.z : k == 1 ? a.x : a.y;
    const float gu = k == 0 ? g.y : k == 1 ? g.z : g.x, gv = k == 0 ? g.z : k == 1 ? g.x : g.y;
    const float mu = k == 0 ? bmin.y : k == 1 ? bmin.z : bmin.x, mv = k == 0 ? bmin.z : k == 1 ? bmin.x : bmin.y;
    const int su = k == 0 ? 4 : k == 1 ? 16 : 1, sv = k == 0 ? 16 : k == 1 ? 1 : 4;      // bit strides of u and v in the brick mask
    const float delta = r * 0.0625f;
    bool ok = (ak == mk_) & (bk < 0.0f);
    ok &= (mu >= 4.0f * r) & (mv >= 4.0f * r) & (delta >= (fabsf(mu) + fabsf(mv) + 8.0f * r) * 0x1p-21f);
    ok = ok && fabsf(gu) < 1.0e30f && fabsf(gv) < 1.0e30f;                // 1/b finite on both axes (no 0 * inf below)
    if (!ok) return -1.0f;
    const float u0 = au - mu, v0 = av - mv;
    float first = __uint_as_float(0x7F800000u);
    bool clean = true;
    for (int cv = 0; cv < 4; ++cv) {
        const float va = ((float)cv * r - delta - v0) * gv, vb = ((float)(cv + 1) * r + delta - v0) * gv;
        const float v_in = fminf(va, vb), v_out = fmaxf(va, vb);
        for (int cu = 0; cu < 4; ++cu) {
            const bool occupied = (mask >> (cu * su + cv * sv)) & 1ull;
            const float ua = ((float)cu * r - delta - u0) * gu, ub = ((float)(cu + 1) * r + delta - u0) * gu;
            const float s_in = fmaxf(fmaxf(fminf(ua, ub), v_in), 0.0f), s_out = fminf(fmaxf(ua, ub), v_out);
            clean &= (s_in == s_in) & (s_out == s_out);               // NaN cannot happen with finite operands; stay on the safe side
            first = (occupied & (s_in <= s_out)) ? fminf(first, s_in) : first;
        }
    }
    return clean ? first * (1.0f - 0x1p-18f) : -1.0f;                  // the slab parameters carry a few ulps of their own
}

// svo_trace_params.tile_cost_dev: the step count of a ray that ends (or turns into its shadow ray) is folded into its tile's
// record - [frame][tile][primary | shadow] maxima, what svo_tile_order sorts the next frame's tiles by.  Rare blocks only.
__device__ __forceinline__ void note_tile_cost(int outk, uint32_t steps)
{
    const TraceArgs T = args_reloaded();
    if (!T.tile_cost) return;
    const int k = outk & 0x7FFFFFFF;
    int tile, frame = 0;
    if (T.from_camera) {
        const int per = T.w * T.h;
        frame = k / per;
        const int r = k - frame * per;
        const int ly = r / T.w, lx = r - ly * T.w;
        tile = (ly / TILE_H) * T.tiles_per_row + lx / TILE_W;
    } else tile = k >> 6;
    atomicMax(&T.tile_cost[((size_t)frame * (size_t)T.ntiles + (size_t)tile) * 2 + (outk < 0 ? 1 : 0)], steps);
}

// (the bounded instantiations) no hit of the lane's tree march can lie in front of its far end any more: the smallest t a later hit of
// this chunk can report is tw + (tree-level t - leaf_back); inside a brick the tree level's t is the one the brick was entered at
template <bool GLSL>
__device__ __forceinline__ bool past_far_end(int mode, float t, float tt_saved, float tw, float eps, float far)
{
    const float tt = mode == M_TWIG ? tt_saved : t;
    return (mode == M_TREE || mode == M_TWIG) && tw + (GLSL ? tt : tt - eps) >= far;
}

// ---- what the blocks below write more than once ------------------------------------------------------------------------

// the flag word of a shadow ray that ends with `verdict` (SVO_SHADOWED, SVO_ERR_FLAG) instead of leaving its record "traced, lit"
__device__ __forceinline__ uint32_t shadow_flags(int normal_mode, uint32_t verdict)
{
    return SVO_HIT_FLAG | SVO_SHADOW_TRACED | verdict | (normal_mode == SVO_NORMAL_FACE ? (uint32_t)SVO_FACE_NORMAL : 0u);
}
// the lane's ray has ended and its record is written: its step count goes to its tile's cost (if the launch asks for it)
__device__ __forceinline__ void retire(int &mode, bool want_cost, int outk, uint32_t guard)
{
    if (want_cost) note_tile_cost(outk, guard);
    mode = M_DONE;
}

} // namespace svo

#include "chunk_step_cxx.hip.h"
#include "step_cxx.hip.h"

namespace svo {

// The two steps: the hand-scheduled statements, or (-DSVO_CXX_STEP) their C++ twins, behind one name each.
#ifdef SVO_CXX_STEP
template <bool BIG, bool GLSL, bool SEG> using ChunkStep = ChunkStepCxx<BIG, GLSL, SEG>;
#define SVO_MARCH_STEPS march_steps_cxx
#else
template <bool BIG, bool GLSL, bool SEG> using ChunkStep = ChunkStepAsm<BIG, GLSL, SEG>;
#define SVO_MARCH_STEPS march_steps_asm
#endif

// BIG: the large-world instantiation - the chunk's wide tree is a 64-bit address per lane and the brick masks are addressed with
// 64 bits (step_asm.hip.h: march_steps_asm<true, GLSL>), for wide pools of 4 GiB and more and mask pools of 2^29 bricks and more; the same
// kernel otherwise, the same results.
// GLSL: the shader twin's march (svo_trace_params.semantics = SVO_SEMANTICS_GLSL; shaders/Chunkmarch.glsl): the guarded escape
// distance and the LEAF hit at t inside the step (step_asm.hip.h), the entry condition and the missing containment re-check here.
// SEG: the bounded instantiations (svo_trace_segments; ray lists only): ray k ends at `far` = A.tmax[k], one more lane value, loaded with
// the ray at refill (+inf once the lane turns into a shadow ray).  The step itself is untouched.  Between two statements a marching lane
// whose tree march can no longer hit in front of the far end - tw + (t - leaf_back) >= far with the TREE level's t, which never decreases
// inside the chunk; see kernel_literal.hip.h and DESIGN.md 6g - gives its chunk up the way a lane that marched out of it does (M_WORLD,
// escape pending): so a ray ends INSIDE a chunk, a statement late at the most.  The chunk step, where tw changes, ends the ray once
// tw - leaf_back >= far, and the hit blocks apply the strict compare t < far (a dropped hit writes the miss record and casts no shadow ray).
template <int MAXLV, int REFILL, int WAVES_PER_SIMD, bool BIG, bool GLSL, bool SEG = false>
__global__ __launch_bounds__(64, WAVES_PER_SIMD) void k_trace_stack(TraceArgs A)
{
    __shared__ uint32_t stk[MAXLV / 2 + 1][64];     // wide node index per wide level of the current path (level 0 is node 0)
    __shared__ float tile_ray[SEG ? 12 : 11][64];
    // the chunk table (bmin, levels, wide offset, brick offset) of worlds of up to 64 chunks - the reference's default is 4x4x4 -
    // staged in LDS: the chunk step then reads it there instead of waiting for a 32-byte global load per lane (the block runs
    // in six of ten passes and a wave waits out the slowest lane's load each time)
    // (the large-world instantiation holds 126 chunks - a 10x1x10 grid of depth-12 chunks is 68 GB of pools - for 1.5 KB more LDS
    // per wave: 22 instead of 24 waves fit a CU's 160 KB; 126, not 128 - and 62, not 64, under the deepest instantiation's descent
    // column, which takes as much: the table and the 32 bytes of chunk_grid below together take what the table alone took, so
    // that none of the 7,424- and 7,680-byte instantiations crosses an LDS allocation step)
    constexpr int CHUNK_TAB = (BIG && MAXLV <= 10) ? 126 : MAXLV > 16 ? 62 : 64;      // (the deep instantiations' descent column already takes the room)
    __shared__ uint32_t chunk_tab[6][CHUNK_TAB];
    __shared__ __attribute__((aligned(16))) ChunkGrid chunk_grid;       // (32 B: 5,920 B of LDS per wave where the table holds 64 chunks; 24 waves per CU could take 6,826)
    stk[0][threadIdx.x] = 0u;              // o, d, 1/d, world-entry t, output index (as int; -1 = no ray)
    const int lane = threadIdx.x;
    const bool want_cost = A.tile_cost != nullptr;      // (one SGPR held; the blocks below must not re-read the kernel arguments for a feature that is off)
    const bool light_clear = (A.light_clear & LIGHT_CLEAR_NODES) != 0;      // shadow rays retire at clear cells (light_clearance.hip.h); the C++ step ignores the bit, which is always right
    const int n_chunks = A.dimw * A.dimh * A.dimd;
    const bool chunks_in_lds = n_chunks <= CHUNK_TAB;
    if (lane == 0) {
        chunk_grid.inv = A.inv_chunksize;
        for (int a = 0; a < 3; ++a) chunk_grid.off[a] = A.cbase[a] - A.ccm[a];
        chunk_grid.dimw = A.dimw; chunk_grid.dimh = A.dimh; chunk_grid.dimd = A.dimd;
        chunk_grid.table_in_lds = chunks_in_lds ? 1u : 0u;
    }
    if (chunks_in_lds)
        for (int i = lane; i < n_chunks; i += 64) {
            const DevWide ch = A.wchunks[i];
            chunk_tab[0][i] = __float_as_uint(ch.bmin[0]); chunk_tab[1][i] = __float_as_uint(ch.bmin[1]); chunk_tab[2][i] = __float_as_uint(ch.bmin[2]);
            chunk_tab[3][i] = ch.levels; chunk_tab[4][i] = ch.wide_off; chunk_tab[5][i] = (uint32_t)ch.twig_off;
        }
    __syncthreads();
#ifdef SVO_STACK_TIMING
    const unsigned long long t_begin = __builtin_amdgcn_s_memrealtime();
    unsigned n_iters = 0, n_tree_lanes = 0, n_twig_lanes = 0, n_world_lanes = 0;
    unsigned n_world_runs = 0, n_hit_runs = 0, n_refill = 0, n_tilegen = 0, n_fix = 0;
    unsigned n_lane_twig = 0;
    unsigned n_lane_busy = 0;       // per lane: asm steps it entered a statement for as a marching lane; the wave's maximum is its critical path
    unsigned n_creep_runs = 0, n_creep_rounds = 0, n_dbg = 0;   // block runs, rounds
    unsigned n_wsteps = 0, n_lsteps = 0, n_hit_wait = 0, n_dead_wait = 0, n_wsteps_b = 0, n_lsteps_b = 0, n_world_wait = 0, n_twig_b = 0;   // step bodies executed, marching lanes summed over them; M_HIT / M_DONE lanes summed over them
#endif
    [[maybe_unused]] StepStats step_stats;      // the asm step's own counters (the timing build's; the others leave them untouched)

    const V3 wlo = ld3(A.worldmin), whi = ld3(A.worldmax);
    const V3 sdir = ld3(A.sdir);
    const V3 sg = recip(sdir);                      // 1/sdir: the same quotient for every shadow ray
    const float eps = A.eps;
    const bool eps_pow2 = (__float_as_uint(eps) & 0x807FFFFFu) == 0u && __float_as_uint(eps) >= 0x00800000u && __float_as_uint(eps) < 0x7F800000u;
    const float csize = A.chunksize;

    // ---- wave state (uniform) ------------------------------------------------------------
    // The image is dealt out as TILE_REGIONS screen regions (column strips of 8x8 tiles; row bands when the raster has
    // fewer than 8 tile columns, e.g. ray lists), each behind its own cursor.  A wave starts in the region of its XCD:
    // an XCD's waves then march rays that traverse the same part of the world, and that XCD's private L2 holds it.
    // A wave whose region is used up moves on to the next one (work stealing).
    const int tr_cols = A.tiles_per_row;
    const int tr_rows = A.ntiles / (tr_cols > 0 ? tr_cols : 1);
    const bool by_cols = tr_cols >= TILE_REGIONS;
    const int reg_q = (by_cols ? tr_cols : tr_rows) / TILE_REGIONS, reg_rem = (by_cols ? tr_cols : tr_rows) % TILE_REGIONS;
    int region = (int)(__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & (TILE_REGIONS - 1));    // HW_REG_XCC_ID[3:0]
    int regions_left = TILE_REGIONS;
    int tile_first = 0;             // first ray id of the tile being handed out
    int tile_next = 64;             // next unassigned slot of that tile (64 = exhausted)
    bool more = true;               // tiles left in the global cursor
    unsigned rays_marched = 0;      // per lane, summed at exit

    // ---- lane state ------------------------------------------------------------------------
    int mode = M_DONE;
    int outk = 0;                   // output record of the ray; bit 31 set: the lane marches that pixel's shadow ray
    V3 alpha = mk(0, 0, 0), beta = mk(0, 0, 1), g = mk(0, 0, 0);
    float tw = 0.0f;                // chunkmarch's t (src/Traverse.cpp:135)
    [[maybe_unused]] float far = __uint_as_float(0x7F800000u);     // (SEG) the ray's far end
    int cw = 0;
    uint32_t guard = 0;
    // The level being marched (tree: src/Traverse.cpp:74-113, brick: :50-72) as one "frame": p = O + beta*t is
    // tested against the box [Blo, Blo+Bsize] and located on a lattice of pitch `res` anchored at Blo.
    // Entering a brick swaps the frame (and parks the tree level's t / counter); leaving swaps it back.
    V3 O = mk(0, 0, 0), Blo = mk(0, 0, 0);
    // (the box edge, 1/res and the step cap follow from mode and res: chunk edge / 4 voxels, A.cap_tree / A.cap_twig)
    float res = 1.0f, t = 0.0f;
    int cnt = 0;                    // steps LEFT of the level's cap (counts down: cap - the reference's loop counter); in M_HIT: the brick cell that was hit (or SVO_CELL_NONE: a LEAF)
    float tt_saved = 0.0f, t_miss = 0.0f;  // tree-level t at the brick's entry; ... after the brick march has missed
    int it_saved = 0;
    // chunk
    V3 clo = mk(0, 0, 0);
    WideRef<BIG> wide_b = 0;        // the chunk's top wide node: byte offset into the wide pool (BIG: its address)
    // entry `e` (64 per wide node, counted from the chunk's top wide node) of the current chunk's wide tree
    auto ld_wide = [&](uint32_t e) -> uint32_t {
        if constexpr (BIG) return *reinterpret_cast<const uint32_t *>((size_t)wide_b + ((size_t)e << 2));
        else return ld_node(A.wide, wide_b + (e << 2));
    };
    uint32_t twig_off = 0;
    int levels = 0, ci = -1;
    // descent cache: cell coordinates of the last tree step and the level of the node it ended at
    // (valid: deepest wide level whose node index is cached; plev: reference level of the node the last tree step ended at)
    int pux = 0, puy = 0, puz = 0, valid = 0, plev = 0;
    // brick
    unsigned long long bmask = 0;
    // the steps (step_asm.hip.h) keep the level's box edge and the chunk's wide-level count / tree-level pitch instead of deriving them per step
    float bsize = 0.0f, res_tree = 1.0f;
    int nw_chunk = 1;
    const uint32_t lds_lane = (uint32_t)(size_t)(__attribute__((address_space(3))) uint32_t *)&stk[0][lane];
    StepUniform SU;
    SU.csize = csize; SU.eps = eps; SU.eps2 = 2.0f * eps; SU.cap_twig = A.cap_twig; SU.wide = A.wide; SU.mask = A.mask; SU.descend_shift = MAXLV <= 10 ? DESCEND_SHIFT_SHALLOW : DESCEND_SHIFT_DEEP;
    // ... and the chunk step's (chunk_step_asm.hip.h)
    const uint32_t lds_tab = (uint32_t)(size_t)(__attribute__((address_space(3))) uint32_t *)&chunk_tab[0][0];
    ChunkStepUniform CU;
    CU.wlo = wlo; CU.whi = whi; CU.csize = csize; CU.eps = eps; CU.cap_chunk = A.cap_chunk; CU.cap_tree = A.cap_tree; CU.wide = A.wide;
    CU.kernarg = __builtin_amdgcn_kernarg_segment_ptr();
    // creeping rays: |creepn| = consecutive advances of this ray by less than 2 EPS (kept across level changes: a ray pinned
    // on a chunk face creeps at every level); > 0 only while the cell located last is known to be empty (creep block armed)
    int creepn = 0;
    for (;;) {
        // ==== refill retired lanes =============================================================
        unsigned long long dead = vote(mode == M_DONE);
        while (more && vote_count(dead) >= REFILL) {
            if (tile_next >= 64) {
                int t32 = -1, tcol = 0, trow = 0, tframe = 0;   // raster index of the tile, its column and row, its frame
                const uint32_t *order = args_reloaded().tile_order;
                if (order) {                                    // caller's order (longest tiles first): one cursor, frame after frame
                    regions_left = 0;
                    unsigned long long tix = 0;
                    if (lane == 0) tix = atomicAdd(&A.work[WORK_CURSOR0], 1ull);
                    int t = __builtin_amdgcn_readfirstlane((int)tix);
                    if (t < A.ntiles * A.nframes) {
                        tframe = t / A.ntiles; t -= tframe * A.ntiles;
                        t32 = (int)order[t];
                        // the caller's array: anything that is not a tile index reads as "this entry has no tile" (an empty tile:
                        // its 64 slots hold no ray) instead of indexing the raster or the ray list out of range
                        if ((uint32_t)t32 >= (uint32_t)A.ntiles) { t32 = 0; tframe = -1; }
                        trow = t32 / tr_cols; tcol = t32 - trow * tr_cols;
                    }
                }
                while (regions_left > 0) {
                    const int span = reg_q + (region < reg_rem ? 1 : 0);                    // columns (rows) of this region
                    const int first = region * reg_q + (region < reg_rem ? region : reg_rem);
                    const int count = span * (by_cols ? tr_rows : tr_cols);          // tiles of this region in one frame
                    unsigned long long tix = 0;
                    if (lane == 0) tix = atomicAdd(&A.work[WORK_CURSOR0 + region], 1ull);
                    int t = __builtin_amdgcn_readfirstlane((int)tix);
                    if (t < count * A.nframes) {                                    // frame after frame within the region
                        if (A.nframes > 1) { tframe = t / count; t -= tframe * count; }
                        if (by_cols) { trow = t / span; tcol = first + (t - trow * span); }
                        else { trow = first + t / tr_cols; tcol = t % tr_cols; }
                        t32 = trow * tr_cols + tcol;
                        break;
                    }
                    region = (region + 1) & (TILE_REGIONS - 1);
                    --regions_left;
                }
                if (t32 < 0) { more = false; break; }
                tile_first = t32 * 64;
                tile_next = 0;
#ifdef SVO_STACK_TIMING
                ++n_tilegen;
#endif
                // all 64 lanes generate the tile's rays (src/Traverse.cpp:135-140 included) and park them in LDS
                {
                    const TraceArgs T = args_reloaded();
                    const int id = tile_first + lane;
                    bool ok;
                    int k = -1;
                    V3 o = mk(0, 0, 0), d = mk(0, 0, 1);
                    if (T.from_camera) {
                        const int lx = tcol * TILE_W + (lane & (TILE_W - 1));
                        const int ly = trow * TILE_H + lane / TILE_W;
                        ok = (lx < T.w) & (ly < T.h) & (tframe >= 0);      // (tframe < 0: an entry of the caller's tile order that names no tile)
                        k = (tframe * T.h + ly) * T.w + lx;
                        int px = 0, py = 0;
                        if (ok) local_to_pixel(T, lx, ly, px, py);
                        if (ok && (py >= T.imgh || px >= T.imgw)) { store_miss(A.out, k, 0); ok = false; }
                        if (ok) camera_ray(camera_reloaded(tframe), T.imgw, T.imgh, px, py, o, d);
                    } else {
                        ok = id < T.n && tframe >= 0;
                        k = id;
                        if (ok) { o = ld3(T.origins + 3 * (long long)id); d = ld3(T.dirs + 3 * (long long)id); }
                        if constexpr (SEG) tile_ray[11][lane] = ok ? T.tmax[id] : 0.0f;
                    }
                    const V3 gg = recip(d);
                    float t0 = 0.0f;
                    if (ok) {
                        bool hit = true;
                        if (!inside(o, wlo, whi)) t0 = (GLSL ? enter_glsl(o, gg, wlo, whi, hit) : enter(o, d, wlo, whi, hit)) + eps;
                        rays_marched++;
                        if (!hit) { store_miss(A.out, k, 0); ok = false; }
                    }
                    tile_ray[0][lane] = o.x; tile_ray[1][lane] = o.y; tile_ray[2][lane] = o.z;
                    tile_ray[3][lane] = d.x; tile_ray[4][lane] = d.y; tile_ray[5][lane] = d.z;
                    tile_ray[6][lane] = gg.x; tile_ray[7][lane] = gg.y; tile_ray[8][lane] = gg.z;
                    tile_ray[9][lane] = t0;
                    tile_ray[10][lane] = __int_as_float(ok ? k : -1);
                    __syncthreads();                        // one wave per block: orders the LDS writes before the reads
                }
            }
#ifdef SVO_STACK_TIMING
            ++n_refill;
#endif
            const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(dead >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)dead, 0u));
            const int avail = 64 - tile_next;
            if (mode == M_DONE && rank < avail) {
                const int slot = tile_next + rank;
                const int k = __float_as_int(tile_ray[10][slot]);
                if (k >= 0) {
                    outk = k;                               // (bit 31 clear: primary ray)
                    alpha = mk(tile_ray[0][slot], tile_ray[1][slot], tile_ray[2][slot]);
                    beta = mk(tile_ray[3][slot], tile_ray[4][slot], tile_ray[5][slot]);
                    g = mk(tile_ray[6][slot], tile_ray[7][slot], tile_ray[8][slot]);
                    tw = tile_ray[9][slot];
                    if constexpr (SEG) far = tile_ray[11][slot];
                    cw = 0; guard = 0; creepn = 0;
                    mode = M_WORLD;
                }
            }
            const int ndead = vote_count(dead);
            tile_next += (ndead < avail) ? ndead : avail;
            __syncthreads();                                // reads done before a later tile overwrites the buffer
            dead = vote(mode == M_DONE);
        }
        if (dead == ~0ull) break;                       // nothing alive and nothing left to fetch
#ifdef SVO_STACK_TIMING
        ++n_iters;
        n_tree_lanes += __popcll(__ballot(mode == M_TREE)); n_twig_lanes += __popcll(__ballot(mode == M_TWIG));
        n_world_lanes += __popcll(__ballot(mode == M_WORLD));
#endif

        // ==== votes: which of the rare blocks run this iteration ================================
        const int n_busy = vote_count(vote(mode == M_TREE || mode == M_TWIG));
        const int n_world = vote_count(vote(mode == M_WORLD));
        const int n_hit = vote_count(vote(mode == M_HIT));
        // (n > 0 && (n >= VOTE || n_busy < VOTE_BUSY) as one scalar compare against a selected threshold)
        const bool few_busy = n_busy < VOTE_BUSY;
        bool run_world = n_world >= (few_busy ? 1 : VOTE_WORLD);
        if (!run_world && n_world > 0) run_world = vote(mode == M_WORLD && creepn <= -CREEP_SERIOUS) != 0ull;
        const bool run_hit = n_hit >= (few_busy ? 1 : VOTE_HIT);

        if (SVO_UNLIKELY(mode != M_DONE && mode != M_HIT && ++guard > STEP_GUARD)) {     // runaway ray: give up, flag it
            if (outk < 0) store_flags(A.out, outk & 0x7FFFFFFF, shadow_flags(A.normal_mode, SVO_ERR_FLAG));
            else store_miss(A.out, outk, SVO_ERR_FLAG);
            mode = M_DONE;
        }

        // ---- chunk step: src/Traverse.cpp:142-156 -------------------------------------------
#ifdef SVO_STACK_TIMING
        n_world_runs += run_world; n_hit_runs += run_hit;
#endif
        // (the votes are wave-uniform: a scalar branch over a block that does not run - folded into the lane mask, a pass without the
        // block paid the mask's scalar arithmetic and an EXEC round trip; the empty statement keeps the two tests apart)
        if (SVO_LIKELY(run_world)) { asm volatile("");
        // (chunk_step_asm.hip.h, or its C++ twin) the step as one statement - the only place that writes the chunk's lane registers; the rays
        // that end here come back as a mask, their records are stored behind it
        const ChunkGrid G = chunk_grid;                 // (two LDS reads at a uniform address)
        const unsigned long long missed = ChunkStep<BIG, GLSL, SEG>::template run<CHUNK_TAB>(
            mode, tw, cw, ci, valid, pux, puy, puz, clo, wide_b, twig_off, levels, O, t, cnt, Blo, res, bsize, res_tree, nw_chunk,
            alpha, beta, g, far, G.inv, G.off[0], G.off[1], G.off[2], G.dimw, G.dimh, G.dimd,
            (uint32_t)__builtin_amdgcn_readfirstlane((int)G.table_in_lds), lds_tab, CU);
        if (__builtin_amdgcn_inverse_ballot_w64(missed)) {        // (the mask is the branch's EXEC: no lane value is formed)
            int k = outk;
            asm("" : "+v"(k));                      // (a value of its own: the record's 64-bit index is formed here, not held as a pair across the loop)
            if (k >= 0) store_miss(A.out, k, 0);
            retire(mode, want_cost, k, guard);      // shadow miss: record already says "traced, lit"
        }
        }

        // ---- the steps of the current level: tree (src/Traverse.cpp:79-111) or brick (:54-70); step_cxx.hip.h states what one step does.
        //      The step repeats at once, without the refill / vote / block checks around it, while every live lane of the
        //      wave is marching and nothing else can be due: that is the state of the waves that carry a launch's longest
        //      rays after the tile cursors ran dry, alone on their SIMD and bound by their own instruction stream.
        int pass = 0;
        // in the bulk: STEP_EXTRA more steps, decided once per pass of the outer loop (n_busy: before the chunk step)
        const int fixed_steps = (n_busy >= STEP_LANES && vote(creepn > 0 || creepn <= -4 * CREEP_SERIOUS) == 0ull) ? STEP_EXTRA : 0;
        // the lanes that march a shadow ray: they change kind only in the hit block, so once per pass of the outer loop
        const unsigned long long shadow_lanes = light_clear ? vote(outk < 0) : 0ull;
        for (;;) {
        // (step_asm.hip.h, or its C++ twin) the steps of this pass in one statement: 1 + fixed_steps at first, DRAIN_STEPS while the inner repeat lasts
#ifdef SVO_STACK_TIMING
        n_lane_twig += mode == M_TWIG ? (pass == 0 ? 1u + (unsigned)fixed_steps : (unsigned)DRAIN_STEPS) : 0u;        // ... of them started inside a brick
        n_lane_busy += (mode == M_TREE || mode == M_TWIG) ? (pass == 0 ? 1u + (unsigned)fixed_steps : (unsigned)DRAIN_STEPS) : 0u;     // steps of the coming statement this lane starts as a marching lane (an upper bound on its own steps)
        { const int nm = __popcll(__ballot(mode == M_TREE || mode == M_TWIG)); n_wsteps += nm > 0; n_lsteps += nm; if (more) { n_wsteps_b += nm > 0; n_lsteps_b += nm; n_hit_wait += __popcll(__ballot(mode == M_HIT)); n_dead_wait += __popcll(__ballot(mode == M_DONE)); n_world_wait += __popcll(__ballot(mode == M_WORLD)); n_twig_b += __popcll(__ballot(mode == M_TWIG)); } }
#endif
        const int nsteps = pass == 0 ? 1 + fixed_steps : DRAIN_STEPS;
        const int sure_miss = SVO_SURE_MISS_WHEN;      // (step_asm_body.inc: bricks whose march is bound to miss are not entered)
        SVO_MARCH_STEPS<BIG, GLSL>(mode, O, Blo, bsize, res, t, cnt, tt_saved, t_miss, it_saved, tw, cw, pux, puy, puz, valid, plev, bmask, creepn,
                               beta, g, clo, alpha, levels, nw_chunk, res_tree, wide_b, twig_off, lds_lane, SU, nsteps | (sure_miss << 16), shadow_lanes, step_stats);
        pass += nsteps - 1;

        // Loop control is wave-uniform (scalar compare and branch).  In the bulk the number of extra steps was fixed before
        // the loop: nothing is looked at between them - the checks around the step (refill, three votes, guard, creep vote,
        // hit blocks) cost a quarter of an iteration, even one ballot per step 2 %; the lanes that wait a step or two
        // longer for a refill or a vote cost less.  The per-lane runaway guard is settled after the loop, which ends
        // after 256 steps at the latest so that the outer loop's check sees a runaway ray.
        ++pass;
        if (pass <= fixed_steps) continue;
        if (more || pass >= 256) break;
        const unsigned long long marching = vote(mode == M_TREE || mode == M_TWIG);
        if (marching == 0ull || marching != vote(mode != M_DONE) || vote(creepn > 0 || creepn <= -4 * CREEP_SERIOUS) != 0ull) break;
        if constexpr (SEG) if (vote(past_far_end<GLSL>(mode, t, tt_saved, tw, eps, far)) != 0ull) break;       // a lane of the draining wave has reached its far end
        }
        guard += pass - 1;
        if constexpr (SEG) {
            if (past_far_end<GLSL>(mode, t, tt_saved, tw, eps, far)) {                               // leave the chunk as the step does (its S_LEAVE out of a brick, then out of the tree)
                if (mode == M_TWIG) O = alpha + beta * tw;  // the chunk march's p: what the chunk step takes the escape from
                creepn = creepn > 0 ? -creepn : creepn;     // (disarmed: the lane marches no cell)
                cw |= CW_ESCAPE_PENDING;
                mode = M_WORLD;
            }
        }

#include "creep_block.inc"

        // ---- hits.  A shadow ray only sets a flag; a primary hit waits (M_HIT) until the wave votes to
        //      resolve: G-buffer record, then the lane becomes its own shadow ray -------------------
        if (mode == M_HIT && outk < 0) {
            store_flags(A.out, outk & 0x7FFFFFFF, shadow_flags(A.normal_mode, SVO_SHADOWED));
            retire(mode, want_cost, outk, guard);
        }
        if constexpr (SEG) {
            if (mode == M_HIT && !(tw < far)) {             // a hit at or behind the far end: the miss record, no shadow ray (no vote needed)
                store_miss(A.out, outk, 0);
                retire(mode, want_cost, outk, guard);
            }
        }
        if (run_hit) { asm volatile("");
        if (mode == M_HIT) {
            // which voxel: the node comes from the descent cache; the frame still describes the level that hit
            const int nw = levels ? (levels + 1) >> 1 : 1;
            const uint32_t wn = valid > 0 ? stk[valid][lane] : 0u, slot = wide_slot(pux, puy, puz, 2 * (nw - 1 - valid));
            const uint32_t word = ld_wide((wn << 6) + slot);        // the terminal entry again (material / brick index) ...
            // ... and the reference node it stands for (svo_hit.node): the entry's wide node keeps the index of the child block it
            // expands and of its eight grandchild blocks (wide_tree.hip.h: wbase); level 0 is the chunk's root, node 0
            uint32_t node = 0u;
            if (plev != 0) {
                const uint32_t ci = ((slot >> 1) & 1u) | ((slot >> 2) & 2u) | ((slot >> 3) & 4u);
                const uint32_t gi = (slot & 1u) | ((slot >> 1) & 2u) | ((slot >> 2) & 4u);
                size_t wnode_in_pool;                               // the wide node's index in the pool: the chunk's top wide node + wn
                if constexpr (BIG) wnode_in_pool = (((size_t)wide_b - (size_t)A.wide) >> 8) + wn;
                else wnode_in_pool = (wide_b >> 8) + wn;
                const uint32_t *wb = A.wbase + wnode_in_pool * WIDE_BASE_WORDS;
                const int level_child = 2 * valid + 1 - (2 * nw - levels);
                // one load at a selected index, issued while the entry is on its way and waited for together with it (it was two
                // loads behind a lane-divergent branch, each with a wait of its own)
                const bool child = plev == level_child;
                node = wb[child ? 0u : 1u + ci] + (child ? ci : gi);
            }
            const uint32_t hitc = (uint32_t)cnt;                    // which brick cell (or SVO_CELL_NONE: a LEAF)
            V3 vlo;
            float vsize;
            uint32_t material;                                      // (bit 16: the hit brick's clear flag, which store_hit cuts off)
            if (hitc == SVO_CELL_NONE) {                            // LEAF node: frame = tree level (Blo = clo, res = cell)
                const int low = (1 << (levels - plev)) - 1;
                vlo = mk(Blo.x + (float)(pux & ~low) * res, Blo.y + (float)(puy & ~low) * res, Blo.z + (float)(puz & ~low) * res);
                vsize = res * (float)(low + 1);
                material = word & 0xFFFFu;
            } else {                                                // brick cell: frame = brick (Blo = node box, res = voxel)
                vlo = mk(Blo.x + (float)(hitc & 3u) * res, Blo.y + (float)((hitc >> 2) & 3u) * res, Blo.z + (float)(hitc >> 4) * res);
                vsize = res;
                // most bricks hold one material (grow() fills a brick with its node's): it is kept per brick next to the masks, 64
                // bricks to a cache line; only a brick of several materials (0xFFFF) is read itself, 128 B for one cell
                const unsigned long long brick = (unsigned long long)twig_off + (word & WIDE_PAYLOAD);
                // (BMAT_CLEAR_BIT of the word is the brick's clear flag, light_clearance.hip.h; BMAT_SEVERAL carries none)
                const uint32_t bw = A.bmat[brick];
                material = bw == BMAT_SEVERAL ? A.twig[brick * TWIG_WORDS + hitc] : (bw & BMAT_MATERIAL_MASK) | ((bw & BMAT_CLEAR_BIT) << 1);
            }
            const V3 point = alpha + beta * (tw - eps);
            // The shadow ray's first sample is its origin itself (tw = 0, t = 0, p = alpha = point), and the reference locates it by the
            // brick step's own arithmetic.  The frame still is the hit brick's (Blo its box, res its voxel, bmask its cells): inside the
            // box, a cell of 0..3 per axis (a difference rounded up to the far face gives 4: not settled, which is always right).  That
            // cell occupied: the reference's march returns a hit in its first brick cell, the ray is shadowed, whatever the
            // light and the pools' bits.  That cell empty and the brick's flag set: the ray is lit (6u).  One evaluation of the cell for
            // both; the verdict rides in bit 16 of `material`, which store_hit cuts off, and in the record's flags.
            // (the switches are read from the arguments here, as A.shadow is: a wave-uniform bool kept from the kernel's top costs a
            // scalar spill; the shader's twin and bounded rays never settle a ray: no code in their instantiations; either bit of
            // A.light_clear implies A.shadow)
            uint32_t dark = 0u;
            if constexpr (!GLSL && !SEG) {
                const uint32_t use = (uint32_t)A.light_clear & (uint32_t)(LIGHT_CLEAR_BRICKS | LIGHT_CLEAR_DARK);
                if (use != 0u) {                                // (wave-uniform: a scalar branch; inside, no lane branches - a LEAF hit computes
                    const float inv_res = recip_pow2(res);      //  a cell of its tree frame and is masked out by hitc)
                    // (the sign is that of the difference, not of the quotient: a voxel above 1 takes a denormal difference below 0 to -0)
                    const float dx = point.x - Blo.x, dy = point.y - Blo.y, dz = point.z - Blo.z;
                    const uint32_t ux = (uint32_t)(int)(dx * inv_res), uy = (uint32_t)(int)(dy * inv_res), uz = (uint32_t)(int)(dz * inv_res);
                    const bool located = (hitc != SVO_CELL_NONE) & (dx >= 0.0f) & (dy >= 0.0f) & (dz >= 0.0f) & ((ux | uy | uz) <= 3u);
                    // (integer arithmetic on the switch word: as wave-uniform bools the two switches are hoisted to the kernel's top as
                    // lane masks and cost four scalar spills)
                    const uint32_t occupied = (uint32_t)(bmask >> ((uz * 16u + uy * 4u + ux) & 63u)) & 1u;
                    const uint32_t on = (use >> (1u + occupied)) & (occupied | (material >> 16)) & 1u;      // occupied: the DARK bit; empty: the BRICKS bit and the brick's flag
                    const uint32_t settle = located ? on : 0u;
                    material = (material & 0xFFFFu) | (settle << 16);
                    dark = (settle & occupied) * (uint32_t)SVO_SHADOWED;
                } else {
                    material &= 0xFFFFu;
                }
            }
            const bool face = A.normal_mode == SVO_NORMAL_FACE;
            const V3 n = face ? face_normal(point, vlo, vlo + vsize, beta) : cube_normal_pow2(point, vlo, vsize, eps);
            const uint32_t flags = SVO_HIT_FLAG | (A.shadow ? SVO_SHADOW_TRACED : 0u) | (face ? (uint32_t)SVO_FACE_NORMAL : 0u) | dark;
            store_hit(A.out, outk, tw, n, material, flags, (uint32_t)ci, node, hitc);
            retire(mode, want_cost, outk, guard);
            if (A.shadow) {                             // the lane becomes its own shadow ray
                alpha = point; beta = sdir; g = sg;
                outk |= (int)0x80000000;
                if constexpr (SEG) far = __uint_as_float(0x7F800000u);    // (the light is a direction: its ray has no far end)
                tw = 0.0f; cw = 0; guard = 0; creepn = 0;
                bool hit = true;
                if (!inside(alpha, wlo, whi)) tw = (GLSL ? enter_glsl(alpha, g, wlo, whi, hit) : enter(alpha, beta, wlo, whi, hit)) + eps;
                // settled above, lit or shadowed: the record is final as store_hit wrote it
                const bool settled = !GLSL && !SEG && (material >> 16) != 0u;
                mode = hit && !settled ? M_WORLD : M_DONE;  // a shadow ray that misses the world box stays "lit"
                rays_marched++;
            }
        } }
    }

    unsigned total = rays_marched;
    for (int off = 32; off > 0; off >>= 1) total += __shfl_down(total, off, 64);
    if (lane == 0 && total) atomicAdd(&A.work[1], (unsigned long long)total);
#ifdef SVO_STACK_TIMING
    unsigned busiest = n_lane_busy;
    for (int off = 32; off > 0; off >>= 1) busiest = max(busiest, (unsigned)__shfl_xor((int)busiest, off, 64));
    unsigned busiest_twig = n_lane_busy == busiest ? n_lane_twig : 0u;          // the busiest lane's share inside bricks
    for (int off = 32; off > 0; off >>= 1) busiest_twig = max(busiest_twig, (unsigned)__shfl_xor((int)busiest_twig, off, 64));
    if (lane == 0 && A.counters) {       // diagnostic build only: per-wave [start, end] in 10 ns ticks, iterations, rays
        uint4 c; c.x = (uint32_t)t_begin; c.y = (uint32_t)__builtin_amdgcn_s_memrealtime(); c.z = n_iters; c.w = total;
        reinterpret_cast<uint4 *>(A.counters)[6 * blockIdx.x] = c;
        uint4 e; e.x = n_world_runs | (n_hit_runs << 16); e.y = n_refill | (n_tilegen << 12) | (n_fix << 20); e.z = n_tree_lanes; e.w = n_twig_lanes | (n_world_lanes << 20);
        reinterpret_cast<uint4 *>(A.counters)[6 * blockIdx.x + 1] = e;
        uint4 f; f.x = n_creep_runs | (busiest_twig << 16); f.y = busiest; f.z = n_creep_rounds; f.w = n_dbg;
        reinterpret_cast<uint4 *>(A.counters)[6 * blockIdx.x + 2] = f;
        uint4 h; h.x = n_wsteps; h.y = n_lsteps; h.z = n_hit_wait; h.w = n_dead_wait;
        reinterpret_cast<uint4 *>(A.counters)[6 * blockIdx.x + 3] = h;
        uint4 h2; h2.x = n_wsteps_b; h2.y = n_lsteps_b; h2.z = n_world_wait; h2.w = n_twig_b;
        reinterpret_cast<uint4 *>(A.counters)[6 * blockIdx.x + 4] = h2;
        uint4 h3; h3.x = step_stats.steps; h3.y = step_stats.lanes; h3.z = step_stats.stalls; h3.w = step_stats.chased;
        reinterpret_cast<uint4 *>(A.counters)[6 * blockIdx.x + 5] = h3;
    }
#endif
}

} // namespace svo
