// builder.hip — device-side world generation: the World::init half of the boundary on the GPU.
//
// Produces pools bit-identical to terrain.cpp (and therefore to the reference's algorithm) for the same
// parameters:
//   BoundsPyramid::computeBase        src/BoundsPyramid.cpp:92-104   -> k_noise_base   (one thread per texel)
//   BoundsPyramid::computeBoundsAbove src/BoundsPyramid.cpp:106-135  -> k_mip_level    (one thread per coarse texel)
//   grow()                            src/Octree.cpp:74-176          -> level-synchronous BFS:
//        k_classify (EMPTY / LEAF / TWIG / BRANCH per frontier node, src/Octree.cpp:105-121)
//        exclusive scans of the BRANCH and TWIG flags (rocPRIM) == the reference queue's append order
//        k_emit     (node words, the 8 children of every BRANCH into the next frontier, :155-174)
//        k_bricks_rows (one thread per brick z-row: 4 column lookups, 16 cells, one 32-byte store, :122-154)
//   Ocroot::build (the water plane)   src/Octree.cpp:320-436         -> DeviceFiller below: the depth-first fill as three
//        level-synchronous sweeps (classify top-down, count bottom-up, number top-down); the node words never visit the host
//
// Layout on the device: the pyramid is the same flat array per bound as on the host (level lv at (4^lv-1)/3,
// row-major): mip kernels read/write whole rows coalesced; frontier entries are 16 B {x, y, z, slot}.
// Compile with -ffp-contract=off: every float op must round separately, exactly like terrain.cpp.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <thread>
#include <vector>

#include "bfs.hip.h"
#include "hip_own.h"
#include "terrain.h"

namespace svo {

namespace {

// ---- 2-D simplex noise, the same sequence of float operations as terrain.cpp's Noise2::eval ------------
__device__ __forceinline__ float d_wrap289(float x) { return x - floorf(x * (1.0f / 289.0f)) * 289.0f; }
__device__ __forceinline__ float d_perm(float x) { return d_wrap289(((x * 34.0f) + 1.0f) * x); }
__device__ __forceinline__ float d_frac(float x) { return x - floorf(x); }

__device__ float d_simplex2(float vx, float vy)
{
    const float SKEW = 0.366025403784439f, UNSKEW = 0.211324865405187f;
    const float OFF2 = -0.577350269189626f, INV41 = 0.024390243902439f;
    const float skew = vx * SKEW + vy * SKEW;
    float cx = floorf(vx + skew), cy = floorf(vy + skew);
    const float unskew = cx * UNSKEW + cy * UNSKEW;
    const float d0x = vx - cx + unskew, d0y = vy - cy + unskew;
    const bool lower = d0x > d0y;
    const float sx = lower ? 1.0f : 0.0f, sy = lower ? 0.0f : 1.0f;
    const float d1x = (d0x + UNSKEW) - sx, d1y = (d0y + UNSKEW) - sy;
    const float d2x = d0x + OFF2, d2y = d0y + OFF2;
    cx = cx - 289.0f * floorf(cx / 289.0f);
    cy = cy - 289.0f * floorf(cy / 289.0f);
    const float h[3] = { d_perm(d_perm(cy + 0.0f) + cx + 0.0f), d_perm(d_perm(cy + sy) + cx + sx), d_perm(d_perm(cy + 1.0f) + cx + 1.0f) };
    const float dx[3] = { d0x, d1x, d2x }, dy[3] = { d0y, d1y, d2y };
    float w[3], g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float m = 0.5f - (dx[k] * dx[k] + dy[k] * dy[k]);
        m = (m < 0.0f) ? 0.0f : m;
        m = m * m;
        m = m * m;
        const float gx = 2.0f * d_frac(h[k] * INV41) - 1.0f;
        const float gh = fabsf(gx) - 0.5f;
        const float ga = gx - floorf(gx + 0.5f);
        m *= 1.79284291400159f - 0.85373472095314f * (ga * ga + gh * gh);
        w[k] = m;
        g[k] = ga * dx[k] + gh * dy[k];
    }
    return 130.0f * (w[0] * g[0] + w[1] * g[1] + w[2] * g[2]);
}

__global__ __launch_bounds__(256) void k_noise_base(float *lo, float *hi, uint32_t size, float period, float xshift, float zshift)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)size * size) return;
    const uint32_t x = (uint32_t)(i % size), z = (uint32_t)(i / size);
    const float n = d_simplex2(((float)x + xshift) * period, ((float)z + zshift) * period);
    lo[i] = n;
    hi[i] = n;
}

// coarse texel k = min / max over its 2x2 footprint, folded into the initial +1 / -1 in the reference's order
// (row z even: pair (x, x+1), then row z odd) — src/BoundsPyramid.cpp:115-134
__global__ __launch_bounds__(256) void k_mip_level(const float *flo, const float *fhi, float *clo, float *chi, uint32_t s)
{
    const uint32_t up = s / 2;
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (uint64_t)up * up) return;
    const uint32_t cx = (uint32_t)(k % up), cz = (uint32_t)(k / up);
    float mn = 1.0f, mx = -1.0f;
#pragma unroll
    for (uint32_t r = 0; r < 2; ++r) {
        const uint64_t at = (uint64_t)(2 * cz + r) * s + 2 * cx;
        const float a = flo[at], b = flo[at + 1];
        const float ab = (b < a) ? b : a;
        mn = (ab < mn) ? ab : mn;
        const float c = fhi[at], d = fhi[at + 1];
        const float cd = (c < d) ? d : c;
        mx = (mx < cd) ? cd : mx;
    }
    clo[k] = mn;
    chi[k] = mx;
}

struct DevPyramid {
    const float *lo, *hi;       // flat, level lv at (4^lv - 1) / 3
    uint32_t size, levels;
    float amplitude, shift;
};

__device__ __forceinline__ uint64_t d_level_offset(uint32_t lv) { return ((1ull << (2 * lv)) - 1) / 3; }

// BoundsPyramid::bound, src/BoundsPyramid.cpp:146-174 (== HeightPyramid::bound in terrain.cpp)
__device__ float d_bound(const DevPyramid &P, const float *q, float x, float z, uint32_t lv)
{
    const uint64_t a = (uint64_t)(x * (float)P.size);
    const uint64_t b = (uint64_t)(z * (float)P.size);
    if (lv <= P.levels) {
        const uint32_t sh = P.levels - lv;              // d = 2^sh: the reference's divisions by d are shifts
        return q[d_level_offset(lv) + ((b >> sh) << lv) + (a >> sh)] * P.amplitude + P.shift;
    }
    const float *base = P.lo + d_level_offset(P.levels);
    const uint64_t m = P.size - 1;
    const uint64_t a1 = (a + 1) & m, b1 = (b + 1) & m;
    const float t = (float)(x * (float)P.size) - (float)a;
    const float s = (float)(z * (float)P.size) - (float)b;
    auto mix = [](float v0, float v1, float w) { return (float)((double)(v1 * w) + (1.0 - (double)w) * (double)v0); };
    const float r0 = mix(base[b * P.size + a], base[b * P.size + a1], t);
    const float r1 = mix(base[b1 * P.size + a], base[b1 * P.size + a1], t);
    return mix(r0, r1, s) * P.amplitude + P.shift;
}

__device__ __forceinline__ uint32_t d_height_material(float y)
{   // src/Octree.cpp:69-72, in double
    double v = (double)y / 0.03;
    if (v < 1.0) v = 1.0;
    if (4.0 < v) v = 4.0;
    return (uint32_t)(uint16_t)v;
}

using Cell = BfsCell<float>;        // frontier entry: the node's corner in world units and its slot (bfs.hip.h: k_level_totals, k_emit)

constexpr unsigned FILL_BLOCK = 1024;     // threads per block of the sweeps that number nodes through block_take (hip_own.h)

struct GrowArgs {
    float px, py, pz, size;     // chunk position / edge
    float edge;                 // node edge at this level
    uint32_t level, depth;
    uint32_t coarse_depth;      // 0 = off
    float rmin[3], rmax[3];     // refine box
};

// type of every frontier node (src/Octree.cpp:105-121) + its flags for the scan (BRANCH in the low half, TWIG in the high half of
// one 64-bit word: one scan ranks both; the level's totals follow from the scan, k_level_totals)
__global__ __launch_bounds__(256) void k_classify(const Cell *frontier, uint32_t n, GrowArgs G, DevPyramid P,
                                                  uint32_t *word, unsigned long long *flags)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Cell e = frontier[i];
    const float px = (e.x - G.px) / G.size, py = (e.y - G.py) / G.size, pz = (e.z - G.pz) / G.size;
    const float low = d_bound(P, P.lo, px, pz, G.level);
    const float high = d_bound(P, P.hi, px, pz, G.level);
    uint32_t w, br = 0, tw = 0;
    if (high < e.y) {
        w = node_make(EMPTY, 0);
    } else if (low > e.y + G.edge) {
        w = node_make(LEAF, d_height_material(py));
    } else {
        const bool coarse_brick = G.coarse_depth != 0 && G.level == G.coarse_depth - TWIG_LEVELS &&
            !(e.x + G.edge >= G.rmin[0] && e.y + G.edge >= G.rmin[1] && e.z + G.edge >= G.rmin[2] &&
              G.rmax[0] >= e.x && G.rmax[1] >= e.y && G.rmax[2] >= e.z);
        if (G.level == G.depth - TWIG_LEVELS || coarse_brick) { w = node_make(TWIG, 0); tw = 1; }
        else { w = node_make(BRANCH, 0); br = 1; }
    }
    word[i] = w;
    flags[i] = (unsigned long long)br | ((unsigned long long)tw << 32);
}

// Bricks (src/Octree.cpp:122-147), one thread per (brick, z-row): the row's four column heights are looked up with
// the reference's float operations (one lookup per column serves its four y-layers, :131-144), then the row's 16
// cells (index z*16 + y*4 + x) go out as one 32-byte store.  4 threads per brick, 128 B per brick contiguous.
__global__ __launch_bounds__(256) void k_bricks_rows(const Cell *jobs, uint32_t n, GrowArgs G, DevPyramid P, uint16_t *twig)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n * 4u) return;
    const uint32_t j = i >> 2, z = i & 3u;
    const Cell e = jobs[j];
    const float px = (e.x - G.px) / G.size, py = (e.y - G.py) / G.size, pz = (e.z - G.pz) / G.size;
    const float voxel = G.edge / (float)(1 << TWIG_LEVELS);
    const float dz = ((float)z * voxel) / G.size;
    const uint32_t mat = d_height_material(py);
    float h[4];
#pragma unroll
    for (uint32_t x = 0; x < 4; ++x) {
        const float dx = ((float)x * voxel) / G.size;
        h[x] = d_bound(P, P.hi, px + dx, pz + dz, G.level + TWIG_LEVELS);
    }
    uint32_t w[8];                                   // cells (y, x) of this z-row: index y*4 + x, two per dword
#pragma unroll
    for (uint32_t y = 0; y < 4; ++y) {
        const float floor_y = e.y + (float)y * voxel;
        const uint32_t c0 = (h[0] >= floor_y) ? mat : 0u, c1 = (h[1] >= floor_y) ? mat : 0u;
        const uint32_t c2 = (h[2] >= floor_y) ? mat : 0u, c3 = (h[3] >= floor_y) ? mat : 0u;
        w[2 * y] = c0 | (c1 << 16);
        w[2 * y + 1] = c2 | (c3 << 16);
    }
    uint4 *dst = reinterpret_cast<uint4 *>(twig + (uint64_t)e.slot * TWIG_WORDS + z * 16);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

} // namespace

// One chunk column's pyramid on the device.
struct DevicePyramidBuilder {
    DevBuf<float> lo, hi;
    DevPyramid view{};
    int build(const ColumnPyramid &a, hipStream_t s)
    {
        uint32_t levels = 0;
        while ((1u << levels) < a.res) ++levels;
        const size_t total = HeightPyramid::level_offset(levels + 1);
        int rc;
        if ((rc = lo.reserve(total, false, s)) != SVO_OK || (rc = hi.reserve(total, false, s)) != SVO_OK) return rc;
        float *blo = lo.p + HeightPyramid::level_offset(levels), *bhi = hi.p + HeightPyramid::level_offset(levels);
        hipLaunchKernelGGL(k_noise_base, dim3(blocks_for((uint64_t)a.res * a.res, 256)), dim3(256), 0, s, blo, bhi, a.res, a.period, a.xshift, a.zshift);
        for (uint32_t lv = levels; lv > 0; --lv) {
            const uint32_t sdim = 1u << lv;
            hipLaunchKernelGGL(k_mip_level, dim3(blocks_for((uint64_t)(sdim / 2) * (sdim / 2), 256)), dim3(256), 0, s,
                               lo.p + HeightPyramid::level_offset(lv), hi.p + HeightPyramid::level_offset(lv),
                               lo.p + HeightPyramid::level_offset(lv - 1), hi.p + HeightPyramid::level_offset(lv - 1), sdim);
        }
        HIP_TRY(hipGetLastError());
        view.lo = lo.p; view.hi = hi.p; view.size = a.res; view.levels = levels; view.amplitude = a.amplitude; view.shift = a.yshift;
        return SVO_OK;
    }
};

// ---- Ocroot::build / Ocroot::destroy on the device (src/Octree.cpp:320-436 / :203-318; terrain.cpp's Filler is build's host twin) ----
// The reference edits depth-first in child-slot order and APPENDS as it goes: a node the region cuts - EMPTY for build, LEAF for
// destroy - becomes a BRANCH whose 8-block lands at the pool's tail (a "split"), or - at the brick level - a TWIG whose brick
// lands at the brick pool's tail.  So the index a new block / brick gets is the number of splits / new bricks that precede it
// in depth-first preorder.  Three level-synchronous sweeps over the nodes the region touches give exactly that:
//   A (top-down)   k_fill_classify: what the visit does at each node (its action), the 8 children of every node the visit
//                  descends into appended to the next level's list (any order: the lists only link parents to children)
//   B (bottom-up)  k_fill_count: splits / new bricks in each node's subtree
//   C (top-down)   k_fill_number: preorder prefix of those counts = each event's index; node words written, new blocks
//                  initialised (EMPTY for build, the split LEAF's material for destroy), brick edits listed for k_brick_edit
// A node the edit creates has no slot until sweep C: until its parent numbers it, its list entry carries FILL_VIRTUAL and what
// the reference would read there (EMPTY, or LEAF + material).
enum FillAction : uint32_t { FILL_NONE = 0, FILL_SET, FILL_NEW_BRICK, FILL_SPLIT, FILL_BRICK, FILL_DESCEND };
static_assert(FILL_DESCEND < (1u << FILL_ACTION_BITS), "every FillAction fits fill_pack's action field");
enum EditOp : uint32_t { EDIT_BUILD = 0, EDIT_DESTROY = 1 };
constexpr uint32_t FILL_VIRTUAL = 0x80000000u, FILL_VIRTUAL_LEAF = 0x00010000u;

// The region of an edit: two predicates over a node's or a brick cell's closed box [l, h] - touch for cubesIntersect(box, region),
// inside for cube_is_inside(region, box).  The sweeps see the region nowhere else.
struct BoxRegion {              // the closed box [lo, hi]
    float lo[3], hi[3];
    // cubesIntersect on closed boxes (src/Traverse.cpp:173-178), the host Filler's expressions
    __device__ bool touch(float lx, float ly, float lz, float hx, float hy, float hz) const
    {
        return hx >= lo[0] && hy >= lo[1] && hz >= lo[2] && hi[0] >= lx && hi[1] >= ly && hi[2] >= lz;
    }
    // cubeIsInside (src/Traverse.cpp:180-185)
    __device__ bool inside(float lx, float ly, float lz, float hx, float hy, float hz) const
    {
        return lx >= lo[0] && ly >= lo[1] && lz >= lo[2] && hi[0] >= hx && hi[1] >= hy && hi[2] >= hz;
    }
};
struct BallRegion {             // the closed ball |p - c| <= radius, r2 = radius * radius (include/svo.h: svo_world_edit_ball)
    float c[3], r2;
    // distance from c to the box [l, h] along one axis: 0 between the faces
    __device__ static float gap(float l, float h, float p)
    {
        float d = l - p;
        if (!(d > 0.0f)) { d = p - h; if (!(d > 0.0f)) d = 0.0f; }
        return d;
    }
    // distance from c to the box's farther face along one axis
    __device__ static float reach(float l, float h, float p)
    {
        const float u = p - l, v = h - p;
        return (u < v) ? v : u;
    }
    __device__ bool touch(float lx, float ly, float lz, float hx, float hy, float hz) const
    {
        const float dx = gap(lx, hx, c[0]), dy = gap(ly, hy, c[1]), dz = gap(lz, hz, c[2]);
        return dx * dx + dy * dy + dz * dz <= r2;
    }
    // the box's farthest corner lies in the ball
    __device__ bool inside(float lx, float ly, float lz, float hx, float hy, float hz) const
    {
        const float fx = reach(lx, hx, c[0]), fy = reach(ly, hy, c[1]), fz = reach(lz, hz, c[2]);
        return fx * fx + fy * fy + fz * fz <= r2;
    }
};

struct FillArgs {
    float edge;                 // node edge at this level
    uint32_t level, maxlevel;   // maxlevel = depth - TWIG_LEVELS: nodes cut there become bricks
    uint32_t material;          // build: what the region is filled with
    uint32_t op;                // EDIT_BUILD / EDIT_DESTROY
};

// act[i] = fill_pack(action, kids) (kids = index of the node's child block in the next level's list; svo_format.h)
template <class Region>
__global__ __launch_bounds__(FILL_BLOCK) void k_fill_classify(const Cell *cells, uint32_t n, FillArgs F, Region R, const uint32_t *tree,
                                                              uint32_t *act, Cell *next, uint32_t *counters /* [0] child blocks, [1] brick edits */)
{
    __shared__ uint32_t sh[FILL_BLOCK / 64 + 1];
    const uint32_t i = blockIdx.x * FILL_BLOCK + threadIdx.x;
    const bool live = i < n;
    const Cell e = live ? cells[i] : Cell{ 0.0f, 0.0f, 0.0f, 0u };
    const float hx = e.x + F.edge, hy = e.y + F.edge, hz = e.z + F.edge;
    uint32_t a = FILL_NONE, word = node_make(EMPTY, 0);
    const bool touch = live && R.touch(e.x, e.y, e.z, hx, hy, hz);
    if (touch) {
        if (!(e.slot & FILL_VIRTUAL)) word = tree[e.slot];
        else if (e.slot & FILL_VIRTUAL_LEAF) word = node_make(LEAF, e.slot & 0xFFFFu);
        const bool inside = R.inside(e.x, e.y, e.z, hx, hy, hz);
        const uint32_t type = node_type(word);
        if (F.op == EDIT_BUILD) {           // buildCube, src/Octree.cpp:338-430
            if (type == EMPTY) a = inside ? FILL_SET : (F.level == F.maxlevel ? FILL_NEW_BRICK : FILL_SPLIT);
            else if (type == TWIG) a = FILL_BRICK;
            else if (type == BRANCH) a = FILL_DESCEND;
        } else {                            // destroyCube, src/Octree.cpp:220-312: whatever lies inside goes, LEAF nodes the region cuts are split
            if (type == EMPTY) a = FILL_NONE;
            else if (inside) a = FILL_SET;
            else if (type == LEAF) a = F.level == F.maxlevel ? FILL_NEW_BRICK : FILL_SPLIT;
            else if (type == TWIG) a = FILL_BRICK;
            else a = FILL_DESCEND;
        }
    }
    const bool has_kids = a == FILL_SPLIT || a == FILL_DESCEND;
    const uint32_t kids = block_take<FILL_BLOCK>(&counters[0], has_kids, sh);
    if (has_kids) {
        const float half = F.edge * 0.5f;
        const uint32_t first = node_offset(word);
        const uint32_t inherit = FILL_VIRTUAL | (F.op == EDIT_DESTROY ? FILL_VIRTUAL_LEAF | (node_offset(word) & 0xFFFFu) : 0u);
#pragma unroll
        for (uint32_t c = 0; c < 8; ++c) {
            const float ox = (c & 1) ? 1.0f : 0.0f, oy = (c & 2) ? 1.0f : 0.0f, oz = (c & 4) ? 1.0f : 0.0f;
            Cell ch; ch.x = e.x + ox * half; ch.y = e.y + oy * half; ch.z = e.z + oz * half;
            ch.slot = a == FILL_DESCEND ? first + c : inherit;
            next[8 * (uint64_t)kids + c] = ch;
        }
    }
    (void)block_take<FILL_BLOCK>(&counters[1], a == FILL_NEW_BRICK || a == FILL_BRICK, sh);
    if (live) act[i] = fill_pack(a, has_kids ? kids : 0u);
}

// cnt[i] = {splits, new bricks} in the subtree of node i, itself included
__global__ __launch_bounds__(256) void k_fill_count(const uint32_t *act, uint32_t n, const uint2 *cnt_next, uint2 *cnt)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t a = fill_action(act[i]), kids = fill_kids(act[i]);
    uint2 v = make_uint2(a == FILL_SPLIT ? 1u : 0u, a == FILL_NEW_BRICK ? 1u : 0u);
    if (a == FILL_SPLIT || a == FILL_DESCEND) {
#pragma unroll
        for (uint32_t c = 0; c < 8; ++c) { const uint2 k = cnt_next[8 * (uint64_t)kids + c]; v.x += k.x; v.y += k.y; }
    }
    cnt[i] = v;
}

struct DevBrickOp { uint64_t brick; float x, y, z, voxel; uint32_t fresh, init; };     // fresh: a brick this edit appends, every cell starts as `init`

// On entry cnt[i] = {splits, new bricks} that precede node i's own events in preorder (the root: 0, 0); the node's children
// get theirs (their subtree counts are replaced by the running prefix), new nodes get their slots, node words are written.
__global__ __launch_bounds__(FILL_BLOCK) void k_fill_number(Cell *cells, uint32_t n, FillArgs F, const uint32_t *act, const uint2 *cnt,
                                                            Cell *next, uint2 *cnt_next, uint32_t trees0, uint32_t twigs0,
                                                            uint32_t *tree, DevBrickOp *ops, uint32_t *op_cursor)
{
    __shared__ uint32_t sh[FILL_BLOCK / 64 + 1];
    const uint32_t i = blockIdx.x * FILL_BLOCK + threadIdx.x;
    const bool live = i < n;
    const uint32_t a = live ? fill_action(act[i]) : (uint32_t)FILL_NONE, kids = live ? fill_kids(act[i]) : 0u;
    const uint32_t op_slot = block_take<FILL_BLOCK>(op_cursor, a == FILL_NEW_BRICK || a == FILL_BRICK, sh);     // (any order: k_brick_edit treats the ops alike)
    if (a == FILL_NONE) return;
    const Cell e = cells[i];                // (its slot is a real one by now: the parent's turn came a launch earlier)
    const uint2 base = cnt[i];
    switch (a) {
    case FILL_SET:
        tree[e.slot] = F.op == EDIT_BUILD ? node_make(LEAF, F.material) : node_make(EMPTY, 0);
        break;
    case FILL_NEW_BRICK:
    case FILL_BRICK: {
        const uint32_t word = tree[e.slot];
        DevBrickOp op;
        op.fresh = a == FILL_NEW_BRICK ? 1u : 0u;
        op.init = F.op == EDIT_DESTROY ? node_offset(word) & 0xFFFFu : 0u;        // Octwig(material of the LEAF that is cut) / Octwig(0)
        if (a == FILL_NEW_BRICK) { op.brick = twigs0 + base.y; tree[e.slot] = node_make(TWIG, (uint32_t)op.brick); }
        else op.brick = node_offset(word);
        op.x = e.x; op.y = e.y; op.z = e.z; op.voxel = F.edge / (float)(1 << TWIG_LEVELS);
        ops[op_slot] = op;
        break;
    }
    default: {
        uint2 run = base;
        uint32_t first = 0, inherit = node_make(EMPTY, 0);
        if (a == FILL_SPLIT) {
            if (F.op == EDIT_DESTROY) inherit = tree[e.slot];                     // 8 LEAF children of the same material
            first = trees0 + 8u * base.x;
            tree[e.slot] = node_make(BRANCH, first);
            run.x += 1;
        }
#pragma unroll
        for (uint32_t c = 0; c < 8; ++c) {
            const uint64_t k = 8 * (uint64_t)kids + c;
            if (a == FILL_SPLIT) { tree[first + c] = inherit; next[k].slot = first + c; }
            const uint2 sub = cnt_next[k];
            cnt_next[k] = run;
            run.x += sub.x; run.y += sub.y;
        }
    }
    }
}

// The brick half of both edits (src/Octree.cpp:395-410 / :285-300): build - a cell that is empty and whose voxel box touches the
// region takes the material; destroy - a cell whose voxel box touches the region is emptied (the region's touch on closed boxes).
template <class Region>
__global__ __launch_bounds__(256) void k_brick_edit(uint16_t *twig, const DevBrickOp *ops, uint32_t n, uint32_t edit, Region R, uint32_t material)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n * 64u) return;
    const DevBrickOp op = ops[i >> 6];
    const uint32_t cell = i & 63u, cx = cell & 3u, cy = (cell >> 2) & 3u, cz = cell >> 4;
    uint16_t *p = twig + op.brick * TWIG_WORDS + cell;
    const uint32_t before = op.fresh ? op.init : (uint32_t)*p;
    const float lx = op.x + (float)cx * op.voxel, ly = op.y + (float)cy * op.voxel, lz = op.z + (float)cz * op.voxel;
    const float hx = lx + op.voxel, hy = ly + op.voxel, hz = lz + op.voxel;
    const bool touch = R.touch(lx, ly, lz, hx, hy, hz);
    uint32_t after = before;
    if (edit == EDIT_BUILD) { if (before == 0u && touch) after = material; }
    else if (touch) after = 0u;
    if (op.fresh || after != before) *p = (uint16_t)after;
}

struct DeviceFiller {
    struct Level { DevBuf<Cell> cells; DevBuf<uint32_t> act; DevBuf<uint2> cnt; uint32_t n = 0; };
    std::vector<Level> lv;
    DevBuf<uint32_t> counters;      // [2 * level + {0, 1}] of sweep A, [64] the op cursor of sweep C
    DevBuf<DevBrickOp> ops;
    Pinned<uint32_t> h_counters;

    // Ocroot::build (edit = EDIT_BUILD: region R filled with `material`) or Ocroot::destroy (EDIT_DESTROY: emptied) applied
    // to the chunk in `tree` (trees nodes) and `twig` (twigs bricks) whose frame - position, size, depth - is c's; both buffers grow
    // as needed, the capacities cap = { tree, twig } follow the reference's doubling.
    template <class Region>
    int fill(const ChunkPools &c, uint64_t cap[2], const Region &R, uint32_t material, DevBuf<uint32_t> &tree, uint64_t &trees,
             DevBuf<uint16_t> &twig, uint64_t &twigs, hipStream_t s, uint32_t edit)
    {
        int rc;
        const uint32_t maxlevel = c.depth - TWIG_LEVELS;
        if (lv.size() < maxlevel + 2) lv.resize(maxlevel + 2);
        if ((rc = counters.reserve(80, false, s)) != SVO_OK) return rc;
        if ((rc = h_counters.alloc(80)) != SVO_OK) return rc;
        HIP_TRY(hipMemsetAsync(counters.p, 0, 80 * sizeof(uint32_t), s));
        FillArgs F{};
        F.maxlevel = maxlevel; F.material = material; F.op = edit;
        // sweep A
        if ((rc = lv[0].cells.reserve(1, false, s)) != SVO_OK) return rc;
        const Cell root = { c.position[0], c.position[1], c.position[2], 0u };
        HIP_TRY(hipMemcpyAsync(lv[0].cells.p, &root, sizeof root, hipMemcpyHostToDevice, s));
        lv[0].n = 1;
        float edge = c.size;
        uint32_t last = 0, brick_edits = 0;
        std::vector<float> edges(maxlevel + 1);
        for (uint32_t level = 0; level <= maxlevel; ++level) {
            Level &L = lv[level], &N = lv[level + 1];
            const uint32_t n = L.n;
            edges[level] = edge;
            last = level;
            if ((rc = L.act.reserve(n, false, s)) != SVO_OK || (rc = L.cnt.reserve(n, false, s)) != SVO_OK ||
                (rc = N.cells.reserve((uint64_t)n * 8, false, s)) != SVO_OK) return rc;
            F.level = level; F.edge = edge;
            hipLaunchKernelGGL(k_fill_classify<Region>, dim3(blocks_for(n, FILL_BLOCK)), dim3(FILL_BLOCK), 0, s, L.cells.p, n, F, R, tree.p, L.act.p, N.cells.p, counters.p + 2 * level);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(h_counters.p, counters.p + 2 * level, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            brick_edits += h_counters.p[1];
            // (also what fill_pack can hold: child-block indices stay below FILL_KIDS_LIMIT = 2^28)
            if ((uint64_t)h_counters.p[0] >= FILL_KIDS_LIMIT) { set_error("device builder: the fill's frontier exceeds 2^31 nodes"); return SVO_ERR_UNSUPPORTED; }
            N.n = h_counters.p[0] * 8u;
            edge = edge * 0.5f;
            if (N.n == 0) break;
            // a node at maxlevel is never split and grow() puts no BRANCH there
            if (level == maxlevel) { set_error("device builder: BRANCH below level depth-2"); return SVO_ERR_MALFORMED_TREE; }
        }
        // sweep B
        for (int level = (int)last; level >= 0; --level) {
            Level &L = lv[(size_t)level], &N = lv[(size_t)level + 1];
            hipLaunchKernelGGL(k_fill_count, dim3(blocks_for(L.n, 256)), dim3(256), 0, s, L.act.p, L.n, N.cnt.p, L.cnt.p);
        }
        HIP_TRY(hipGetLastError());
        uint2 total;
        HIP_TRY(hipMemcpyAsync(h_counters.p, lv[0].cnt.p, sizeof(uint2), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        total.x = h_counters.p[0]; total.y = h_counters.p[1];
        const uint64_t trees1 = trees + 8ull * total.x, twigs1 = twigs + total.y;
        if (trees1 >= (1ull << 30) || twigs1 >= (1ull << 30)) { set_error("device builder: chunk exceeds the 30-bit node offset"); return SVO_ERR_UNSUPPORTED; }
        if ((rc = tree.reserve(trees1, true, s)) != SVO_OK || (rc = twig.reserve(std::max<uint64_t>(twigs1, 1) * TWIG_WORDS, true, s)) != SVO_OK ||
            (rc = ops.reserve(std::max<uint32_t>(brick_edits, 1u), false, s)) != SVO_OK) return rc;
        if (total.y) HIP_TRY(hipMemsetAsync(twig.p + twigs * TWIG_WORDS, 0, (size_t)total.y * TWIG_WORDS * sizeof(uint16_t), s));
        HIP_TRY(hipMemsetAsync(lv[0].cnt.p, 0, sizeof(uint2), s));
        // sweep C
        for (uint32_t level = 0; level <= last; ++level) {
            Level &L = lv[level], &N = lv[level + 1];
            F.level = level; F.edge = edges[level];
            hipLaunchKernelGGL(k_fill_number, dim3(blocks_for(L.n, FILL_BLOCK)), dim3(FILL_BLOCK), 0, s, L.cells.p, L.n, F, L.act.p, L.cnt.p, N.cells.p, N.cnt.p,
                               (uint32_t)trees, (uint32_t)twigs, tree.p, ops.p, counters.p + 64);
        }
        if (brick_edits)
            hipLaunchKernelGGL(k_brick_edit<Region>, dim3(blocks_for((uint64_t)brick_edits * 64, 256)), dim3(256), 0, s, twig.p, ops.p, brick_edits, edit,
                               R, material);
        HIP_TRY(hipGetLastError());
        // capacity bookkeeping of the reference's appends (src/Octree.cpp:349-351,365-368; terrain.cpp's Filler)
        if (total.x) while (trees1 >= cap[0]) cap[0] *= 2;
        while (twigs1 > cap[1]) cap[1] *= 2;
        trees = trees1; twigs = twigs1;
        return SVO_OK;
    }
};

struct DeviceGrower {
    DevBuf<uint32_t> tree;
    DevBuf<uint16_t> twig;
    uint64_t hint_tree = 1024, hint_twig = 0;   // what the previous chunk needed: the next one starts there instead of doubling its way up

    // grow() (bfs_grow over the arrays B) and - if the terrain has water - Ocroot::build behind it, both on the device.  Node words and
    // bricks stay in HBM: tree_dev / bricks_dev receive the device arrays, c.trees_on_device / c.twigs_on_device their lengths; the
    // host copies are fetched on request (device.hip: fetch_pools).
    int grow(ChunkPools &c, const float position[3], float size, uint32_t depth, const DevPyramid &P, const TerrainParams &tp, hipStream_t s,
             BfsArrays &B, DeviceFiller &filler, DevBuf<uint32_t> &tree_dev, DevBuf<uint16_t> &bricks_dev)
    {
        c.position[0] = position[0]; c.position[1] = position[1]; c.position[2] = position[2];
        c.size = size; c.depth = depth;
        uint64_t trees = 1, twigs = 0, cap[2] = { 16, 16 };
        int rc;
        if ((rc = tree.reserve(hint_tree, false, s)) != SVO_OK || (hint_twig && (rc = twig.reserve(hint_twig, false, s)) != SVO_OK)) return rc;
        GrowArgs G{};
        G.px = position[0]; G.py = position[1]; G.pz = position[2]; G.size = size; G.depth = depth;
        const bool coarse = tp.coarse_depth >= TWIG_LEVELS && tp.coarse_depth < depth;
        G.coarse_depth = coarse ? tp.coarse_depth : 0;
        for (int a = 0; a < 3; ++a) { G.rmin[a] = tp.refine_min[a]; G.rmax[a] = tp.refine_max[a]; }
        rc = bfs_grow<float>(B, Cell{ position[0], position[1], position[2], 0u }, size, trees, twigs, tree.p, s,
            [&](uint32_t level, float edge, const Cell *frontier, uint32_t n, uint32_t *word, unsigned long long *flags) -> int {
                if (level >= 32) { set_error("device builder: more than 32 levels"); return SVO_ERR_UNSUPPORTED; }
                G.level = level; G.edge = edge;
                hipLaunchKernelGGL(k_classify, dim3(blocks_for(n, 256)), dim3(256), 0, s, frontier, n, G, P, word, flags);
                return SVO_OK;
            },
            [&](uint64_t nb, uint64_t nt) -> int {
                if (trees + 8 * nb >= (1ull << 30) || twigs + nt >= (1ull << 30)) { set_error("device builder: chunk exceeds the 30-bit node offset"); return SVO_ERR_UNSUPPORTED; }
                // capacity bookkeeping exactly as the host builder (src/Octree.cpp:149-150,160-161)
                if (nb) while (trees + 8 * nb >= cap[0]) cap[0] *= 2;
                while (twigs + nt > cap[1]) cap[1] *= 2;
                const int r = tree.reserve(trees + 8 * nb, true, s);
                return r != SVO_OK ? r : twig.reserve((twigs + nt) * TWIG_WORDS, true, s);
            },
            [&](const Cell *jobs, uint32_t nt) { hipLaunchKernelGGL(k_bricks_rows, dim3(blocks_for((uint64_t)nt * 4, 256)), dim3(256), 0, s, jobs, nt, G, P, twig.p); });
        if (rc != SVO_OK) return rc;
        if (tp.water) {     // World::g_chunk, src/World.cpp:316-320: everything of the chunk below the water level
            const BoxRegion R = { { position[0], position[1], position[2] }, { position[0] + size, tp.water_level, position[2] + size } };
            if ((rc = filler.fill(c, cap, R, tp.water_material, tree, trees, twig, twigs, s, EDIT_BUILD)) != SVO_OK) return rc;
        }
        c.tree_capacity = cap[0]; c.twig_capacity = cap[1];
        c.tree.clear(); c.twig.clear();
        c.trees_on_device = trees;
        c.twigs_on_device = twigs;
        hint_tree = std::max<uint64_t>(hint_tree, tree.cap); hint_twig = std::max<uint64_t>(hint_twig, twig.cap);
        tree_dev = std::move(tree); bricks_dev = std::move(twig);   // hand the arrays over; the next chunk gets fresh ones
        return SVO_OK;
    }
};

// The builders and their working buffers.  svo_world_shift, the edits, compact / coarsen and the grid calls keep one between calls on
// an uploaded world (created by the first of them, freed with the device copy) - a few hundred MB for depth-12 chunks, DESIGN.md §6o
// has the figures - so that an interactive caller's edits and slides do not pay some forty hipMalloc / hipFree each.
struct BuilderContext {
    DevicePyramidBuilder pyr;
    DeviceGrower grower;
    DeviceFiller filler;
    BfsArrays bfs;                          // the grower's and grid.hip's level arrays
    DevBuf<uint32_t> edit_tree;             // the pools an edit, compact / coarsen or the grid writes before they are installed
    DevBuf<uint16_t> edit_twig;
    LodScratch lod;
    GridScratch grid;
};
static BuilderContext &builder_context(svo_world &w)
{
    if (!w.builder_ctx) w.builder_ctx = new BuilderContext();
    return *static_cast<BuilderContext *>(w.builder_ctx);
}
BfsArrays &bfs_arrays(svo_world &w) { return builder_context(w).bfs; }
LodScratch &lod_scratch(svo_world &w) { return builder_context(w).lod; }
GridScratch &grid_scratch(svo_world &w) { return builder_context(w).grid; }
int edit_scratch(svo_world &w, uint64_t trees, uint64_t twigs, uint32_t **tree, uint16_t **twig)
{
    BuilderContext &ctx = builder_context(w);
    int rc;
    if ((rc = ctx.edit_tree.reserve(std::max<uint64_t>(trees, 1), false, nullptr)) != SVO_OK ||
        (rc = ctx.edit_twig.reserve(std::max<uint64_t>(twigs, 1) * TWIG_WORDS, false, nullptr)) != SVO_OK) return rc;
    *tree = ctx.edit_tree.p; *twig = ctx.edit_twig.p;
    return SVO_OK;
}

// A chunk of a terrain window grown on the device with its device arrays (node words, bricks); a GrownWindow lists them in walk
// order, and a failure on the way frees whatever was grown.
struct GrownChunk { ChunkPools meta; int index = 0; DevBuf<uint32_t> tree_dev; DevBuf<uint16_t> twig_dev; };
using GrownWindow = std::vector<GrownChunk>;

// World::g_pyramid + g_chunk (src/World.cpp:296-321) on the device for every chunk of `win`, a column's pyramid built once.
static int grow_window(const TerrainWindow &win, const TerrainParams &tp, BuilderContext &ctx, hipStream_t s, GrownWindow &out)
{
    for (int k = 0; k < win.size(); ++k) {
        const TerrainWindow::Chunk at = win.chunk(k);
        int rc;
        if (k % win.column_height() == 0 && (rc = ctx.pyr.build(column_pyramid(tp, at.x, at.z), s)) != SVO_OK) return rc;
        GrownChunk &e = out.emplace_back();
        e.index = at.index;
        if ((rc = ctx.grower.grow(e.meta, at.position, (float)win.chunksize, tp.depth, ctx.pyr.view, tp, s, ctx.bfs, ctx.filler, e.tree_dev, e.twig_dev)) != SVO_OK) return rc;
    }
    return SVO_OK;
}

// World::init on the device, pools left in HBM: noise, mips, grow() and the water fill (Ocroot::build) as kernels (above).
// Neither node words nor bricks visit the host (fetched on request: device.hip, fetch_pools).  The pools are packed exactly as
// svo_world_upload packs them; the world is uploaded to `device` when this returns.
static int generate_world_resident_impl(svo_world &w, int device)
{
    const bool timing = std::getenv("SVO_BUILD_TIMING") != nullptr;
    auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t0 = now();
    auto lapt = [&](const char *what) { if (timing) { (void)hipDeviceSynchronize(); const double t1 = now(); std::fprintf(stderr, "[svo build] %-28s %.1f ms\n", what, (t1 - t0) * 1e3); t0 = t1; } };
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("svo_world_generate: no HIP device for the device builder"); return SVO_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) { set_error("svo_world_generate: build_device out of range"); return SVO_ERR_INVALID_ARG; }
    HIP_TRY(hipSetDevice(device));
    w.chunks.assign((size_t)w.width * w.height * w.depth, ChunkPools());
    GrownWindow grown;
    hipStream_t s = nullptr;
    {
        BuilderContext ctx;                 // (its buffers are gone before the pools are allocated)
        const int rc = grow_window(TerrainWindow::whole(w.width, w.height, w.depth, w.chunksize, w.chunkcoordmin), w.terrain, ctx, s, grown);
        if (rc != SVO_OK) return rc;
        lapt("noise + mips + grow + fill");
    }
    for (const GrownChunk &e : grown) w.chunks[(size_t)e.index] = e.meta;
    // pack: the layout of svo_world_upload
    plan_pools(w);
    int rc = alloc_pools(w, device);
    if (rc != SVO_OK) return rc;
    lapt("alloc pools");
    for (const GrownChunk &e : grown)
        if ((rc = copy_chunk(w, e.index, e.tree_dev.p, e.twig_dev.p, hipMemcpyDeviceToDevice, 0, e.meta.trees_on_device, 0, e.meta.twigs_on_device, s)) != SVO_OK) return rc;
    HIP_TRY(hipMemcpyAsync(w.hbm->chunks.p, w.table.data(), w.chunks.size() * sizeof(DevChunk), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    grown.clear();
    lapt("pack + masks");
    const bool literal_only = build_wide_all(w, s) != SVO_OK;         // (a complete world either way: see svo_world_upload)
    lapt("wide trees");
    HIP_TRY(hipDeviceSynchronize());
    return literal_only ? SVO_OK_LITERAL_ONLY : SVO_OK;
}

void free_builder_context(svo_world &w)
{
    delete static_cast<BuilderContext *>(w.builder_ctx);
    w.builder_ctx = nullptr;
}

// World::shift (src/World.cpp:334-378) on an uploaded world: the plane of chunks entering the grid is generated on the device
// the pools live on (grow_window, with the builders the world keeps) and takes the slots of the plane that leaves -
// the toroidal index of a chunk coordinate does not depend on chunkcoordmin -, then chunkcoordmin moves.
static int shift_world_resident_impl(svo_world &w, int axis, int sign)
{
    HIP_TRY(hipSetDevice(w.device));
    BuilderContext &ctx = builder_context(w);
    // The whole entering plane is generated before any of it is installed: a failure on the way (device memory, mostly) leaves
    // the world as it was.  Once the installs have begun they all happen and chunkcoordmin moves - no launch sees a grid whose
    // slots hold chunks of two positions of the window ("none sees a mixture", svo.h); a wide tree that could not be rebuilt on
    // the way only takes the stack kernel away (SVO_OK_LITERAL_ONLY).
    GrownWindow plane;
    int rc = grow_window(TerrainWindow::whole(w.width, w.height, w.depth, w.chunksize, w.chunkcoordmin).entering(axis, sign), w.terrain, ctx, nullptr, plane);
    if (rc != SVO_OK) return rc;
    int status = SVO_OK;
    for (const GrownChunk &e : plane) {
        rc = install_resident_chunk(w, e.index, e.meta, e.tree_dev.p, e.twig_dev.p);
        if (rc < 0) return rc;                      // a HIP failure in the middle of the copies: the device is in no state to go on with
        if (rc != SVO_OK) status = rc;
    }
    w.chunkcoordmin[axis] += sign;
    return status;
}

int shift_world_resident(svo_world &w, int axis, int sign) { return fenced("svo_world_shift", [&] { return shift_world_resident_impl(w, axis, sign); }); }

// Ocroot::build / destroy / replace + World::modify (src/Octree.cpp:203-443, src/World.cpp:268-274; the caller's pattern is
// src/Main.cpp:340-367) on an uploaded world, without the host: the chunk's pools are copied out of the packed pools, edited by
// the three sweeps above and installed again with svo_world_update's slot logic.  A host copy of the chunk, if there was one,
// is dropped (svo_world_chunk fetches the edited pools on request).
template <class Region>
static int edit_resident_impl(svo_world &w, int chunk, int op, const Region &R, uint32_t material)
{
    HIP_TRY(hipSetDevice(w.device));
    HIP_TRY(hipDeviceSynchronize());              // ordered behind every launch issued before it, like svo_world_update
    hipStream_t s = nullptr;
    const ChunkPools &c = w.chunks[(size_t)chunk];
    const DevChunk &e = w.table[(size_t)chunk];
    uint64_t trees = c.tree_count(), twigs = c.twig_count();
    BuilderContext &ctx = builder_context(w);
    DevBuf<uint32_t> &tree = ctx.edit_tree;
    DevBuf<uint16_t> &twig = ctx.edit_twig;
    int rc;
    if ((rc = tree.reserve(trees + 1024, false, s)) != SVO_OK || (rc = twig.reserve((twigs + 16) * TWIG_WORDS, false, s)) != SVO_OK) return rc;
    HIP_TRY(hipMemcpyAsync(tree.p, w.hbm->tree.p + e.tree_off, trees * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    if (twigs) HIP_TRY(hipMemcpyAsync(twig.p, w.hbm->twig.p + e.twig_off * TWIG_WORDS, twigs * TWIG_WORDS * sizeof(uint16_t), hipMemcpyDeviceToDevice, s));
    uint64_t cap[2] = { c.tree_capacity, c.twig_capacity };
    if (op == SVO_EDIT_DESTROY || op == SVO_EDIT_REPLACE)
        if ((rc = ctx.filler.fill(c, cap, R, material, tree, trees, twig, twigs, s, EDIT_DESTROY)) != SVO_OK) return rc;
    if (op == SVO_EDIT_BUILD || op == SVO_EDIT_REPLACE)
        if ((rc = ctx.filler.fill(c, cap, R, material, tree, trees, twig, twigs, s, EDIT_BUILD)) != SVO_OK) return rc;
    return install_rebuilt(w, chunk, c.depth, cap, trees, twigs, tree.p, twig.p);
}

int edit_box_resident(svo_world &w, int chunk, int op, const float lo[3], const float hi[3], uint32_t material)
{
    const BoxRegion R = { { lo[0], lo[1], lo[2] }, { hi[0], hi[1], hi[2] } };
    return fenced("svo_world_edit_box", [&] { return edit_resident_impl(w, chunk, op, R, material); });
}

// The same edit with the closed ball |p - centre| <= radius as its region (svo_world_edit_ball).
int edit_ball_resident(svo_world &w, int chunk, int op, const float centre[3], float radius, uint32_t material)
{
    const BallRegion R = { { centre[0], centre[1], centre[2] }, radius * radius };
    return fenced("svo_world_edit_ball", [&] { return edit_resident_impl(w, chunk, op, R, material); });
}

int generate_world_resident(svo_world &w, int device)
{
    const int rc = fenced("svo_world_generate (device builder)", [&] { return generate_world_resident_impl(w, device); });
    if (rc < 0) release_device(w);
    return rc;
}

} // namespace svo
