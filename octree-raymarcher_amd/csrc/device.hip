// device.hip — device half of the C ABI: HBM residency of a world and the trace launches.
//
//   svo_world_upload  <- World::load_gpu + RootAllocator::alloc   src/World.cpp:57-94, src/Allocator.cpp:28-35
//   svo_world_update  <- World::modify + RootAllocator::subst     src/World.cpp:268-274, src/Allocator.cpp:37-55
//   svo_trace*        <- World::draw / draw_shadowmap             src/World.cpp:162-266
//   svo_world_locate  <- traverse over a point list               src/Traverse.cpp:34-48 (locate.hip.h)
//   svo_hit_ao        <- (none: the reference has no ambient occlusion)                    (ao.hip.h)
//   svo_trace_reflections <- (none: the reference has no reflections)                      (reflect.hip.h)
//   svo_trace_instances   <- (none: the reference's one moving object is a rasterised mesh, src/Worm.cpp)   (instances.hip.h)
//
// The reference's first-fit free-list allocator over GL buffers is not reproduced: a world is
// packed into one flat pool per kind with per-chunk slots sized by the chunk's host capacity
// (the reference also sizes GPU slots by capacity, src/Allocator.cpp:30-33), and a chunk that
// outgrows its slot moves to the pool tail.
//
// No CPU fallback: every entry point fails with SVO_ERR_NO_DEVICE / SVO_ERR_HIP when HIP does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "kernel_literal.hip.h"
#include "kernel_stack.hip.h"
#include "see_through.hip.h"
#include "local_shadows.hip.h"
#include "light_list.hip.h"
#include "instances.hip.h"
#include "reflect.hip.h"
#include "shadowmap.hip.h"
#include "locate.hip.h"
#include "ao.hip.h"
#include "hit_voxels.hip.h"
#include "hip_own.h"
#include "wide_tree.hip.h"
#include "light_clearance.hip.h"

using namespace svo;

namespace svo {

// bit w of mask[b] = (brick b cell w != 0).  One thread per 16-byte eighth of a brick (8 cells -> one mask byte):
// 16 B per lane, fully coalesced reads of the twig pool, byte stores into the little-endian uint64 masks.  The eight lanes of
// a brick also agree on bmat[b]: the brick's material if all its non-empty cells hold the same one (what grow() produces), 0 for an
// empty brick, 0xFFFF if it holds several (the hit block then reads the cell itself).  Bit 15 is the brick's clear flag
// (light_clearance.hip.h k_clear_bricks), written 0 here: a rebuilt chunk has none; a brick of one material of 0x8000 and above is
// stored as 0xFFFF, which is right and only slower for such a brick.
__global__ __launch_bounds__(256) void k_brick_masks(const uint16_t *twig, uint64_t *mask, uint16_t *bmat, uint64_t first, uint64_t count)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;      // eighth-of-brick index
    const bool live = i < count * 8;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (live) v = reinterpret_cast<const uint4 *>(twig + first * TWIG_WORDS)[i];
    const uint32_t w[4] = { v.x, v.y, v.z, v.w };
    uint32_t bits = 0, lo = 0xFFFFu, hi = 0u;                       // smallest / largest non-zero material of this eighth
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t a = w[k] & 0xFFFFu, b = w[k] >> 16;
        bits |= (a ? 1u : 0u) << (2 * k);
        bits |= (b ? 1u : 0u) << (2 * k + 1);
        if (a) { lo = a < lo ? a : lo; hi = a > hi ? a : hi; }
        if (b) { lo = b < lo ? b : lo; hi = b > hi ? b : hi; }
    }
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) {                                   // the brick's eight lanes are neighbours (256 % 8 == 0)
        const uint32_t lo2 = __shfl_xor(lo, d, 64), hi2 = __shfl_xor(hi, d, 64);
        lo = lo2 < lo ? lo2 : lo; hi = hi2 > hi ? hi2 : hi;
    }
    if (!live) return;
    reinterpret_cast<uint8_t *>(mask + first)[i] = (uint8_t)bits;
    if ((i & 7u) == 0u) bmat[first + (i >> 3)] = (uint16_t)(hi == 0u ? 0u : (lo == hi && lo < BMAT_CLEAR_BIT ? lo : BMAT_SEVERAL));
}

// svo_tile_order: key = primary + shadow step maxima of the tile (saturating), value = the tile's index
__global__ __launch_bounds__(256) void k_tile_keys(const uint32_t *cost, uint32_t *keys, uint32_t *idx, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t a = cost[2 * i], b = cost[2 * i + 1];
    keys[i] = a + b < a ? 0xFFFFFFFFu : a + b;
    idx[i] = (uint32_t)i;
}

// ---- the large device buffers of a world (tree, brick, mask, material, wide pools, the wide builder's scratch) -------------
// A caller that replaces its world - destroy + generate, a re-pack after an edit outgrew the pools - asks for the sizes it has
// just given back.  hipFree + hipMalloc of multi-GB buffers is not free on every runtime (on the development pool a hipMalloc
// behind a large hipFree stalled for ~4 s about once in ten 12-GB cycles, scripts/alloc_probe.py), so buffers of 1 MiB and more
// go to a small per-process cache instead of back to the driver and are handed out again to requests they fit (best fit, at
// most 25 % + 1 MiB larger than asked for).  At most POOL_CACHE_SLOTS buffers are held; svo_device_cache_trim() returns them.
constexpr size_t POOL_CACHE_SLOTS = 8, POOL_CACHE_MIN = 1u << 20;
struct PoolBuf { void *p; size_t bytes; int device; };
static std::mutex g_pool_mutex;
static std::vector<PoolBuf> g_pool_cache;                   // what pool_free has kept

hipError_t pool_malloc(void **out, size_t *asked, int device)
{
    const size_t bytes = *asked ? *asked : 1;
    *asked = bytes;
    {
        std::lock_guard<std::mutex> lock(g_pool_mutex);
        size_t best = g_pool_cache.size();
        for (size_t i = 0; i < g_pool_cache.size(); ++i) {
            const PoolBuf &b = g_pool_cache[i];
            if (b.device == device && b.bytes >= bytes && b.bytes <= bytes + bytes / 4 + POOL_CACHE_MIN && (best == g_pool_cache.size() || b.bytes < g_pool_cache[best].bytes)) best = i;
        }
        if (best != g_pool_cache.size()) {
            *out = g_pool_cache[best].p;
            *asked = g_pool_cache[best].bytes;
            g_pool_cache.erase(g_pool_cache.begin() + (long)best);
            return hipSuccess;
        }
    }
    hipError_t e = hipMalloc(out, bytes);
    if (e != hipSuccess) {                                  // the cache may be what stands in the way: give it back and try once more
        svo_device_cache_trim();
        e = hipMalloc(out, bytes);
    }
    if (e != hipSuccess) *out = nullptr;
    return e;
}
void pool_free(void *p, size_t bytes, int device)
{
    if (!p) return;
    const PoolBuf b{ p, bytes, device };
    void *evict = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_pool_mutex);
        if (b.bytes >= POOL_CACHE_MIN) {
            if (g_pool_cache.size() >= POOL_CACHE_SLOTS) {  // full: the smallest buffer makes room (the large ones are the expensive ones)
                size_t small = 0;
                for (size_t i = 1; i < g_pool_cache.size(); ++i) if (g_pool_cache[i].bytes < g_pool_cache[small].bytes) small = i;
                if (g_pool_cache[small].bytes < b.bytes) { evict = g_pool_cache[small].p; g_pool_cache[small] = b; }
                else evict = p;
            } else g_pool_cache.push_back(b);
        } else evict = p;
    }
    if (evict) (void)hipFree(evict);
}

// the see-through view (see_through.hip.h) and the continuation scratch: every change to the pools drops the view
static void drop_view(svo_world &w)
{
    if (w.hbm->view_wide.p || w.hbm->view_mask.p) (void)hipDeviceSynchronize();
    w.hbm->view_wide = Pooled<uint32_t>(); w.hbm->view_mask = Pooled<uint64_t>(); w.hbm->view_material = 0;
}

// the parent index (hit_voxels.hip.h): every change to the pools drops it, the next svo_hit_voxels call builds it again
static void drop_parents(svo_world &w)
{
    Hbm &d = *w.hbm;
    if (d.parent.p || d.parent_level.p || d.chunk_trees.p) (void)hipDeviceSynchronize();
    d.parent = Pooled<uint32_t>(); d.parent_level = Pooled<uint8_t>(); d.chunk_trees = DevBuf<uint32_t>();
    d.parents_ok = false;
}

int release_device(svo_world &w, bool keep_builder)
{
    if (w.hbm) {
        (void)hipSetDevice(w.device);
        drop_view(w);
        drop_parents(w);
        if (!keep_builder) free_builder_context(w);
        (void)hipDeviceSynchronize();                       // the large buffers may be handed to another world at once: nothing may still use them
        delete w.hbm;
        w.hbm = nullptr;
    }
    w.device = -1;
    w.table.clear(); w.tree_slot.clear(); w.twig_slot.clear(); w.wtable.clear(); w.wide_slot.clear();
    w.tree_pool_len = w.twig_pool_len = w.tree_pool_cap = w.twig_pool_cap = 0;
    w.wide_pool_len = w.wide_pool_cap = 0;
    return SVO_OK;
}

} // namespace svo

extern "C" {

int svo_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void *svo_device_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) { set_error("svo_device_alloc: hipMalloc failed"); return nullptr; }
    return p;
}
void svo_device_free(void *p) { if (p) (void)hipFree(p); }
void svo_device_cache_trim(void)
{
    std::vector<PoolBuf> out;
    { std::lock_guard<std::mutex> lock(g_pool_mutex); out.swap(g_pool_cache); }
    int cur = 0;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    for (const PoolBuf &b : out) { (void)hipSetDevice(b.device); (void)hipFree(b.p); }
    if (have) (void)hipSetDevice(cur);
}
int svo_memcpy_h2d(void *dst, const void *src, size_t bytes) { HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return SVO_OK; }
int svo_memcpy_d2h(void *dst, const void *src, size_t bytes) { HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return SVO_OK; }
int svo_stream_synchronize(void *stream) { HIP_TRY(hipStreamSynchronize((hipStream_t)stream)); return SVO_OK; }

} // extern "C"

namespace svo {

// the base of a tree slot at or behind `len` node words: base % 8 == 7, so that the 8-blocks behind a chunk's root are 8-aligned
static uint64_t tail_slot(uint64_t len) { return ((len + 8) & ~(uint64_t)7) - 1; }

// slots: capacity-sized like the reference (src/Allocator.cpp:30-33), 8-node / 1-brick granular, plus tail slack so that a
// chunk that outgrows its slot can be re-packed without a full re-upload
void plan_pools(svo_world &w)
{
    const size_t n = w.chunks.size();
    w.table.assign(n, DevChunk());
    w.wtable.assign(n, DevWide());
    w.tree_slot.assign(n, 0); w.twig_slot.assign(n, 0); w.wide_slot.assign(n, 0);
    uint64_t tcur = 0, bcur = 0;
    for (size_t i = 0; i < n; ++i) {
        const ChunkPools &c = w.chunks[i];
        const uint64_t tcap = std::max<uint64_t>(c.tree_capacity, c.tree_count());
        const uint64_t bcap = std::max<uint64_t>(c.twig_capacity, c.twig_count());
        const uint64_t base = tail_slot(tcur);
        DevChunk &e = w.table[i];
        e.bmin[0] = c.position[0]; e.bmin[1] = c.position[1]; e.bmin[2] = c.position[2];
        e.levels = c.depth - TWIG_LEVELS;
        e.tree_off = base;
        e.twig_off = bcur;
        w.tree_slot[i] = tcap; w.twig_slot[i] = bcap;
        tcur = base + tcap;
        bcur += bcap;
    }
    w.tree_pool_len = tcur; w.twig_pool_len = bcur;
    w.tree_pool_cap = tcur + tcur / 4 + 64;
    w.twig_pool_cap = bcur + bcur / 4 + 16;
}

int alloc_pools(svo_world &w, int device)
{
    if (hipSetDevice(device) != hipSuccess) { set_error("svo_world_upload: hipSetDevice failed"); return SVO_ERR_NO_DEVICE; }
    Hbm &d = *(w.hbm = new Hbm());                                     // (both callers start from a released world: nothing is replaced)
    w.device = device;
    const size_t n = w.chunks.size();
    if (d.tree.alloc(w.tree_pool_cap, device) != hipSuccess ||
        d.twig.alloc(w.twig_pool_cap * TWIG_WORDS, device) != hipSuccess ||
        d.mask.alloc(w.twig_pool_cap, device) != hipSuccess ||
        d.bmat.alloc(w.twig_pool_cap, device) != hipSuccess ||
        d.chunks.reserve(n, false, nullptr) != SVO_OK ||
        d.wchunks.reserve(n, false, nullptr) != SVO_OK ||
        d.work.reserve(WORK_SLOTS * WORK_SLOT_WORDS, false, nullptr) != SVO_OK) {
        set_error("svo_world_upload: hipMalloc failed"); return SVO_ERR_OUT_OF_MEMORY;
    }
    if (hipMemset(d.tree.p, 0, w.tree_pool_cap * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(d.mask.p, 0, w.twig_pool_cap * sizeof(uint64_t)) != hipSuccess ||
        hipMemset(d.bmat.p, 0, w.twig_pool_cap * sizeof(uint16_t)) != hipSuccess ||
        hipMemset(d.work.p, 0, WORK_SLOTS * WORK_SLOT_WORDS * sizeof(unsigned long long)) != hipSuccess) { set_error("svo_world_upload: hipMemset failed"); return SVO_ERR_HIP; }
    w.wide_ok = false;                                                  // until build_wide_all has run
    return SVO_OK;
}

// (world.h) host vectors are copied synchronously out of pageable memory, device buffers in order on `stream`
int copy_chunk(svo_world &w, int i, const uint32_t *tree, const uint16_t *twig, hipMemcpyKind kind,
               uint64_t tl, uint64_t tr, uint64_t bl, uint64_t br, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const DevChunk &e = w.table[(size_t)i];
    auto copy = [&](void *dst, const void *src, size_t bytes) {
        return kind == hipMemcpyDeviceToDevice ? hipMemcpyAsync(dst, src, bytes, kind, s) : hipMemcpy(dst, src, bytes, kind);
    };
    if (tl < tr) HIP_TRY(copy(w.hbm->tree.p + e.tree_off + tl, tree + tl, (tr - tl) * sizeof(uint32_t)));
    if (bl >= br) return SVO_OK;
    HIP_TRY(copy(w.hbm->twig.p + (e.twig_off + bl) * TWIG_WORDS, twig + bl * TWIG_WORDS, (br - bl) * TWIG_WORDS * sizeof(uint16_t)));
    return launch_per_element("brick masks", (int64_t)(br - bl) * 8, s, k_brick_masks, w.hbm->twig.p, w.hbm->mask.p, w.hbm->bmat.p, e.twig_off + bl, br - bl);
}

// A chunk built on the device keeps its node words and bricks there until somebody asks for the host copy.
int fetch_pools(svo_world &w, int chunk)
{
    ChunkPools &c = w.chunks[(size_t)chunk];
    if (!c.twigs_on_device && !c.trees_on_device) return SVO_OK;
    if (!w.hbm || !w.hbm->twig.p || !w.hbm->tree.p) { set_error("fetch_pools: the device copy is gone"); return SVO_ERR_NOT_UPLOADED; }
    HIP_TRY(hipSetDevice(w.device));
    if (c.trees_on_device) {
        const uint64_t n = c.trees_on_device;
        c.tree.resize(n);
        HIP_TRY(hipMemcpy(c.tree.data(), w.hbm->tree.p + w.table[(size_t)chunk].tree_off, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        c.trees_on_device = 0;
    }
    if (c.twigs_on_device) {
        const uint64_t n = c.twigs_on_device;
        c.twig.resize(n * TWIG_WORDS);
        HIP_TRY(hipMemcpy(c.twig.data(), w.hbm->twig.p + w.table[(size_t)chunk].twig_off * TWIG_WORDS, n * TWIG_WORDS * sizeof(uint16_t), hipMemcpyDeviceToHost));
        c.twigs_on_device = 0;
    }
    return SVO_OK;
}

// The wide-tree builder's scratch for a chunk of at most B BRANCH nodes (= wide nodes a level can have): the two fronts, the flags and
// ranks of a level's entries (64 per wide node), the entry references, a throw-away wide tree of B nodes and its bases (the count
// pass of expand_into_scratch), then the scan's own scratch - kept 256-byte aligned: what precedes it is rounded up to 64 words.
// Every offset grows with B: a scratch laid out for a larger chunk serves a smaller one as it is (reserve_wide_scratch).
static WideLayout wide_layout(uint64_t B, size_t scan_bytes)
{
    WideLayout L;
    L.next = B; L.flag = L.next + B; L.rank = L.flag + 64 * B; L.wref = L.rank + 64 * B; L.wide = L.wref + 64 * B; L.wbase = L.wide + 64 * B;
    L.scan = ((L.wbase + WIDE_BASE_WORDS * B + 1024 + 63) / 64) * 64;
    L.scan_words = (scan_bytes + 3) / 4 + 64; L.total = L.scan + L.scan_words;
    return L;
}

// The wide tree of chunk `chunk` (wide_tree.hip.h) from its node words in the tree pool, level by level, into
// wide_dst / wbase_dst (room for slot_cap wide nodes); *count = wide nodes written.  The per-entry reference indices that link
// one level to the next live in the builder's scratch, which reserve_wide_scratch has laid out for this chunk or a larger one.
// (results of this file's wide-tree helpers that are not svo_status values: they never leave this file)
constexpr int WIDE_SLOT_FULL = 100;     // expand_wide_chunk: the chunk's wide tree does not fit slot_cap
constexpr int WIDE_POOL_LIMIT = 101;    // build_wide_all's grow_pool: the pool would need 2^32 wide nodes or more (the literal kernel marches)
static int expand_wide_chunk(svo_world &w, int chunk, hipStream_t s, uint32_t *wide_dst, uint32_t *wbase_dst, uint64_t slot_cap, uint64_t *count_out)
{
    Hbm &d = *w.hbm;
    const ChunkPools &c = w.chunks[(size_t)chunk];
    const DevChunk &e = w.table[(size_t)chunk];
    const uint32_t levels = c.depth - TWIG_LEVELS;
    const uint32_t nw = levels == 0 ? 1u : (levels + 1u) / 2u;
    const int pad = (int)(2u * nw - levels);
    const uint64_t B = c.tree_count() / 8 + 1;                          // most BRANCH nodes (= wide nodes) a level can have
    const WideLayout &L = d.wlayout;
    uint32_t *const ws = d.wscratch.p;
    uint32_t *front = ws, *next = ws + L.next, *flag = ws + L.flag, *rank = ws + L.rank, *wref_dst = ws + L.wref;
    const uint32_t *tree = d.tree.p + e.tree_off;
    HIP_TRY(hipMemsetAsync(front, 0, sizeof(uint32_t), s));             // the top wide node expands reference node 0
    if (d.wide_tail.alloc(2) != SVO_OK) { set_error("wide tree: hipHostMalloc failed"); return SVO_ERR_OUT_OF_MEMORY; }
    uint32_t count = 1, first = 0;
    // the scan's own scratch lies behind the builder's (sized for the largest level): no hipMalloc / hipFree per chunk
    void *tmp = ws + L.scan;
    const size_t tmp_bytes = L.scan_words * sizeof(uint32_t);
    int rc = SVO_OK;
    for (uint32_t k = 0; k < nw && count > 0; ++k) {
        if ((uint64_t)first + count > slot_cap) { rc = WIDE_SLOT_FULL; break; }      // (the callers turn this into a larger slot, or into an error)
        const uint32_t n = count * 64u;
        hipLaunchKernelGGL(k_wide_expand, dim3((n + 255) / 256), dim3(256), 0, s, tree, front, count, first,
                           k == 0 ? pad : 0, 2u * k + 1u - (uint32_t)pad, wide_dst, wref_dst, wbase_dst, flag);
        if (hipGetLastError() != hipSuccess) { set_error("wide tree: launch failed"); rc = SVO_ERR_HIP; break; }
        if (k + 1 == nw) { first += count; count = 0; break; }         // grandchildren of the last wide level are never BRANCH
        size_t bytes = 0;
        if (hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, flag, rank, (int)n, s) != hipSuccess) { rc = SVO_ERR_HIP; break; }
        if (bytes > tmp_bytes) { set_error("wide tree: the scan asks for more scratch than was reserved"); rc = SVO_ERR_HIP; break; }
        uint32_t *tail = d.wide_tail.p;                                 // pinned: a pageable destination stages every 4-byte copy
        if (hipcub::DeviceScan::ExclusiveSum(tmp, bytes, flag, rank, (int)n, s) != hipSuccess ||
            hipMemcpyAsync(&tail[0], rank + (n - 1), 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(&tail[1], flag + (n - 1), 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) { set_error("wide tree: scan failed"); rc = SVO_ERR_HIP; break; }
        const uint32_t total = tail[0] + tail[1];
        if ((uint64_t)total > B) { set_error("wide tree: more BRANCH nodes than the tree can hold"); rc = SVO_ERR_MALFORMED_TREE; break; }
        if (total) {
            hipLaunchKernelGGL(k_wide_link, dim3((n + 255) / 256), dim3(256), 0, s, count, first, first + count, flag, rank, wide_dst, wref_dst, next);
            if (hipGetLastError() != hipSuccess) { rc = SVO_ERR_HIP; break; }
        }
        first += count; count = total;
        std::swap(front, next);
    }
    (void)hipStreamSynchronize(s);
    if (rc == SVO_OK && count_out) *count_out = first;
    return rc;
}

// scratch for the builder (wide_layout) of a chunk of `trees` node words; one that is large enough already is kept as it is laid out
static int reserve_wide_scratch(svo_world &w, uint64_t trees)
{
    Hbm &d = *w.hbm;
    const uint64_t B = trees / 8 + 1;
    size_t scan_bytes = 0;
    uint32_t *nul = nullptr;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, nul, nul, (int)(64 * B), (hipStream_t)nullptr) != hipSuccess) { set_error("wide tree: scan size query failed"); return SVO_ERR_HIP; }
    const WideLayout L = wide_layout(B, scan_bytes);
    if (L.scan_words <= d.wlayout.scan_words && L.scan <= d.wlayout.scan) return SVO_OK;
    if (d.wscratch.p) { (void)hipDeviceSynchronize(); d.wscratch = Pooled<uint32_t>(); d.wlayout = WideLayout(); }
    if (d.wscratch.alloc(L.total, w.device) != hipSuccess) { set_error("wide tree: hipMalloc of the builder scratch failed"); return SVO_ERR_OUT_OF_MEMORY; }
    d.wlayout = L;
    return SVO_OK;
}
static bool wide_fits(const svo_world &w, int chunk)
{
    const ChunkPools &c = w.chunks[(size_t)chunk];
    // (a wide entry keeps its reference node's level in 5 bits; WIDE_MAX_LEVELS branch levels, i.e. chunk depth <= 24, are marched)
    // and the builder scans one level's entries (64 per wide node) with 32-bit counts: < 2^31 entries per chunk
    return c.depth - TWIG_LEVELS <= WIDE_MAX_LEVELS && c.twig_count() <= (uint64_t)WIDE_PAYLOAD_MASK && (c.tree_count() / 8 + 1) * 64 < (1ull << 31);
}

static void drop_wide(svo_world &w)
{
    drop_view(w);
    if (w.hbm->clear.prepared()) drop_clearance(w);
    if (w.hbm->wide.p || w.hbm->wbase.p) (void)hipDeviceSynchronize();
    w.hbm->wide = Pooled<uint32_t>(); w.hbm->wbase = Pooled<uint32_t>();
    w.wide_ok = false;
    w.wide_pool_len = w.wide_pool_cap = w.wide_nodes_used = 0;
}
static void drop_wide_scratch(svo_world &w, bool failed = true)
{
    // after a successful rebuild an interactive caller (one that has edited or slid the world: builder_ctx) keeps the scratch for
    // the next one; everybody else gets the ~1 GB back
    if (!failed && w.builder_ctx) return;
    if (w.hbm->wscratch.p) { (void)hipDeviceSynchronize(); w.hbm->wscratch = Pooled<uint32_t>(); }
    w.hbm->wlayout = WideLayout();
}
// the failure exit of a wide-tree build: no wide pool (the literal kernel marches the world) and no scratch
static int wide_failed(svo_world &w, int rc, const char *why = nullptr)
{
    drop_wide(w); drop_wide_scratch(w);
    if (why) set_error(why);
    return rc;
}

// Chunk `chunk`'s wide tree into the throw-away tree of the builder's scratch, reserved for this chunk first (room for all
// its BRANCH nodes: *wide / *wbase, *count wide nodes)
static int expand_into_scratch(svo_world &w, int chunk, hipStream_t s, uint32_t **wide, uint32_t **wbase, uint64_t *count)
{
    const uint64_t trees = w.chunks[(size_t)chunk].tree_count(), B = trees / 8 + 1;
    int rc = reserve_wide_scratch(w, trees);
#ifdef SVO_TEST_HOOKS
    // (the `hooks` variant only) SVO_TEST_FAIL_WIDE=1 makes the wide-tree build fail as an allocation failure would
    const char *fail = std::getenv("SVO_TEST_FAIL_WIDE");
    if (rc == SVO_OK && fail && fail[0] == '1') { set_error("wide tree: injected allocation failure"); rc = SVO_ERR_OUT_OF_MEMORY; }
#endif
    if (rc != SVO_OK) return rc;
    *wide = w.hbm->wscratch.p + w.hbm->wlayout.wide; *wbase = w.hbm->wscratch.p + w.hbm->wlayout.wbase;
    rc = expand_wide_chunk(w, chunk, s, *wide, *wbase, B, count);
    if (rc == WIDE_SLOT_FULL) { set_error("wide tree: more wide nodes than BRANCH nodes"); rc = SVO_ERR_MALFORMED_TREE; }
    return rc;
}

// a chunk's entry of the stack kernel's table: its frame from the chunk table, its top wide node at wide_off
static DevWide wide_entry(const DevChunk &e, uint32_t wide_off)
{
    return DevWide{ { e.bmin[0], e.bmin[1], e.bmin[2] }, e.levels, wide_off, 0u, e.twig_off };
}

// Wide trees of every chunk from the node words, which must already be in the tree pool.
int build_wide_all(svo_world &w, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const size_t n = w.chunks.size();
    // wide_ok says "the wide pool is complete": false from here until the build pass has succeeded, so that a failure
    // on the way (scratch or pool allocation, a malformed tree) leaves a world the literal kernel marches, never a
    // stack kernel reading a null or half-written pool
    drop_wide(w);
    bool fits = true;
    size_t sample = 0;                                                  // the chunk with the most nodes stands for all of them
    for (size_t i = 0; i < n; ++i) {
        if (w.chunks[i].tree_count() > w.chunks[sample].tree_count()) sample = i;
        if (!wide_fits(w, (int)i)) fits = false;
    }
    w.wtable.assign(n, DevWide()); w.wide_slot.assign(n, 0);
    if (!fits) return SVO_OK;                                           // the literal kernel marches such a world
    // One pass (until round 4 every chunk was expanded twice: a count pass into scratch sized the pool, a build pass filled it): the
    // largest chunk is counted, the pool is sized from its wide nodes per BRANCH node (+ 35 %) for all chunks, and every chunk is built in
    // place behind the previous one's slot (= its wide nodes + 1/8 + 16); a pool that turns out too small is grown (x 1.5, copied):
    // entries hold wide-node indices relative to their chunk's top node, so a built chunk can move.
    uint64_t count0 = 0;
    uint32_t *tmp_wide, *tmp_wbase;
    int rc = expand_into_scratch(w, (int)sample, s, &tmp_wide, &tmp_wbase, &count0);
    if (rc != SVO_OK) return wide_failed(w, rc);
    Hbm &d = *w.hbm;
    uint64_t branches = 0;
    for (size_t i = 0; i < n; ++i) branches += w.chunks[i].tree_count() / 8 + 1;
    const double per_branch = (double)count0 / (double)(w.chunks[sample].tree_count() / 8 + 1);
    uint64_t cap = (uint64_t)((double)branches * per_branch * 1.35) + 32 * n + 64;
    cap = std::max<uint64_t>(cap, count0 + count0 / 8 + 16 + 64);
#ifdef SVO_TEST_HOOKS
    // (the `hooks` variant only) SVO_TEST_WIDE_ESTIMATE=<factor> scales the estimate, so that the tests reach the growth path
    if (const char *e = std::getenv("SVO_TEST_WIDE_ESTIMATE")) cap = std::max<uint64_t>(64, (uint64_t)((double)cap * std::atof(e)));
#endif
    auto alloc_pool = [&](uint64_t nodes, Pooled<uint32_t> &wide, Pooled<uint32_t> &wbase) {
        if (nodes >= (1ull << 32)) return false;
        if (wide.alloc(nodes * 64, w.device) != hipSuccess) return false;
        if (wbase.alloc(nodes * WIDE_BASE_WORDS, w.device) != hipSuccess) { wide = Pooled<uint32_t>(); return false; }
        return true;
    };
    if (cap >= (1ull << 32)) return wide_failed(w, SVO_OK);                   // wide node indices are 32-bit (1 TiB of wide nodes): literal kernel
    if (!alloc_pool(cap, d.wide, d.wbase)) return wide_failed(w, SVO_ERR_OUT_OF_MEMORY, "wide tree: hipMalloc of the pool failed");
    uint64_t cur = 0, used = 0;
    auto grow_pool = [&](uint64_t at_least) -> int {
        uint64_t bigger = std::max<uint64_t>(cap + cap / 2, at_least + at_least / 16 + 64);
        if (bigger >= (1ull << 32)) return WIDE_POOL_LIMIT;
        Pooled<uint32_t> nw, nb;
        if (!alloc_pool(bigger, nw, nb)) return SVO_ERR_OUT_OF_MEMORY;
        if (hipMemcpyAsync(nw.p, d.wide.p, cur * 64 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s) != hipSuccess ||
            hipMemcpyAsync(nb.p, d.wbase.p, cur * WIDE_BASE_WORDS * sizeof(uint32_t), hipMemcpyDeviceToDevice, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) return SVO_ERR_HIP;
        d.wide = std::move(nw); d.wbase = std::move(nb); cap = bigger;      // (nw / nb take the old pools back to the cache)
        return SVO_OK;
    };
    for (size_t i = 0; i < n; ) {
        uint64_t count = 0;
        rc = expand_wide_chunk(w, (int)i, s, d.wide.p + cur * 64, d.wbase.p + cur * WIDE_BASE_WORDS, cap - cur, &count);
        const uint64_t slot = count + count / 8 + 16;
        if (rc == WIDE_SLOT_FULL || (rc == SVO_OK && cur + slot > cap)) {        // (grow, then this chunk again)
            const uint64_t bound = w.chunks[i].tree_count() / 8 + 1;
            const int g = grow_pool(cur + (rc == SVO_OK ? slot : std::min<uint64_t>(bound, 2 * (cap - cur) + 1024)));
            if (g == WIDE_POOL_LIMIT) return wide_failed(w, SVO_OK);
            if (g != SVO_OK) return wide_failed(w, g, "wide tree: growing the pool failed");
            continue;
        }
        if (rc != SVO_OK) return wide_failed(w, rc);
        w.wtable[i] = wide_entry(w.table[i], (uint32_t)cur);
        w.wide_slot[i] = slot;
        cur += slot;
        used += count;
        ++i;
    }
    if (hipMemcpy(d.wchunks.p, w.wtable.data(), n * sizeof(DevWide), hipMemcpyHostToDevice) != hipSuccess)
        return wide_failed(w, SVO_ERR_HIP, "wide tree: chunk table copy failed");
    w.wide_pool_len = cur; w.wide_pool_cap = cap; w.wide_nodes_used = used;
    w.wide_ok = true;
    // the builder's scratch (fronts, flags, ranks and a throw-away tree of the largest chunk: ~1 GB at C3) is only needed
    // here and by svo_world_update, which re-reserves what the edited chunk needs
    (void)hipStreamSynchronize(s);
    drop_wide_scratch(w, false);
    return SVO_OK;
}

// One chunk again after an edit: in place if its wide tree still fits the slot, at the pool's tail if that has room,
// otherwise everything is rebuilt.
int rebuild_wide_chunk(svo_world &w, int chunk, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (!w.wide_ok || !wide_fits(w, chunk)) return build_wide_all(w, stream);
    // any failure below leaves the chunk's old wide tree in the pool while tree[] has changed: the pool is dropped
    // (wide_ok = false) and the literal kernel takes over until a full rebuild succeeds
    uint64_t count = 0;
    uint32_t *tmp_wide, *tmp_wbase;
    const int rc = expand_into_scratch(w, chunk, s, &tmp_wide, &tmp_wbase, &count);
    if (rc != SVO_OK) return wide_failed(w, rc);
    DevWide &v = w.wtable[(size_t)chunk];
    if (count > w.wide_slot[(size_t)chunk]) {
        const uint64_t want = count + count / 4 + 16;
        if (w.wide_pool_len + want > w.wide_pool_cap) { drop_wide_scratch(w); return build_wide_all(w, stream); }
        v.wide_off = (uint32_t)w.wide_pool_len;
        w.wide_slot[(size_t)chunk] = want;
        w.wide_pool_len += want;
    }
    v = wide_entry(w.table[(size_t)chunk], v.wide_off);
    if (hipMemcpyAsync(w.hbm->wide.p + (uint64_t)v.wide_off * 64, tmp_wide, count * 64 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(w.hbm->wbase.p + (uint64_t)v.wide_off * WIDE_BASE_WORDS, tmp_wbase, count * WIDE_BASE_WORDS * sizeof(uint32_t), hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(w.hbm->wchunks.p + chunk, &v, sizeof(DevWide), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) return wide_failed(w, SVO_ERR_HIP, "wide tree: copy of the rebuilt chunk failed");
    drop_wide_scratch(w, false);
    return SVO_OK;
}

static int world_upload_impl(svo_world *w, int device, bool force = false)
{
    if (!w) return SVO_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("svo_world_upload: no HIP device"); return SVO_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) { set_error("svo_world_upload: device index out of range"); return SVO_ERR_INVALID_ARG; }
    // a world generated on this device is already resident there, pools packed exactly as below
    bool resident_only = false;
    for (const ChunkPools &c : w->chunks) resident_only |= c.twigs_on_device != 0 || c.trees_on_device != 0;
    if (resident_only && w->device == device && !force) return SVO_OK;
    // the one layout the pools cannot take, refused while a resident world is still intact
    for (const ChunkPools &c : w->chunks)
        if (c.size != (float)w->chunksize) { set_error("svo_world_upload: every chunk's size must equal chunksize"); return SVO_ERR_UNSUPPORTED; }
    for (size_t i = 0; i < w->chunks.size(); ++i) {                     // moving elsewhere: the host copy must be complete first
        const int rc = fetch_pools(*w, (int)i);
        if (rc != SVO_OK) return rc;
    }
    release_device(*w, w->device == device);                            // a re-pack on the same device keeps the builders' buffers: the caller may be one of them
    plan_pools(*w);
    const size_t n = w->chunks.size();
    int rc = alloc_pools(*w, device);
    for (size_t i = 0; i < n && rc == SVO_OK; ++i) {
        const ChunkPools &c = w->chunks[i];
        rc = copy_chunk(*w, (int)i, c.tree.data(), c.twig.data(), hipMemcpyHostToDevice, 0, c.tree.size(), 0, c.twig_count(), nullptr);
    }
    if (rc != SVO_OK) { release_device(*w); return rc; }
    // the stack kernel's wide trees: a failure here (device memory, mostly) leaves a complete world for the literal kernel
    // (build_wide_all has dropped whatever it had begun), and the caller is told so
    const bool literal_only = build_wide_all(*w, nullptr) != SVO_OK;
    if (hipMemcpy(w->hbm->chunks.p, w->table.data(), n * sizeof(DevChunk), hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        set_error("svo_world_upload: chunk table copy failed"); release_device(*w); return SVO_ERR_HIP;
    }
    return literal_only ? SVO_OK_LITERAL_ONLY : SVO_OK;
}

// Chunk `chunk` of an uploaded world, its host metadata (frame, depth, capacities, counts) already current, into its slots from host
// vectors (node words [tl, tr) and bricks [bl, br) changed) or device buffers (the whole chunk): in place if it fits, an outgrown pool
// at the pools' tail if that has room, otherwise the world is packed again.  Launches of this world may still be in flight on the
// caller's streams, which are not ordered against the copies (a march that reads a half-rewritten tree could follow a stale BRANCH
// chain): like World::modify on the GL queue (src/World.cpp:268-274), the device is drained first.
static int install_chunk(svo_world &w, int chunk, const uint32_t *tree, const uint16_t *twig, hipMemcpyKind kind,
                         uint64_t tl, uint64_t tr, uint64_t bl, uint64_t br)
{
    HIP_TRY(hipSetDevice(w.device));
    HIP_TRY(hipDeviceSynchronize());
    drop_view(w);                                                       // rebuilt from the new pools at the next see-through launch
    drop_parents(w);                                                    // ... and at the next svo_hit_voxels call
    drop_clearance(w);                                                  // ... and only by svo_world_prepare_light
    ChunkPools &c = w.chunks[(size_t)chunk];
    DevChunk &e = w.table[(size_t)chunk];
    const uint64_t trees = c.tree_count(), twigs = c.twig_count();
    const bool tree_fits = trees <= w.tree_slot[(size_t)chunk], twig_fits = twigs <= w.twig_slot[(size_t)chunk];
    const bool trace = std::getenv("SVO_BUILD_TIMING") != nullptr;
    if (trace) std::fprintf(stderr, "[svo install] chunk %d: %s\n", chunk, tree_fits && twig_fits ? "in place" : "outgrew its slot");
    bool table_dirty = e.levels != c.depth - TWIG_LEVELS || e.bmin[0] != c.position[0] || e.bmin[1] != c.position[1] || e.bmin[2] != c.position[2];
    if (!tree_fits || !twig_fits) {
        const uint64_t tbase = tail_slot(w.tree_pool_len);
        const uint64_t need_t = tree_fits ? 0 : c.tree_capacity, need_b = twig_fits ? 0 : c.twig_capacity;
        if ((!tree_fits && tbase + need_t > w.tree_pool_cap) || (!twig_fits && w.twig_pool_len + need_b > w.twig_pool_cap)) {
            // no room: a chunk that lives on the device comes to the host, then everything is fetched and packed afresh
            if (trace) std::fprintf(stderr, "[svo install] chunk %d: no room at the tails, packing the world again\n", chunk);
            if (kind == hipMemcpyDeviceToDevice) {
                c.tree.resize(trees); c.twig.resize(twigs * TWIG_WORDS);
                c.trees_on_device = c.twigs_on_device = 0;
                HIP_TRY(hipMemcpy(c.tree.data(), tree, trees * sizeof(uint32_t), hipMemcpyDeviceToHost));
                if (twigs) HIP_TRY(hipMemcpy(c.twig.data(), twig, twigs * TWIG_WORDS * sizeof(uint16_t), hipMemcpyDeviceToHost));
            }
            const int rc = world_upload_impl(&w, w.device, true);
            if (w.hbm) drop_clearance(w);                               // (the re-pack is part of an edit, not a fresh upload)
            return rc;
        }
        if (!tree_fits) { e.tree_off = tbase; w.tree_slot[(size_t)chunk] = need_t; w.tree_pool_len = tbase + need_t; }
        if (!twig_fits) { e.twig_off = w.twig_pool_len; w.twig_slot[(size_t)chunk] = need_b; w.twig_pool_len += need_b; }
        table_dirty = true;
        tl = 0; tr = trees; bl = 0; br = twigs;                         // a chunk that moved is copied whole, both pools
    }
    e.levels = c.depth - TWIG_LEVELS;
    e.bmin[0] = c.position[0]; e.bmin[1] = c.position[1]; e.bmin[2] = c.position[2];
    int rc = copy_chunk(w, chunk, tree, twig, kind, tl, std::min(tr, trees), bl, std::min(br, twigs), nullptr);
    if (rc != SVO_OK) return rc;
    if (table_dirty) HIP_TRY(hipMemcpy(w.hbm->chunks.p + chunk, &e, sizeof(DevChunk), hipMemcpyHostToDevice));
    // the stack kernel's view of the chunk: rebuilt from the node words now in the pool
    // (the pools and the chunk table already hold the new chunk: a wide tree that cannot be rebuilt - rebuild_wide_chunk has dropped
    // the wide pool then - leaves a world the literal kernel marches, and the caller is told so instead of being told "error"
    // about a change that took effect)
    rc = rebuild_wide_chunk(w, chunk, nullptr);
    HIP_TRY(hipDeviceSynchronize());
    return rc == SVO_OK ? SVO_OK : SVO_OK_LITERAL_ONLY;
}

// A chunk built on the device (World::shift on an uploaded world, the box edit, compact / coarsen: builder.hip, compact.hip) takes
// slot `chunk`: its host copy is dropped (svo_world_chunk fetches the pools on request) and the pools are installed device-to-device.
int install_resident_chunk(svo_world &w, int chunk, const ChunkPools &meta, const uint32_t *tree_dev, const uint16_t *twig_dev)
{
    if (w.device < 0 || chunk < 0 || chunk >= (int)w.chunks.size()) return SVO_ERR_INVALID_ARG;
    ChunkPools &c = w.chunks[(size_t)chunk];
    std::memcpy(c.position, meta.position, sizeof c.position);
    c.size = meta.size; c.depth = meta.depth;
    c.tree_capacity = std::max(c.tree_capacity, meta.tree_capacity);    // (svo_world_update keeps the slot's capacity as the floor too)
    c.twig_capacity = std::max(c.twig_capacity, meta.twig_capacity);
    std::vector<uint32_t>().swap(c.tree);
    std::vector<uint16_t>().swap(c.twig);
    c.trees_on_device = meta.trees_on_device; c.twigs_on_device = meta.twigs_on_device;
    classify_world(w);
    return install_chunk(w, chunk, tree_dev, twig_dev, hipMemcpyDeviceToDevice, 0, c.trees_on_device, 0, c.twigs_on_device);
}

static int world_update_impl(svo_world *w, int chunk, const svo_chunk_desc *desc,
                             uint64_t tree_left, uint64_t tree_right, uint64_t twig_left, uint64_t twig_right, int realloc_)
{
    if (!w || !desc || chunk < 0 || chunk >= (int)w->chunks.size() || !desc->tree || !desc->trees) return SVO_ERR_INVALID_ARG;
    // 1. adopt the edited pools on the host (validated like svo_world_create).
    //    The reference re-sends only the ranges Ocroot::build / destroy report as dirty unless the pools were reallocated
    //    (src/World.cpp:268-274, glBufferSubData); the host copy kept here follows suit when it can - it is current, the chunk's
    //    frame is unchanged, the pools have not shrunk and the caller does not ask for `realloc` - and is patched over the dirty ranges
    //    (and whatever was appended) instead of being replaced: copying a depth-12 chunk's 280 MB took 46 of an update's 64 ms.
    //    Either way the result is validated as a whole before HBM sees any of it, and a patch that fails is taken back.
    ChunkPools &cur = w->chunks[(size_t)chunk];
    const uint64_t old_trees = cur.tree.size(), old_twigs = cur.twig_count();
    const bool patch = !realloc_ && cur.trees_on_device == 0 && cur.twigs_on_device == 0 && old_trees != 0 &&
        desc->trees >= old_trees && desc->twigs >= old_twigs && (desc->twigs == 0 || desc->twig) &&
        std::memcmp(cur.position, desc->position, sizeof cur.position) == 0 && cur.size == desc->size && cur.depth == desc->depth;
    std::string why;
    int rc;
    if (patch) {
        // the ranges that change on the host: the caller's, clamped, widened over what was appended
        uint64_t tl = std::min<uint64_t>(tree_left, desc->trees), tr = std::min<uint64_t>(std::max(tree_right, tree_left), desc->trees);
        uint64_t bl = std::min<uint64_t>(twig_left, desc->twigs), br = std::min<uint64_t>(std::max(twig_right, twig_left), desc->twigs);
        if (desc->trees > old_trees) { tl = std::min(tl, old_trees); tr = desc->trees; }
        if (desc->twigs > old_twigs) { bl = std::min(bl, old_twigs); br = desc->twigs; }
        const uint64_t keep_t = std::min(tr, old_trees), keep_b = std::min(br, old_twigs);          // what a failed patch has to restore
        std::vector<uint32_t> undo_t(cur.tree.begin() + (ptrdiff_t)std::min(tl, keep_t), cur.tree.begin() + (ptrdiff_t)keep_t);
        std::vector<uint16_t> undo_b(cur.twig.begin() + (ptrdiff_t)(std::min(bl, keep_b) * TWIG_WORDS), cur.twig.begin() + (ptrdiff_t)(keep_b * TWIG_WORDS));
        cur.tree.resize(desc->trees);
        cur.twig.resize(desc->twigs * TWIG_WORDS);
        if (tl < tr) std::memcpy(cur.tree.data() + tl, desc->tree + tl, (tr - tl) * sizeof(uint32_t));
        if (bl < br) std::memcpy(cur.twig.data() + bl * TWIG_WORDS, desc->twig + bl * TWIG_WORDS, (br - bl) * TWIG_WORDS * sizeof(uint16_t));
        const uint64_t cap_t0 = cur.tree_capacity, cap_b0 = cur.twig_capacity;
        cur.fit_capacity(cur.tree.size(), cur.twig_count());
        rc = validate_chunk(cur, why);
        if (rc != SVO_OK) {
            cur.tree.resize(old_trees); cur.twig.resize(old_twigs * TWIG_WORDS);
            std::copy(undo_t.begin(), undo_t.end(), cur.tree.begin() + (ptrdiff_t)std::min(tl, keep_t));
            std::copy(undo_b.begin(), undo_b.end(), cur.twig.begin() + (ptrdiff_t)(std::min(bl, keep_b) * TWIG_WORDS));
            cur.tree_capacity = cap_t0; cur.twig_capacity = cap_b0;
            set_error("svo_world_update: " + why); return rc;
        }
        tree_left = tl; tree_right = tr; twig_left = bl; twig_right = br;       // what HBM receives below
    } else {
        ChunkPools next;
        std::memcpy(next.position, desc->position, sizeof next.position);
        next.size = desc->size; next.depth = desc->depth;
        next.tree.assign(desc->tree, desc->tree + desc->trees);
        if (desc->twigs) next.twig.assign(desc->twig, desc->twig + desc->twigs * TWIG_WORDS);
        next.tree_capacity = cur.tree_capacity;
        next.twig_capacity = cur.twig_capacity;
        next.fit_capacity(next.tree.size(), next.twig_count());
        rc = validate_chunk(next, why);
        if (rc != SVO_OK) { set_error("svo_world_update: " + why); return rc; }
        if (next.size != (float)w->chunksize) { set_error("svo_world_update: chunk size must equal chunksize"); return SVO_ERR_UNSUPPORTED; }
        cur.tree.swap(next.tree);
        cur.twig.swap(next.twig);
        cur.twigs_on_device = 0;       // the caller's pools replace whatever lived only on the device
        cur.trees_on_device = 0;
        std::memcpy(cur.position, next.position, sizeof cur.position);
        cur.size = next.size; cur.depth = next.depth;
        cur.tree_capacity = next.tree_capacity; cur.twig_capacity = next.twig_capacity;
        if (realloc_ || desc->trees != old_trees || desc->twigs != old_twigs) { tree_left = 0; tree_right = desc->trees; twig_left = 0; twig_right = desc->twigs; }
    }
    classify_world(*w);
    if (w->device < 0) return SVO_OK;
    // 2. refresh HBM
    return install_chunk(*w, chunk, cur.tree.data(), cur.twig.data(), hipMemcpyHostToDevice, tree_left, tree_right, twig_left, twig_right);
}

} // namespace svo

extern "C" {

// nothing throws across the C ABI: host-side allocations of the two entry points below are fenced here
int svo_world_upload(svo_world *w, int device)
{
    try { return world_upload_impl(w, device); }
    catch (const std::bad_alloc &) { set_error("svo_world_upload: out of host memory"); return SVO_ERR_OUT_OF_MEMORY; }
    catch (...) { set_error("svo_world_upload: unexpected exception"); return SVO_ERR_HIP; }
}

int svo_world_update(svo_world *w, int chunk, const svo_chunk_desc *desc,
                     uint64_t tree_left, uint64_t tree_right, uint64_t twig_left, uint64_t twig_right, int realloc_)
{
    try { return world_update_impl(w, chunk, desc, tree_left, tree_right, twig_left, twig_right, realloc_); }
    catch (const std::bad_alloc &) { set_error("svo_world_update: out of host memory"); return SVO_ERR_OUT_OF_MEMORY; }
    catch (...) { set_error("svo_world_update: unexpected exception"); return SVO_ERR_HIP; }
}

} // extern "C"

namespace svo {

// k_trace_stack's instantiations, by depth class, GLSL before CPU semantics: the large-world instantiation (BIG: 64-bit wide-tree and mask
// addresses, where 32-bit offsets do not reach) in two depth classes - a world that large is built of deep chunks -, the default one in four
constexpr int STACK_REFILL = 8;         // retired lanes per wave that trigger a refill (cheap: rays are staged in LDS)
constexpr int STACK_WAVES = 6;          // waves per SIMD the stack kernel is register-budgeted for: 80 VGPRs (the asm step holds 63; spills sit in the rare blocks)
using StackKernel = void (*)(TraceArgs);
template <int MAXLV, bool BIG, bool GLSL, bool SEG> constexpr StackKernel stack_kernel = k_trace_stack<MAXLV, STACK_REFILL, STACK_WAVES, BIG, GLSL, SEG>;
constexpr int STACK_CLASSES = 12;       // depth class x semantics; the bounded set (svo_trace_segments) follows in the same order
#define STACK_PAIR(MAXLV, BIG, SEG) stack_kernel<MAXLV, BIG, true, SEG>, stack_kernel<MAXLV, BIG, false, SEG>
#define STACK_SET(SEG) STACK_PAIR(10, true, SEG), STACK_PAIR(22, true, SEG), STACK_PAIR(6, false, SEG), STACK_PAIR(10, false, SEG), STACK_PAIR(16, false, SEG), STACK_PAIR(22, false, SEG)
static const StackKernel STACK_KERNELS[] = { STACK_SET(false), STACK_SET(true) };      // launch_stack computes the index
#undef STACK_SET
#undef STACK_PAIR
static_assert(sizeof(STACK_KERNELS) / sizeof(StackKernel) == 2 * STACK_CLASSES, "an unbounded and a bounded instantiation per class");
static_assert(sizeof(STACK_KERNELS) / sizeof(StackKernel) == sizeof(Hbm::stack_blocks) / sizeof(int), "one grid size per instantiation");

} // namespace svo

extern "C" {

// ---------------------------------------------------------------------------------------------
// the world box's minimum on axis a (src/Traverse.cpp:129-133)
static float world_min(const svo_world *w, int a) { return (float)(w->chunkcoordmin[a] * (int)(float)w->chunksize); }
// Where the rays of pixels that have nothing to march start, along -x (k_continuation, k_local_rays): below the world box on y and z
// (by the box's extent), so that the line never meets the box
static V3 miss_ray_origin(const svo_world *w)
{
    const float cs = (float)w->chunksize;
    return V3{ world_min(w, 0), world_min(w, 1) - (float)w->height * cs - cs, world_min(w, 2) - (float)w->depth * cs - cs };
}

// What every entry point refuses in a svo_trace_params (null: the defaults), with the message of `who`.  The entry points differ in
// what they look at before which of these (svo_trace asks for residency between the first and the second, and reads the kernel id
// last of all), so `which` picks the checks of one call; what a call returns when several faults meet is part of the ABI by now.
enum { PRM_SEE_THROUGH = 1, PRM_SEMANTICS = 2, PRM_KERNEL = 4, PRM_ALL = 7 };
static int refuse_params(const char *who, const svo_trace_params *prm, int which = PRM_ALL)
{
    const auto refuse = [who](const char *what) { set_error(std::string(who) + what); return SVO_ERR_INVALID_ARG; };
    if (!prm) return SVO_OK;
    if ((which & PRM_SEE_THROUGH) && prm->see_through > 0xFFFFu) return refuse(": see_through is a 16-bit material");
    if ((which & PRM_SEMANTICS) && prm->semantics != SVO_SEMANTICS_CPU && prm->semantics != SVO_SEMANTICS_GLSL) return refuse(": unknown semantics");
    if ((which & PRM_KERNEL) && prm->kernel != SVO_KERNEL_AUTO && prm->kernel != SVO_KERNEL_LITERAL && prm->kernel != SVO_KERNEL_STACK) return refuse(": unknown kernel id");
    return SVO_OK;
}

// The params of the march a stage issues on a ray list of its own: the caller's, without the per-ray and per-tile buffers (they are
// sized for the caller's frame) and, unless the stage keeps them, without shadow rays
static svo_trace_params own_list_params(const svo_trace_params &prm, bool keep_shadow)
{
    svo_trace_params march = prm;
    if (!keep_shadow) march.shadow = 0;
    march.counters_dev = nullptr; march.tile_cost_dev = nullptr; march.tile_order_dev = nullptr;
    return march;
}

// shadow direction = normalize(-light_dir), glm::normalize semantics; no direction or (0, 0, 0): the reference's light
static void shadow_direction(const float *light_dir, float sdir[3])
{
    float l[3] = { 1.0f, -1.0f, 0.0f };                                  // src/Main.cpp:116 (normalised below)
    if (light_dir && (light_dir[0] != 0.0f || light_dir[1] != 0.0f || light_dir[2] != 0.0f))
        std::memcpy(l, light_dir, sizeof l);
    const float nx = -l[0], ny = -l[1], nz = -l[2];
    const float inv = 1.0f / std::sqrt(nx * nx + ny * ny + nz * nz);
    sdir[0] = nx * inv; sdir[1] = ny * inv; sdir[2] = nz * inv;
}

static int fill_common(svo_world *w, const svo_trace_params *prm, TraceArgs &A)
{
    if (!w) return SVO_ERR_INVALID_ARG;
    if (const int rc = refuse_params("svo_trace", prm, PRM_SEE_THROUGH)) return rc;
    if (w->device < 0) { set_error("svo_trace: world is not uploaded"); return SVO_ERR_NOT_UPLOADED; }
    if (const int rc = refuse_params("svo_trace", prm, PRM_SEMANTICS)) return rc;
    std::memset(&A, 0, sizeof A);
    const float cs = (float)w->chunksize;
    const int dims[3] = { w->width, w->height, w->depth };
    for (int a = 0; a < 3; ++a) {
        A.worldmin[a] = world_min(w, a);
        A.worldmax[a] = (float)(w->chunkcoordmin[a] + dims[a]) * cs;
    }
    A.chunksize = cs;
    A.inv_chunksize = 1.0f / cs;
    A.dimw = w->width; A.dimh = w->height; A.dimd = w->depth;
    for (int a = 0; a < 3; ++a) {
        A.ccm[a] = w->chunkcoordmin[a];
        A.cbase[a] = positive_mod(w->chunkcoordmin[a], dims[a]);
    }
    A.chunks = w->hbm->chunks.p; A.tree = w->hbm->tree.p; A.twig = w->hbm->twig.p; A.mask = w->hbm->mask.p;
    A.wchunks = w->hbm->wchunks.p; A.wide = w->hbm->wide.p; A.wbase = w->hbm->wbase.p; A.bmat = w->hbm->bmat.p;
    const bool glsl = prm && prm->semantics == SVO_SEMANTICS_GLSL;      // defaults: src/Traverse.cpp:8,54,79,142 / shaders/Chunkmarch.glsl:1-3,17
    A.glsl = glsl ? 1 : 0;
    A.eps = (prm && prm->eps != 0.0f) ? prm->eps : (glsl ? 1.0f / 4096.0f : 1.0f / 8192.0f);
    A.cap_chunk = (prm && prm->max_chunk_steps > 0) ? prm->max_chunk_steps : (glsl ? 256 : 1000);
    A.cap_tree = (prm && prm->max_tree_steps > 0) ? prm->max_tree_steps : (glsl ? 512 : 1000);
    A.cap_twig = (prm && prm->max_twig_steps > 0) ? prm->max_twig_steps : (glsl ? 64 : 1000);
    A.guard_eps = glsl ? A.eps : -INFINITY;
    A.leaf_back = glsl ? 0.0f : A.eps;
    A.shadow = (prm && prm->shadow) ? 1 : 0;
    A.normal_mode = (prm && prm->normal_mode == SVO_NORMAL_FACE) ? SVO_NORMAL_FACE : SVO_NORMAL_CUBE;
    shadow_direction(prm ? prm->light_dir : nullptr, A.sdir);
    A.counters = prm ? prm->counters_dev : nullptr;
    A.exact_geometry = w->exact_geometry ? 1 : 0;
    A.tile_cost = prm ? prm->tile_cost_dev : nullptr;
    A.tile_order = prm ? prm->tile_order_dev : nullptr;
    A.work = w->hbm->work.p;                 // the launch picks its slot
    return SVO_OK;
}

// The stack kernel's default instantiation addresses wide-tree entries by a 32-bit byte offset into the wide pool and brick masks by
// a 32-bit byte offset into the mask pool (8 B per brick): pools of 2^30 entries (4 GiB; the benchmark world has 0.2 G) / 2^29 bricks
// and more are marched by the large-world instantiation (64-bit addresses; until round 4 by the literal kernel, 5-17 times slower).
static bool stack_needs_big(const svo_world *w)
{
#ifdef SVO_FORCE_WIDE64
    return true;                    // (the `wide64` variant of the Makefile: the large-world kernel on every world, for the tests)
#else
    return w->wide_pool_cap * 64 >= (1ull << 30) || w->twig_pool_cap >= (1ull << 29);
#endif
}

static int pick_kernel(const svo_world *w, const svo_trace_params *prm, const TraceArgs &A)
{
    if (const int rc = refuse_params("svo_trace", prm, PRM_KERNEL)) return rc;
    const int want = prm ? prm->kernel : SVO_KERNEL_AUTO;
    // (brick indices and wide node indices are 32-bit in the kernel at any size: fewer than 2^32 bricks / wide nodes per world)
    // (... and chunk indices are formed with 24-bit multiplies, kernel_stack.hip.h chunk_index_u24: fewer than 2^24 chunks)
    const bool stack_ok = w->exact_geometry && w->max_levels <= (int)WIDE_MAX_LEVELS && w->wide_ok && w->twig_pool_cap < (1ull << 32) &&
                          (long long)w->width * w->height * w->depth < (1ll << 24);
    if (want == SVO_KERNEL_LITERAL) return SVO_KERNEL_LITERAL;
    if (want == SVO_KERNEL_STACK) {
        if (!stack_ok) { set_error("svo_trace: SVO_KERNEL_STACK needs exact geometry, chunk depth <= 24, fewer than 2^24 chunks and the world's wide trees (svo_world_info.wide_nodes)"); return SVO_ERR_UNSUPPORTED; }
        return SVO_KERNEL_STACK;
    }
    return (stack_ok && !A.counters) ? SVO_KERNEL_STACK : SVO_KERNEL_LITERAL;
}

// Persistent grid = the waves the instantiation can keep resident (occupancy query, once per world and instantiation: they differ in
// LDS), never more than tiles / tiles_per_wave.
static int launch_stack(svo_world *w, const TraceArgs &A, int tiles_per_wave, int in_flight, hipStream_t s)
{
    const int lv = w->max_levels;
    const int depth = stack_needs_big(w) ? (lv <= 10 ? 0 : 1) : lv <= 6 ? 2 : lv <= 10 ? 3 : lv <= 16 ? 4 : 5;
    const int which = 2 * depth + (A.glsl ? 0 : 1) + (A.tmax ? STACK_CLASSES : 0);
    const StackKernel kernel = STACK_KERNELS[which];
    int &resident = w->hbm->stack_blocks[which];
    if (resident <= 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, w->device) != hipSuccess) return SVO_ERR_HIP;
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, 0) != hipSuccess || per_cu <= 0) per_cu = 16;
        resident = prop.multiProcessorCount * per_cu;
#ifdef SVO_TEST_HOOKS
        if (const char *cap = std::getenv("SVO_GRID_WAVES_PER_CU")) { const int c = std::atoi(cap); if (c > 0) resident = prop.multiProcessorCount * std::min(c, per_cu); }     // experiments (scripts/sweep_grid.sh)
#endif
    }
    const int64_t per_wave = tiles_per_wave > 1 ? tiles_per_wave : 1;
    const int64_t tiles = (int64_t)A.ntiles * (A.nframes > 0 ? A.nframes : 1);
    // launches the caller keeps in flight share the wave slots: 2/n each (include/svo.h, svo_trace_params.launches_in_flight)
    const int64_t slots = in_flight >= 2 ? std::max<int64_t>(1, (int64_t)resident * 2 / in_flight) : resident;
    const int blocks = (int)std::min<int64_t>((tiles + per_wave - 1) / per_wave, slots);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64), 0, s, A);
    return SVO_OK;
}

// The see-through view of material m (see_through.hip.h) for a stack-kernel launch on `s`: built on the device at the first such
// launch after a change to the pools, rebuilt in place when m changes - on the device behind every launch of the world issued
// before (the work-slot events), so that none still reading the old view sees the new one - and awaited by every launch that uses it.
static int use_view(svo_world *w, uint32_t m, TraceArgs &A, hipStream_t s)
{
    Hbm &d = *w->hbm;
    if (d.view_material != m) {
        const uint64_t n4 = w->wide_pool_len * 16, bricks = w->twig_pool_len;       // (64 entries = 16 uint4 per wide node)
        if (!d.view_wide.p) {
            if (d.view_wide.alloc(std::max<uint64_t>(n4, 1) * 4, w->device) != hipSuccess ||
                d.view_mask.alloc(std::max<uint64_t>(bricks, 1), w->device) != hipSuccess) {
                d.view_wide = Pooled<uint32_t>();
                set_error("svo_trace: hipMalloc of the see-through view failed"); return SVO_ERR_OUT_OF_MEMORY;
            }
        } else {
            for (Event &e : d.work_done) if (e.e) if (const int rc = e.wait(s)) return rc;
        }
        d.view_material = 0;                                            // (until the build below is issued)
        int rc;                                                         // (both sizes before either launch: a view is never half built)
        if ((rc = launch_fits("svo_trace", (int64_t)n4)) != SVO_OK || (rc = launch_fits("svo_trace", (int64_t)bricks * 8)) != SVO_OK) return rc;
        if ((rc = launch_per_element("svo_trace", (int64_t)n4, s, k_view_wide, reinterpret_cast<const uint4 *>(d.wide.p), reinterpret_cast<uint4 *>(d.view_wide.p), n4, m)) != SVO_OK ||
            (rc = launch_per_element("svo_trace", (int64_t)bricks * 8, s, k_view_mask, d.twig.p, d.mask.p, d.view_mask.p, bricks, m)) != SVO_OK) return rc;
        if ((rc = d.view_built.record(s)) != SVO_OK) return rc;
        d.view_material = m;
    } else {
        if (const int rc = d.view_built.wait(s)) return rc;
    }
    A.wide = d.view_wide.p;
    A.mask = d.view_mask.p;
    return SVO_OK;
}

static int launch(svo_world *w, const svo_trace_params *prm, TraceArgs &A, hipStream_t s)
{
    const int kernel = pick_kernel(w, prm, A);
    if (kernel < 0) return kernel;
    HIP_TRY(hipSetDevice(w->device));
    const uint32_t see = prm ? prm->see_through : 0u;
    if (see && kernel == SVO_KERNEL_STACK) {
        const int rc = use_view(w, see, A, s);
        if (rc != SVO_OK) return rc;
    }
    if (kernel == SVO_KERNEL_STACK)
        if (const int rc = gate_light_clearance(*w, prm, A, see, s)) return rc;
    // every launch gets its own {tile cursor, ray count} slot so that launches on different streams may overlap
    Hbm &d = *w->hbm;
    d.work_last = d.work_next;
    d.work_next = (d.work_next + 1) % WORK_SLOTS;
    A.work = d.work.p + WORK_SLOT_WORDS * d.work_last;
    // a slot coming round again must not be reset under a launch that still reads it: order behind that launch
    Event &ev = d.work_done[d.work_last];
    if (const int rc = ev.wait(s)) return rc;
    HIP_TRY(hipMemsetAsync(A.work, 0, WORK_SLOT_WORDS * sizeof(unsigned long long), s));
    if (A.n <= 0) return ev.record(s) == SVO_OK ? SVO_OK : SVO_ERR_HIP;
    if (kernel == SVO_KERNEL_LITERAL) {
        const auto literal = see ? (A.tmax ? k_trace_literal<true, true> : k_trace_literal<true, false>) : (A.tmax ? k_trace_literal<false, true> : k_trace_literal<false, false>);
        if (const int rc = launch_per_element("svo_trace", A.n, s, literal, A, see)) return rc;      // (see == 0: ST is off and `ignore` is not read)
    } else {
        if (A.ntiles > (1 << 25)) { set_error("svo_trace: more than 2^31 rays in one stack-kernel launch"); return SVO_ERR_UNSUPPORTED; }
        if (A.tile_cost) HIP_TRY(hipMemsetAsync(A.tile_cost, 0, (size_t)A.ntiles * (size_t)(A.from_camera ? A.nframes : 1) * 2 * sizeof(uint32_t), s));
        const int rc = launch_stack(w, A, prm ? prm->tiles_per_wave : 0, prm ? prm->launches_in_flight : 0, s);
        if (rc != SVO_OK) { set_error("svo_trace: device query failed"); return rc; }
        HIP_TRY(hipGetLastError());
    }
    return ev.record(s);
}

static int fill_cameras(const svo_camera *cams, int nframes, TraceArgs &A)
{
    if (!cams || nframes < 1 || nframes > MAX_FRAMES) { set_error("svo_trace: between 1 and 16 cameras per launch"); return SVO_ERR_INVALID_ARG; }
    for (int f = 0; f < nframes; ++f) {
        const svo_camera &c = cams[f];
        if (c.width <= 0 || c.height <= 0) { set_error("svo_trace: bad camera"); return SVO_ERR_INVALID_ARG; }
        if (c.width != cams[0].width || c.height != cams[0].height) { set_error("svo_trace_frames: the cameras of one launch share one image size"); return SVO_ERR_INVALID_ARG; }
        A.cams[f] = frame_cam(c);
    }
    A.from_camera = 1;
    A.nframes = nframes;
    A.imgw = cams[0].width; A.imgh = cams[0].height;
    return SVO_OK;
}

// Camera-mode launch of A.nframes frames.  The stack kernel marches them behind one set of cursors (its persistent
// waves drain once per launch, not once per frame); any other kernel gets one launch per frame.
static int launch_frames(svo_world *w, const svo_trace_params *prm, TraceArgs &A, const char *who, hipStream_t s)
{
    A.n = (int64_t)A.w * A.h;
    A.tiles_per_row = (A.w + TILE_W - 1) / TILE_W;
    const int64_t tiles = (int64_t)A.tiles_per_row * ((A.h + TILE_H - 1) / TILE_H);
    if (tiles * A.nframes > 0x3FFFFFFF || A.n * A.nframes > 0x7FFFFFFF) { set_error(std::string(who) + ": image too large"); return SVO_ERR_UNSUPPORTED; }
    A.ntiles = (int32_t)tiles;
    if (A.nframes == 1) return launch(w, prm, A, s);
    const int kernel = pick_kernel(w, prm, A);
    if (kernel < 0) return kernel;
    if (kernel == SVO_KERNEL_STACK) return launch(w, prm, A, s);
    if (prm && prm->counters_dev) { set_error(std::string(who) + ": work counters are per launch of one frame"); return SVO_ERR_UNSUPPORTED; }
    const int nframes = A.nframes;
    char *out = static_cast<char *>(A.out);
    for (int f = 0; f < nframes; ++f) {
        TraceArgs F = A;
        F.nframes = 1; F.cams[0] = A.cams[f];
        F.out = out + (size_t)f * (size_t)A.n * sizeof(svo_hit);
        const int rc = launch(w, prm, F, s);
        if (rc != SVO_OK) return rc;
    }
    return SVO_OK;
}

int svo_trace_frames(svo_world *w, const svo_camera *cams, int nframes, const svo_trace_params *prm,
                     int x0, int y0, int rw, int rh, svo_hit *out_dev, void *stream)
{
    TraceArgs A;
    int rc = fill_common(w, prm, A);
    if (rc != SVO_OK) return rc;
    if ((rc = fill_cameras(cams, nframes, A)) != SVO_OK) return rc;
    if (!out_dev || rw < 0 || rh < 0 || x0 < 0 || y0 < 0) { set_error("svo_trace: bad rectangle or output"); return SVO_ERR_INVALID_ARG; }
    A.x0 = x0; A.y0 = y0; A.w = rw; A.h = rh;
    A.bh = rh > 0 ? rh : 1; A.ystep = 0;
    A.out = out_dev;
    return launch_frames(w, prm, A, "svo_trace", (hipStream_t)stream);
}

int svo_trace(svo_world *w, const svo_camera *cam, const svo_trace_params *prm,
              int x0, int y0, int rw, int rh, svo_hit *out_dev, void *stream)
{
    return svo_trace_frames(w, cam, 1, prm, x0, y0, rw, rh, out_dev, stream);
}

int svo_trace_rows_frames(svo_world *w, const svo_camera *cams, int nframes, const svo_trace_params *prm,
                          int band0, int band_stride, int nbands, int band_height, svo_hit *out_dev, void *stream)
{
    TraceArgs A;
    int rc = fill_common(w, prm, A);
    if (rc != SVO_OK) return rc;
    if ((rc = fill_cameras(cams, nframes, A)) != SVO_OK) return rc;
    if (!out_dev || band0 < 0 || band_stride <= 0 || nbands < 0 || band_height <= 0) { set_error("svo_trace_rows: bad band partition"); return SVO_ERR_INVALID_ARG; }
    A.x0 = 0; A.y0 = band0 * band_height; A.w = cams[0].width; A.h = nbands * band_height;
    A.bh = band_height; A.ystep = band_stride * band_height;
    A.out = out_dev;
    return launch_frames(w, prm, A, "svo_trace_rows", (hipStream_t)stream);
}

int svo_trace_rows(svo_world *w, const svo_camera *cam, const svo_trace_params *prm,
                   int band0, int band_stride, int nbands, int band_height, svo_hit *out_dev, void *stream)
{
    return svo_trace_rows_frames(w, cam, 1, prm, band0, band_stride, nbands, band_height, out_dev, stream);
}

// the ray-list launch of svo_trace_rays (tmax_dev == nullptr) and svo_trace_segments (the bounded kernels)
static int trace_list(svo_world *w, const float *origins_dev, const float *dirs_dev, const float *tmax_dev, int64_t n,
                      const svo_trace_params *prm, svo_hit *out_dev, void *stream)
{
    TraceArgs A;
    int rc = fill_common(w, prm, A);
    if (rc != SVO_OK) return rc;
    if (n < 0 || (n > 0 && (!origins_dev || !dirs_dev || !out_dev))) { set_error("svo_trace_rays: bad ray list"); return SVO_ERR_INVALID_ARG; }
    A.from_camera = 0; A.nframes = 1;
    A.origins = origins_dev; A.dirs = dirs_dev; A.tmax = tmax_dev;
    A.n = n;
    A.w = 64; A.h = 1; A.bh = 1; A.tiles_per_row = 1;
    const int64_t tiles = (n + 63) / 64;
    if (tiles > 0x3FFFFFFF) { set_error("svo_trace_rays: too many rays"); return SVO_ERR_UNSUPPORTED; }
    A.ntiles = (int32_t)tiles;
    A.out = out_dev;
    return launch(w, prm, A, (hipStream_t)stream);
}

int svo_trace_rays(svo_world *w, const float *origins_dev, const float *dirs_dev, int64_t n,
                   const svo_trace_params *prm, svo_hit *out_dev, void *stream)
{
    return trace_list(w, origins_dev, dirs_dev, nullptr, n, prm, out_dev, stream);
}

int svo_trace_segments(svo_world *w, const float *origins_dev, const float *dirs_dev, const float *tmax_dev, int64_t n,
                       const svo_trace_params *prm, svo_hit *out_dev, void *stream)
{
    if (n > 0 && !tmax_dev) { set_error("svo_trace_segments: tmax_dev is NULL"); return SVO_ERR_INVALID_ARG; }
    if (n == 0) tmax_dev = nullptr;                                     // (nothing is launched: the work slot is reset as svo_trace_rays resets it)
    return trace_list(w, origins_dev, dirs_dev, tmax_dev, n, prm, out_dev, stream);
}

// ParallaxAlpha's second march (shaders/ParallaxAlpha.Fragment.glsl:141-199,276-335): the surface, the continuation list of the
// pixels that hit material m (see_through.hip.h k_continuation), one ray-list launch on the see-through world into behind_dev.
int svo_trace_translucent(svo_world *w, const svo_camera *cam, const svo_trace_params *prm, int x0, int y0, int rw, int rh,
                          svo_hit *surface_dev, svo_hit *behind_dev, void *stream)
{
    if (!w || !prm || !cam || !surface_dev || !behind_dev) { set_error("svo_trace_translucent: bad argument"); return SVO_ERR_INVALID_ARG; }
    const uint32_t m = prm->see_through;
    if (m == 0u || m > 0xFFFFu) { set_error("svo_trace_translucent: see_through must be a material in 1..0xFFFF"); return SVO_ERR_INVALID_ARG; }
    if (w->device < 0) { set_error("svo_trace_translucent: world is not uploaded"); return SVO_ERR_NOT_UPLOADED; }
    hipStream_t s = (hipStream_t)stream;
    svo_trace_params surface = *prm;
    surface.see_through = 0;
    const int rc = svo_trace(w, cam, &surface, x0, y0, rw, rh, surface_dev, stream);
    if (rc != SVO_OK) return rc;
    const int64_t n = (int64_t)rw * rh;
    if (n == 0) return SVO_OK;
    HIP_TRY(hipSetDevice(w->device));
    // the list lives in the world's scratch: calls on different streams are ordered behind one another
    return w->hbm->cont.use(RayList::floats(n, false), "svo_trace_translucent", s, [&](float *scratch) {
        const RayList list(scratch, n, false);
        const int rc = launch_per_element("svo_trace_translucent", n, s, k_continuation, make_frame(*cam, x0, y0, rw, rh), m, miss_ray_origin(w),
                                          reinterpret_cast<uint4 *>(surface_dev), list.origins, list.dirs);
        if (rc != SVO_OK) return rc;
        const svo_trace_params behind = own_list_params(*prm, true);
        return svo_trace_rays(w, list.origins, list.dirs, n, &behind, behind_dev, stream);
    });
}

// Mirror reflections (reflect.hip.h): the mirror ray of every pixel that hit `material` on a voxel with a box, ONE ray-list launch into
// reflect_dev.  svo_shade_reflections (shade.hip) rebuilds the rays from the same records and blends what they saw.
int svo_trace_reflections(svo_world *w, const svo_camera *cam, const svo_trace_params *prm, uint32_t material, int x0, int y0, int rw, int rh,
                          const svo_hit *gbuffer_dev, const svo_voxel *voxels_dev, svo_hit *reflect_dev, void *stream)
{
    if (!w || !prm || !rect_ok(cam, x0, y0, rw, rh) || material > 0xFFFFu) { set_error("svo_trace_reflections: bad world, camera, params, rectangle or material"); return SVO_ERR_INVALID_ARG; }
    const int64_t n = (int64_t)rw * rh;
    if (n > 0 && (!gbuffer_dev || !voxels_dev || !reflect_dev)) { set_error("svo_trace_reflections: NULL buffer"); return SVO_ERR_INVALID_ARG; }
    const svo_trace_params march = own_list_params(*prm, true);
    TraceArgs A;                                                        // (for the launch's resolved eps; checks see_through, semantics, residency and the kernel id)
    int rc = fill_common(w, &march, A);
    if (rc != SVO_OK) return rc;
    if ((rc = pick_kernel(w, &march, A)) < 0) return rc;
    if (n == 0) return SVO_OK;
    if (n > 0x7FFFFFFF) { set_error("svo_trace_reflections: image too large"); return SVO_ERR_UNSUPPORTED; }
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(w->device));
    // the list lives in the world's scratch: calls on different streams are ordered behind one another
    return w->hbm->mirror.use(RayList::floats(n, false), "svo_trace_reflections", s, [&](float *scratch) {
        const RayList list(scratch, n, false);
        const int rc = launch_per_element("svo_trace_reflections", n, s, k_mirror_rays, make_frame(*cam, x0, y0, rw, rh), A.eps, material, miss_ray_origin(w),
                                          reinterpret_cast<const uint4 *>(gbuffer_dev), reinterpret_cast<const uint4 *>(voxels_dev), list.origins, list.dirs);
        if (rc != SVO_OK) return rc;
        return svo_trace_rays(w, list.origins, list.dirs, n, &march, reflect_dev, stream);
    });
}

// Shadows from the point light and the spotlight (local_shadows.hip.h): the ray list of every light asked for, ONE ray-list launch
// for all of them (the stack kernel's persistent waves drain once, not once per light), the fold into gbuffer_dev's flag words.
int svo_trace_local_shadows(svo_world *w, const svo_camera *cam, const svo_trace_params *prm, const float *point_position, const float *spot_position,
                            int x0, int y0, int rw, int rh, svo_hit *gbuffer_dev, void *stream)
{
    if (!w || !prm || !gbuffer_dev || (!point_position && !spot_position) || !rect_ok(cam, x0, y0, rw, rh)) {
        set_error("svo_trace_local_shadows: bad argument"); return SVO_ERR_INVALID_ARG;
    }
    TraceArgs A;                                                        // (for the launch's resolved eps; checks see_through, semantics and residency)
    int rc = fill_common(w, prm, A);
    if (rc != SVO_OK) return rc;
    LocalLights L;
    std::memset(&L, 0, sizeof L);
    if (point_position) { std::memcpy(L.pos[L.count], point_position, 12); L.bit[L.count++] = SVO_SHADOWED_POINT; }
    if (spot_position) { std::memcpy(L.pos[L.count], spot_position, 12); L.bit[L.count++] = SVO_SHADOWED_SPOT; }
    const int64_t n = (int64_t)rw * rh, rays = n * L.count;
    if (n == 0) return SVO_OK;
    if (rays > 0x7FFFFFFF) { set_error("svo_trace_local_shadows: image too large"); return SVO_ERR_UNSUPPORTED; }
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(w->device));
    // the records and the list live in the world's scratch: calls on different streams are ordered behind one another
    return w->hbm->local.use(RayList::floats(rays, true), "svo_trace_local_shadows", s, [&](float *scratch) {
        const RayList list(scratch, rays, true);
        const PixelFrame F = make_frame(*cam, x0, y0, rw, rh);
        int rc = launch_per_element("svo_trace_local_shadows", n, s, k_local_rays, F, A.eps, L, miss_ray_origin(w), reinterpret_cast<const uint4 *>(gbuffer_dev),
                                    list.origins, list.dirs);
        if (rc != SVO_OK) return rc;
        const svo_trace_params march = own_list_params(*prm, false);
        // (unbounded on purpose: ending each ray at its light through svo_trace_segments was measured and is slower)
        rc = svo_trace_rays(w, list.origins, list.dirs, rays, &march, reinterpret_cast<svo_hit *>(list.records), stream);
        if (rc != SVO_OK) return rc;
        return launch_per_element("svo_trace_local_shadows", n, s, k_local_resolve, F, A.eps, L, reinterpret_cast<const uint4 *>(list.records),
                                  reinterpret_cast<uint4 *>(gbuffer_dev));
    });
}

// A list of point lights (light_list.hip.h): the candidate masks and their counts, the scan that ranks the pairs light-major, the
// compacted ray list, ONE ray-list launch of `cap` rays - the host never learns how many pairs there are -, the fold into one word
// per pixel.  The scratch: the RayList of cap slots, then the [light][block] counts, their exclusive sums, the two totals, the scan's own.
int svo_trace_lights(svo_world *w, const svo_camera *cam, const svo_trace_params *prm, const svo_light *lights, int nlights, int64_t max_rays,
                     int x0, int y0, int rw, int rh, const svo_hit *gbuffer_dev, uint32_t *visible_dev, uint32_t *count_dev, void *stream)
{
    if (!w || !prm || !lights || !gbuffer_dev || !visible_dev || nlights < 1 || nlights > MAX_LIGHTS || max_rays < 0 || !rect_ok(cam, x0, y0, rw, rh)) {
        set_error("svo_trace_lights: bad argument"); return SVO_ERR_INVALID_ARG;
    }
    LightList L;
    std::memset(&L, 0, sizeof L);
    for (int j = 0; j < nlights; ++j) {
        const svo_light &l = lights[j];
        if (!std::isfinite(l.position[0]) || !std::isfinite(l.position[1]) || !std::isfinite(l.position[2]) || !(l.reach > 0.0f && l.reach < INFINITY)) {
            set_error("svo_trace_lights: a light's position is not finite, or its reach is not a finite number above 0"); return SVO_ERR_INVALID_ARG;
        }
        std::memcpy(L.pos[j], l.position, sizeof L.pos[j]);
        L.reach2[j] = l.reach * l.reach;
    }
    L.count = nlights;
    TraceArgs A;                                                        // (for the launch's resolved eps; checks see_through, semantics and residency)
    int rc = fill_common(w, prm, A);
    if (rc != SVO_OK) return rc;
    const int64_t n = (int64_t)rw * rh, cap = max_rays > 0 ? max_rays : n;
    if (n == 0) return SVO_OK;
    if (n * nlights > 0x7FFFFFFF || cap > 0x7FFFFFFF) { set_error("svo_trace_lights: image or list too large"); return SVO_ERR_UNSUPPORTED; }
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(w->device));
    const uint32_t nblocks = blocks_for((uint64_t)n, LIGHT_BLOCK), items = nblocks * (uint32_t)nlights;
    size_t scan_bytes = 0;
    uint32_t *nul = nullptr;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, nul, nul, (int)items, s) != hipSuccess) { set_error("svo_trace_lights: scan size query failed"); return SVO_ERR_HIP; }
    const size_t list_words = RayList::floats(cap, true), head_words = (list_words + 2 * (size_t)items + 2 + 63) / 64 * 64;
    // the records, the list and the ranks live in the world's scratch: calls on different streams are ordered behind one another
    return w->hbm->lights.use(head_words + (scan_bytes + 3) / 4 + 64, "svo_trace_lights", s, [&](float *scratch) -> int {
        const RayList list(scratch, cap, true);
        uint32_t *counts = reinterpret_cast<uint32_t *>(scratch + list_words), *base = counts + items, *total = base + items;
        const PixelFrame F = make_frame(*cam, x0, y0, rw, rh);
        const uint4 *gbuffer = reinterpret_cast<const uint4 *>(gbuffer_dev);
        const char *who = "svo_trace_lights";
        int rc = launch_per_element(who, n, s, k_light_cull, F, A.eps, L, gbuffer, visible_dev, counts, nblocks);
        if (rc != SVO_OK) return rc;
        if (hipcub::DeviceScan::ExclusiveSum(scratch + head_words, scan_bytes, counts, base, (int)items, s) != hipSuccess) { set_error("svo_trace_lights: scan failed"); return SVO_ERR_HIP; }
        hipLaunchKernelGGL(k_light_total, dim3(1), dim3(1), 0, s, counts, base, items, (uint32_t)cap, total, count_dev);
        if ((rc = launch_status(who)) != SVO_OK) return rc;
        rc = launch_per_element(who, n, s, k_light_emit, F, A.eps, L, miss_ray_origin(w), gbuffer, visible_dev, base, nblocks, total, (uint32_t)cap, list.origins, list.dirs);
        if (rc != SVO_OK) return rc;
        const svo_trace_params march = own_list_params(*prm, false);
        // (unbounded on purpose, as svo_trace_local_shadows' launch is: DESIGN.md 6g)
        rc = svo_trace_rays(w, list.origins, list.dirs, cap, &march, reinterpret_cast<svo_hit *>(list.records), stream);
        if (rc != SVO_OK) return rc;
        return launch_per_element(who, n, s, k_light_resolve, F, A.eps, L, gbuffer, base, nblocks, (uint32_t)cap, reinterpret_cast<const uint4 *>(list.records), visible_dev);
    });
}

// ---- voxel model instances (instances.hip.h) ----------------------------------------------------------------------------------------
// What both instance calls settle before any device work, in the ABI's order: the arguments, then what fill_common / pick_kernel
// refuse for either world (As, Am: the scene's and the model's resolved launch), then the sizes.  SVO_OK with n == 0: nothing to do.
static int instance_call(const char *who, svo_world *scene, svo_world *model, const svo_camera *cam, const svo_trace_params *prm, const svo_instance *inst,
                         int ninst, int64_t max_rays, float bias, int x0, int y0, int rw, int rh, bool buffers, InstanceList &I, svo_trace_params &march,
                         TraceArgs &As, int64_t &n, int64_t &cap)
{
    const auto refuse = [who](const char *what) { set_error(std::string(who) + what); return SVO_ERR_INVALID_ARG; };
    if (!scene || !model || !prm || !inst || !buffers || ninst < 1 || ninst > MAX_INSTANCES || max_rays < 0 || !rect_ok(cam, x0, y0, rw, rh)) return refuse(": bad argument");
    std::memset(&I, 0, sizeof I);
    for (int j = 0; j < ninst; ++j) {
        const svo_instance &in = inst[j];
        for (int a = 0; a < 9; ++a) if (!std::isfinite(in.rot[a])) return refuse(": an instance's rotation is not finite");
        for (int a = 0; a < 3; ++a) if (!std::isfinite(in.pos[a])) return refuse(": an instance's position is not finite");
        if (!(in.scale > 0.0f && in.scale < INFINITY)) return refuse(": an instance's scale is not a finite number above 0");
        std::memcpy(I.rot[j], in.rot, sizeof I.rot[j]);
        std::memcpy(I.pos[j], in.pos, sizeof I.pos[j]);
        I.scale[j] = in.scale;
        I.inv[j] = 1.0f / in.scale;
    }
    I.count = ninst;
    if (!(bias >= 0.0f)) return refuse(": bias is negative or not a number");
    if (scene->device >= 0 && model->device >= 0 && scene->device != model->device) return refuse(": the scene and the model are on different devices");
    march = own_list_params(*prm, false);
    TraceArgs Am;
    int rc = fill_common(scene, &march, As);
    if (rc != SVO_OK) return rc;
    if ((rc = pick_kernel(scene, &march, As)) < 0) return rc;
    if ((rc = fill_common(model, &march, Am)) != SVO_OK) return rc;
    if ((rc = pick_kernel(model, &march, Am)) < 0) return rc;
    for (int a = 0; a < 3; ++a) { I.bmin[a] = Am.worldmin[a]; I.bmax[a] = Am.worldmax[a]; }
    n = (int64_t)rw * rh; cap = max_rays > 0 ? max_rays : n;
    if (n == 0) return SVO_OK;
    if (n * ninst > 0x7FFFFFFF || cap > 0x7FFFFFFF) { set_error(std::string(who) + ": image or list too large"); return SVO_ERR_UNSUPPORTED; }
    return SVO_OK;
}

// The model list's scratch, in floats from its start: the RayList of cap slots with records, stage 1's far ends, the pair masks,
// the [instance][block] counts, their exclusive sums, the two totals; the scan's own follows at `head`
struct InstanceScratch {
    uint32_t nblocks, items;
    size_t list, head, scan_bytes = 0;
    InstanceScratch(int64_t n, int64_t cap, int ninst, bool far_ends) : nblocks(blocks_for((uint64_t)n, LIGHT_BLOCK)), items(nblocks * (uint32_t)ninst),
        list(RayList::floats(cap, true) + (far_ends ? (size_t)cap : 0)), head((list + (size_t)n + 2 * (size_t)items + 2 + 63) / 64 * 64) {}
    size_t floats() const { return head + (scan_bytes + 3) / 4 + 64; }
};

// Cull, scan, total and emit of either stage into the model list: what the two calls share up to the march
static int instance_list(bool shadow, const char *who, const InstanceScratch &L, float *scratch, const PixelFrame &F, float bias, V3 S, const InstanceList &I, svo_world *model,
                         const uint4 *records, int64_t n, int64_t cap, const uint32_t *owner, V3 scene_miss, float *scene_origins, float *scene_dirs,
                         uint32_t *count_dev, hipStream_t s)
{
    const RayList list(scratch, cap, true);
    float *tmax = shadow ? nullptr : list.dirs + 3 * cap;
    uint32_t *masks = reinterpret_cast<uint32_t *>(scratch + L.list), *counts = masks + n, *base = counts + L.items, *total = base + L.items;
    int rc = launch_per_element(who, n, s, shadow ? k_inst_cull<true> : k_inst_cull<false>, F, bias, S, I, records, masks, counts, L.nblocks, owner, scene_miss, scene_origins, scene_dirs);
    if (rc != SVO_OK) return rc;
    size_t scan_bytes = L.scan_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(scratch + L.head, scan_bytes, counts, base, (int)L.items, s) != hipSuccess) { set_error(std::string(who) + ": scan failed"); return SVO_ERR_HIP; }
    hipLaunchKernelGGL(k_light_total, dim3(1), dim3(1), 0, s, counts, base, L.items, (uint32_t)cap, total, count_dev);
    if ((rc = launch_status(who)) != SVO_OK) return rc;
    return launch_per_element(who, n, s, shadow ? k_inst_emit<true> : k_inst_emit<false>, F, bias, S, I, miss_ray_origin(model), records, masks, base, L.nblocks, total, (uint32_t)cap,
                              list.origins, list.dirs, tmax);
}

static int instance_scan_size(const char *who, InstanceScratch &L, hipStream_t s)
{
    uint32_t *nul = nullptr;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, L.scan_bytes, nul, nul, (int)L.items, s) != hipSuccess) { set_error(std::string(who) + ": scan size query failed"); return SVO_ERR_HIP; }
    return SVO_OK;
}

// Stage 1: the pixels' rays into each instance's space, ONE bounded ray-list launch of `cap` rays on the model - each ray ends at what
// the G-buffer holds -, the nearest hit per pixel back into the frame.  The list lives in the MODEL's scratch.
int svo_trace_instances(svo_world *scene, svo_world *model, const svo_camera *cam, const svo_trace_params *prm, const svo_instance *inst, int ninst, int64_t max_rays,
                        int x0, int y0, int rw, int rh, const svo_hit *gbuffer_dev, svo_hit *merged_dev, uint32_t *owner_dev, uint32_t *count_dev, void *stream)
{
    const char *who = "svo_trace_instances";
    InstanceList I;
    svo_trace_params march;
    TraceArgs As;
    int64_t n, cap;
    int rc = instance_call(who, scene, model, cam, prm, inst, ninst, max_rays, 0.0f, x0, y0, rw, rh, gbuffer_dev && merged_dev && owner_dev, I, march, As, n, cap);
    if (rc != SVO_OK || n == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(model->device));
    InstanceScratch L(n, cap, ninst, true);
    if ((rc = instance_scan_size(who, L, s)) != SVO_OK) return rc;
    // the records, the list and the ranks live in the model's scratch: calls on different streams are ordered behind one another
    return model->hbm->instances.use(L.floats(), who, s, [&](float *scratch) -> int {
        const RayList list(scratch, cap, true);
        const PixelFrame F = make_frame(*cam, x0, y0, rw, rh);
        const uint4 *gbuffer = reinterpret_cast<const uint4 *>(gbuffer_dev);
        const V3 none = V3{ 0.0f, 0.0f, 0.0f };
        int rc = instance_list(false, who, L, scratch, F, 0.0f, none, I, model, gbuffer, n, cap, nullptr, none, nullptr, nullptr, count_dev, s);
        if (rc != SVO_OK) return rc;
        rc = trace_list(model, list.origins, list.dirs, list.dirs + 3 * cap, cap, &march, reinterpret_cast<svo_hit *>(list.records), stream);
        if (rc != SVO_OK) return rc;
        const uint32_t *masks = reinterpret_cast<const uint32_t *>(scratch + L.list), *base = masks + n + L.items;
        return launch_per_element(who, n, s, k_inst_resolve, F, I, gbuffer, masks, base, L.nblocks, (uint32_t)cap, reinterpret_cast<const uint4 *>(list.records),
                                  reinterpret_cast<uint4 *>(merged_dev), owner_dev);
    });
}

// Stage 2: from every usable, not yet shadowed record of merged_dev the ray towards the directional light - into each instance's space
// and ONE unbounded launch of `cap` rays on the model, and for the pixels an instance owns ONE launch of w*h rays on the scene (the
// terrain's pixels had theirs from svo_trace) -, the fold into the flag words.  The model list lives in the model's scratch, the scene
// list in the scene's.
int svo_trace_instance_shadows(svo_world *scene, svo_world *model, const svo_camera *cam, const svo_trace_params *prm, const svo_instance *inst, int ninst,
                               int64_t max_rays, float bias, int x0, int y0, int rw, int rh, svo_hit *merged_dev, const uint32_t *owner_dev, uint32_t *count_dev,
                               void *stream)
{
    const char *who = "svo_trace_instance_shadows";
    InstanceList I;
    svo_trace_params march;
    TraceArgs As;
    int64_t n, cap;
    int rc = instance_call(who, scene, model, cam, prm, inst, ninst, max_rays, bias, x0, y0, rw, rh, merged_dev && owner_dev, I, march, As, n, cap);
    if (rc != SVO_OK || n == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(model->device));
    InstanceScratch L(n, cap, ninst, false);
    if ((rc = instance_scan_size(who, L, s)) != SVO_OK) return rc;
    const float b = bias > 0.0f ? bias : As.eps;
    const V3 S = V3{ As.sdir[0], As.sdir[1], As.sdir[2] };
    return scene->hbm->instance_scene.use(RayList::floats(n, true), who, s, [&](float *scene_scratch) -> int {
        return model->hbm->instance_shadows.use(L.floats(), who, s, [&](float *scratch) -> int {
            const RayList list(scratch, cap, true), scene_list(scene_scratch, n, true);
            const PixelFrame F = make_frame(*cam, x0, y0, rw, rh);
            uint4 *merged = reinterpret_cast<uint4 *>(merged_dev);
            int rc = instance_list(true, who, L, scratch, F, b, S, I, model, merged, n, cap, owner_dev, miss_ray_origin(scene), scene_list.origins, scene_list.dirs,
                                         count_dev, s);
            if (rc != SVO_OK) return rc;
            if ((rc = svo_trace_rays(model, list.origins, list.dirs, cap, &march, reinterpret_cast<svo_hit *>(list.records), stream)) != SVO_OK) return rc;
            if ((rc = svo_trace_rays(scene, scene_list.origins, scene_list.dirs, n, &march, reinterpret_cast<svo_hit *>(scene_list.records), stream)) != SVO_OK) return rc;
            const uint32_t *masks = reinterpret_cast<const uint32_t *>(scratch + L.list), *base = masks + n + L.items;
            return launch_per_element(who, n, s, k_inst_fold, F, I, masks, base, L.nblocks, (uint32_t)cap, reinterpret_cast<const uint4 *>(list.records),
                                      reinterpret_cast<const uint4 *>(scene_list.records), merged);
        });
    });
}

// ---- the directional light's shadow map (shadowmap.hip.h) -------------------------------------------------------------------------
// what svo_shadowmap_render and svo_shadowmap_apply ask of a map before anything else
static bool map_ok(const svo_shadowmap *m)
{
    if (!m || !m->depth_dev) return false;
    if (m->width < 8 || m->width > 16384 || m->width % 8 || m->height < 8 || m->height > 16384 || m->height % 8) return false;
    if (!(m->half_width > 0.0f && m->half_width < INFINITY && m->half_height > 0.0f && m->half_height < INFINITY)) return false;
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(m->origin[a]) || !std::isfinite(m->direction[a]) || !std::isfinite(m->right[a]) || !std::isfinite(m->up[a])) return false;
    const float q = m->direction[0] * m->direction[0] + m->direction[1] * m->direction[1] + m->direction[2] * m->direction[2];
    return std::fabs(q - 1.0f) <= 1e-3f;
}

static MapFrame map_frame(const svo_shadowmap &m)
{
    MapFrame M;
    std::memcpy(M.origin, m.origin, sizeof M.origin); std::memcpy(M.dir, m.direction, sizeof M.dir);
    std::memcpy(M.right, m.right, sizeof M.right); std::memcpy(M.up, m.up, sizeof M.up);
    M.half_w = m.half_width; M.half_h = m.half_height; M.width = m.width; M.height = m.height;
    return M;
}

// A map that holds the whole world box, host only: the basis in double from the hint (0,1,0) - (0,0,1) within 8 degrees of vertical -,
// the plane `back` in front of the nearest corner, the half extents a margin over the farthest one, everything rounded to float once.
int svo_shadowmap_fit(const svo_world *w, const float direction[3], int width, int height, svo_shadowmap *out)
{
    if (!w || !direction || !out || width < 8 || width > 16384 || width % 8 || height < 8 || height > 16384 || height % 8) {
        set_error("svo_shadowmap_fit: bad argument"); return SVO_ERR_INVALID_ARG;
    }
    double d[3] = { direction[0], direction[1], direction[2] };
    const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (!(len > 0.0 && len < INFINITY)) { set_error("svo_shadowmap_fit: the direction is zero or not finite"); return SVO_ERR_INVALID_ARG; }
    for (double &c : d) c /= len;
    const double hint[3] = { 0.0, std::fabs(d[1]) > 0.99 ? 0.0 : 1.0, std::fabs(d[1]) > 0.99 ? 1.0 : 0.0 };     // cos 8 deg = 0.990
    double r[3] = { d[1] * hint[2] - d[2] * hint[1], d[2] * hint[0] - d[0] * hint[2], d[0] * hint[1] - d[1] * hint[0] };
    const double rl = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    for (double &c : r) c /= rl;
    const double u[3] = { r[1] * d[2] - r[2] * d[1], r[2] * d[0] - r[0] * d[2], r[0] * d[1] - r[1] * d[0] };
    const double cs = (double)w->chunksize;
    const int dims[3] = { w->width, w->height, w->depth };
    double lo[3], hi[3], mid[3], diag = 0.0;
    for (int a = 0; a < 3; ++a) {
        lo[a] = (double)w->chunkcoordmin[a] * cs; hi[a] = lo[a] + (double)dims[a] * cs; mid[a] = 0.5 * (lo[a] + hi[a]);
        diag += (hi[a] - lo[a]) * (hi[a] - lo[a]);
    }
    diag = std::sqrt(diag);
    double near_s = INFINITY, far_a = 0.0, far_b = 0.0;
    for (int k = 0; k < 8; ++k) {
        double q[3];
        for (int a = 0; a < 3; ++a) q[a] = ((k >> a & 1) ? hi[a] : lo[a]) - mid[a];
        near_s = std::min(near_s, q[0] * d[0] + q[1] * d[1] + q[2] * d[2]);
        far_a = std::max(far_a, std::fabs(q[0] * r[0] + q[1] * r[1] + q[2] * r[2]));
        far_b = std::max(far_b, std::fabs(q[0] * u[0] + q[1] * u[1] + q[2] * u[2]));
    }
    // the margins cover the rounding to float of the origin, of the basis (2^-24 of a lever of at most the diagonal plus the offset) and of the extents
    const double back = near_s - 2.0 - diag / 1024.0;
    for (int a = 0; a < 3; ++a) {
        out->origin[a] = (float)(mid[a] + d[a] * back);
        out->direction[a] = (float)d[a]; out->right[a] = (float)r[a]; out->up[a] = (float)u[a];
    }
    out->half_width = (float)(far_a * (1.0 + 1.0 / 1024.0) + 1.0);
    out->half_height = (float)(far_b * (1.0 + 1.0 / 1024.0) + 1.0);
    out->width = width; out->height = height;
    return SVO_OK;
}

// The depth image of the world seen from the light: the texel rays in tile order (shadowmap.hip.h), ONE ray-list launch into scratch
// records, the fold into depth_dev.
int svo_shadowmap_render(svo_world *w, const svo_shadowmap *map, const svo_trace_params *prm, void *stream)
{
    if (!w || !prm || !map_ok(map)) { set_error("svo_shadowmap_render: bad argument"); return SVO_ERR_INVALID_ARG; }
    const svo_trace_params march = own_list_params(*prm, false);
    TraceArgs A;                                                        // (checks see_through, semantics, residency and the kernel id before any device work)
    int rc = fill_common(w, &march, A);
    if (rc != SVO_OK) return rc;
    if ((rc = pick_kernel(w, &march, A)) < 0) return rc;
    const MapFrame M = map_frame(*map);
    const int64_t n = M.count();                                        // (<= 2^28)
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(w->device));
    // the records and the list live in the world's scratch: calls on different streams are ordered behind one another
    return w->hbm->shadowmap.use(RayList::floats(n, true), "svo_shadowmap_render", s, [&](float *scratch) {
        const RayList list(scratch, n, true);
        int rc;
        if ((rc = launch_per_element("svo_shadowmap_render", n, s, k_shadowmap_rays, M, list.origins, list.dirs)) != SVO_OK) return rc;
        if ((rc = svo_trace_rays(w, list.origins, list.dirs, n, &march, reinterpret_cast<svo_hit *>(list.records), stream)) != SVO_OK) return rc;
        return launch_per_element("svo_shadowmap_render", n, s, k_shadowmap_depth, M, reinterpret_cast<const uint4 *>(list.records), map->depth_dev);
    });
}

int svo_shadowmap_apply(const svo_camera *cam, const svo_shadowmap *map, float eps, float bias, int x0, int y0, int rw, int rh,
                        svo_hit *gbuffer_dev, void *stream)
{
    if (!gbuffer_dev || !rect_ok(cam, x0, y0, rw, rh) || !(eps >= 0.0f) || !(bias >= 0.0f) || !map_ok(map)) {
        set_error("svo_shadowmap_apply: bad argument"); return SVO_ERR_INVALID_ARG;
    }
    return launch_per_element("svo_shadowmap_apply", (int64_t)rw * rh, (hipStream_t)stream, k_shadowmap_apply, make_frame(*cam, x0, y0, rw, rh),
                              eps == 0.0f ? 1.0f / 8192.0f : eps, map_frame(*map), static_cast<const float *>(map->depth_dev), bias,
                              reinterpret_cast<uint4 *>(gbuffer_dev));
}

// Point queries (locate.hip.h): one thread per point, the tree pool (SVO_KERNEL_LITERAL) or the wide pool (SVO_KERNEL_STACK; AUTO where
// svo_trace would march with the stack kernel).  No launch slot, no scratch, no see-through view: the kernels compare the material read.
int svo_world_locate(svo_world *w, const float *points_dev, int64_t n, const svo_trace_params *prm, svo_voxel *out_dev, void *stream)
{
    if (!w || n < 0 || (n > 0 && (!points_dev || !out_dev))) { set_error("svo_world_locate: bad point list or output"); return SVO_ERR_INVALID_ARG; }
    int rc = refuse_params("svo_world_locate", prm);
    if (rc != SVO_OK) return rc;
    TraceArgs A;
    if ((rc = fill_common(w, prm, A)) != SVO_OK) return rc;             // (residency; the world box, the tables and the pools)
    A.counters = nullptr; A.tile_cost = nullptr; A.tile_order = nullptr;   // only kernel, semantics and see_through are read
    const int kernel = pick_kernel(w, prm, A);
    if (kernel < 0) return kernel;
    if (n == 0) return SVO_OK;
    if ((rc = launch_fits("svo_world_locate", n)) != SVO_OK) return rc;
    HIP_TRY(hipSetDevice(w->device));
    A.from_camera = 0; A.nframes = 1;
    A.origins = points_dev; A.n = n; A.out = out_dev;
    const uint32_t see = prm ? prm->see_through : 0u;
    return launch_per_element("svo_world_locate", n, (hipStream_t)stream, kernel == SVO_KERNEL_STACK ? k_locate_wide : k_locate_literal, A, see);
}

// Voxel ambient occlusion (ao.hip.h): svo_world_locate's walks on the eight lattice cells around the open cell in front of every hit's
// face, folded in registers.  Kernel selection, and no launch slot, no scratch and no cache, as svo_world_locate.
int svo_hit_ao(svo_world *w, const svo_camera *cam, const svo_trace_params *prm, float cell, int x0, int y0, int rw, int rh,
               const svo_hit *gbuffer_dev, const svo_voxel *voxels_dev, float *ao_dev, void *stream)
{
    if (!w || !rect_ok(cam, x0, y0, rw, rh) || !(cell >= 0.0f && cell < INFINITY)) { set_error("svo_hit_ao: bad world, camera, rectangle or cell"); return SVO_ERR_INVALID_ARG; }
    const int64_t n = (int64_t)rw * rh;
    if (n > 0 && (!gbuffer_dev || !voxels_dev || !ao_dev)) { set_error("svo_hit_ao: NULL buffer"); return SVO_ERR_INVALID_ARG; }
    int rc = refuse_params("svo_hit_ao", prm);
    if (rc != SVO_OK) return rc;
    TraceArgs A;
    if ((rc = fill_common(w, prm, A)) != SVO_OK) return rc;             // (residency; the world box, the tables, the pools and the resolved eps)
    A.counters = nullptr; A.tile_cost = nullptr; A.tile_order = nullptr;   // only eps, kernel, semantics and see_through are read
    const int kernel = pick_kernel(w, prm, A);
    if (kernel < 0) return kernel;
    if (n == 0) return SVO_OK;
    if (n > 0x7FFFFFFF) { set_error("svo_hit_ao: image too large"); return SVO_ERR_UNSUPPORTED; }
    HIP_TRY(hipSetDevice(w->device));
    A.n = n;
    const PixelFrame F = make_frame(*cam, x0, y0, rw, rh);
    const uint32_t see = prm ? prm->see_through : 0u;
    const uint4 *g = reinterpret_cast<const uint4 *>(gbuffer_dev), *v = reinterpret_cast<const uint4 *>(voxels_dev);
    // eight lanes per pixel
    return launch_per_element("svo_hit_ao", n * 8, (hipStream_t)stream, kernel == SVO_KERNEL_STACK ? k_hit_ao<true> : k_hit_ao<false>, A, F, cell, see, g, v, ao_dev);
}

// The parent index for a svo_hit_voxels call on `s`: built on the device at the first call after a change to the pools - level 0
// everywhere, the roots' kernel, one sweep per further BRANCH level - and awaited by every call on another stream.
static int use_parents(svo_world *w, hipStream_t s)
{
    Hbm &d = *w->hbm;
    if (d.parents_ok) return d.parents_built.wait(s);
    const size_t n = w->chunks.size(), blocks = (size_t)(w->tree_pool_cap >> 3) + 1;
    std::vector<uint32_t> trees(n);
    uint64_t most = 0;                                                  // most 8-blocks a chunk holds
    for (size_t i = 0; i < n; ++i) {
        trees[i] = (uint32_t)w->chunks[i].tree_count();                 // (< 2^30: offsets are 30-bit)
        most = std::max<uint64_t>(most, (w->chunks[i].tree_count() - 1) / 8);
    }
    if (d.parent.alloc(blocks, w->device) != hipSuccess || d.parent_level.alloc(blocks, w->device) != hipSuccess ||
        d.chunk_trees.reserve(n, false, nullptr) != SVO_OK) {
        d.parent = Pooled<uint32_t>(); d.parent_level = Pooled<uint8_t>(); d.chunk_trees = DevBuf<uint32_t>();
        set_error("svo_hit_voxels: hipMalloc of the parent index failed"); return SVO_ERR_OUT_OF_MEMORY;
    }
    HIP_TRY(hipMemcpy(d.chunk_trees.p, trees.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(d.parent_level.p, 0, blocks, s));
    if (const int rc = launch_per_element("svo_hit_voxels", (int64_t)n, s, k_parent_roots, d.chunks.p, d.chunk_trees.p, (uint32_t)n, d.tree.p, d.parent.p, d.parent_level.p)) return rc;
    if (most) {
        const dim3 grid(blocks_for(most, 256), (unsigned)std::min<size_t>(n, 65535));
        for (int L = 1; L < w->max_levels; ++L)
            hipLaunchKernelGGL(k_parent_sweep, grid, dim3(256), 0, s, d.chunks.p, d.chunk_trees.p, (uint32_t)n, d.tree.p, d.parent.p, d.parent_level.p, (uint32_t)L);
    }
    HIP_TRY(hipGetLastError());
    if (const int rc = d.parents_built.record(s)) return rc;
    d.parents_ok = true;
    return SVO_OK;
}

// The box of every hit (hit_voxels.hip.h): one thread per record, the walk up through the parent index and the replay down.  No launch
// slot and no scratch: calls on different streams are ordered behind one another only while the index is being built.
int svo_hit_voxels(svo_world *w, const svo_hit *gbuffer_dev, int64_t n, svo_voxel *out_dev, void *stream)
{
    if (!w || n < 0 || (n > 0 && (!gbuffer_dev || !out_dev))) { set_error("svo_hit_voxels: bad G-buffer or output"); return SVO_ERR_INVALID_ARG; }
    if (w->device < 0) { set_error("svo_hit_voxels: world is not uploaded"); return SVO_ERR_NOT_UPLOADED; }
    if (n == 0) return SVO_OK;
    if (const int rc = launch_fits("svo_hit_voxels", n)) return rc;
    HIP_TRY(hipSetDevice(w->device));
    hipStream_t s = (hipStream_t)stream;
    try {
        if (const int rc = use_parents(w, s)) return rc;
    } catch (const std::bad_alloc &) { set_error("svo_hit_voxels: out of host memory"); return SVO_ERR_OUT_OF_MEMORY; }
    const Hbm &d = *w->hbm;
    return launch_per_element("svo_hit_voxels", n, s, k_hit_voxels, reinterpret_cast<const uint4 *>(gbuffer_dev), out_dev, n, d.chunks.p,
                              d.chunk_trees.p, (uint32_t)w->chunks.size(), d.tree.p, d.parent.p, d.parent_level.p, (float)w->chunksize);
}

int svo_tile_order(svo_world *w, const uint32_t *cost_dev, uint32_t *order_dev, int ntiles, void *stream)
{
    if (!w || !cost_dev || !order_dev || ntiles < 0) return SVO_ERR_INVALID_ARG;
    if (w->device < 0) return SVO_ERR_NOT_UPLOADED;
    if (ntiles == 0) return SVO_OK;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(w->device));
    // scratch of the sort: keys in / out, indices in, and hipcub's own (cached in the handle, grown on demand)
    size_t cub_bytes = 0;
    uint32_t *nul = nullptr;
    if (hipcub::DeviceRadixSort::SortPairsDescending(nullptr, cub_bytes, nul, nul, nul, nul, ntiles, 0, 32, s) != hipSuccess) return SVO_ERR_HIP;
    const size_t need = (size_t)ntiles * 3 * sizeof(uint32_t) + cub_bytes + 256;
    // calls on different streams (one cost / order pair per launch in flight) share it: a sort that shared its keys need not even yield a permutation
    return w->hbm->sort.use(need, "svo_tile_order", s, [&](unsigned char *scratch) -> int {
        uint32_t *keys = reinterpret_cast<uint32_t *>(scratch), *keys_out = keys + ntiles, *idx = keys_out + ntiles;
        void *tmp = reinterpret_cast<char *>(idx + ntiles) + ((256 - ((size_t)ntiles * 12) % 256) % 256);
        if (const int rc = launch_per_element("svo_tile_order", ntiles, s, k_tile_keys, cost_dev, keys, idx, ntiles)) return rc;
        if (hipcub::DeviceRadixSort::SortPairsDescending(tmp, cub_bytes, keys, keys_out, idx, order_dev, ntiles, 0, 32, s) != hipSuccess) { set_error("svo_tile_order: sort failed"); return SVO_ERR_HIP; }
        return SVO_OK;
    });
}

int svo_trace_last_ray_count(svo_world *w, void *stream, uint64_t *rays)
{
    if (!w || !rays) return SVO_ERR_INVALID_ARG;
    if (w->device < 0) return SVO_ERR_NOT_UPLOADED;
    HIP_TRY(hipSetDevice(w->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    unsigned long long v[2] = { 0, 0 };
    HIP_TRY(hipMemcpy(v, w->hbm->work.p + WORK_SLOT_WORDS * w->hbm->work_last, sizeof v, hipMemcpyDeviceToHost));
    *rays = v[1];
    return SVO_OK;
}

int svo_world_prepare_light(svo_world *w, const float light_dir[3], void *stream)
{
    if (!w) return SVO_ERR_INVALID_ARG;
    if (w->device < 0) { set_error("svo_world_prepare_light: world is not uploaded"); return SVO_ERR_NOT_UPLOADED; }
    float sdir[3];
    shadow_direction(light_dir, sdir);
    return prepare_light(*w, sdir, (hipStream_t)stream);
}

int svo_world_prepared_light(svo_world *w, void *stream, float shadow_dir[3], uint64_t *clear_nodes)
{
    if (!w || !shadow_dir || !clear_nodes) return SVO_ERR_INVALID_ARG;
    if (w->device < 0) { set_error("svo_world_prepared_light: world is not uploaded"); return SVO_ERR_NOT_UPLOADED; }
    const LightClearance &c = w->hbm->clear;
    shadow_dir[0] = shadow_dir[1] = shadow_dir[2] = 0.0f;
    *clear_nodes = 0;
    if (!c.prepared()) return SVO_OK;
    std::memcpy(shadow_dir, c.sdir, sizeof c.sdir);
    return c.state == ClearState::UNUSED ? SVO_OK : read_clear_count(*w, (hipStream_t)stream, 0, clear_nodes);
}

int svo_world_prepared_bricks(svo_world *w, void *stream, uint64_t *flagged)
{
    if (!w || !flagged) return SVO_ERR_INVALID_ARG;
    if (w->device < 0) { set_error("svo_world_prepared_bricks: world is not uploaded"); return SVO_ERR_NOT_UPLOADED; }
    *flagged = 0;
    return w->hbm->clear.state == ClearState::BRICKS ? read_clear_count(*w, (hipStream_t)stream, 1, flagged) : SVO_OK;
}

} // extern "C"
