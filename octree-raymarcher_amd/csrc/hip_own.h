// hip_own.h — what the .hip files share: the HIP status mapping, the "one thread per element, blocks of 256" launch with its size
// check and error mapping, block_take and block_sum64 for the numbering and counting kernels, the owners of HIP resources (a call's
// Arena of the pool cache among them) and svo::Hbm, the device half of a world
// (the struct behind svo_world::hbm).  HIP only: world.h stays free of it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "world.h"
#include "light_gate.h"

namespace svo {

inline int hip_status(hipError_t e)
{
    return e == hipErrorOutOfMemory ? SVO_ERR_OUT_OF_MEMORY : (e == hipErrorNoDevice || e == hipErrorInvalidDevice) ? SVO_ERR_NO_DEVICE : SVO_ERR_HIP;
}
#define HIP_TRY(expr)                                                                              \
    do { if (hipError_t e_ = (expr); e_ != hipSuccess) { svo::set_error(std::string(#expr) + ": " + hipGetErrorString(e_)); return svo::hip_status(e_); } } while (0)

inline unsigned blocks_for(uint64_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

// what a launch left behind, as the status and the message of `who`
inline int launch_status(const char *who)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return SVO_OK;
    set_error(std::string(who) + ": " + hipGetErrorString(e));
    return hip_status(e);
}

// n elements at one thread each in blocks of 256 are a grid one launch can have; refused for `who` otherwise (HIP is not touched)
inline int launch_fits(const char *who, int64_t n)
{
    if ((n + 255) / 256 <= 0x7FFFFFFF) return SVO_OK;
    set_error(std::string(who) + ": too many elements for one launch");
    return SVO_ERR_UNSUPPORTED;
}

// kernel(args...), one thread per element of n >= 0 in blocks of 256: nothing for n == 0, launch_fits' refusal, the launch, its status
template <typename... Params, typename... Args>
int launch_per_element(const char *who, int64_t n, hipStream_t s, void (*kernel)(Params...), Args... args)
{
    if (n == 0) return SVO_OK;
    if (const int rc = launch_fits(who, n)) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, args...);
    return launch_status(who);
}

// Consecutive values from *ctr for the threads of a block of BLOCK threads that raise `pred` - ONE global atomic per block.  The
// level-synchronous sweeps number millions of nodes through a handful of counters, and same-address atomics are served one after the
// other (≈ 5.7 ns each here, even at the one per wave the compiler already folds a uniform atomicAdd to: a sweep over 4.8 M nodes took
// 0.86 ms).  Every thread of the block calls this (no early return before it); sh holds BLOCK / 64 + 1 words.
template <unsigned BLOCK> __device__ __forceinline__ uint32_t block_take(uint32_t *ctr, bool pred, uint32_t *sh)
{
    constexpr unsigned WAVES = BLOCK / 64;
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned long long m = __ballot(pred);
    if (lane == 0u) sh[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t tot = 0u;
        for (unsigned w = 0; w < WAVES; ++w) { const uint32_t c = sh[w]; sh[w] = tot; tot += c; }
        sh[WAVES] = tot ? atomicAdd(ctr, tot) : 0u;
    }
    __syncthreads();
    const uint32_t r = sh[WAVES] + sh[wv] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                                        // (sh may serve a second call)
    return r;
}

// The sum of v over the threads of a block of BLOCK threads (a power of two) added to *total, 64 bits - by the same argument ONE
// global atomic per block, none when the sum is 0.  Every thread of the block calls this; sh holds BLOCK words.
template <unsigned BLOCK> __device__ __forceinline__ void block_sum64(unsigned long long v, unsigned long long *sh, unsigned long long *total)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t s = BLOCK / 2; s > 0u; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0u && sh[0] != 0ull) atomicAdd(total, sh[0]);
}

// ---- owners: each frees what it holds, none can be copied; the two that change hands can be moved --------------------------------
struct NoCopy { NoCopy() = default; NoCopy(const NoCopy &) = delete; NoCopy &operator=(const NoCopy &) = delete; };

template <typename T> struct DevBuf {                       // cap elements of device memory
    T *p = nullptr; size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }     // (o frees what this held)
    ~DevBuf() { if (p) (void)hipFree(p); }
    int reserve(size_t n, bool keep, hipStream_t s)         // at least n elements (an empty one: exactly n; else doubling), the old contents copied if `keep`
    {
        if (n <= cap) return SVO_OK;
        DevBuf q; q.cap = std::max(n, cap * 2);
        if (hipMalloc((void **)&q.p, q.cap * sizeof(T)) != hipSuccess) { q.p = nullptr; set_error("device builder: hipMalloc failed"); return SVO_ERR_OUT_OF_MEMORY; }
        if (keep && p && cap) { if (hipMemcpyAsync(q.p, p, cap * sizeof(T), hipMemcpyDeviceToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return SVO_ERR_HIP; }
        *this = std::move(q);
        return SVO_OK;
    }
};

// device memory of the pool cache (device.hip: the large buffers of a world); the handle knows what the cache needs to take it back
hipError_t pool_malloc(void **out, size_t *bytes, int device);      // *bytes: asked for -> handed out (a cached buffer may be larger); *out = null if it fails
void pool_free(void *p, size_t bytes, int device);
template <typename T> struct Pooled {
    T *p = nullptr; size_t bytes = 0; int device = -1;
    Pooled() = default;
    Pooled(Pooled &&o) noexcept : p(o.p), bytes(o.bytes), device(o.device) { o.p = nullptr; o.bytes = 0; }
    Pooled &operator=(Pooled &&o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); std::swap(device, o.device); return *this; }
    ~Pooled() { if (p) pool_free(p, bytes, device); }
    // n elements on `dev`, whatever it held goes back to the cache first
    hipError_t alloc(size_t n, int dev) { *this = Pooled(); bytes = n * sizeof(T); device = dev; return pool_malloc((void **)&p, &bytes, dev); }
};

// The working memory of one call as one buffer of the pool cache carved into 256-byte aligned parts, at least 1 MiB: add() every
// part, alloc(), then at<T>(k).  Declared before the call's SyncAtExit, so that it goes back to the cache behind the work
struct Arena {
    Pooled<unsigned char> mem;
    std::vector<size_t> off;
    size_t bytes = 0;
    size_t add(size_t n) { off.push_back(bytes); bytes += (n + 255) & ~(size_t)255; return off.size() - 1; }
    int alloc(const char *who, int device)
    {
        if (mem.alloc(std::max<size_t>(bytes, (size_t)1 << 20), device) == hipSuccess) return SVO_OK;
        set_error(std::string(who) + ": no device memory for the working arrays");
        return SVO_ERR_OUT_OF_MEMORY;
    }
    template <typename T> T *at(size_t k) const { return reinterpret_cast<T *>(mem.p + off[k]); }
};
struct SyncAtExit { hipStream_t s; ~SyncAtExit() { (void)hipStreamSynchronize(s); } };

template <typename T> struct Pinned : NoCopy {              // n elements of pinned host memory, allocated once
    T *p = nullptr;
    ~Pinned() { if (p) (void)hipHostFree(p); }
    int alloc(size_t n) { if (!p) HIP_TRY(hipHostMalloc((void **)&p, n * sizeof(T))); return SVO_OK; }
};

// What compact.hip and grid.hip keep between calls on a world.  Its builder context (builder.hip) owns them beside the builders' own
// arrays and the loop's (bfs.hip.h: BfsArrays); nothing aliases anything else, a world that uses all of them keeps all of them.
struct LodScratch {
    struct Level { DevBuf<uint32_t> old, kids, slot, cand; DevBuf<uint2> res, cnt; };    // compact.hip: LodLevel says what each holds
    std::vector<Level> lv;
    DevBuf<uint32_t> ctr;                                   // [2 * level + {0, 1}] of sweep A
};
struct GridScratch {
    DevBuf<uint32_t> pyramid, counts;                       // the summary pyramid; [0] MIXED entries above its base, [1] in it
    DevBuf<unsigned char> reduce_tmp;
};
LodScratch &lod_scratch(svo_world &w);
GridScratch &grid_scratch(svo_world &w);

// A chunk rebuilt on the device (trees node words at tree_dev, twigs bricks at twig_dev) takes the place of `chunk`: the old position
// and size, the new depth, the capacities { tree, twig } the caller arrived at (the edits: the old ones, doubled as the reference doubles
// them) or, null, fresh ones fitted to the counts (compact, coarsen, the grid; install_resident_chunk keeps the slot's as the floor).
inline int install_rebuilt(svo_world &w, int chunk, uint32_t depth, const uint64_t *capacity, uint64_t trees, uint64_t twigs, const uint32_t *tree_dev, const uint16_t *twig_dev)
{
    const ChunkPools &old = w.chunks[(size_t)chunk];
    ChunkPools meta;
    std::memcpy(meta.position, old.position, sizeof meta.position);
    meta.size = old.size; meta.depth = depth;
    if (capacity) { meta.tree_capacity = capacity[0]; meta.twig_capacity = capacity[1]; }
    else meta.fit_capacity(trees, twigs);
    meta.trees_on_device = trees; meta.twigs_on_device = twigs;
    return install_resident_chunk(w, chunk, meta, tree_dev, twig_dev);
}

// An event that orders the streams of a world's callers behind one another: created by its first use, destroyed with its owner.
struct Event : NoCopy {
    hipEvent_t e = nullptr;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    // `s` goes on behind the last record(); before the first one there is nothing to wait for (the event is created instead)
    int wait(hipStream_t s) { if (e) HIP_TRY(hipStreamWaitEvent(s, e, 0)); else HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); return SVO_OK; }
    int record(hipStream_t s) { if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); HIP_TRY(hipEventRecord(e, s)); return SVO_OK; }
};

// A scratch buffer of the world that calls on any stream use one after the other.  use() is the only way to it: at least n elements,
// `s` ordered behind the call that used it last, work(buffer), and - if that returned SVO_OK - the mark the next call waits for.
template <typename T> class OrderedScratch {
    DevBuf<T> buf; Event done;
public:
    template <typename Work> int use(size_t n, const char *who, hipStream_t s, Work &&work)
    {
        if (n > buf.cap) {                                  // too small: replaced by one of n elements, once the device is through with the old one
            if (buf.p) HIP_TRY(hipDeviceSynchronize());
            buf = DevBuf<T>();
            if (buf.reserve(n, false, nullptr) != SVO_OK) { set_error(std::string(who) + ": hipMalloc failed"); return SVO_ERR_OUT_OF_MEMORY; }
        }
        if (const int rc = done.wait(s)) return rc;
        if (const int rc = work(buf.p)) return rc;
        return done.record(s);
    }
};

// A float scratch as the ray list of `rays` rays a stage marches on its own: [rays] records of 8 words where the stage keeps the
// march's output there too, then the origins and the directions, [2][rays][3]
struct RayList {
    float *records, *origins, *dirs;
    static size_t floats(int64_t rays, bool with_records) { return (size_t)rays * (with_records ? 14 : 6); }
    RayList(float *p, int64_t rays, bool with_records) : records(with_records ? p : nullptr), origins(p + (with_records ? 8 * rays : 0)), dirs(origins + 3 * rays) {}
};

// The wide-tree builder's scratch in uint32 words from its start (device.hip: wide_layout is the one place that knows it); the
// fronts begin at 0, the scan's own scratch is the tail
struct WideLayout { uint64_t next = 0, flag = 0, rank = 0, wref = 0, wide = 0, wbase = 0, scan = 0, scan_words = 0, total = 0; };

// Light clearance (svo_world_prepare_light; light_clearance.hip.h has the pass, light_gate.h the states, their transitions and the
// launches' use of them): WIDE_CLEAR_BIT of the wide pool's EMPTY entries and BMAT_CLEAR_BIT of the bricks, as `state` says, for `sdir`
struct LightClearance {
    ClearState state = ClearState::FRESH;
    float sdir[3] = { 0.0f, 0.0f, 0.0f };                   // the prepared shadow direction (UNUSED, NODES, BRICKS)
    Pooled<uint4> place;                                    // the pass's scratch: 16 bytes per wide node, kept until the pools change
    DevBuf<unsigned long long> count;                       // [0] EMPTY reference nodes found clear, [1] bricks flagged
    Event built;                                            // launches that use the bits wait for it
    bool prepared() const { return state == ClearState::UNUSED || state == ClearState::NODES || state == ClearState::BRICKS; }
};

// What an uploaded world keeps on the device.  release_device (device.hip) lets go of it as a whole.
struct Hbm {
    DevBuf<DevChunk> chunks; DevBuf<DevWide> wchunks;       // the chunk tables (host mirrors: svo_world::table / wtable)
    Pooled<uint32_t> tree; Pooled<uint64_t> mask;
    Pooled<uint16_t> twig, bmat;                            // bmat: per brick its one material / 0 (empty) / 0xFFFF (several), written with the masks; bit 15: the clear flag
    Pooled<uint32_t> wide, wbase;                           // wide tree of every chunk (wide_tree.hip.h) and, per wide node, the reference blocks it expands
    Pooled<uint32_t> wscratch; WideLayout wlayout;          // the wide builder's scratch and how it is laid out
    Pinned<uint32_t> wide_tail;                             // the wide builder's per-level read-back
    DevBuf<unsigned long long> work;                        // WORK_SLOTS x {tile cursor, rays marched}: one slot per launch in flight
    unsigned work_next = 0, work_last = 0;                  // ring cursor; slot of the most recent launch
    Event work_done[WORK_SLOTS];                            // recorded behind the launch that used the slot
    OrderedScratch<unsigned char> sort;                     // svo_tile_order
    OrderedScratch<float> cont;                             // svo_trace_translucent: a RayList without records, one ray per pixel
    OrderedScratch<float> mirror;                           // svo_trace_reflections: a RayList without records, one ray per pixel
    OrderedScratch<float> local;                            // svo_trace_local_shadows: a RayList with records, one ray per pixel and light asked for
    OrderedScratch<float> lights;                           // svo_trace_lights: a RayList with records of `cap` slots, the block counts, their sums, the scan's own
    OrderedScratch<float> instances;                        // svo_trace_instances, on the MODEL: a RayList with records and far ends of `cap` slots, the pair masks, the ranks
    OrderedScratch<float> instance_shadows;                 // svo_trace_instance_shadows, on the MODEL: the same without far ends
    OrderedScratch<float> instance_scene;                   // svo_trace_instance_shadows, on the SCENE: a RayList with records, one ray per pixel
    OrderedScratch<float> shadowmap;                        // svo_shadowmap_render: a RayList with records, one ray per texel in tile order
    // see-through view (svo_trace_params.see_through, see_through.hip.h): the wide and mask pools with one material taken out, built
    // on the device at the first launch that asks for it, dropped by every change to the pools
    Pooled<uint32_t> view_wide; Pooled<uint64_t> view_mask;
    uint32_t view_material = 0;                             // material the view holds; 0 = no view
    Event view_built;                                       // launches on other streams wait for it
    // parent index (svo_hit_voxels, hit_voxels.hip.h): per 8-block of the tree pool the chunk-relative index of the BRANCH that owns it
    // and the block's level (0 = not reachable), and per chunk its node count; built on the device at the first svo_hit_voxels call,
    // dropped by every change to the pools
    Pooled<uint32_t> parent; Pooled<uint8_t> parent_level; DevBuf<uint32_t> chunk_trees;
    bool parents_ok = false;                                // the build has been issued
    Event parents_built;                                    // calls on other streams wait for it
    LightClearance clear;
    int stack_blocks[24] = {};                              // persistent-grid size per k_trace_stack instantiation (device.hip: STACK_KERNELS); 0 = not queried yet
};

} // namespace svo
