// world.h — the svo_world handle behind include/svo.h.
#pragma once
#include <new>
#include <string>
#include <vector>
#ifdef __HIP__
#include <hip/hip_runtime_api.h>
#endif
#include "../../include/svo.h"
#include "svo_format.h"
#include "terrain.h"

namespace svo { struct Hbm; }

struct svo_world {
    // World (src/World.h:44-57)
    int width = 0, height = 0, depth = 0, chunksize = 0;
    int chunkcoordmin[3] = { 0, 0, 0 };
    std::vector<svo::ChunkPools> chunks;          // World::index() order
    svo::TerrainParams terrain;                   // generator parameters (svo_world_generate), for svo_world_shift
    bool has_terrain = false;

    // geometry class
    bool exact_geometry = false;                  // every voxel corner is an exact float
    int  max_levels = 0;                          // max over chunks of depth - TWIG_LEVELS

    // device residency: the numbers the host half reads; everything HIP owns is behind `hbm` (hip_own.h), which only the .hip files see
    int device = -1;
    svo::Hbm *hbm = nullptr;                      // non-null exactly while device >= 0 (alloc_pools / release_device)
    std::vector<svo::DevChunk> table; std::vector<svo::DevWide> wtable;    // host mirrors of hbm->chunks / wchunks
    std::vector<uint64_t> tree_slot, twig_slot, wide_slot;   // capacity of each chunk's slots (nodes / bricks / wide nodes)
    uint64_t tree_pool_len = 0, twig_pool_len = 0;    // elements in use (incl. alignment padding)
    uint64_t tree_pool_cap = 0, twig_pool_cap = 0;    // elements allocated
    uint64_t wide_pool_len = 0, wide_pool_cap = 0, wide_nodes_used = 0;
    bool wide_ok = false;                         // the wide pool is complete: every chunk's bricks fit the 26-bit payload and the build succeeded
    void *builder_ctx = nullptr;                  // builder.hip: working buffers svo_world_shift / svo_world_edit_box keep between calls
};

namespace svo {
constexpr unsigned WORK_SLOTS = 64;               // launches of one world that overlap freely; the 65th waits (on the device) for the 1st
void set_error(const std::string &msg);
// the C ABI's fence against std::bad_alloc: f's status, or "<who>: out of host memory"
template <class F> int fenced(const char *who, F &&f)
{
    try { return f(); }
    catch (const std::bad_alloc &) { set_error(std::string(who) + ": out of host memory"); return SVO_ERR_OUT_OF_MEMORY; }
}
int  validate_chunk(const ChunkPools &c, std::string &why);
bool chunk_is_exact(const ChunkPools &c, int chunksize);
void classify_world(svo_world &w);
// device.hip: frees the world's device copy; keep_builder keeps builder_ctx (a re-pack on the same device, maybe by one of the builders)
int  release_device(svo_world &w, bool keep_builder = false);
// device.hip: HBM residency building blocks shared by svo_world_upload and the device-resident generator
void plan_pools(svo_world &w);                    // slots, offsets and pool sizes from the chunks' capacities (host only)
int  alloc_pools(svo_world &w, int device);       // hipMalloc + clear of the pools planned above; sets w.device and w.hbm
#ifdef __HIP__
// node words [tl, tr) and bricks [bl, br) of chunk i from host vectors (hipMemcpyHostToDevice, synchronous) or device buffers
// (hipMemcpyDeviceToDevice, on `stream`) into its slots, then the masks of those bricks
int  copy_chunk(svo_world &w, int i, const uint32_t *tree, const uint16_t *twig, hipMemcpyKind kind,
                uint64_t tl, uint64_t tr, uint64_t bl, uint64_t br, void *stream);
#endif
int  fetch_pools(svo_world &w, int chunk);        // node words / bricks that live only on the device -> host copy of that chunk
int  build_wide_all(svo_world &w, void *stream);  // wide trees (wide_tree.hip.h) of all chunks from the node words in the tree pool
// a chunk built on the device (its pools at tree_dev / twig_dev, meta.trees_on_device nodes / meta.twigs_on_device bricks) takes
// slot `chunk` of an uploaded world: device-to-device, no host copy made, through svo_world_update's install path
int  install_resident_chunk(svo_world &w, int chunk, const ChunkPools &meta, const uint32_t *tree_dev, const uint16_t *twig_dev);
int  rebuild_wide_chunk(svo_world &w, int chunk, void *stream);
// builder.hip: World::init on the device, pools left in HBM (the world is uploaded to `device` when this returns)
int  generate_world_resident(svo_world &w, int device);
void free_builder_context(svo_world &w);
// builder.hip: Ocroot::build / destroy / replace + World::modify on an uploaded world
int  edit_box_resident(svo_world &w, int chunk, int op, const float lo[3], const float hi[3], uint32_t material);
// builder.hip: the same edit with the closed ball |p - centre| <= radius as its region
int  edit_ball_resident(svo_world &w, int chunk, int op, const float centre[3], float radius, uint32_t material);
// builder.hip: World::shift's entering plane generated on the device the world is uploaded to
int  shift_world_resident(svo_world &w, int axis, int sign);
// builder.hip: the edit's output pools, which svo_world_edit_box keeps between calls, lent to compact.hip and grid.hip (grown to
// `trees` node words and `twigs` bricks)
int  edit_scratch(svo_world &w, uint64_t trees, uint64_t twigs, uint32_t **tree, uint16_t **twig);
// compact.hip: Ocroot::defragcopy (lod = false) or Ocroot::lodmm (lod = true) + World::modify on an uploaded world
int  rebuild_resident(svo_world &w, int chunk, bool lod);
} // namespace svo

#include "chunk_pools.h"                          // validate_chunk's forward pass; it comes with the declaration (it needs the ones above)
