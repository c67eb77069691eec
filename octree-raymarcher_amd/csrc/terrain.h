// terrain.h — host-side chunk pools and the terrain generator of libsvo_amd.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "svo_format.h"

namespace svo {

// Ocdelta (src/Octree.h:47-54): dirty node / brick index range of an edit.
struct DirtyRange {
    uint64_t left = UINT64_MAX, right = 0;
    bool realloc = false;
};

// The host copy of one chunk == Ocroot (src/Octree.h:56-76).
struct ChunkPools {
    float    position[3] = { 0, 0, 0 };
    float    size = 0;
    uint32_t depth = 0;
    uint64_t tree_capacity = 16, twig_capacity = 16;   // treestoragesize / twigstoragesize
    std::vector<uint32_t> tree;                        // node words
    std::vector<uint16_t> twig;                        // 64 cells per brick
    // > 0: the chunk was built on the device and its bricks have not been fetched to the host yet (`twig` is empty);
    // svo_world_chunk / a move to another device fetch them (device.hip: fetch_pools)
    uint64_t twigs_on_device = 0;
    uint64_t twig_count() const { return twigs_on_device ? twigs_on_device : twig.size() / TWIG_WORDS; }
    // the same for the node words (`tree` is empty until fetched): the device builder runs Ocroot::build on the device too
    uint64_t trees_on_device = 0;
    uint64_t tree_count() const { return trees_on_device ? trees_on_device : tree.size(); }
    void reserve_tree(uint64_t need);
    // the capacities of a chunk whose pools arrive whole (svo_world_create / _update, compact, coarsen): doubled until `trees` node
    // words with a block of 8 to spare and `twigs` bricks fit
    void fit_capacity(uint64_t trees, uint64_t twigs);
};

// What one height pyramid is built from (column_pyramid below).
struct ColumnPyramid { uint32_t res; float amplitude, period, xshift, yshift, zshift; };

// BoundsPyramid (src/BoundsPyramid.h) as one flat array per bound.
struct HeightPyramid {
    uint32_t size = 0, levels = 0;
    float amplitude = 0, shift = 0;
    std::vector<float> lo, hi;                         // level lv at level_offset(lv), (2^lv)^2 entries
    static size_t level_offset(uint32_t lv) { return (((size_t)1 << (2 * lv)) - 1) / 3; }
    void  build(const ColumnPyramid &a);
    float bound(const std::vector<float> &q, float x, float z, uint32_t lv) const;
    float min(float x, float z, uint32_t lv) const { return bound(lo, x, z, lv); }
    float max(float x, float z, uint32_t lv) const { return bound(hi, x, z, lv); }
};

struct TerrainParams {
    uint32_t depth = 8, pyramid_resolution = 0;
    float amplitude = 64.0f, yshift = 16.0f;
    int32_t seed = 0, water = 1;
    float water_level = 6.0f;
    uint32_t water_material = 6;
    int32_t threads = 0;
    uint32_t coarse_depth = 0;                         // sparse refinement, see include/svo.h
    float refine_min[3] = { 0, 0, 0 }, refine_max[3] = { 0, 0, 0 };
};

float simplex2(float x, float y);
void  grow_chunk(ChunkPools &c, const float position[3], float size, uint32_t depth, const HeightPyramid &pyr,
                 const TerrainParams *sparse = nullptr);
void  fill_box(ChunkPools &c, const float lo[3], const float hi[3], uint16_t material, DirtyRange &dtree, DirtyRange &dtwig);

// ---- the terrain window walk: which chunks a terrain world holds and how each is grown (World::init, World::shift) ----
inline int positive_mod(int n, int m) { return (m + (n % m)) % m; }   // src/World.cpp:276-279
// World::index (src/World.cpp:288-293): the slot of chunk (x, y, z) in a w x h x d toroidal grid
inline int chunk_index(int x, int y, int z, int w, int h, int d) { return positive_mod(y, h) * w * d + positive_mod(z, d) * w + positive_mod(x, w); }
// the base resolution of a column's height pyramid: one texel per voxel column of a chunk unless `requested` says otherwise
inline uint32_t pyramid_resolution_or_default(uint32_t requested, uint32_t depth) { return requested ? requested : (1u << depth); }

// World::g_pyramid (src/World.cpp:296-306): the height pyramid of chunk column (cx, cz)
ColumnPyramid column_pyramid(const TerrainParams &tp, int cx, int cz);

// A box [lo, hi) of chunk coordinates in a world's toroidal grid, walked column by column - z outer, x inner, y innermost -
// because the chunks of one (x, z) column share one height pyramid.  World::init's window is the whole grid at chunkcoordmin,
// World::shift's the plane that enters the grid.
struct TerrainWindow {
    int lo[3], hi[3];
    int grid[3];                                       // the world's width, height, depth
    int chunksize;
    struct Chunk { int x, y, z, index; float position[3]; };

    static TerrainWindow whole(int w, int h, int d, int chunksize, const int ccm[3])
    { return { { ccm[0], ccm[1], ccm[2] }, { ccm[0] + w, ccm[1] + h, ccm[2] + d }, { w, h, d }, chunksize }; }
    TerrainWindow entering(int axis, int sign) const;  // the plane that enters when the window steps by `sign` (+-1) along `axis`
    int   column_height() const { return hi[1] - lo[1]; }
    int   size() const { return (hi[0] - lo[0]) * column_height() * (hi[2] - lo[2]); }
    Chunk chunk(int k) const;                          // k-th of the walk; a column's first at k % column_height() == 0
};
// World::g_chunk (src/World.cpp:308-321) for every chunk of `win`: grown, then the water filled in, in walk order; the columns
// are spread over tp.threads host threads.  -1: a thread ran out of host memory.
int generate_window(const TerrainWindow &win, const TerrainParams &tp, std::vector<ChunkPools> &chunks);

} // namespace svo
