/*
 * svo.h — C ABI of the MI355X-native sparse-voxel-octree ray traverser.
 *
 * This is the drop-in boundary for the ONE hot path of jfjell/Octree-Raymarcher that this
 * repository rebuilds: the per-pixel SVO march.  Every entry point names the reference
 * interface it replaces (paths relative to the reference checkout):
 *
 *   svo_world_generate   <- World::init / g_pyramid / g_chunk      src/World.cpp:19-43,296-321
 *                           grow()                                 src/Octree.cpp:74-176
 *                           BoundsPyramid::init                    src/BoundsPyramid.cpp:47-78
 *                           Ocroot::build (water plane)            src/Octree.cpp:319-436
 *   svo_world_create     <- a World whose chunk[] the caller already owns (Ocroot, src/Octree.h:56-76)
 *   svo_chunk_from_grid / svo_world_chunk_from_grid <- grow() (src/Octree.cpp:74-176) over a grid instead of the height pyramid
 *   svo_world_chunk_to_grid <- (no counterpart) the chunk's voxels back as a dense grid
 *   svo_chunk_from_mesh / svo_world_chunk_from_mesh <- (no counterpart) the tree of a triangle mesh's shell without the dense grid, to
 *                           depth 16, on the host or on the device
 *   svo_chunk_fill_enclosed / svo_world_chunk_fill_enclosed <- (no counterpart) the cells a chunk's voxels enclose, filled on the tree
 *                           without a dense grid, to depth 16, on the host or on the device
 *   svo_chunk_combine / svo_world_chunk_combine <- (no counterpart) two chunks of one depth combined cell by cell on their trees
 *   svo_chunk_stamp / svo_world_chunk_stamp <- (no counterpart) a chunk placed into another at a cell offset, in one of 48 orientations
 *                           (union, B under / over A, subtraction, intersection), to depth 16, on the host or on the device
 *   svo_chunk_extract / svo_world_chunk_extract <- (no counterpart) the stamp's inverse: a cube of cells copied out of a chunk at a cell
 *                           offset, in one of 48 orientations, into a chunk of its own, to depth 16, on the host or on the device
 *   svo_grid_add_mesh / svo_device_grid_add_mesh <- (no counterpart: the reference rasterises its one mesh, src/Worm.cpp, with GL) a
 *                           triangle mesh voxelised into a dense grid, on the host or in device memory
 *   svo_grid_fill_enclosed / svo_device_grid_fill_enclosed <- (no counterpart) the cells that such a shell encloses, filled
 *   svo_world_upload     <- World::load_gpu + RootAllocator::alloc src/World.cpp:57-94, src/Allocator.cpp:28-35
 *   svo_world_update     <- World::modify + RootAllocator::subst   src/World.cpp:268-274, src/Allocator.cpp:37-55
 *   svo_trace            <- World::draw (+ draw_shadowmap)         src/World.cpp:162-266
 *                           fragment main                          shaders/World.Fragment.glsl:162-203
 *   svo_trace_frames     <- several World::draw calls in one launch (the frame's light and eye passes,
 *                           src/Main.cpp:190-222; stereo / split-screen views; a pipelined renderer's next frames)
 *   svo_trace_rows(_frames) <- the same over the interleaved row bands of one rank (multi-GPU partition)
 *   svo_trace_rays       <- chunkmarch over a ray list             src/Traverse.cpp:127-171
 *   svo_trace_segments   <- (no counterpart: chunkmarch has no far end) the same list with a far end per ray: line of sight,
 *                           picking with a reach, short occlusion rays, a light inside the world
 *   svo_tile_order       <- (no counterpart: the GL rasteriser schedules fragments itself) longest-first tile order of the
 *                           next World::draw from the previous one's per-tile step counts
 *   svo_world_destroy    <- World::deinit                          src/World.cpp:129-151
 *   svo_world_index*     <- World::index / index_float             src/World.cpp:276-293,323-332
 *   svo_world_locate     <- World::index_float + World::index (src/World.cpp:288-293,323-332) + traverse (src/Traverse.cpp:34-48)
 *                           + the cell lookup of twigmarch (:58-67) over a device point list
 *   svo_hit_voxels       <- hit.bmin / hit.size, the Leaf that rootmarch hands to fragment main (shaders/World.Fragment.glsl:168-172): the box
 *                           traverse() holds at the hit node (src/Traverse.cpp:34-48) and twigmarch's leafmin / leafsize (:66), from the
 *                           record's ids; what the caller's edit cursor is placed from (src/Main.cpp:317,340-367)
 *   svo_hit_uv           <- leafUV on cubeUV                        shaders/World.Fragment.glsl:5-15, shaders/Chunkmarch.glsl:138-149
 *   svo_shade_textured   <- texture(Diffuse / Specular, uv) in fragment main   shaders/World.Fragment.glsl:178-190, src/Atlas.cpp:18-32
 *   svo_chunk_write/read <- Ocroot::write / Ocroot::read           src/Octree.cpp:178-201
 *   svo_world_shift      <- World::shift                           src/World.cpp:334-378
 *   svo_world_edit_box   <- Ocroot::build / destroy / replace + World::modify   src/Octree.cpp:203-443, src/World.cpp:268-274
 *                           (the caller's pattern: src/Main.cpp:340-367)
 *   svo_world_compact    <- Ocroot::defragcopy + World::modify(realloc)   src/Octree.cpp:445-614, src/World.cpp:268-274
 *   svo_world_coarsen    <- Ocroot::lodmm + World::modify(realloc)        src/Octree.cpp:626-765, src/MisraGries.h
 *                           (the caller's pattern: key 'g', src/Main.cpp:438-448)
 *   svo_shade(_packed)   <- lighting of fragment main               shaders/World.Fragment.glsl:63-138,180-197
 *   svo_trace_params.see_through <- the `ignore` material of treemarch / twigmarch   shaders/Chunkmarch.glsl:190-191,240-241,280
 *   svo_trace_translucent <- the second march from a translucent hit   shaders/ParallaxAlpha.Fragment.glsl:141-199,276-335
 *   svo_shade_translucent <- its blend by the path length through the liquid   shaders/ParallaxAlpha.Fragment.glsl:226-234,315-323
 *   svo_shade_sky        <- Skybox::draw behind the world (src/Main.cpp:227)   src/Skybox.cpp, shaders/Skybox.*.glsl
 *   svo_frame_rgba8      <- the RGBA8 colour attachment and its alpha of 1     src/GBuffer.cpp, shaders/GBuffer.Fragment.glsl
 *   svo_cursor_place     <- computeTarget + ImaginaryCube::position      src/Main.cpp:314-319, src/ImaginaryCube.cpp:59-62
 *   svo_shade_boxes      <- ImaginaryCube::draw and the lights' marker cubes over the finished image (src/Main.cpp:223-225)
 *                           src/ImaginaryCube.cpp:64-87, shaders/Imag.Fragment.glsl, src/Light.cpp:141-155, shaders/Light.Fragment.glsl
 *   svo_world_edit_cube  <- modify(): one cube to every chunk that holds one of its corners   src/Main.cpp:321-368
 *   svo_world_edit_ball  <- (no counterpart; the reference edits cubes only) destroyCube / buildCube with a closed ball as the region
 *   svo_world_edit_ball_all <- (no counterpart; the reference edits cubes only) one ball to every chunk whose box it touches
 *   svo_trace_local_shadows <- (a departure: the reference gives the directional light's shadow term to all three lights,
 *                           shaders/World.Fragment.glsl:186-190) one occlusion ray per hit towards the point light and the spotlight
 *   svo_trace_lights     <- (a departure: the reference has three lights, src/Main.cpp:101-131) up to 32 point lights with a reach
 *                           each, one occlusion ray per hit and light that can reach it, in one compacted ray list
 *   svo_shade_lights     <- (a departure, with it) computePointLight_BlinnPhong (shaders/World.Fragment.glsl:80-97) per light of
 *                           the list, windowed to the reach, added to the shaded image
 *   svo_trace_instances  <- (a departure: the reference's only moving object is a rasterised mesh, src/Worm.cpp) up to 32 placements
 *                           of one voxel model, marched in the model's own space and folded into the frame; svo_trace_instance_shadows: their shadows
 *   svo_shadowmap_render <- World::draw_shadowmap under the OrthoCamera (src/World.cpp:162-203, shaders/ShadowmapWorld.Fragment.glsl,
 *                           src/Main.cpp:149,190-198): the world marched once from the directional light into a depth image
 *   svo_shadowmap_apply  <- computeShadow                          shaders/World.Fragment.glsl:140-155,186
 *   svo_shadowmap_fit    <- the OrthoCamera's placement and glm::ortho(-w, w, -h, h)   src/Main.cpp:149, src/Camera.cpp:50-53
 *   svo_hit_ao           <- (a departure: the reference has no ambient occlusion; its ambient term is one constant per material,
 *                           shaders/World.Fragment.glsl:63-73) contact darkening from the eight lattice cells around each hit's face
 *   svo_shade_ao         <- (a departure, with it) that factor on the shaded image
 *   svo_trace_reflections <- (a departure: the reference has no reflections) one mirror ray per hit of a material, off the axis-aligned
 *                           face of the voxel that was hit
 *   svo_shade_reflections <- (a departure, with it) what those rays saw, blended over the shaded image by a Fresnel term
 *
 * Conventions
 *   - plain C, opaque handle, caller owns every buffer it passes in;
 *   - every function returns an int status: SVO_OK (0), a positive "done, but" status (SVO_OK_LITERAL_ONLY) or a negative
 *     svo_status (nothing was changed unless the entry point says otherwise); nothing aborts
 *     or throws across this boundary (the reference uses assert/die(), src/Util.cpp:72-78);
 *   - pointers named *_dev are DEVICE pointers (HBM of the device the world was uploaded to),
 *     all others are host pointers;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); launches are
 *     asynchronous on that stream, no host synchronisation happens inside svo_trace*;
 *   - one handle may be used by one host thread at a time; different handles are independent;
 *   - svo_trace* launches of one world may overlap on different streams (frames in flight); each
 *     launch owns a private work-cursor slot from a 64-entry ring, and a launch that comes round
 *     to a slot still in use is ordered on the device behind that earlier launch;
 *   - svo_world_update / svo_world_shift / svo_world_edit_box / svo_world_edit_ball(_all) / svo_world_compact / svo_world_coarsen /
 *     svo_world_chunk_from_grid / svo_world_chunk_from_mesh / svo_world_upload are ordered behind every launch issued before them on any stream
 *     (they drain the device before touching HBM, as World::modify is ordered on the GL queue) and have completed when they return: launches issued afterwards see
 *     the new world, launches issued before saw the old one, none sees a mixture.
 *
 * Semantics are those of the reference's CPU march (src/Traverse.cpp): EPS = 1/8192, step caps
 * 1000/1000/1000, closed-box containment, restart-from-root descent.  The extra per-hit outputs
 * (voxel box -> normal, material) follow shaders/Chunkmarch.glsl:128-136,190-295 and
 * shaders/World.Fragment.glsl:162-178.  There is no CPU fallback in this library: without a
 * usable HIP device every device entry point returns SVO_ERR_NO_DEVICE.
 */
#ifndef SVO_H
#define SVO_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVO_ABI_VERSION 4           /* 2: svo_trace_params.normal_mode, SVO_FACE_NORMAL, error bit in the packed record
                                       3: svo_trace_params.tile_cost_dev / tile_order_dev, svo_tile_order
                                       4: SVO_OK_LITERAL_ONLY, svo_device_cache_trim, svo_trace_params.semantics;
                                          4 later gained svo_world_compact and svo_world_coarsen (functions added, nothing changed),
                                          svo_trace_params.see_through (was padding: zeroed structs keep their results),
                                          svo_trace_translucent and svo_shade_translucent,
                                          svo_trace_local_shadows and SVO_LOCAL_SHADOWS / SVO_SHADOWED_POINT / SVO_SHADOWED_SPOT,
                                          svo_trace_segments,
                                          svo_world_locate and svo_voxel,
                                          svo_hit_voxels, svo_hit_uv, svo_shade_textured and svo_atlas,
                                          svo_shade_sky, svo_sky and svo_frame_rgba8,
                                          svo_cursor_place, svo_shade_boxes, svo_box and svo_world_edit_cube,
                                          svo_chunk_from_grid, svo_world_chunk_from_grid and svo_world_chunk_to_grid,
                                          svo_world_edit_ball and svo_world_edit_ball_all,
                                          svo_shadowmap, svo_shadowmap_fit, svo_shadowmap_render and svo_shadowmap_apply,
                                          svo_hit_ao and svo_shade_ao,
                                          svo_trace_reflections, svo_shade_reflections and svo_mirror,
                                          svo_world_prepare_light, svo_world_prepared_light and SVO_SHADOW_NO_CLEARANCE (a bit of
                                          svo_trace_params.shadow, which was any non-zero value: such callers keep their results),
                                          svo_world_prepared_bricks and SVO_SHADOW_NO_BRICK_CLEARANCE (another such bit),
                                          svo_trace_lights, svo_shade_lights, svo_light and SVO_MAX_LIGHTS,
                                          svo_trace_instances, svo_trace_instance_shadows, svo_instance and SVO_MAX_INSTANCES,
                                          svo_grid_add_mesh, svo_device_grid_add_mesh, svo_grid_fill_enclosed,
                                          svo_device_grid_fill_enclosed and svo_mesh,
                                          svo_chunk_from_mesh, svo_world_chunk_from_mesh and SVO_MESH_MIN_DEPTH / SVO_MESH_MAX_DEPTH,
                                          svo_chunk_fill_enclosed, svo_world_chunk_fill_enclosed and SVO_FILL_MIN_DEPTH / SVO_FILL_MAX_DEPTH,
                                          svo_chunk_combine, svo_world_chunk_combine, SVO_COMBINE_* and SVO_COMBINE_MIN_DEPTH / SVO_COMBINE_MAX_DEPTH,
                                          svo_chunk_stamp, svo_world_chunk_stamp, svo_placement and SVO_STAMP_MIN_DEPTH / SVO_STAMP_MAX_DEPTH,
                                          svo_chunk_extract, svo_world_chunk_extract and SVO_EXTRACT_MIN_DEPTH / SVO_EXTRACT_MAX_DEPTH
                                          (functions added, nothing changed) */

typedef enum svo_status {
    SVO_OK                 =  0,
    SVO_OK_LITERAL_ONLY    =  1,   /* svo_world_upload / svo_world_generate on a device: the world IS resident;
                                      svo_world_update / svo_world_edit_box / svo_world_shift: the change HAS been applied - every
                                      later launch sees the new world - but the stack kernel's wide trees could not be rebuilt (out
                                      of device memory, mostly): SVO_KERNEL_AUTO marches with the literal kernel, SVO_KERNEL_STACK is
                                      refused, until a later update / edit / shift / upload rebuilds them.  svo_last_error() says why */
    SVO_ERR_INVALID_ARG    = -1,
    SVO_ERR_NO_DEVICE      = -2,   /* no HIP device / HIP call failed; see svo_last_error() */
    SVO_ERR_OUT_OF_MEMORY  = -3,
    SVO_ERR_MALFORMED_TREE = -4,   /* node word points outside its pool, cycles, too deep */
    SVO_ERR_NOT_UPLOADED   = -5,
    SVO_ERR_UNSUPPORTED    = -6,
    SVO_ERR_HIP            = -7
} svo_status;

/* Node word (src/Octree.h:8-26, src/Octree.cpp:38-53): type = value >> 30, offset = value & 0x3FFFFFFF. */
enum { SVO_EMPTY = 0, SVO_LEAF = 1, SVO_BRANCH = 2, SVO_TWIG = 3 };
#define SVO_TWIG_LEVELS 2           /* src/Octree.h:30-33 */
#define SVO_TWIG_SIZE   4
#define SVO_TWIG_WORDS  64          /* uint16 cells per brick, index z*16 + y*4 + x */

/* One chunk as the caller holds it on the host == the public part of Ocroot (src/Octree.h:56-76).
 * tree[0] is the root; a BRANCH's 8 children are contiguous, slot = x + 2y + 4z. */
typedef struct svo_chunk_desc {
    float           position[3];
    float           size;
    uint32_t        depth;          /* leaf voxel edge = size / 2^depth; TWIG nodes sit at level depth-2 */
    uint32_t        _pad;
    const uint32_t *tree;
    uint64_t        trees;
    const uint16_t *twig;           /* twigs * 64 cells */
    uint64_t        twigs;
} svo_chunk_desc;

/* Terrain parameters of World::g_pyramid / g_chunk (src/World.cpp:296-321). */
typedef struct svo_terrain_params {
    uint32_t depth;                 /* TREE_MAX_DEPTH, reference 8 */
    uint32_t pyramid_resolution;    /* PYRAMID_RESOLUTION, reference 256; 0 = 2^depth */
    float    amplitude;             /* 64 */
    float    yshift;                /* 16 */
    int32_t  seed;                  /* integer offset added to the noise x/z shift; reference = 0 */
    int32_t  water;                 /* !=0: Ocroot::build(y < water_level, water_material) */
    float    water_level;           /* 6 */
    uint32_t water_material;        /* 6 */
    int32_t  threads;               /* host threads for generation; 0 = hardware concurrency */
    /* Sparse refinement (a build extension for deep trees, BASELINE configs[4]; 0 = off = the reference):
     * a node at level coarse_depth-2 whose box does not touch [refine_min, refine_max] (world units,
     * closed) becomes a brick sampled at level coarse_depth by the rule of src/Octree.cpp:120-154 instead
     * of being subdivided down to depth-2.  Full depth only inside the refine box. */
    uint32_t coarse_depth;
    float    refine_min[3];
    float    refine_max[3];
    /* 0 = generate on host threads; k > 0 = generate on HIP device k-1 (noise, mips, the level-synchronous BFS and
     * the water fill as kernels, bit-identical pools that never visit the host). */
    int32_t  build_device_plus1;
} svo_terrain_params;

/* Pinhole camera of the build (the reference rasterises the world box and uses
 * normalize(hitpoint - eye), shaders/World.Fragment.glsl:165; one ray per pixel here).
 * dir(px,py) = normalize(forward + right*u + up*v),
 *   u = (((px+0.5)/width )*2 - 1) * tan_half_x,   v = (1 - ((py+0.5)/height)*2) * tan_half_y,
 * all in float, no FMA contraction.  The caller supplies the orthonormal basis and the tangents. */
typedef struct svo_camera {
    float   eye[3];
    float   forward[3];
    float   right[3];
    float   up[3];
    float   tan_half_x;
    float   tan_half_y;
    int32_t width;                  /* full image size the pixel coordinates refer to */
    int32_t height;
} svo_camera;

enum {                              /* svo_trace_params.kernel */
    SVO_KERNEL_AUTO    = 0,         /* fastest kernel valid for this world */
    SVO_KERNEL_LITERAL = 1,         /* one thread per ray, restart-from-root, any geometry */
    SVO_KERNEL_STACK   = 2          /* persistent waves, LDS descent stack, ballot refill: exact geometry, chunk depth <= 24
                                       (chunks of one world may differ in depth); worlds beyond 4 GiB of wide nodes get its
                                       large-world instantiation; SVO_ERR_UNSUPPORTED otherwise (AUTO falls back to LITERAL) */
};

typedef struct svo_trace_params {
    float    eps;                   /* 0 = 1/8192 (src/Traverse.cpp:8) */
    int32_t  max_chunk_steps;       /* 0 = 1000   (src/Traverse.cpp:142) */
    int32_t  max_tree_steps;        /* 0 = 1000   (src/Traverse.cpp:79) */
    int32_t  max_twig_steps;        /* 0 = 1000   (src/Traverse.cpp:54) */
    int32_t  shadow;                /* !=0: one shadow ray per primary hit toward -light_dir.  Bit SVO_SHADOW_NO_CLEARANCE (2 or 3 instead
                                       of 1): the same shadow rays, never ended early by svo_world_prepare_light's bits - the same records,
                                       more steps; for A/B runs.  Bit SVO_SHADOW_NO_BRICK_CLEARANCE (5 instead of 1): the bits are used, the
                                       per-brick flags that settle a lit shadow ray at its primary hit are not.  Bit
                                       SVO_SHADOW_NO_DARK_BIRTH (9 instead of 1): a shadow ray whose origin lies in an occupied cell of the
                                       brick its primary ray hit is marched (two steps) instead of being settled "shadowed" at the hit;
                                       SVO_SHADOW_NO_CLEARANCE and SVO_SHADOW_NO_BRICK_CLEARANCE (no shadow ray is settled at its primary hit)
                                       switch that off too.  The same records with every combination */
    float    light_dir[3];          /* directionalLight.direction, default normalize(1,-1,0) (src/Main.cpp:116) */
    int32_t  kernel;                /* SVO_KERNEL_* */
    int32_t  tiles_per_wave;        /* SVO_KERNEL_STACK launch shape: every persistent wave is handed at least this
                                       many 8x8-pixel tiles.  0 / 1 = as many waves as there are tiles (up to what the
                                       device keeps resident): shortest single frame.  4 suits small images with
                                       several frames in flight (waves keep refilling instead of draining) */
    uint32_t *counters_dev;         /* optional [n][4] u32 per ray: node words, brick cells, chunk
                                       descriptors, tree steps (reference restart-from-root counts);
                                       only honoured by SVO_KERNEL_LITERAL */
    int32_t  normal_mode;           /* SVO_NORMAL_CUBE (0): svo_hit.normal = the reference's cubeNormal, bit for bit - NaN where
                                       its integer vector is (0,0,0): 0.1 % of the hits at depth 8, 14 % at depth 12.
                                       SVO_NORMAL_FACE (1): the unit vector of the voxel face the sample point
                                       alpha + beta*(t - EPS) lies closest to (axis of the largest |point - centre|, first axis
                                       on ties; signed like that component, against the ray if it is exactly 0) - the face the
                                       ray entered through, defined for every hit; such records carry SVO_FACE_NORMAL */
    int32_t  launches_in_flight;    /* SVO_KERNEL_STACK launch shape: how many launches of this world the caller keeps in flight on different
                                       streams (0 / 1 = one: the launch takes every wave slot of the device - shortest single launch).
                                       With n >= 2 a launch takes 2/n of the wave slots, so that at least two launches are resident
                                       side by side and one's drain (its longest rays) runs under another's bulk instead of
                                       holding slots the next launch waits for.  Never changes the records */
    /* Frame-to-frame tile scheduling for the shortest SINGLE frame (the reference's caller issues one World::draw per
     * displayed frame, src/Main.cpp:190-222).  A frame takes as long as its bulk or its longest ray, whichever is longer;
     * handing the tiles out longest-first starts the long rays at once.  SVO_KERNEL_STACK only; both optional:
     *   tile_cost_dev   [nframes][ntiles][2] u32, written: the largest step count of a primary ray of the 8x8-pixel tile and
     *                   of a shadow ray of it (ntiles = ceil(w/8) * ceil(h/8) of the traced raster, row-major);
     *   tile_order_dev  [ntiles] u32, read: the order in which every frame's tiles are handed out (a permutation of
     *                   0..ntiles-1, e.g. svo_tile_order of the previous frame's cost: temporal coherence makes it a good
     *                   predictor).  The records written are the same with any order. */
    uint32_t       *tile_cost_dev;
    const uint32_t *tile_order_dev;
    int32_t  semantics;             /* which of the reference's two marches (SURVEY.md App. B lists their differences):
                                       SVO_SEMANTICS_CPU (0): src/Traverse.cpp - what every default above quotes;
                                       SVO_SEMANTICS_GLSL (1): shaders/Chunkmarch.glsl, the march the reference RENDERS with - eps 0 means
                                       1/4096 (:17), step caps 0 mean 256 / 512 / 64 (:1-3), cubeEscapeDistance returns BIGEPS = 1/16 for a
                                       distance below EPS (:107-114: no ray creeps along a lattice plane for thousands of steps), a ray from
                                       outside enters the world only if the box lies ahead of it (tnear > 0, slabs by multiplication with
                                       1 / dir, :116-126), no chunk containment re-check (:297-330), a LEAF hit is reported at t without the
                                       CPU code's back-off (:263-268; svo_hit.t is then the shader's sigma), brick cells are found by
                                       multiplying with 1 / leafsize (:201,212).  Both kernels, the oracle and its Python twin implement it */
    uint32_t see_through;           /* 0 = off.  m in 1..0xFFFF: every ray (shadow rays too) is marched as if each LEAF node of material m
                                       (offset & 0xFFFF == m) were EMPTY and each brick cell holding m were 0 - shaders/Chunkmarch.glsl's
                                       `ignore` (:190-191,240-241,280), used by ParallaxAlpha.Fragment.glsl (:147,181).  The records equal,
                                       bit for bit, those of the same world with those words rewritten to 0 (node, cell and chunk included).
                                       Above 0xFFFF: SVO_ERR_INVALID_ARG.  The stack kernel marches a see-through copy of the world's wide
                                       and mask pools, built on the device at the first such launch and kept for one material at a time
                                       (svo_world_info does not count it; at most 1.4 GB at C3 size); every change to the pools drops it */
} svo_trace_params;
enum { SVO_NORMAL_CUBE = 0, SVO_NORMAL_FACE = 1 };
enum { SVO_SHADOW_NO_CLEARANCE = 2, SVO_SHADOW_NO_BRICK_CLEARANCE = 4, SVO_SHADOW_NO_DARK_BIRTH = 8 };
enum { SVO_SEMANTICS_CPU = 0, SVO_SEMANTICS_GLSL = 1 };

/* G-buffer record, 32 bytes per pixel / per ray. */
enum {
    SVO_HIT_FLAG      = 1u << 0,    /* primary ray hit a voxel */
    SVO_SHADOW_TRACED = 1u << 1,    /* a shadow ray was cast from this hit */
    SVO_SHADOWED      = 1u << 2,    /* ... and it hit something */
    SVO_FACE_NORMAL   = 1u << 3,    /* normal[] is the entered-face normal (svo_trace_params.normal_mode = SVO_NORMAL_FACE) */
    SVO_SEE_THROUGH   = 1u << 4,    /* svo_trace_translucent: the surface hit is of the see-through material; the behind record is its continuation */
    SVO_LOCAL_SHADOWS  = 1u << 5,   /* svo_trace_local_shadows has been through this record: bits 6 and 7 are valid for it */
    SVO_SHADOWED_POINT = 1u << 6,   /* ... the point light is occluded (or, not asked for, a copy of SVO_SHADOWED) */
    SVO_SHADOWED_SPOT  = 1u << 7,   /* ... the spotlight is */
    SVO_ERR_FLAG      = 1u << 15    /* runaway ray: given up after 2^22 march steps of the kernel's own counting (only rays that
                                       creep through all three nested loops of the reference get there; the stack kernel
                                       takes creeping stretches in closed form and finishes rays the literal kernel gives
                                       up).  A primary ray is then recorded as a miss, a shadow ray as "traced, not occluded".  WHICH rays
                                       get there depends on the kernel (each counts its own steps; the stack kernel also counts the passes a
                                       lane waits for a vote): records carrying this flag are outside the cross-kernel equality */
};
#define SVO_CELL_NONE 0xFFu         /* hit a LEAF node, not a brick cell */

typedef struct svo_hit {
    float    t;                     /* sigma distance exactly as chunkmarch accumulates it (src/Traverse.cpp:160-161) */
    float    normal[3];             /* cubeNormal of alpha + beta*(t - EPS) on the hit voxel (shaders/Chunkmarch.glsl:128-136) */
    uint16_t material;              /* LEAF offset or brick cell value */
    uint16_t flags;
    uint32_t chunk;                 /* World::index() linear chunk index */
    uint32_t node;                  /* index in that chunk's tree[] of the LEAF/TWIG node hit */
    uint32_t cell;                  /* brick cell word z*16+y*4+x, or SVO_CELL_NONE */
} svo_hit;

typedef struct svo_world svo_world;

typedef struct svo_world_info {
    int32_t  width, height, depth, chunksize;
    int32_t  chunkcoordmin[3];
    int32_t  uploaded_device;       /* -1 if not uploaded */
    uint64_t total_trees, total_twigs;
    uint64_t tree_pool_bytes, twig_pool_bytes, mask_pool_bytes;
    int32_t  max_chunk_depth;
    int32_t  exact_geometry;        /* 1: all voxel corners are exact floats -> SVO_KERNEL_STACK allowed */
    uint64_t wide_pool_bytes;       /* the stack kernel's derived view of the trees (two levels per node) + its reference node indices */
    uint64_t wide_nodes;            /* wide nodes in use (64 entries each) */
} svo_world_info;

/* ---- world construction (host) ------------------------------------------------------------ */

/* World::init(w,h,d,s): generate w*h*d chunks of Simplex terrain.  Chunk (x,y,z) sits at
 * (chunkcoordmin + (x,y,z)) * chunksize; linear index = World::index(). */
int svo_world_generate(int w, int h, int d, int chunksize, const int chunkcoordmin[3],
                       const svo_terrain_params *terrain, svo_world **out);

/* Wrap chunks the caller generated/edited itself.  `chunks` has w*h*d entries in World::index()
 * order; pools are COPIED.  Node words are validated (SVO_ERR_MALFORMED_TREE). */
int svo_world_create(const svo_chunk_desc *chunks, int n, int w, int h, int d, int chunksize,
                     const int chunkcoordmin[3], svo_world **out);

int  svo_world_info_get(const svo_world *, svo_world_info *out);
/* Borrow the host copy of chunk i (valid until the world is destroyed or chunk i is replaced: svo_world_update,
 * svo_world_edit_box, a svo_world_shift that slides it out).  A chunk built or edited on the device is fetched on the first request. */
int  svo_world_chunk(const svo_world *, int i, svo_chunk_desc *out);
void svo_world_destroy(svo_world *);

/* Ocroot::write / Ocroot::read (src/Octree.cpp:178-201): one chunk per file, the reference's raw layout —
 * a 64-byte header (position f32x3 @0, size f32 @12, depth u32 @16, trees u64 @24, twigs u64 @32,
 * treestoragesize u64 @40, twigstoragesize u64 @48, modified u8 @56; the first 64 bytes of Ocroot on x86-64),
 * then trees*4 bytes of node words, then twigs*128 bytes of bricks.  svo_chunk_read allocates *tree / *twig
 * with malloc (caller frees with svo_chunk_free) and validates sizes against the file length. */
int  svo_chunk_write(const char *path, const svo_chunk_desc *chunk, uint64_t treestoragesize, uint64_t twigstoragesize);
int  svo_chunk_read(const char *path, svo_chunk_desc *out, uint64_t *treestoragesize, uint64_t *twigstoragesize);
void svo_chunk_free(svo_chunk_desc *chunk);

/* World::index_float / World::index (src/World.cpp:323-332, 288-293). */
int  svo_world_index_float(const svo_world *, const float p[3], int q[3]);
int  svo_world_index(const svo_world *, int x, int y, int z);

/* ---- device residency -------------------------------------------------------------------- */

/* Pack every chunk's tree[] / twig[] into one flat HBM pool each (+ the 64-bit brick occupancy
 * masks derived from twig[]), build the chunk table, on HIP device `device`. */
int svo_world_upload(svo_world *, int device);

/* Replace chunk `chunk` by `desc` (edited pools) and refresh HBM: ranges [tree_left,tree_right)
 * nodes and [twig_left,twig_right) bricks are re-sent in place; realloc!=0 (or growth beyond the
 * chunk's slot) re-packs the chunk at the pool tail == Ocdelta semantics, src/Octree.h:47-54.
 * As with the reference's glBufferSubData, with realloc == 0 only the ranges (and whatever desc holds beyond the chunk's previous
 * length) are taken from desc - the library's own host copy and HBM keep the rest - so they must cover every word that changed;
 * the result is validated as a whole and a malformed one is refused with nothing changed (SVO_ERR_MALFORMED_TREE). */
int svo_world_update(svo_world *, int chunk, const svo_chunk_desc *desc,
                     uint64_t tree_left, uint64_t tree_right,
                     uint64_t twig_left, uint64_t twig_right, int realloc);

/* World::shift (src/World.cpp:334-378): slide the grid by one chunk along one axis (offset = +-1 on exactly one
 * axis).  The entering plane of chunks is generated with the world's terrain parameters and replaces, at its
 * toroidal World::index(), the plane that leaves; chunkcoordmin moves.  Only for worlds made by svo_world_generate.
 * On an uploaded world the plane is generated on the device the pools live on and installed device-to-device (host
 * copies of those chunks are made on request, svo_world_chunk); otherwise on the host. */
int svo_world_shift(svo_world *, const int offset[3]);

/* Ocroot::build / destroy / replace (src/Octree.cpp:203-443) followed by World::modify (src/World.cpp:268-274) on chunk
 * `chunk` of an UPLOADED world, run on the device the pools live on: the closed box [lo, hi] is filled with `material`
 * where the chunk is empty (SVO_EDIT_BUILD), emptied (SVO_EDIT_DESTROY), or emptied and then filled (SVO_EDIT_REPLACE).
 * Node blocks and bricks are appended in the reference's depth-first order, so the pools equal what the reference's
 * edit leaves, index for index; its storage sizes double by the reference's rule.  The box is in world coordinates and may
 * extend beyond the chunk (the reference's caller applies the same cube to every chunk it overlaps, src/Main.cpp:322-338).
 * Nothing visits the host; a host copy of the chunk is made again on request (svo_world_chunk).
 * SVO_ERR_NOT_UPLOADED on a world that is not resident. */
enum { SVO_EDIT_BUILD = 0, SVO_EDIT_DESTROY = 1, SVO_EDIT_REPLACE = 2 };
int svo_world_edit_box(svo_world *, int chunk, int op, const float lo[3], const float hi[3], uint16_t material);

/* modify() (src/Main.cpp:321-338) with destroy / build / replace (:340-367): the cube [bmin, bmin + size] goes to every chunk that holds
 * one of its eight corners - what pressing `x` / `z` / `c` does with the edit cursor (svo_cursor_place's box: bmin and size as read back
 * from it).  For i = 0..7, every operation in float and separately rounded:
 *   p = bmin + vec3(bool(i & 4), bool(i & 2), bool(i & 1)) * size;
 *   j = World::index(World::index_float(p))   (src/World.cpp:288-293,323-332);
 *   the corner is dropped unless isInsideCube(p, chunk[j].position, chunk[j].position + chunksize) (closed): a corner outside the
 *   world wraps to a chunk that does not hold it;
 *   otherwise chunk j takes svo_world_edit_box(j, op, bmin, bmin + size, material).
 * Each distinct chunk is edited ONCE, in the order of its first appearance; the reference edits once per corner, up to eight times on
 * one chunk.  The two are equal because a repeated Ocroot::build / destroy / replace of the same box leaves the pools as they are,
 * index for index and in size (tests/test_boxes_cpu.py checks this against the CPU oracle for all three operations).
 * chunks_out[0..*nchunks_out) receives those chunks in that order; both may be NULL.  They are written before the first edit.
 * The corner rule's limitation is the reference's: a cube wider than a chunk skips the chunks that lie between its corners.
 * Returns the largest positive status of the edits (SVO_OK_LITERAL_ONLY) or the first negative one; the edits stop at a failing chunk,
 * and AN EDIT APPLIED BEFORE THE FAILING ONE STAYS APPLIED.  A NULL world or bmin, !(size > 0), a NaN or infinite bmin / size or an
 * unknown op: SVO_ERR_INVALID_ARG; then a world that is not resident: SVO_ERR_NOT_UPLOADED - both before anything changes or is written. */
int svo_world_edit_cube(svo_world *, int op, const float bmin[3], float size, uint16_t material, int chunks_out[8], int *nchunks_out);

/* svo_world_edit_box with the closed ball { p : |p - centre| <= radius } in the place of the closed box: a round hole, a crater, a round
 * brush.  The reference edits cubes only; the result is defined by its destroyCube / buildCube recursion (src/Octree.cpp:203-430) with
 * cubesIntersect(box, region) replaced by touch(box) and cube_is_inside(region, box) by inside(box) - visiting order, appends, the brick
 * level, Octwig(material of the LEAF that is cut) and the doubling of the storage sizes stay as they are, so the pools are specified
 * index for index.  Both predicates are in float, every operation separately rounded; R2 = radius * radius, lo the box's min corner as
 * the box edit forms it, hi = lo + edge, c = centre:
 *   touch:  per axis d = lo - c; if !(d > 0): d = c - hi; if still !(d > 0): d = 0;   touch = dx*dx + dy*dy + dz*dz <= R2
 *   inside: per axis u = c - lo, v = hi - c, f = (u < v) ? v : u;                      inside = fx*fx + fy*fy + fz*fz <= R2
 * (sums left to right).  A brick cell is edited iff touch(its box) - the conservative, closed rule the box edit applies to cells: build
 * writes `material` to touched cells that hold 0, destroy writes 0 to touched cells, replace is destroy then build.  On exact geometry
 * (power-of-two chunk size, integer position) the edit changes exactly the cells a pass over all cells with that rule would change
 * (DESIGN.md 6n).  An R2 that overflows to +inf is legal: everything is touched.
 * Ordered, complete and reported like svo_world_edit_box: an uploaded world only, the device drained first, SVO_OK or
 * SVO_OK_LITERAL_ONLY, the host copy of the chunk dropped and fetched again on request.
 * A NULL world or centre, a chunk out of range, an unknown op, a NaN or infinite centre, !(radius > 0) or an infinite radius:
 * SVO_ERR_INVALID_ARG; then a world that is not resident: SVO_ERR_NOT_UPLOADED - both before anything changes. */
int svo_world_edit_ball(svo_world *, int chunk, int op, const float centre[3], float radius, uint16_t material);

/* The ball to every chunk whose box [position, position + (float)chunksize] it touches (the same touch, evaluated on the host), in
 * ascending World::index() order, each chunk once.  Unlike svo_world_edit_cube's corner rule NO CHUNK BETWEEN THE EXTREMES IS SKIPPED: a
 * ball wider than a chunk reaches every chunk it overlaps.
 * *nchunks_out (may be NULL) always receives the number of touched chunks; chunks_out (may be NULL) receives them, chunks_cap is its
 * length.  If chunks_out is given and the count exceeds chunks_cap the call is SVO_ERR_INVALID_ARG and nothing is edited - the count is
 * still reported, so the caller can retry.  The list is written before the first edit.  A ball that touches no chunk: SVO_OK, count 0.
 * Returns the largest positive status of the edits (SVO_OK_LITERAL_ONLY) or the first negative one; the edits stop at a failing chunk,
 * and AN EDIT APPLIED BEFORE THE FAILING ONE STAYS APPLIED.  Argument checks as svo_world_edit_ball (without the chunk): a refused
 * argument writes nothing.  The count needs no device: it is reported, and a chunks_cap it exceeds refused, before a world that is not
 * resident is (SVO_ERR_NOT_UPLOADED, the list not written). */
int svo_world_edit_ball_all(svo_world *, int op, const float centre[3], float radius, uint16_t material,
                            int *chunks_out, int chunks_cap, int *nchunks_out);

/* Ocroot::defragcopy (src/Octree.cpp:445-614) followed by World::modify with realloc (src/World.cpp:268-274) on chunk `chunk`:
 * the chunk is rebuilt from its root into fresh pools - depth-first, root at 0, blocks at 1 + 8k - so that what no BRANCH reaches
 * (blocks and bricks that edits left behind) is gone, a brick of one value becomes an EMPTY / LEAF node, a BRANCH of eight equal
 * EMPTY / LEAF children becomes that node, and a BRANCH over two levels of EMPTY / LEAF nodes becomes one brick.  The pools
 * equal, index for index, what the reference's recursion leaves; the chunk's storage capacities do not shrink.
 * On an uploaded world it runs on the device the pools live on (nothing visits the host; a host copy is made again on request,
 * svo_world_chunk), otherwise on the host pools.  SVO_OK, or SVO_OK_LITERAL_ONLY as for svo_world_edit_box. */
int svo_world_compact(svo_world *, int chunk);
/* Ocroot::lodmm (src/Octree.cpp:626-765) followed by World::modify with realloc: chunk `chunk` one level coarser, depth ->
 * depth - 1 (position and size unchanged).  Every BRANCH at level depth-3 becomes a brick whose cells are the majority
 * (MisraGriesCounter<8>, src/MisraGries.h) of the 8 cells under each; BRANCHes above it are kept, every other node is compacted as
 * by svo_world_compact.  SVO_ERR_UNSUPPORTED on a chunk of depth 2 (nothing changes); host / device as svo_world_compact. */
int svo_world_coarsen(svo_world *, int chunk);

/* ---- your own voxels: chunks from dense grids, and back ------------------------------------------------------------
 * A grid is N*N*N uint16_t materials, N = 2^depth, x fastest: cell (x, y, z) at (z*N + y)*N + x - the brick's own order,
 * z*16 + y*4 + x, at full size.  0 means empty.  depth lies in [SVO_GRID_MIN_DEPTH, SVO_GRID_MAX_DEPTH] (depth 10 is a 2 GiB grid);
 * anything else is SVO_ERR_INVALID_ARG.  A grid in device memory (grid_dev) is 16-byte aligned, as every device allocation and every
 * torch tensor is; one that is not is SVO_ERR_INVALID_ARG too.
 *
 * The tree of a grid is grow()'s (src/Octree.cpp:74-176) with "all cells equal" in the place of the height bounds, in integers:
 *   a node at level L with integer corner (x, y, z) covers the cells [x, x+e) x [y, y+e) x [z, z+e), e = N >> L; the root is level 0
 *   at (0, 0, 0), slot 0;
 *   all cells 0:                  EMPTY (the word 0);
 *   all cells equal m != 0:       LEAF | m - at level depth-2 too: a uniform 4^3 block is a LEAF, never a TWIG;
 *   otherwise, at L == depth-2:   TWIG | k, k = the number of TWIGs before it in visiting order,
 *                                 twig[k*64 + cz*16 + cy*4 + cx] = grid(x+cx, y+cy, z+cz);
 *   otherwise:                    BRANCH | first, first = 1 + 8 * (the number of BRANCHes before it in visiting order); child c sits at
 *                                 first + c with corner (x + (c&1)*e/2, y + ((c>>1)&1)*e/2, z + (c>>2)*e/2);
 *   visiting order is the FIFO queue's: levels in order, within a level the nodes in the order their parents were visited, children
 *   in slot order.
 * So trees = 1 + 8 * BRANCHes, the pools pass svo_world_create's validation, and they are minimal: no BRANCH has eight equal EMPTY /
 * LEAF children and no brick holds a single value (svo_world_compact leaves them as they are). */
#define SVO_GRID_MIN_DEPTH 2
#define SVO_GRID_MAX_DEPTH 10

/* The tree of `grid` (host memory) as malloc'ed pools in *out, with the given frame; the caller frees them with svo_chunk_free.
 * This is how a world is made from grids without a device (svo_world_create), and the host twin of svo_world_chunk_from_grid.
 * A NULL argument, a depth out of range, a size that is not greater than 0 or not finite: SVO_ERR_INVALID_ARG; SVO_ERR_OUT_OF_MEMORY. */
int svo_chunk_from_grid(const uint16_t *grid, uint32_t depth, const float position[3], float size, svo_chunk_desc *out);

/* Chunk `chunk` of an UPLOADED world is replaced by the tree of grid_dev (device memory), built on the device the pools live on:
 * position and size stay, `depth` becomes the chunk's depth (chunks of one world may differ in depth).  The pools never visit the
 * host and equal svo_chunk_from_grid's index for index; a host copy is made again on request (svo_world_chunk), and svo_world_info
 * follows.  Ordered and complete like svo_world_edit_box (it drains the device first); installed like svo_world_coarsen's result (the
 * chunk's storage capacities do not shrink).  SVO_OK, or SVO_OK_LITERAL_ONLY as for svo_world_edit_box.
 * A NULL world or grid, a chunk or depth out of range, a misaligned grid: SVO_ERR_INVALID_ARG; then a world that is not resident:
 * SVO_ERR_NOT_UPLOADED; no device memory for the working arrays: SVO_ERR_OUT_OF_MEMORY; 2^30 nodes or bricks: SVO_ERR_UNSUPPORTED -
 * all before anything changes. */
int svo_world_chunk_from_grid(svo_world *, int chunk, const uint16_t *grid_dev, uint32_t depth);

/* The inverse: grid_dev receives the (2^depth)^3 cells of chunk `chunk`, whatever the chunk's own depth D.  Output cell (x, y, z)
 * reports the finest voxel (X, Y, Z), per axis X = x << (D - depth) if depth <= D (the min-corner voxel of the cell - no filtering:
 * svo_world_coarsen is the majority filter), else X = x >> (depth - D) (replication).  That voxel's material is found by descending from
 * the root by integer coordinates: EMPTY gives 0, LEAF offset & 0xFFFF, TWIG the brick cell; blocks no BRANCH reaches are never
 * visited, and nothing is read out of range whatever the pools hold (a word that points beyond them reads as 0).
 * Argument and status rules are svo_world_locate's: a NULL world or grid, a chunk or depth out of range, a misaligned grid:
 * SVO_ERR_INVALID_ARG; then a world that is not resident: SVO_ERR_NOT_UPLOADED - settled before any device work.  Asynchronous on
 * `stream` and ordered against updates, edits and shifts like svo_world_locate; it takes no launch slot and no scratch. */
int svo_world_chunk_to_grid(svo_world *, int chunk, uint32_t depth, uint16_t *grid_dev, void *stream);

/* ---- grids from triangle meshes: a voxeliser and an interior fill ------------------------------------------------------
 * svo_grid_add_mesh rasterises a triangle mesh into a grid as above (N = 2^depth cells per axis, x fastest, depth in
 * [SVO_GRID_MIN_DEPTH, SVO_GRID_MAX_DEPTH]); svo_grid_fill_enclosed makes the shell it leaves solid.  Each has a host form (every
 * pointer host memory) and a device form (svo_device_*: the svo_mesh struct on the host, its three arrays and the grid in device
 * memory, the grid 16-byte aligned); neither the mesh nor the grid of a device call visits the host.  The two forms give the same
 * grid, cell for cell.  The way on from the grid: svo_world_chunk_from_grid -> svo_trace_instances, or svo_chunk_from_grid ->
 * svo_world_create.
 *
 * For every cell,  grid[cell] = max(what it held, the largest material of the triangles that overlap it);  no other cell changes.
 * THE CALLER CLEARS THE GRID FIRST (or leaves in it what the mesh is to be merged with).  The result does not depend on the order of
 * the triangles, two calls give what one call on the concatenated mesh gives, and a triangle of material 0 changes nothing.
 *
 * The overlap rule is conservative (a cell that the triangle touches is marked) and closed (touching counts).  Every operation below
 * is a float operation, separately rounded (nothing is contracted into a fused multiply-add), and a comparison with a NaN is false:
 *   inv = 1.0f / cell, rounded once on the host; a vertex v goes to grid units per axis as g = (v - origin) * inv;
 *   dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z;   cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x);
 *   e0 = v1 - v0, e1 = v2 - v1, e2 = v0 - v2, n = cross(e0, e1)     (v0, v1, v2 in grid units).
 * A triangle is DROPPED - it overlaps nothing - if one of its three indices is >= nvertices (nothing is read out of range, whatever
 * the index array holds), if one of its nine grid coordinates is not finite, or if n is (0, 0, 0).  Otherwise it overlaps the cell
 * p = (x, y, z) (the integer min corner as floats; the cell's box is [p, p + 1]) iff all of these hold:
 *   box     per axis k:  p[k] <= hi[k]  and  p[k] + 1 >= lo[k],   lo = min(min(v0, v1), v2) and hi likewise the max;
 *   plane   c[k] = n[k] > 0 ? 1 : 0,  d1 = dot(c - v0, n),  d2 = dot((1 - c) - v0, n),  q = dot(p, n):   (q + d1) * (q + d2) <= 0;
 *   edges   for (i, j, w) in ((x, y, z), (y, z, x), (z, x, y)):  s = n[w] >= 0 ? 1 : -1,  and for each edge k = 0, 1, 2:
 *             a = -e_k[j] * s,  b = e_k[i] * s,  de = ((-(a*v_k[i] + b*v_k[j])) + max0(a)) + max0(b),  max0(t) = t > 0 ? t : 0:
 *             (a*p[i] + b*p[j]) + de >= 0.
 * "Closed" on the lattice: a face that lies exactly in a lattice plane marks the cells on BOTH of its sides.  An axis-aligned cube
 * with its corners at cells 4 and 8 marks the cells 3 .. 8 per axis (6^3 - 2^3 = 208 cells), not 4 .. 7; a caller who wants 4 .. 7
 * moves or shrinks the mesh by a fraction of a cell.
 *
 * The fill: an empty cell (value 0) is OUTSIDE iff a path of 6-neighbour steps through empty cells connects it to an empty cell with
 * a coordinate of 0 or N - 1.  Every empty cell that is not outside becomes `material`; nothing else changes; *filled_out (may be
 * NULL) receives how many cells were filled.
 *
 * Refusals, settled before any device work, nothing written: SVO_ERR_INVALID_ARG for a NULL mesh or grid, NULL vertices or indices
 * with a non-zero count, a depth out of range, a misaligned device grid, a cell that is not finite or not > 0, an inv that is not
 * finite, an origin that is not finite, a fill with material 0.  ntriangles == 0 is SVO_OK and touches nothing.
 * The device forms are world-less, like svo_shade: they run on the calling thread's current device, on `stream`, take their working
 * memory from the library's device buffer cache (svo_device_cache_trim returns it), HAVE COMPLETED WHEN THEY RETURN (they need
 * totals on the host) and synchronise `stream` only, not the device - with the cache's two exceptions: a cache that is full of larger
 * buffers gives the arena back with hipFree, and an allocation that fails is tried again after svo_device_cache_trim; both wait for
 * the device.  SVO_ERR_NO_DEVICE, SVO_ERR_HIP, SVO_ERR_OUT_OF_MEMORY as elsewhere; svo_device_grid_add_mesh (the device form only)
 * refuses a mesh of 2^31 - 1 triangles or more with SVO_ERR_UNSUPPORTED, before any device work. */
typedef struct svo_mesh {
    const float    *vertices;       /* [nvertices][3] */
    const uint32_t *indices;        /* [ntriangles][3] */
    const uint16_t *materials;      /* [ntriangles], or NULL: every triangle carries `material` */
    uint32_t        nvertices, ntriangles;
    float           origin[3];      /* the grid's min corner, in the mesh's coordinates */
    float           cell;           /* edge of one grid cell, in the mesh's coordinates */
    uint16_t        material;       /* used when materials == NULL */
    uint16_t        _pad[3];        /* 56 bytes */
} svo_mesh;

int svo_grid_add_mesh(const svo_mesh *mesh, uint32_t depth, uint16_t *grid);
int svo_device_grid_add_mesh(const svo_mesh *mesh, uint32_t depth, uint16_t *grid_dev, void *stream);
int svo_grid_fill_enclosed(uint16_t *grid, uint32_t depth, uint16_t material, uint64_t *filled_out);
int svo_device_grid_fill_enclosed(uint16_t *grid_dev, uint32_t depth, uint16_t material, uint64_t *filled_out, void *stream);

/* ---- chunks straight from triangle meshes: the sparse voxeliser ---------------------------------------------------------
 * The tree of the grid that svo_grid_add_mesh would leave, built WITHOUT that grid, for depth in [SVO_MESH_MIN_DEPTH,
 * SVO_MESH_MAX_DEPTH] - beyond SVO_GRID_MAX_DEPTH, where the grid would not fit.  Definition: let G be the (2^depth)^3 grid, all 0;
 * every mesh of the list, in any order, is added to it by the rule stated above for svo_grid_add_mesh (the drop rules, the closed
 * conservative overlap test, the largest material where triangles meet, material 0 changing nothing, inv = 1 / cell rounded once on
 * the host; every mesh carries its own origin and cell); the result is the tree of G by the rule stated above for
 * svo_chunk_from_grid (EMPTY / LEAF / BRANCH nodes and TWIGs at level depth-2, FIFO visiting order, a uniform 4^3 block a LEAF,
 * minimal pools).  For depth <= SVO_GRID_MAX_DEPTH that is, index for index, svo_chunk_from_grid of svo_grid_add_mesh of a cleared
 * grid; above it the same sentences define it.  G is never allocated: working memory is proportional to the number of (triangle,
 * cell) overlaps - a cell's Morton key (3 * depth bits) and its material (16 bits) are one 64-bit word, which is why depth ends at 16.
 * The host form and the device form give the same pools.
 *
 * THERE IS NO INTERIOR FILL IN THIS CALL: the result is the shell.  From outside it renders and shadows like the solid; an edit that
 * cuts it open (svo_world_edit_box / _ball) finds it hollow until svo_world_chunk_fill_enclosed / svo_chunk_fill_enclosed (below) has
 * made it solid, as svo_grid_fill_enclosed does behind svo_grid_add_mesh.  The chunk is REPLACED, nothing is merged with what it held (svo_(world_)chunk_combine, below, merges two chunks).  One call builds one
 * chunk: a mesh that spans several chunks is passed to every one of them with origin = that chunk's min corner in the mesh's
 * coordinates and cell = the chunk's size / 2^depth - the closed rule marks the cells on both sides of a chunk border alike.
 * Cost: every triangle is tested against every cell of its clamped cell box (on the device: one wave per 4^3-cell tile of the box,
 * up to (2^depth / 4)^3 tiles for one triangle that spans the grid; no tile is rejected early), so a few huge triangles at a high
 * depth cost what their boxes hold, not what their surfaces hold.
 *
 * svo_chunk_from_mesh (host; every pointer host memory): malloc'ed pools in *out with the given frame, freed with svo_chunk_free -
 * what svo_world_create takes.  It needs no device.
 * svo_world_chunk_from_mesh (device; the svo_mesh structs on the host, their arrays device memory on the world's device): chunk
 * `chunk` of an UPLOADED world is replaced; position and size stay, `depth` becomes the chunk's depth.  Ordered, complete and
 * installed like svo_world_chunk_from_grid (it drains the device first; masks, wide tree, light-clearance state, svo_world_info and
 * the host copy on request follow as there); SVO_OK, or SVO_OK_LITERAL_ONLY as for svo_world_edit_box.  Neither the meshes nor the
 * pools visit the host; the working arrays come from the library's device buffer cache.
 *
 * nmeshes == 0, or meshes of which every triangle is dropped or misses the grid: SVO_OK, the chunk is the one word EMPTY, 0 bricks.
 * Refusals, all before anything changes: SVO_ERR_INVALID_ARG for a NULL world / out / position, nmeshes < 0 or nmeshes > 0 with NULL
 * meshes, a depth out of range, a chunk out of range, per mesh what svo_grid_add_mesh refuses of a mesh (NULL vertices or indices
 * with a non-zero count, a cell that is not finite or not > 0, an inv or an origin that is not finite), on the host form a size that
 * is not finite or not > 0; then SVO_ERR_NOT_UPLOADED (device form, a world that is not resident); SVO_ERR_UNSUPPORTED for 2^31 - 1
 * triangles or more (device form: in one mesh or in the list), 2^31 - 1 overlaps or more, 2^30 nodes or bricks;
 * SVO_ERR_OUT_OF_MEMORY when the working arrays do not fit (device: tried again after svo_device_cache_trim). */
#define SVO_MESH_MIN_DEPTH 2
#define SVO_MESH_MAX_DEPTH 16
int svo_chunk_from_mesh(const svo_mesh *meshes, int nmeshes, uint32_t depth, const float position[3], float size, svo_chunk_desc *out);
int svo_world_chunk_from_mesh(svo_world *, int chunk, const svo_mesh *meshes, int nmeshes, uint32_t depth);

/* ---- the sparse interior fill: svo_grid_fill_enclosed's rule on the tree ------------------------------------------------------
 * What svo_grid_fill_enclosed does to a dense grid, done to a chunk's pools WITHOUT that grid, for a chunk depth in
 * [SVO_FILL_MIN_DEPTH, SVO_FILL_MAX_DEPTH]: a shell from svo_(world_)chunk_from_mesh becomes solid, and so does any other chunk - from
 * a grid, generated, edited.  Definition: let D be the chunk's depth, N = 2^D and G the N^3 grid of the chunk's finest voxels, as
 * svo_world_chunk_to_grid at depth D reports them (EMPTY: 0, LEAF: offset & 0xFFFF, TWIG: the brick cell; a value of 0 is empty however
 * it is stored; only what the root reaches counts).  svo_grid_fill_enclosed's rule is applied to G: an empty cell is OUTSIDE iff
 * 6-neighbour steps through empty cells connect it to an empty cell with a coordinate of 0 or N - 1; every other empty cell becomes
 * `material`; nothing else changes; *filled_out (may be NULL) receives how many cells changed (at most 2^48).  The result is the tree
 * of that grid by the rule stated above for svo_chunk_from_grid: FIFO visiting order, a uniform 4^3 block a LEAF, minimal pools.  It is
 * ALWAYS rebuilt, also when nothing was filled: pools that were not minimal or not in FIFO order come back minimal and in FIFO order.
 * For D <= SVO_GRID_MAX_DEPTH that is, index for index, svo_chunk_from_grid of svo_grid_fill_enclosed of the chunk's grid; above it
 * the same sentences define it.  G is never allocated: working memory is proportional to the chunk's node words and bricks.  The
 * host form and the device form give the same pools and the same count, and neither has more node words or bricks than the part of
 * the input the root reaches.
 * NEIGHBOURING CHUNKS ARE NOT CONSULTED: the chunk's own six faces are the outside.  A cavity that a neighbouring chunk would close
 * stays open, and a shell that continues into the neighbour is open where it crosses the face.
 *
 * svo_chunk_fill_enclosed (host; `in` and `*out` host pools): *out receives malloc'ed pools with in's frame, freed with
 * svo_chunk_free; `in` is not modified; out may not alias in.  It needs no device.
 * svo_world_chunk_fill_enclosed (device): chunk `chunk` of an UPLOADED world is replaced by its filled form, built on the world's
 * device; position, size and depth stay.  Ordered, complete and installed like svo_world_chunk_from_mesh (it drains the device first;
 * masks, wide tree, light-clearance state, svo_world_info and the host copy on request follow as there); SVO_OK, or
 * SVO_OK_LITERAL_ONLY as for svo_world_edit_box.  The pools do not visit the host; the working arrays come from the library's device
 * buffer cache.
 *
 * Refusals, all before anything changes: SVO_ERR_INVALID_ARG for a NULL world / in / out, out == in, a chunk out of range, material 0,
 * NULL pools in `in`, and (host form) pools that svo_world_create's validation would refuse; then SVO_ERR_NOT_UPLOADED (device form);
 * SVO_ERR_UNSUPPORTED for a chunk depth outside [2, 16] and for a chunk that holds a TWIG above level depth-2 (the sparsely refined
 * chunks of svo_terrain_params.coarse_depth: their bricks' cells are larger than a voxel, and the tree of the filled grid could be
 * larger than the input); SVO_ERR_OUT_OF_MEMORY when the working arrays do not fit (device: tried again after
 * svo_device_cache_trim). */
#define SVO_FILL_MIN_DEPTH 2
#define SVO_FILL_MAX_DEPTH 16
int svo_chunk_fill_enclosed(const svo_chunk_desc *in, uint16_t material, svo_chunk_desc *out, uint64_t *filled_out);
int svo_world_chunk_fill_enclosed(svo_world *, int chunk, uint16_t material, uint64_t *filled_out);

/* ---- chunk CSG: two chunks combined cell by cell, on their trees ----------------------------------------------------------------
 * A mesh added into a terrain chunk, a solid carved out of the terrain, two models united, two solids intersected - at every depth
 * the sparse voxeliser and the sparse fill reach, WITHOUT a dense grid.  Definition: A and B are two chunks of the same depth D in
 * [SVO_COMBINE_MIN_DEPTH, SVO_COMBINE_MAX_DEPTH], N = 2^D, and G_A, G_B the N^3 grids of their finest voxels, as
 * svo_world_chunk_to_grid at depth D reports them (EMPTY: 0, LEAF: offset & 0xFFFF, TWIG: the brick cell; a value of 0 is empty however
 * it is stored; only what the root reaches counts).  CELLS CORRESPOND BY INDEX: the two chunks' positions and sizes are not consulted,
 * and the result keeps A's frame.  For every cell c,  G[c] = f_op(G_A[c], G_B[c]),  with a = G_A[c] and b = G_B[c]:
 *   SVO_COMBINE_MAX        max(a, b)          svo_grid_add_mesh's merge rule: B's voxels added to what A held
 *   SVO_COMBINE_UNDER      a != 0 ? a : b     SVO_EDIT_BUILD's rule: B only where A is empty
 *   SVO_COMBINE_OVER       b != 0 ? b : a     SVO_EDIT_REPLACE's rule: B on top
 *   SVO_COMBINE_SUBTRACT   b != 0 ? 0 : a     SVO_EDIT_DESTROY's rule: B's shape carved out of A
 *   SVO_COMBINE_INTERSECT  b != 0 ? a : 0     A where B is
 * The result is the tree of G by the rule stated above for svo_chunk_from_grid: FIFO visiting order, a uniform 4^3 block a LEAF,
 * minimal pools.  It is ALWAYS rebuilt, also when B is empty: pools that were not minimal or not in FIFO order come back minimal and
 * in FIFO order.  *changed_out (may be NULL) receives the number of cells with G[c] != G_A[c] (at most 2^48).  For D <=
 * SVO_GRID_MAX_DEPTH that is, index for index, svo_chunk_from_grid of the elementwise combination of the two chunks' grids; above it
 * the same sentences define it.  No grid is allocated: working memory is proportional to the node words and bricks the two roots
 * reach.  The host form and the device form give the same pools and the same count.  For minimal inputs the result has at most
 * trees_A + trees_B node words and at most twigs_A + twigs_B bricks; UNLIKE THE FILL'S IT CAN BE LARGER THAN EITHER INPUT.
 *
 * svo_chunk_combine (host; `a`, `b` and `*out` host pools): *out receives malloc'ed pools with a's frame, freed with svo_chunk_free;
 * `a` and `b` are not modified; out may alias neither; a == b is allowed.  It needs no device.
 * svo_world_chunk_combine (device): A is chunk `chunk` of the UPLOADED world dst, B chunk `src_chunk` of the UPLOADED world src on the
 * same device; A is replaced by the result, built on that device; position, size and depth stay.  src may be dst, and src_chunk ==
 * chunk of the same world is defined (A = B): B is read completely before A is replaced, and src's chunk is never written.  Ordered,
 * complete and installed like svo_world_chunk_fill_enclosed (it drains the device first; masks, wide tree, light-clearance state,
 * svo_world_info and the host copy on request follow as there); SVO_OK, or SVO_OK_LITERAL_ONLY as for svo_world_edit_box.  The pools
 * do not visit the host; the working arrays come from the library's device buffer cache.
 *
 * Refusals, all before anything changes: SVO_ERR_INVALID_ARG for a NULL world / a / b / out, out == a or out == b, a chunk out of range
 * in either world, an unknown op, NULL pools, (host form) a size of `a` that is not finite or not > 0 and pools that svo_world_create's
 * validation would refuse, (device form) two worlds resident on different devices; then SVO_ERR_NOT_UPLOADED for either world (device
 * form); then SVO_ERR_UNSUPPORTED for depths that differ, a depth outside [2, 16], a TWIG above level depth-2 in either chunk (the
 * sparsely refined chunks, refused for the fill's reason) and 2^30 nodes or bricks; SVO_ERR_OUT_OF_MEMORY when the working arrays do not
 * fit (device: tried again after svo_device_cache_trim).  On the device a malformed pool found by the walk is SVO_ERR_MALFORMED_TREE,
 * with nothing installed. */
enum { SVO_COMBINE_MAX = 0, SVO_COMBINE_UNDER = 1, SVO_COMBINE_OVER = 2, SVO_COMBINE_SUBTRACT = 3, SVO_COMBINE_INTERSECT = 4 };
#define SVO_COMBINE_MIN_DEPTH 2
#define SVO_COMBINE_MAX_DEPTH 16
int svo_chunk_combine(const svo_chunk_desc *a, const svo_chunk_desc *b, int op, svo_chunk_desc *out, uint64_t *changed_out);
int svo_world_chunk_combine(svo_world *dst, int chunk, svo_world *src, int src_chunk, int op, uint64_t *changed_out);

/* ---- the stamp: a chunk placed into another at any cell offset, in any orientation of the cube ---------------------------------
 * A depth-6 model put into a depth-12 terrain chunk, the same tree model placed forty times, an instance that came to rest baked into
 * the world - WITHOUT a dense grid and without voxelising anything again.  Definition: A has depth D_A and B depth D_B, both in
 * [SVO_STAMP_MIN_DEPTH, SVO_STAMP_MAX_DEPTH] with D_B <= D_A; N_A = 2^D_A, N_B = 2^D_B, and G_A, G_B the grids of their finest
 * voxels, as svo_world_chunk_to_grid reports them (as for the chunk CSG above).  The two chunks' positions and sizes are not
 * consulted: ONE CELL OF B IS ONE CELL OF A, and the result keeps A's frame.  The placement gives A's cell that B's cube starts at and
 * an orientation orient = perm * 8 + flips: perm indexes the table pi = (x,y,z), (x,z,y), (y,x,z), (y,z,x), (z,x,y), (z,y,x), which
 * gives pi(0), pi(1), pi(2) (axis 0 is x), and flips has one bit per OUTPUT axis.  For a cell p of A take d = p - offset:
 *   if any d_i lies outside [0, N_B):  b = 0
 *   otherwise  q[pi(i)] = (flips bit i) ? N_B - 1 - d_i : d_i  and  b = G_B[q]
 *   G[p] = f_op(G_A[p], b), with f the SVO_COMBINE_* table above, unchanged
 * B's cube therefore covers A's cells [offset, offset + N_B)^3 in every orientation; what lies outside A is dropped.  OUTSIDE B'S CUBE
 * b IS 0, SO SVO_COMBINE_INTERSECT CLEARS A THERE (and SVO_COMBINE_SUBTRACT, MAX, UNDER and OVER leave A as it is).  The orientation
 * is proper (a rotation) iff parity(perm) * (-1)^popcount(flips) = +1; the other 24 are mirrors and are allowed.  The result is the
 * tree of G by svo_chunk_from_grid's rule, ALWAYS rebuilt, in A's frame; *changed_out (may be NULL) receives the number of cells with
 * G[p] != G_A[p].  With D_B = D_A, offset 0 and orient 0 the pools and the count are svo_chunk_combine's, index for index.  No grid is
 * allocated: working memory is proportional to the entries of the walk, which follow the RESULT - a B that is one LEAF word, placed
 * at an odd offset, leaves bricks along all six faces of its cube, so the result can exceed trees_A + trees_B node words and twigs_A
 * + twigs_B bricks.  The host form and the device form give the same pools and the same count.
 *
 * A model that straddles a chunk border is two calls whose offsets differ by N_A on that axis.
 *
 * svo_chunk_stamp (host) and svo_world_chunk_stamp (device) take their chunks, leave B alone and are ordered, complete and installed
 * as svo_chunk_combine and svo_world_chunk_combine; src == dst with src_chunk == chunk is defined: B is read completely before A is
 * replaced.
 *
 * Refusals, in combine's order and all before anything changes or is written: SVO_ERR_INVALID_ARG as there, and for a NULL placement,
 * orient > 47 or an offset outside [-65536, 65536]; then SVO_ERR_NOT_UPLOADED (device form); then SVO_ERR_UNSUPPORTED for D_B > D_A, a
 * depth outside [2, 16], a TWIG above level depth-2 in either chunk and 2^30 entries, nodes or bricks; SVO_ERR_OUT_OF_MEMORY when the
 * working arrays do not fit; on the device a malformed pool found by the walk is SVO_ERR_MALFORMED_TREE, with nothing installed. */
typedef struct svo_placement {      /* 16 bytes */
    int32_t  offset[3];             /* A's cell that B's cube starts at; each in [-65536, 65536] */
    uint32_t orient;                /* 0 .. 47: perm * 8 + flips */
} svo_placement;
#define SVO_STAMP_MIN_DEPTH 2
#define SVO_STAMP_MAX_DEPTH 16
int svo_chunk_stamp(const svo_chunk_desc *a, const svo_chunk_desc *b, const svo_placement *pl, int op, svo_chunk_desc *out, uint64_t *changed_out);
int svo_world_chunk_stamp(svo_world *dst, int chunk, svo_world *src, int src_chunk, const svo_placement *pl, int op, uint64_t *changed_out);

/* ---- the extract: a cube of cells copied out of a chunk at any cell offset, in any orientation of the cube -----------------------
 * The stamp is the editor's paste; this is its copy, and its exact inverse: a piece of a depth-12 terrain chunk lifted out as a depth-6
 * model, a selection saved with svo_chunk_write, a deep chunk split into its eight octants, a chunk turned, mirrored or shifted in
 * place - WITHOUT a dense grid.  Definition: A is the source, of depth D_A, and C the result, of depth D_C <= D_A, both in
 * [SVO_EXTRACT_MIN_DEPTH, SVO_EXTRACT_MAX_DEPTH]; N_A = 2^D_A, N_C = 2^D_C, and G_A the grid of A's finest voxels, as
 * svo_world_chunk_to_grid reports it (as for the chunk CSG above).  Positions and sizes are not consulted: ONE CELL OF A IS ONE CELL OF
 * C.  The placement is the stamp's and is read exactly as the stamp reads it (orient = perm * 8 + flips, pi from the table there,
 * flips one bit per OUTPUT axis).  For every d in [0, N_C)^3 take p = offset + d:
 *   v = G_A[p] if every p_i lies in [0, N_A), else 0
 *   q[pi(i)] = (flips bit i) ? N_C - 1 - d_i : d_i
 *   G_C[q] = v
 * So C, oriented by the placement the way the stamp orients B, is the window [offset, offset + N_C)^3 of A; WHAT LIES OUTSIDE A READS
 * 0.  C is the tree of G_C by svo_chunk_from_grid's rule (FIFO visiting order, a uniform 4^3 block a LEAF, minimal pools), ALWAYS
 * rebuilt; *occupied_out (may be NULL) receives the number of cells of G_C that are not 0.  For D_A <= SVO_GRID_MAX_DEPTH the result
 * is, index for index, svo_chunk_from_grid of that window of svo_world_chunk_to_grid's grid, oriented; above it the same sentences
 * define it.  No grid is allocated: working memory is proportional to the entries of the walk, which follow the RESULT - an A that is
 * one LEAF word, read at an odd offset partly outside, leaves bricks along the faces.  The host form and the device form give the same
 * pools and the same count.
 * With E the one-word EMPTY chunk of A's depth and C = extract(A, pl):  stamp(A, C, pl, SVO_COMBINE_OVER) changes 0 cells;
 * stamp(A, C, pl, SVO_COMBINE_SUBTRACT) changes exactly *occupied_out cells;  stamp(A, C, pl, SVO_COMBINE_INTERSECT) and
 * stamp(E, C, pl, SVO_COMBINE_MAX) give the same pools;  with D_C = D_A, offset 0 and orient 0 the pools are
 * svo_chunk_combine(A, E, SVO_COMBINE_MAX)'s, that is A rebuilt.
 *
 * svo_chunk_extract (host; `a` and `*out` host pools): D_C is `depth`, and *out receives malloc'ed pools with the frame `position` /
 * `size`, as in svo_chunk_from_grid, freed with svo_chunk_free; `a` is not modified; out may not alias a.  It needs no device.
 * svo_world_chunk_extract (device): A is chunk `src_chunk` of the UPLOADED world src, C chunk `chunk` of the UPLOADED world dst on the
 * same device; D_C is that chunk's depth, and its position, size and depth stay; what it held is replaced.  src may be dst, and
 * src_chunk == chunk of the same world is defined - the turn or the shift in place: A is read completely before C is installed.  The
 * source chunk is never written.  Ordered, complete and installed as svo_world_chunk_stamp.  THE DEVICE WALK VISITS ONLY WHAT THE
 * WINDOW REACHES: a malformed word elsewhere in A goes unseen.
 *
 * Refusals, in the stamp's order and all before anything changes or is written: SVO_ERR_INVALID_ARG for a NULL world / a / out, out ==
 * a, a chunk out of range in either world, NULL pools, a NULL placement, orient > 47 or an offset outside [-65536, 65536], (host form)
 * a NULL position, a size that is not finite or not > 0 and pools that svo_world_create's validation would refuse, (device form) two
 * worlds resident on different devices; then SVO_ERR_NOT_UPLOADED for either world (device form); then SVO_ERR_UNSUPPORTED for D_C >
 * D_A (that direction is the stamp into an empty chunk), a depth outside [2, 16], a TWIG above level depth-2 in A (host form: anywhere
 * in A; device form: where the walk meets it) and 2^30 entries, nodes or bricks; SVO_ERR_OUT_OF_MEMORY when the working arrays do not
 * fit; on the device a malformed pool found by the walk is SVO_ERR_MALFORMED_TREE, with nothing installed. */
#define SVO_EXTRACT_MIN_DEPTH 2
#define SVO_EXTRACT_MAX_DEPTH 16
int svo_chunk_extract(const svo_chunk_desc *a, const svo_placement *pl, uint32_t depth, const float position[3], float size, svo_chunk_desc *out, uint64_t *occupied_out);
int svo_world_chunk_extract(svo_world *dst, int chunk, svo_world *src, int src_chunk, const svo_placement *pl, uint64_t *occupied_out);

/* ---- the hot path ------------------------------------------------------------------------ */

/* Trace the pixel rectangle [x0,x0+w) x [y0,y0+h) of `cam`'s image.  out_dev receives w*h
 * records, row-major within the rectangle.  Rays launched = w*h (+ one per hit when shadow). */
int svo_trace(svo_world *, const svo_camera *cam, const svo_trace_params *params,
              int x0, int y0, int w, int h, svo_hit *out_dev, void *stream);

/* Trace the horizontal bands b = band0 + k*band_stride (k = 0..nbands-1) of the full-width image;
 * band b covers rows [b*band_height, (b+1)*band_height).  This is the interleaved tile-row
 * partition used for multi-GPU (rank r of N: band0 = r, band_stride = N, band_height = 8).
 * out_dev receives nbands*band_height*cam->width records, bands stacked in k order; rows that
 * fall below the image are written as misses. */
int svo_trace_rows(svo_world *, const svo_camera *cam, const svo_trace_params *params,
                   int band0, int band_stride, int nbands, int band_height,
                   svo_hit *out_dev, void *stream);

/* Several World::draw calls (src/World.cpp:205-266; the reference issues two marches per displayed frame, the light's
 * and the eye's, src/Main.cpp:190-222) in ONE launch: nframes (1..SVO_MAX_FRAMES) cameras of one image size, the same rectangle / bands of
 * each; frame f's records follow frame f-1's in out_dev (nframes consecutive rasters).  Results are those of nframes
 * separate svo_trace / svo_trace_rows calls.  What it buys: the stack kernel's persistent waves run through all the
 * frames' tiles behind one set of cursors, so they drain once per launch instead of once per frame (stereo pairs,
 * cube-map faces, shadow cascades, several viewports, or simply the next frames of a pipelined renderer). */
#define SVO_MAX_FRAMES 16
int svo_trace_frames(svo_world *, const svo_camera *cams, int nframes, const svo_trace_params *params,
                     int x0, int y0, int w, int h, svo_hit *out_dev, void *stream);
int svo_trace_rows_frames(svo_world *, const svo_camera *cams, int nframes, const svo_trace_params *params,
                          int band0, int band_stride, int nbands, int band_height,
                          svo_hit *out_dev, void *stream);

/* chunkmarch over an explicit list: origins_dev/dirs_dev are [n][3] float on the device. */
int svo_trace_rays(svo_world *, const float *origins_dev, const float *dirs_dev, int64_t n,
                   const svo_trace_params *params, svo_hit *out_dev, void *stream);

/* Bounded rays: svo_trace_rays with a far end per ray, tmax_dev[n] float on the device.  With R[k] the record svo_trace_rays
 * writes for ray k under the same params:
 *   out[k] = R[k], byte for byte (shadow bits included when params->shadow != 0), if R[k] has SVO_HIT_FLAG, has no SVO_ERR_FLAG
 *            and R[k].t < tmax_dev[k] (one float compare, strict);
 *   out[k] = the miss record (all zero) otherwise; no shadow ray is cast from a dropped hit.
 * So tmax = +inf reproduces svo_trace_rays, and tmax <= 0 or NaN (the compare is false) gives a miss.  The march ENDS at the far
 * end, it is not filtered afterwards: a ray stops as soon as no later hit can have t < tmax.  A ray is given up with SVO_ERR_FLAG
 * only where its march has not yet passed tmax; such records stay outside the equality above, as they do between the two kernels.
 * Every field of params means what it means for svo_trace_rays.  counters_dev (literal kernel) counts what the BOUNDED march
 * read - never more than the unbounded one, in any word of any ray; it has no CPU-oracle counterpart.  svo_trace_last_ray_count
 * reports n, plus one per kept hit when params->shadow != 0.  tmax_dev == NULL with n > 0 is SVO_ERR_INVALID_ARG; n == 0 is SVO_OK. */
int svo_trace_segments(svo_world *, const float *origins_dev, const float *dirs_dev, const float *tmax_dev, int64_t n,
                       const svo_trace_params *params, svo_hit *out_dev, void *stream);

/* Point queries: which node, which box, what material lies at each point - traverse() (src/Traverse.cpp:34-48), which the reference
 * calls once per march step, over a device list: points_dev is [n][3] float, out_dev receives n records.  Collision and "is this
 * position solid", standing a body on the terrain, free space for particles, the voxel under an edit cursor - and the voxel box
 * that svo_hit does not carry.  For p = points_dev[3k..3k+2], every operation in float, separately rounded, in the reference's order:
 *   1. the world box of chunkmarch (:129-133): !isInsideCube(p, chunkmin, chunkmax) - closed; NaN and +-inf fail - gives out[k] all zero;
 *   2. i = index(index_float(p)), cmin = chunk[i].position: !isInsideCube(p, cmin, cmin + chunksize) (the check of :154) gives out[k]
 *      all zero - on the world's max faces, where the toroidal index wraps to a chunk that does not hold p;
 *   3. (bmin, size, node) = traverse(p, chunk[i]): the child is chosen by p >= bmin + halfsize per axis;
 *   4. an EMPTY node: { bmin, size, material 0, SVO_LOCATE_INSIDE, i, node, SVO_CELL_NONE };
 *   5. a LEAF node: the same with material = offset & 0xFFFF and SVO_LOCATE_INSIDE | SVO_LOCATE_SOLID (whatever the material: the
 *      march hits every LEAF);
 *   6. a TWIG node: leafsize = size / 4, off = ivec3((p - bmin) / leafsize) - under SVO_SEMANTICS_GLSL ivec3((p - bmin) * (1 / leafsize)).
 *      off outside [0,3]^3 (a point on the chunk's max face; twigmarch returns "no hit" there, :59): the TWIG node's own box,
 *      material 0, SVO_CELL_NONE, SVO_LOCATE_INSIDE.  Otherwise cell = z*16 + y*4 + x, bmin = node bmin + vec3(off) * leafsize,
 *      size = leafsize, material = the brick's cell, SVO_LOCATE_SOLID iff it is not 0;
 *   7. params->see_through = m: a LEAF or a cell of material m is reported with material 0 and without SVO_LOCATE_SOLID; node, cell
 *      and box are unchanged - the records of the same world with those words rewritten to 0.
 * params == NULL means defaults; only kernel, semantics and see_through are read.  SVO_KERNEL_LITERAL walks the tree pool, one load
 * per level, on any geometry; SVO_KERNEL_STACK walks the stack kernel's wide trees, two levels per load, and is refused with
 * SVO_ERR_UNSUPPORTED where svo_trace refuses that kernel (no wide trees, exact_geometry == 0); SVO_KERNEL_AUTO takes the wide walk
 * where it is allowed.  Both write the same records, byte for byte.
 * n < 0, a NULL points_dev / out_dev with n > 0, see_through > 0xFFFF, an unknown semantics or kernel: SVO_ERR_INVALID_ARG; then a world
 * that is not resident: SVO_ERR_NOT_UPLOADED; then n == 0: SVO_OK.  All of these are settled before any device work.
 * Asynchronous on `stream` and ordered against updates, edits and shifts like svo_trace_rays.  The call takes no launch slot and no
 * scratch: calls on different streams are independent, and svo_trace_last_ray_count does not see it. */
enum {
    SVO_LOCATE_INSIDE = 1u << 0,    /* the point lies in the world box and in its chunk's box: every other field is valid */
    SVO_LOCATE_SOLID  = 1u << 1     /* a LEAF node or a brick cell that is not 0 (after see_through) */
};
typedef struct svo_voxel {          /* 32 bytes, laid out like svo_hit */
    float    bmin[3];               /* Tree::bmin of traverse(), or the brick cell's leafmin (src/Traverse.cpp:66) */
    float    size;                  /* Tree::size, or leafsize for a brick cell */
    uint16_t material;              /* 0 for EMPTY / an empty cell; LEAF offset & 0xFFFF; brick cell value */
    uint16_t flags;                 /* SVO_LOCATE_* */
    uint32_t chunk;                 /* World::index() linear chunk index */
    uint32_t node;                  /* index in that chunk's tree[] of the EMPTY / LEAF / TWIG node traverse() ends in */
    uint32_t cell;                  /* brick cell word z*16+y*4+x, or SVO_CELL_NONE */
} svo_voxel;
int svo_world_locate(svo_world *, const float *points_dev, int64_t n,
                     const svo_trace_params *params, svo_voxel *out_dev, void *stream);

/* The box of every hit: out_dev[k] is the voxel that record k of gbuffer_dev names - what fragment main has as `hit` (hit.bmin, hit.size,
 * shaders/World.Fragment.glsl:168-172) and svo_hit has no room for.  It cannot be rebuilt from t (chunkmarch, treemarch and twigmarch
 * each restart t from their own entry point, src/Traverse.cpp:56,81,144,160) but follows from the ids, which every trace entry point
 * writes: picking, the edit cursor (the box goes straight into svo_world_edit_box), leafUV.
 * A record gets a box if it has SVO_HIT_FLAG, has no SVO_ERR_FLAG, chunk < the world's chunk count, node < that chunk's trees, the node
 * is reachable from the chunk's root and is a LEAF (with cell == SVO_CELL_NONE) or a TWIG (with cell <= 63).  Then, every operation in
 * float, separately rounded:
 *   (bmin, size) = what traverse() (src/Traverse.cpp:34-48) holds on arriving at node: from (chunk.position, chunk.size), per level
 *                  halfsize = size * 0.5f, bmin = bmin + vec3(ge) * halfsize with ge the bits of the child slot (x + 2y + 4z);
 *   a brick cell:  leafsize = size / 4, bmin = bmin + vec3(cell & 3, (cell >> 2) & 3, cell >> 4) * leafsize, size = leafsize (:66);
 *   out[k] = { bmin, size, the RECORD's material (a see-through launch's records keep theirs), SVO_LOCATE_INSIDE | SVO_LOCATE_SOLID,
 *              chunk, node, cell }.
 * Every other record - a miss, an error record, ids that name nothing reachable - gives an all-zero out[k]; nothing is read out of
 * range whatever the ids hold.  A G-buffer that went through svo_gbuffer_pack / svo_gbuffer_unpack has lost its ids (unpack zeroes
 * them): take the boxes before packing.
 * The walk needs each node's parent, which the pools do not hold: a parent index - per 8-block of the tree pool the BRANCH that owns it
 * and its level, reachable blocks only, so that a BRANCH word in a block an edit orphaned never counts; 5 bytes per 8 node words - is
 * built on the device at the first call (level-synchronous sweeps, nothing read back) and dropped by every change to the pools
 * (svo_world_update / _edit_box / _shift / _compact / _coarsen / _upload, destroy).  svo_world_info does not count it; if it cannot
 * be allocated the call is SVO_ERR_OUT_OF_MEMORY and nothing is written.
 * n < 0 or a NULL gbuffer_dev / out_dev with n > 0: SVO_ERR_INVALID_ARG; then a world that is not resident: SVO_ERR_NOT_UPLOADED; then
 * n == 0: SVO_OK - all settled before any device work.  Asynchronous on `stream`, ordered against updates, edits and shifts like
 * svo_world_locate; calls of one world on different streams are ordered behind one another only while the index is being built. */
int svo_hit_voxels(svo_world *, const svo_hit *gbuffer_dev, int64_t n, svo_voxel *out_dev, void *stream);

/* leafUV (shaders/World.Fragment.glsl:5-15) per pixel of the rectangle svo_trace(cam, x0, y0, w, h) filled: gbuffer_dev its w*h records,
 * voxels_dev what svo_hit_voxels wrote for them, uv_dev w*h float2.  For a record with SVO_HIT_FLAG, without SVO_ERR_FLAG, whose voxel
 * record has SVO_LOCATE_INSIDE - every float operation separately rounded, eps == 0 meaning 1/8192 (pass the launch's):
 *   point = o + d * (t - eps)       (o, d) the pixel's camera ray as the march forms it;
 *   iuv   = cubeUV(point, bmin, bmin + size)   (shaders/Chunkmarch.glsl:138-149): size = cmax.x - cmin.x, uv = (0, 0), then the six
 *           tests abs(p.x - cmin.x) <= eps: uv = p.yz - cmin.yz; p.x, cmax: p.yz - cmax.yz; p.y, cmin: p.xz - cmin.xz; p.y, cmax;
 *           p.z, cmin: p.xy - cmin.xy; p.z, cmax - in this order, a later one that holds winning; iuv = abs(uv) / size;
 *   iuv  += (vec2(lessThan(iuv, 0.125)) - vec2(greaterThan(iuv, 0.125))) * eps * 2;
 *   uv    = (vec2(m & 0xff, (m >> 8) & 0xff) + iuv) / 256, m the record's material.
 * Every other pixel gets (0, 0).  Any sampler can texture from this.  A NULL pointer, a negative rectangle, a camera without an image
 * size or eps < 0: SVO_ERR_INVALID_ARG.  Asynchronous on `stream`. */
int svo_hit_uv(const svo_camera *cam, float eps, int x0, int y0, int w, int h,
               const svo_hit *gbuffer_dev, const svo_voxel *voxels_dev, float *uv_dev, void *stream);

/* Voxel ambient occlusion (not in the reference: an opt-in departure, as svo_trace_local_shadows is): ao_dev[k] in [0, 1], 1 = open,
 * for pixel k of the rectangle svo_trace(cam, x0, y0, w, h) filled - gbuffer_dev its w*h records (or the surface records of a
 * translucent frame), voxels_dev what svo_hit_voxels wrote for them.  The occluders of a surface point are the eight lattice cells
 * around the open cell in front of the face that was hit; "is this cell solid" is what svo_world_locate answers.  No rays, no sampling.
 * Of params only eps, semantics, kernel and see_through are read (NULL = defaults); eps == 0 means 1/8192, or 1/4096 under
 * SVO_SEMANTICS_GLSL, as in svo_trace_local_shadows.
 * A pixel gets the rule below if its record has SVO_HIT_FLAG and no SVO_ERR_FLAG, its voxel record has SVO_LOCATE_INSIDE and the voxel
 * record's chunk is below the world's chunk count (checked before anything is loaded through it).  Every other pixel gets 1.0f.
 * In float throughout, every operation separately rounded:
 *   1. sample point   (o, d) the pixel's camera ray as the march forms it; P = o + d * (t - eps) - the point the normals and leafUV
 *                     are taken at;
 *   2. face           lo = bmin, hi = bmin + size of the voxel record; the SVO_NORMAL_FACE rule: c = (lo + hi) * 0.5f, q = P - c,
 *                     the axis k is the one of the largest |q| (the first axis on ties), sgn is +1 or -1 like q[k], and against d[k]
 *                     when q[k] is exactly 0;
 *   3. lattice        e = cell if cell > 0; otherwise the finest voxel of the hit's chunk, ldexpf(chunksize, -(int)depth) with depth
 *                     of the voxel record's chunk - a LEAF hit, however large its node, is shaded on the chunk's finest lattice.
 *                     The lattice is anchored at the world origin;
 *   4. the open cell  in front of the face: u < v the two axes other than k; for j in {u, v}: r_j = P[j] / e, g_j = floorf(r_j),
 *                     f_j = r_j - g_j, Q[j] = (g_j + 0.5f) * e; Q[k] = (sgn > 0 ? hi[k] : lo[k]) + sgn * (e * 0.5f).  If r_u or r_v is
 *                     not finite the pixel gets 1.0f;
 *   5. neighbours     (a, b) = (-1,-1), (0,-1), (1,-1), (-1,0), (1,0), (-1,1), (0,1), (1,1): N = Q with N[u] = Q[u] + (float)a * e,
 *                     N[v] = Q[v] + (float)b * e; occ(a, b) = 1 iff the record svo_world_locate writes for N under params has
 *                     SVO_LOCATE_SOLID - a point outside the world or off its chunk is open, a LEAF is solid whatever its material,
 *                     see_through = m opens material m;
 *   6. corners        for (sa, sb) in {-1, +1}^2: s1 = occ(sa, 0), s2 = occ(0, sb), cn = occ(sa, sb);
 *                     level = (s1 && s2) ? 0 : 3 - (s1 + s2 + cn); A(sa, sb) = (float)level / 3.0f;
 *   7. bilinear       l0 = A(-1,-1) + (A(1,-1) - A(-1,-1)) * f_u; l1 = A(-1,1) + (A(1,1) - A(-1,1)) * f_u; ao = l0 + (l1 - l0) * f_v.
 *                     Four open corners give exactly 1, four closed ones exactly 0.
 * Kernel selection is svo_world_locate's: SVO_KERNEL_LITERAL walks the tree pool, SVO_KERNEL_STACK the wide trees (refused with
 * SVO_ERR_UNSUPPORTED where svo_world_locate refuses it), SVO_KERNEL_AUTO the wide trees where they are allowed; all write the same floats.
 * A NULL world or cam, a NULL buffer with w*h > 0, a rectangle that starts or extends backwards, cell negative, NaN or infinite,
 * see_through > 0xFFFF, an unknown semantics or kernel: SVO_ERR_INVALID_ARG; then a world that is not resident: SVO_ERR_NOT_UPLOADED;
 * then w*h == 0: SVO_OK; w*h >= 2^31: SVO_ERR_UNSUPPORTED.  All settled before any device work; a refused call writes nothing.
 * Asynchronous on `stream`, ordered against updates, edits and shifts like svo_world_locate.  No launch slot and no scratch: calls on
 * different streams are independent.  Nothing is cached: the pools are read as they are, the call after an edit sees the edit. */
int svo_hit_ao(svo_world *, const svo_camera *cam, const svo_trace_params *params, float cell,
               int x0, int y0, int w, int h,
               const svo_hit *gbuffer_dev, const svo_voxel *voxels_dev, float *ao_dev, void *stream);

/* svo_hit_ao's factor on an image a shade call has written (n float4 pixels): f = 1.0f - strength * (1.0f - ao); r, g and b are each
 * multiplied by f, the depth float is not written.  ao == 1 gives f == 1 exactly and the pixel keeps its bits; a NaN ao leaves its
 * pixel alone.  It goes after svo_shade* and before svo_shade_sky, svo_shade_boxes and svo_frame_rgba8 (miss pixels have ao == 1).
 * Scaling the whole colour, not only the ambient addend, is a stated departure: svo_shade stays as it is.
 * strength outside [0, 1] or NaN, n < 0, a NULL pointer with n > 0: SVO_ERR_INVALID_ARG; n == 0: SVO_OK.  Asynchronous on `stream`. */
int svo_shade_ao(const float *ao_dev, float strength, int64_t n, float *rgba_dev, void *stream);

/* order_dev[0..ntiles) = the tile indices sorted by descending cost[i][0] + cost[i][1] (a stable device sort; cost_dev as
 * svo_trace_params.tile_cost_dev of ONE frame wrote it).  Asynchronous on `stream`; calls of one world on different streams are
 * ordered behind one another on the device (they share the world's sort scratch), each call's order_dev is complete when the
 * work issued on its own stream before reaches it.  A launch ignores entries of tile_order_dev that are not tile indices (such a
 * tile is skipped, its pixels stay unwritten) rather than read out of range. */
int svo_tile_order(svo_world *, const uint32_t *cost_dev, uint32_t *order_dev, int ntiles, void *stream);

/* See-through materials (shaders/ParallaxAlpha.Fragment.glsl:141-199,276-335): trace the rectangle like svo_trace, and march on
 * past every surface hit of material m = params->see_through (1..0xFFFF; 0 is SVO_ERR_INVALID_ARG).
 *   surface_dev  w*h records: exactly what svo_trace writes with see_through = 0 (shadow included), plus SVO_SEE_THROUGH on every
 *                hit (SVO_HIT_FLAG without SVO_ERR_FLAG) whose material is m;
 *   behind_dev   w*h records: for such a pixel, what svo_trace_rays(see_through = m) writes for the continuation ray - the pixel's
 *                primary direction d from origin p1 = o + d * t1 (o the eye, t1 = surface.t; per component, separately rounded) -
 *                shadow ray included, so behind.t is measured from p1: the path length through the liquid.  All-zero elsewhere.
 * Asynchronous on `stream`; the continuation list lives in the world's scratch (calls of one world on different streams are
 * ordered behind one another on the device).  counters_dev / tile_cost_dev / tile_order_dev apply to the surface launch only, and
 * svo_trace_last_ray_count reports the continuation launch (w*h rays: pixels that are not continued get a ray that misses the world). */
int svo_trace_translucent(svo_world *, const svo_camera *cam, const svo_trace_params *params,
                          int x0, int y0, int w, int h, svo_hit *surface_dev, svo_hit *behind_dev, void *stream);

/* Shadows from the point light and the spotlight, one flag per light.  The reference hands the directional light's shadow term to
 * all three light functions (shaders/World.Fragment.glsl:186-190), and so does svo_shade on a record without SVO_LOCAL_SHADOWS;
 * this call is the opt-in departure.  gbuffer_dev holds the w*h records that svo_trace(cam, params, x0, y0, w, h) wrote (or the
 * surface records of svo_trace_translucent).  For every record with SVO_HIT_FLAG and without SVO_ERR_FLAG, and every light asked
 * for (position L; NULL = not asked for, both NULL is SVO_ERR_INVALID_ARG):
 *   P = o + d * (t - eps)   (o, d) the pixel's camera ray, eps the launch's (0 = 1/8192, 1/4096 under SVO_SEMANTICS_GLSL): the point
 *                           the directional shadow ray starts from; every operation separately rounded;
 *   v = L - P, q = v.x*v.x + v.y*v.y + v.z*v.z (left to right), direction v * (1 / sqrt(q)), dist = sqrt(q);
 *   the ray (P, direction) is marched as svo_trace_rays marches it with `params` and shadow = 0 (eps, caps, semantics, kernel and
 *   see_through are honoured); the light is OCCLUDED iff that ray's record has SVO_HIT_FLAG, has no SVO_ERR_FLAG and its t < dist -
 *   terrain behind the light does not shadow it, a runaway ray is "traced, not occluded".  q == 0 or not finite: no ray, not occluded.
 * The record then gets SVO_LOCAL_SHADOWS, and SVO_SHADOWED_POINT / SVO_SHADOWED_SPOT are written: the occlusion of a light asked for,
 * a copy of the record's SVO_SHADOWED for a light that was not (it keeps the reference's behaviour).  No other byte of the record
 * changes; records without a hit or with SVO_ERR_FLAG stay exactly as they were.  The three bits lie in the low flag byte, so
 * svo_gbuffer_pack carries them and svo_shade(_packed / _translucent) uses them: one shadow factor per light.
 * All the lights' rays go through ONE ray-list launch (svo_trace_last_ray_count then reports lights * w * h: pixels without a usable
 * hit get a ray that misses the world); the list and its records live in the world's scratch, 56 bytes per ray.  Asynchronous on
 * `stream`; calls of one world on different streams are ordered behind one another on the device. */
int svo_trace_local_shadows(svo_world *, const svo_camera *cam, const svo_trace_params *params,
                            const float point_position[3], const float spot_position[3],
                            int x0, int y0, int w, int h, svo_hit *gbuffer_dev, void *stream);

/* ---- shadow map: the directional light rendered once, looked up per frame ---------------------------------
 * The reference shadows its scene with a shadow map: each frame it marches the world from the directional light into a depth image
 * (World::draw_shadowmap, src/World.cpp:162-203) and computeShadow looks every hit point up in it (shaders/World.Fragment.glsl:140-155).
 * svo_trace_params.shadow replaces that with one exact shadow ray per primary hit, paid for on every frame.  The directional light
 * does not move with the camera: with a fixed sun and a world that changes only at edits, render the map once, then trace every
 * frame with shadow = 0 and apply the map - one gather per hit pixel.
 * A departure, as svo_trace_local_shadows is: the reference's pass marches one uniform ray per fragment from the light's position
 * (its per-fragment direction is commented out, shaders/ShadowmapWorld.Fragment.glsl:8), compares an inverse-distance depth, and its
 * sampler wraps (GL_REPEAT, src/Light.cpp:176-179).  Here the light's view is a true orthographic raster of parallel rays, the depth
 * is the march's own t, and a point outside the map is lit.  One bit per light in the record: no PCF (out of scope). */
typedef struct svo_shadowmap {
    float   origin[3];              /* centre of the light's image plane; rays start ON this plane */
    float   direction[3];           /* unit; every ray's direction (directionalLight.direction) */
    float   right[3], up[3];        /* orthonormal with direction (the caller's, as svo_camera's basis is) */
    float   half_width, half_height;    /* world units: glm::ortho(-w, w, -h, h), src/Camera.cpp:50-53 */
    int32_t width, height;          /* texels; multiples of 8, 8..16384 */
    float  *depth_dev;              /* width*height float, row-major, row 0 at +up */
} svo_shadowmap;

/* A map that holds the whole world.  Host only, needs no device.  Fills everything in *out except depth_dev, which is left as it is:
 * direction normalised; right and up completing an orthonormal basis from the hint (0,1,0), or (0,0,1) when the direction is within
 * about 8 degrees of vertical (right = normalize(direction x hint), up = right x direction, as svo_camera's basis is made); the plane
 * placed so that every corner c of the world box (chunkcoordmin * chunksize to + dims * chunksize) has dot(c - origin, direction) >= 1;
 * half extents so that every corner projects strictly inside (-half_width, half_width) x (-half_height, half_height).  Computed in
 * double, rounded to float once; the properties are the contract, not the bits.
 * A NULL argument, a zero, NaN or infinite direction, a width or height that is not a multiple of 8 in 8..16384: SVO_ERR_INVALID_ARG. */
int svo_shadowmap_fit(const svo_world *, const float direction[3], int width, int height, svo_shadowmap *out);

/* Render the map.  Texel (i, j) marches the ray - every operation in float, separately rounded, the shape of svo_camera's u and v -
 *   u = (((i + 0.5f) / width ) * 2 - 1) * half_width
 *   v = (1 - ((j + 0.5f) / height) * 2) * half_height
 *   o = origin + right * u + up * v      (per component, left to right)
 *   d = direction                        (as given, not re-normalised)
 * exactly as svo_trace_rays marches (o, d) under `params` with shadow = 0 and counters_dev / tile_cost_dev / tile_order_dev dropped:
 * eps, the caps, semantics, kernel and see_through are honoured (see_through: a shadow map that water does not darken).
 *   depth_dev[j*width + i] = that record's t if it has SVO_HIT_FLAG and no SVO_ERR_FLAG, +inf otherwise.
 * All texels go through ONE ray-list launch (svo_trace_last_ray_count then reports width*height).  The list is written in tile order -
 * slot tile*64 + jj*8 + ii holds texel (8*(tile % (width/8)) + ii, 8*(tile / (width/8)) + jj) - so that a wave marches an 8x8 block of
 * neighbouring parallel rays; nothing observable depends on it.  The list and its records live in the world's scratch, 56 bytes per
 * texel; calls of one world on different streams are ordered behind one another on the device.
 * SVO_ERR_INVALID_ARG: a NULL world, map, params or depth_dev; a width or height that is not a multiple of 8 in 8..16384; a half_* that
 * is not greater than 0 or not finite; a non-finite origin or basis; | |direction|^2 - 1 | > 1e-3.  Then whatever svo_trace_rays would
 * refuse (SVO_ERR_NOT_UPLOADED and the rest).  All settled before any device work.  Asynchronous on `stream`, ordered against updates,
 * edits and shifts as svo_trace_rays is.  A map rendered before an edit is STALE: nothing invalidates it, re-rendering it is the
 * caller's job. */
int svo_shadowmap_render(svo_world *, const svo_shadowmap *map, const svo_trace_params *params, void *stream);

/* Look the hits of a frame up in the map.  Takes no world.  gbuffer_dev holds the w*h records that svo_trace(cam, ..., x0, y0, w, h)
 * wrote; eps is that launch's (0 = 1/8192; pass 1/4096 under SVO_SEMANTICS_GLSL), as with svo_hit_uv.  For every record with
 * SVO_HIT_FLAG and without SVO_ERR_FLAG, in float, every operation separately rounded:
 *   P  = o + d * (t - eps)                       (o, d) the pixel's camera ray: where the shadow ray would start
 *   q  = P - origin
 *   s  = q.x*D.x + q.y*D.y + q.z*D.z             (left to right; D = direction; likewise a with right, b with up)
 *   fu = (a / half_width  + 1) * 0.5f * (float)width
 *   fv = (1 - b / half_height) * 0.5f * (float)height
 *   inside   = fu >= 0 && fu < width && fv >= 0 && fv < height     (NaN fails)
 *   i = (int)floorf(fu), j = (int)floorf(fv)     nearest sampling, as the reference's; a texel-centre point maps back to i + 0.5
 *   occluded = inside && depth_dev[j*width + i] < s - bias
 * The record gets SVO_SHADOW_TRACED; SVO_SHADOWED is set if occluded and cleared if not; no other byte of it changes.  Records without
 * a usable hit stay byte for byte as they were.  A frame traced with shadow = 0 and then applied has the flag layout of a shadow = 1
 * frame: svo_shade* and svo_gbuffer_pack work on it unchanged.  Outside the map a point is lit (the reference's sampler wraps).
 * Bits 5-7 are not touched; svo_trace_local_shadows copies SVO_SHADOWED for a light not asked for, so svo_shadowmap_apply goes BEFORE it.
 * bias is the caller's, in world units along the light.  A texel is 2*half_width/width world units wide, and under a slanted light
 * the depth varies by about that much across it: one to two texel widths is a good start; too little gives acne, too much detaches
 * shadows from their casters.
 * SVO_ERR_INVALID_ARG: a NULL pointer, a negative rectangle or a camera without an image size, eps < 0, a negative or NaN bias, or the
 * map checks of svo_shadowmap_render.  w*h == 0: SVO_OK.  Asynchronous on `stream`. */
int svo_shadowmap_apply(const svo_camera *cam, const svo_shadowmap *map, float eps, float bias, int x0, int y0, int w, int h,
                        svo_hit *gbuffer_dev, void *stream);

/* ---- packed G-buffer (8 bytes / pixel) for the multi-GPU gather ------------------------------------------
 * { float t; uint32 w } with w = material (bits 0-15) | flags & 0xFF (bits 16-23) | normal code (bits 24-30) |
 * SVO_ERR_FLAG (bit 31): per axis 2 bits (0: -, 1: 0, 2: +) in bits 24-29, bit 30 = NaN normal.  cubeNormal only ever yields
 * normalize(ivec3 in {-1,0,1}^3) (shaders/Chunkmarch.glsl:128-136), so t, normal, material and flags survive the
 * round trip bit for bit; the parity ids (chunk, node, cell) are not carried (unpack zeroes them). */
int svo_gbuffer_pack(const svo_hit *gbuffer_dev, uint64_t *packed_dev, int64_t n, void *stream);
int svo_gbuffer_unpack(const uint64_t *packed_dev, svo_hit *gbuffer_dev, int64_t n, void *stream);

/* ---- shading stage: Blinn-Phong x 3 lights over the G-buffer --------------------
 * shaders/World.Fragment.glsl:63-138,180-197.  The reference multiplies the lights with gamma-decoded samples of
 * its Diffuse / Specular texture atlas, which is not part of the repository; in svo_shade the albedo comes from the
 * material table's diffuse / specular colours instead (pow(colour, gamma)) - svo_shade_textured samples an atlas the caller supplies -,
 * the shadow term from SVO_SHADOWED
 * for all three lights - or, on a record that carries SVO_LOCAL_SHADOWS, from SVO_SHADOWED_POINT for the point light, SVO_SHADOWED_SPOT
 * for the spotlight and SVO_SHADOWED for the directional light.
 * Output per pixel: float4 {r, g, b, depth} with depth = (1/dist - 1/near) / (1/far - 1/near) (gl_FragDepth,
 * World.Fragment.glsl:193-197); misses give {0,0,0,1}. */
typedef struct svo_material { float ambient[3], diffuse[3], specular[3]; float shininess; } svo_material;
typedef struct svo_shade_params {
    struct { float position[3], ambient[3], diffuse[3], specular[3]; float constant, linear, quadratic; } point;
    struct { float position[3], direction[3], ambient[3], diffuse[3], specular[3]; } directional;
    struct { float position[3], direction[3], ambient[3], diffuse[3], specular[3];
             float cos_phi, cos_gamma, constant, linear, quadratic; } spot;
    svo_material materials[8];      /* ML[8], World.Fragment.glsl:63-73 */
    float eps;                      /* 0 = 1/8192 */
    float gamma;                    /* 0 = 2.2 */
    float near_plane, far_plane;    /* 0 = 0.125 / 8192 (shaders/Chunkmarch.glsl:20-21) */
} svo_shade_params;

/* Fill `p` with the reference's lights (src/Main.cpp:101-131) and material table. */
void svo_shade_defaults(svo_shade_params *p);
/* Shade the rectangle a svo_trace(cam, x0, y0, w, h) call filled: gbuffer_dev has w*h records, rgba_dev w*h float4. */
int svo_shade(const svo_camera *cam, const svo_shade_params *p, int x0, int y0, int w, int h,
              const svo_hit *gbuffer_dev, float *rgba_dev, void *stream);
/* The same over the 8-byte records of svo_gbuffer_pack (what rank 0 holds after the multi-GPU gather): 8 B read + 16 B
 * written per pixel instead of 32 + 16; identical colours (the packed record carries t, normal, material, flags). */
int svo_shade_packed(const svo_camera *cam, const svo_shade_params *p, int x0, int y0, int w, int h,
                     const uint64_t *packed_dev, float *rgba_dev, void *stream);

/* svo_shade with the albedo the reference has (shaders/World.Fragment.glsl:178-182): diffuse = pow(texture(Diffuse, uv), gamma) and
 * specular = pow(texture(Specular, uv), gamma) at uv = svo_hit_uv's, in the place of the material table's diffuse / specular colours.
 * The atlas is the caller's: two RGB8 images of width x height texels on the device, rows tightly packed (GL_UNPACK_ALIGNMENT 1), row 0
 * at v = 0, a 256 x 256 grid of tiles - tile (m & 0xff, (m >> 8) & 0xff) belongs to material m.  specular_dev == NULL means the diffuse
 * image (src/Atlas.cpp:31-32).  Sampling is GL_NEAREST (src/Atlas.cpp:18-21) with GL's default repeat wrap:
 *   x = min(int(floor((u - floor(u)) * width)), width - 1), y likewise with v and height; texel = image[(y * width + x) * 3 ..]
 * and a texel byte b decodes to pow(b / 255.0f, gamma) in float, as the material table's colours do.  Everything else is svo_shade:
 * p->eps is the eps of the UV, materials[m].shininess, the shadow bits, depth, misses give {0,0,0,1}.  voxels_dev holds the records
 * svo_hit_voxels wrote for gbuffer_dev; a hit whose voxel record lacks SVO_LOCATE_INSIDE is shaded exactly as svo_shade shades it.
 * So a flat atlas of byte value b gives, bit for bit, svo_shade's image with every material's diffuse and specular set to b / 255.0f. */
typedef struct svo_atlas { const uint8_t *diffuse_dev, *specular_dev; int32_t width, height; } svo_atlas;
int svo_shade_textured(const svo_camera *cam, const svo_shade_params *p, const svo_atlas *atlas, int x0, int y0, int w, int h,
                       const svo_hit *gbuffer_dev, const svo_voxel *voxels_dev, float *rgba_dev, void *stream);

/* ParallaxAlpha's blend (shaders/ParallaxAlpha.Fragment.glsl:226-234,315-323) over the two G-buffers of svo_trace_translucent:
 * C_s = svo_shade of the surface record, C_b = svo_shade of the behind record with its t replaced by t1 + t2 (the distance from the
 * eye, chunkmarch's own t += s), s = clamp(t2 * absorption, 0, 1) with absorption 0 meaning 0.5 (the reference's water alpha);
 * rgb = C_b * (1 - s) + C_s * s, depth = C_b's.  The clamp departs from the reference, whose 1 - s goes negative past a path of
 * 1 / absorption.  A pixel whose behind record misses is C_s; a pixel without SVO_SEE_THROUGH is exactly what svo_shade writes. */
int svo_shade_translucent(const svo_camera *cam, const svo_shade_params *p, float absorption, int x0, int y0, int w, int h,
                          const svo_hit *surface_dev, const svo_hit *behind_dev, float *rgba_dev, void *stream);

/* The skybox behind the misses (src/Skybox.cpp, shaders/Skybox.*.glsl; drawn at depth 1 behind everything, src/Main.cpp:227), over an
 * image that svo_shade, svo_shade_packed, svo_shade_translucent or svo_shade_textured has already written for the same rectangle.
 * Exactly one of gbuffer_dev (the w*h 32-byte records) and packed_dev (svo_gbuffer_pack's 8-byte records) is non-NULL; for a
 * translucent frame pass the surface records.  A pixel is a sky pixel iff its record lacks SVO_HIT_FLAG - exactly the set svo_shade
 * writes as {0,0,0,1}.  A sky pixel gets its r, g and b replaced; its depth float is not written (it stays 1, the skybox's xyww
 * depth); every other pixel, and everything outside w*h pixels, is not written at all.
 * The cube map is the caller's: six size x size RGB8 images on the device, rows tightly packed, row 0 at t = 0 (as glTexImage2D takes
 * them), in the order of GL_TEXTURE_CUBE_MAP_POSITIVE_X + i: +X, -X, +Y, -Y, +Z, -Z - the reference's right, left, top, bottom, front,
 * back (src/Skybox.cpp:15-23,45).  Every operation below is in float and separately rounded, divisions are IEEE:
 *   d        the pixel's direction exactly as the march forms it (svo_camera above).  The reference interpolates the normalised corners
 *            of a rasterised cube instead: a departure a per-pixel renderer has to make.
 *   axis     ax, ay, az = |d.x|, |d.y|, |d.z|; X is the major axis if ax >= ay && ax >= az, otherwise Y if ay >= az, otherwise Z; ma is
 *            that magnitude.  !(ma > 0) - a zero or NaN direction - leaves the pixel as it is.
 *   face     the OpenGL cube-map table; the positive face unless the major component is < 0:
 *              +X: sc = -d.z, tc = -d.y    -X: sc =  d.z, tc = -d.y
 *              +Y: sc =  d.x, tc =  d.z    -Y: sc =  d.x, tc = -d.z
 *              +Z: sc =  d.x, tc = -d.y    -Z: sc = -d.x, tc = -d.y
 *            s = (sc / ma + 1) * 0.5, t = (tc / ma + 1) * 0.5.
 *   texel    T(x, y) = image[(y * size + x) * 3 ..] of the chosen face, a byte b decoding to (float)b / 255.0f - no gamma: the
 *            reference draws the sky with GL_FRAMEBUFFER_SRGB off.
 *   SVO_SKY_NEAREST   x = min(max((int)floor(s * size), 0), size - 1), y likewise from t; the colour is T(x, y).
 *   SVO_SKY_LINEAR    (the reference, src/Skybox.cpp:49-50; CLAMP_TO_EDGE within the face - it does not enable seamless cube maps)
 *            u = s * size - 0.5f, i = floor(u), a = u - i, xl = clamp((int)i, 0, size - 1), xr = clamp((int)i + 1, 0, size - 1);
 *            v, j, b, yl, yr likewise from t; per channel top = T(xl,yl) + (T(xr,yl) - T(xl,yl)) * a,
 *            bot = T(xl,yr) + (T(xr,yr) - T(xl,yr)) * a, c = top + (bot - top) * b - a face of one colour comes out as exactly that colour.
 * A NULL cam, sky, rgba_dev or face pointer, size <= 0, an unknown filter, both record pointers given or neither, a negative
 * rectangle, a camera without an image size: SVO_ERR_INVALID_ARG, settled before any device work.  w*h == 0 is SVO_OK.  Takes no
 * world; asynchronous on `stream`. */
enum { SVO_SKY_LINEAR = 0, SVO_SKY_NEAREST = 1 };
typedef struct svo_sky {
    const uint8_t *faces_dev[6];    /* +X, -X, +Y, -Y, +Z, -Z */
    int32_t size;                   /* faces are size x size RGB8 */
    int32_t filter;                 /* SVO_SKY_LINEAR: the reference */
} svo_sky;
int svo_shade_sky(const svo_camera *cam, const svo_sky *sky, int x0, int y0, int w, int h,
                  const svo_hit *gbuffer_dev, const uint64_t *packed_dev, float *rgba_dev, void *stream);

/* n float4 pixels {r, g, b, depth} to the RGBA8 of the reference's colour attachment (src/GBuffer.cpp): memory order R, G, B, A, one
 * 4-byte store per pixel.  Per colour channel c: NaN or c <= 0 gives 0, c >= 1 gives 255, anything else (uint8_t)(int)(c * 255.0f + 0.5f).
 * A is 255 for every pixel (shaders/GBuffer.Fragment.glsl:10); the depth float does not enter the colour.
 * n < 0, or a NULL pointer with n > 0: SVO_ERR_INVALID_ARG; n == 0: SVO_OK.  Asynchronous on `stream`. */
int svo_frame_rgba8(const float *rgba_dev, int64_t n, uint32_t *out_dev, void *stream);

/* ---- mirror reflections: one bounce off axis-aligned voxel faces --------------------------------------------
 * Not in the reference: an opt-in departure, as svo_trace_local_shadows and svo_hit_ao are.  Every generated world has a lake
 * (svo_terrain_params.water_material); a voxel face is axis-aligned, so its mirror ray is the incoming ray with one sign flipped, and
 * svo_trace_rays marches it.  svo_trace_reflections marches the mirror rays of a rectangle, svo_shade_reflections blends what they saw
 * over the shaded image.  One bounce, no roughness, no refraction direction, no packed-record variant (the voxel boxes need the ids).
 * gbuffer_dev holds the w*h records that svo_trace(cam, params, x0, y0, w, h) wrote (or the surface records of svo_trace_translucent),
 * voxels_dev what svo_hit_voxels wrote for them; both calls only read them.
 * A pixel is a MIRROR PIXEL iff its record has SVO_HIT_FLAG and no SVO_ERR_FLAG, `material` is 0 or the record's material, and its voxel
 * record has SVO_LOCATE_INSIDE.  Its mirror ray, in float, every operation separately rounded - both calls form it with the same code:
 *   1. sample point   (o, d) the pixel's camera ray as the march forms it; P = o + d * (t - eps).  svo_trace_reflections: eps is the
 *                     launch's (0 = 1/8192, or 1/4096 under SVO_SEMANTICS_GLSL, as in svo_trace_local_shadows); svo_shade_reflections:
 *                     p->eps (0 = 1/8192) - pass the launch's;
 *   2. face           lo = bmin, hi = bmin + size of the voxel record; the SVO_NORMAL_FACE rule exactly as svo_hit_ao step 2 states it:
 *                     an axis k and sgn = +1 or -1;
 *   3. origin         O = P with O[k] = (sgn > 0 ? hi[k] : lo[k]) + sgn * eps: on the face plane, pushed out by eps.  P itself lies on
 *                     or inside the closed box of its voxel, and a ray from there hits that voxel again at t = 0;
 *   4. direction      R = d with R[k] = sgn * fabsf(d[k]): the ray always leaves the face; R is not re-normalised.
 *
 * svo_trace_reflections: reflect_dev[k] is, byte for byte, what svo_trace_rays writes for (O, R) under params without counters_dev,
 * tile_cost_dev and tile_order_dev (eps, caps, semantics, kernel, see_through, normal_mode and shadow are honoured), and all zero for a
 * pixel that is not a mirror pixel (it gets a ray that misses the world).  All rays go through ONE ray-list launch
 * (svo_trace_last_ray_count then reports it: w*h rays); the list lives in the world's scratch, 24 bytes per pixel.  Asynchronous on
 * `stream`; calls of one world on different streams are ordered behind one another on the device.  Nothing is cached.
 * A NULL world, cam or params, a NULL buffer with w*h > 0, a rectangle that starts or extends backwards, material > 0xFFFF:
 * SVO_ERR_INVALID_ARG; then what svo_trace refuses in params and the world (see_through > 0xFFFF, SVO_ERR_NOT_UPLOADED, an unknown
 * semantics or kernel, SVO_KERNEL_STACK where it is unsupported); then w*h == 0: SVO_OK; w*h >= 2^31: SVO_ERR_UNSUPPORTED.  All settled
 * before any device work. */
int svo_trace_reflections(svo_world *, const svo_camera *cam, const svo_trace_params *params, uint32_t material,
                          int x0, int y0, int w, int h,
                          const svo_hit *gbuffer_dev, const svo_voxel *voxels_dev, svo_hit *reflect_dev, void *stream);

/* svo_shade_reflections: over an image that svo_shade, svo_shade_textured or svo_shade_translucent wrote for the same rectangle; after
 * svo_shade_ao, before svo_shade_boxes and svo_frame_rgba8 (svo_shade_sky writes other pixels: their order does not matter).
 * For a mirror pixel (above; reflect_dev is what svo_trace_reflections wrote for the same records), with k the face's axis:
 *   c = fabsf(d[k]), x = 1.0f - c;  F = f0 if fresnel == 0, else Schlick's f0 + (1.0f - f0) * (((x*x) * (x*x)) * x);
 *   C = if reflect_dev[k] has SVO_HIT_FLAG: the r, g, b of svo_shade's hit formula for that record with the pixel's eye replaced by O,
 *         its direction by R and t the record's - the point is O + R * (t - eps), the view vector -R; material table, shadow bits and
 *         gamma as in svo_shade; the depth is dropped;
 *       else if sky: svo_shade_sky's lookup with d := R;
 *       else background - also where the sky has no answer, !(ma > 0);
 *   F == 0: the pixel is not written.  Otherwise rgb = rgb * (1.0f - F) + C * F per channel; the depth float is never written.
 * A pixel that is not a mirror pixel is not written at all.
 * A NULL cam, p or mirror, a NULL buffer with w*h > 0, f0 outside [0, 1] or NaN, material > 0xFFFF, a background that is not finite,
 * a sky that svo_shade_sky would refuse, a rectangle that starts or extends backwards: SVO_ERR_INVALID_ARG, settled before any device
 * work.  w*h == 0 is SVO_OK.  Takes no world; asynchronous on `stream`. */
typedef struct svo_mirror {
    uint32_t material;              /* as svo_trace_reflections' */
    float    f0;                    /* reflectance at normal incidence, in [0, 1] */
    int32_t  fresnel;               /* 0: F = f0 everywhere; != 0: Schlick */
    float    background[3];         /* colour of a mirror ray that leaves the world when sky == NULL (or the sky has no answer) */
    const svo_sky *sky;             /* optional: svo_shade_sky's cube map, looked up along the MIRROR ray */
} svo_mirror;
int svo_shade_reflections(const svo_camera *cam, const svo_shade_params *p, const svo_mirror *mirror,
                          int x0, int y0, int w, int h,
                          const svo_hit *gbuffer_dev, const svo_voxel *voxels_dev, const svo_hit *reflect_dev,
                          float *rgba_dev, void *stream);

/* ---- light lists: up to 32 point lights, each with a reach ---------------------------------------------------
 * svo_shade has the reference's three lights, and svo_trace_local_shadows gives the two local ones a padded list of one ray per
 * pixel and light.  A world lit by torches and lamps has dozens of small lights, each reaching a few percent of the screen:
 * svo_trace_lights marches one occlusion ray per hit and light THAT CAN REACH IT, all of them in one compacted list, and
 * svo_shade_lights adds the lights to an image a svo_shade* call has written.  Not in the reference: an opt-in departure. */
#define SVO_MAX_LIGHTS 32
typedef struct svo_light {          /* 64 bytes */
    float position[3]; float reach;      /* reach > 0, finite: beyond it the light adds nothing and casts no ray */
    float ambient[3];  float constant;
    float diffuse[3];  float linear;
    float specular[3]; float quadratic;  /* attenuation 1 / (constant + linear d + quadratic d^2), as svo_shade_params.point */
} svo_light;

/* One word per pixel: bit j of visible_dev[k] is set iff light j reaches pixel k's hit unoccluded.  `lights` is a host array of
 * nlights lights (1..SVO_MAX_LIGHTS); gbuffer_dev holds the w*h records that svo_trace(cam, params, x0, y0, w, h) wrote (or the
 * surface records of svo_trace_translucent, or any records of the caller's) and is not written; visible_dev receives w*h words.
 * Every operation is in float and separately rounded; pixels k are row-major in the rectangle; eps is the launch's (0 = 1/8192,
 * 1/4096 under SVO_SEMANTICS_GLSL), as in svo_trace_local_shadows.  For pixel k with SVO_HIT_FLAG and without SVO_ERR_FLAG and
 * light j at L with reach R:
 *   P = o + d * (t - eps)   (o, d) the pixel's camera ray: the point the directional shadow ray starts from;
 *   v = L - P, q = v.x*v.x + v.y*v.y + v.z*v.z (left to right); q == 0 or not finite: no pair;
 *   in reach   q <= R2, R2 = R * R in float (an R2 that overflows to +inf is legal: everything is in reach);
 *   facing     s = n.x*v.x + n.y*v.y + n.z*v.z (left to right), n the record's normal as it stands; the test is !(s <= 0), so a
 *              NaN normal (the SVO_NORMAL_CUBE hits whose integer vector is zero) faces every light;
 *   (k, j) is a PAIR iff the hit is usable, in reach and facing.  Its ray is (P, v * (1 / sqrtf(q))); it is OCCLUDED iff that ray's
 *   record, marched as svo_trace_rays marches it with `params` and shadow = 0 (eps, caps, semantics, kernel and see_through are
 *   honoured), has SVO_HIT_FLAG, has no SVO_ERR_FLAG and its t < sqrtf(q) - svo_trace_local_shadows' rule word for word: terrain
 *   behind the light does not shadow it, a runaway ray is not occluded.
 * Order and capacity: the pairs are ranked light-major - all pairs of light 0 in ascending k, then light 1, and so on -, so the 64
 * rays of a wave converge on one light.  cap = max_rays > 0 ? max_rays : w*h.  Pair r occupies slot r of the list if r < cap; pairs
 * with r >= cap are DROPPED: not marched, and they count as not occluded (the library's rule for a ray it did not resolve).  Slots
 * from the number of pairs up to cap hold a ray that misses the world.  ONE svo_trace_rays launch of cap rays marches the list
 * (svo_trace_last_ray_count then reports cap).  No host synchronisation is made and the host never learns the number of pairs:
 * that is the point of the cap.
 *   visible_dev[k]  bit j set iff (k, j) is a pair and not occluded; every other bit, and the word of a pixel without a usable hit, is 0;
 *   count_dev       optional (NULL): two uint32 on the device, [0] the number of pairs, [1] min(pairs, cap) - a caller feeds [0]
 *                   into the next frame's max_rays, as it does with svo_tile_order's costs.
 * In this order, all before any device work: a NULL world, cam, params, lights, gbuffer_dev or visible_dev, nlights outside
 * 1..SVO_MAX_LIGHTS, max_rays < 0, a rectangle that starts or extends backwards, a position that is not finite, a reach that is not
 * > 0 or not finite: SVO_ERR_INVALID_ARG; then what svo_trace refuses in params and a world that is not resident
 * (SVO_ERR_NOT_UPLOADED); then w*h == 0: SVO_OK; nlights * w*h > 0x7FFFFFFF or cap > 0x7FFFFFFF: SVO_ERR_UNSUPPORTED.
 * Asynchronous on `stream`.  The list, its records and the ranks live in the world's scratch, 56 bytes per slot plus 8 bytes per
 * light and block of 256 pixels; calls of one world on different streams are ordered behind one another on the device. */
int svo_trace_lights(svo_world *, const svo_camera *cam, const svo_trace_params *params,
                     const svo_light *lights, int nlights, int64_t max_rays,
                     int x0, int y0, int w, int h, const svo_hit *gbuffer_dev,
                     uint32_t *visible_dev, uint32_t *count_dev, void *stream);

/* The lights of a list added to an image that a svo_shade* call has written for the same rectangle (as svo_shade_ao and
 * svo_shade_reflections work over the image): for every record with SVO_HIT_FLAG, rgb += sum over j of C_j.  The depth float, the
 * misses and everything beyond w*h pixels are not written.  visible_dev (svo_trace_lights' words) == NULL: every light is
 * unshadowed.  Albedo (the material table's), shininess, eps and gamma come from p exactly as svo_shade uses them; p's own three
 * lights are ignored.  With pt = eye + beta * (t - eps), lv = L - pt, d = |lv|, l = lv / d, and vdir, hv as in
 * computePointLight_BlinnPhong (shaders/World.Fragment.glsl:80-97):
 *   if !(d > 0) or !(d < reach): C_j = 0
 *   win = clamp(1 - (d / reach)^4, 0, 1)^2          the contribution falls to 0 at the reach, continuously
 *   att = win / (constant + linear d + quadratic d d)
 *   vis = bit j of visible_dev[k] ? 1 : 0
 *   C_j = ((ambient * diffuse_albedo + diffuse * max(n.l, 0) * diffuse_albedo * vis)
 *          + specular * pow(max(vdir.hv, 0), shininess) * specular_albedo * vis) * att
 * The window is what lets svo_trace_lights cull by reach without a seam: outside the reach nothing is added whatever the bit says
 * (such a pixel keeps its bits), and the boundary pixel's contribution is about 0 in both stages.  A NaN normal gives NaN colours, as
 * in svo_shade.  In the stage's arithmetic (compared with a tolerance, not bit for bit).
 * A NULL cam, p, lights, gbuffer_dev or rgba_dev, nlights outside 1..SVO_MAX_LIGHTS, a rectangle that starts or extends backwards:
 * SVO_ERR_INVALID_ARG; a rectangle too large for one launch: SVO_ERR_UNSUPPORTED; an empty one: SVO_OK.  All before HIP is touched.
 * Asynchronous on `stream`.  In a frame: svo_shade* -> svo_trace_lights -> svo_shade_lights -> svo_shade_ao, sky, boxes, RGBA8. */
int svo_shade_lights(const svo_camera *cam, const svo_shade_params *p, const svo_light *lights, int nlights,
                     int x0, int y0, int w, int h, const svo_hit *gbuffer_dev, const uint32_t *visible_dev,
                     float *rgba_dev, void *stream);

/* ---- voxel model instances: up to 32 placements of one model world in a frame ------------------------------
 * Everything above renders ONE static voxel world; moving anything means editing it.  An instance is a rigid placement (rotation,
 * position, uniform scale) of a second uploaded world, the MODEL - in practice a small one, a single chunk from a grid
 * (svo_chunk_from_grid + svo_world_create); it may be the scene's own handle.  One call renders up to 32 placements of one model; a
 * caller with several models calls once per model and feeds merged_dev back in as gbuffer_dev (merged_dev == gbuffer_dev is
 * allowed).  Not in the reference, whose only moving object is a rasterised mesh (src/Worm.cpp): an opt-in departure. */
#define SVO_MAX_INSTANCES 32
typedef struct svo_instance {       /* 64 bytes */
    float rot[9];                   /* R, row-major, model -> world; orthonormal is the caller's business, finite is checked */
    float pos[3];                   /* world position of the model's origin */
    float scale;                    /* > 0, finite: x_world = pos + scale * (R x_model) */
    uint32_t _pad[3];               /* 0 */
} svo_instance;

/* Stage 1, visibility.  gbuffer_dev holds the w*h records that svo_trace(scene, cam, params, x0, y0, w, h) wrote (or any records of
 * the caller's); it is only read, unless it is merged_dev.  merged_dev receives w*h records, owner_dev w*h words.  Every operation is
 * in float and separately rounded; pixels k are row-major in the rectangle; (o, d) is the pixel's camera ray as the march forms it;
 * inv = 1.0f / scale, rounded once on the host; bmin / bmax are the model world's box as floats (chunkcoordmin * chunksize, and that
 * plus dims * chunksize); a record is USABLE when it has SVO_HIT_FLAG and no SVO_ERR_FLAG.  For pixel k and instance j:
 *   1. into model space   u = o - pos;  om[i] = (R[0][i]*u.x + R[1][i]*u.y + R[2][i]*u.z) * inv;  dm[i] = R[0][i]*d.x + R[1][i]*d.y
 *                         + R[2][i]*d.z   (R transposed, summed left to right; dm is not re-normalised, so a distance along the model
 *                         ray is the world's times inv);
 *   2. box rule           tn = 0, tf = +inf; per axis a in x, y, z order: dm[a] == 0: the axis fails unless bmin[a] <= om[a] &&
 *                         om[a] <= bmax[a], and bounds nothing; otherwise r = 1.0f / dm[a], t0 = (bmin[a] - om[a]) * r,
 *                         t1 = (bmax[a] - om[a]) * r, swapped if t1 < t0, then if (t0 > tn) tn = t0; if (t1 < tf) tf = t1 (a NaN
 *                         compares false and bounds nothing).  The box is missed if an axis fails or tn > tf;
 *   3. pair               far = gbuffer[k] usable ? gbuffer[k].t * inv : +inf.  (k, j) is a PAIR iff the box is not missed and
 *                         tn < far.  Its ray is (om, dm) with far end `far`.
 * Order and capacity are svo_trace_lights': the pairs are ranked instance-major - all pairs of instance 0 in ascending k, then
 * instance 1, and so on; cap = max_rays > 0 ? max_rays : w*h; pair r occupies slot r of the list if r < cap, pairs with r >= cap are
 * DROPPED and count as "no hit"; slots from the number of pairs up to cap hold a ray that misses the model, with far end 0.  ONE
 * svo_trace_segments launch of cap rays marches the list on the MODEL world (svo_trace_last_ray_count of the model then reports cap),
 * with `params` and shadow = 0, without counters_dev, tile_cost_dev and tile_order_dev; eps, caps, semantics, kernel, normal_mode and
 * see_through are honoured, in model units.  No host synchronisation is made.
 *   4. resolve            pair (k, j) HITS iff it has a slot and its record M is usable (the launch has applied M.t < far); its world
 *                         distance is tw = M.t * scale.  Among the hitting pairs of pixel k the smallest tw wins, the lowest j among
 *                         equals.  With a winner merged[k] is: t = tw; normal[i] = R[i][0]*n.x + R[i][1]*n.y + R[i][2]*n.z with n
 *                         M's normal (a NaN stays NaN); material, chunk, node and cell from M; flags = SVO_HIT_FLAG |
 *                         (M.flags & SVO_FACE_NORMAL); and owner[k] = j + 1.  Otherwise merged[k] = gbuffer[k] byte for byte and
 *                         owner[k] = 0.
 *   count_dev             optional (NULL): two uint32 on the device, [0] the number of pairs, [1] min(pairs, cap) - [0] feeds the
 *                         next frame's max_rays.
 * THE IDS OF AN OWNED PIXEL BELONG TO THE MODEL WORLD: a per-hit stage that takes a world (svo_hit_voxels, svo_hit_ao,
 * svo_trace_reflections, svo_trace_lights, ...) is fed such pixels with `model` as its world, or not at all; svo_shade* take no world
 * and work on merged_dev as it stands.
 * In this order, all before any device work: a NULL scene, model, cam, params, inst, gbuffer_dev, merged_dev or owner_dev, ninst
 * outside 1..SVO_MAX_INSTANCES, max_rays < 0, a rectangle that starts or extends backwards, a rot or pos entry that is not finite, a
 * scale that is not > 0 or not finite, scene and model resident on different devices: SVO_ERR_INVALID_ARG; then what svo_trace
 * refuses in params, for the scene and then the model, and a world that is not resident (SVO_ERR_NOT_UPLOADED); then w*h == 0:
 * SVO_OK; then ninst * w*h > 0x7FFFFFFF or cap > 0x7FFFFFFF: SVO_ERR_UNSUPPORTED.
 * Asynchronous on `stream`.  The list, its records and the ranks live in the MODEL's scratch, 60 bytes per slot plus 4 per pixel and
 * 8 per instance and block of 256 pixels; calls that share a model are ordered behind one another on the device.
 * The list is marched in MODEL units from the eye's place in model space: a distance d in the world is d / scale there.  Keep scale near
 * 1 (author a small object as a small chunk): from t = 2048 model units on, t + eps no longer advances a float t and the march of such a
 * ray costs about sixty times more. */
int svo_trace_instances(svo_world *scene, svo_world *model, const svo_camera *cam, const svo_trace_params *params,
                        const svo_instance *inst, int ninst, int64_t max_rays,
                        int x0, int y0, int w, int h, const svo_hit *gbuffer_dev,
                        svo_hit *merged_dev, uint32_t *owner_dev, uint32_t *count_dev, void *stream);

/* Stage 2, shadows from the directional light, on what stage 1 wrote: instances shadow the terrain, the terrain shadows instances,
 * instances shadow each other and themselves.  S = normalize(-params->light_dir), the direction svo_trace's own shadow rays have;
 * b = bias > 0 ? bias : the launch's resolved eps (0 = 1/8192, 1/4096 under SVO_SEMANTICS_GLSL).
 *   1. a pixel is CONSIDERED iff merged[k] is usable and has no SVO_SHADOWED; its point is P = o + d * (t - b);
 *   2. model launch   (k, j) is a pair iff the ray (P, S), taken into instance j's space as in stage 1, does not miss the box
 *                     (far = +inf).  Ranking, cap, dropping, count_dev and scratch as in stage 1; ONE svo_trace_rays launch of cap
 *                     rays on the model with shadow = 0.  A pair is OCCLUDED iff it has a slot and its record is usable;
 *   3. scene launch   ONE svo_trace_rays launch of w*h rays on the scene with shadow = 0: a considered pixel with owner != 0 gets
 *                     (P, S), every other pixel the ray that misses the scene (svo_trace_reflections' padding); occluded iff the
 *                     record is usable.  (The scene's own pixels had their shadow rays from svo_trace.)
 *   4. fold           every considered pixel gets SVO_SHADOW_TRACED, and SVO_SHADOWED if anything occluded it.  No other byte of
 *                     merged_dev changes.
 * bias exists because P, re-derived in a rotated or scaled model space, can land a rounding error inside the voxel it left: at
 * bias = 0 (the march's eps) a rotated instance may show shadow acne on itself; a few eps (1/256) cures it.
 * Argument rules as for svo_trace_instances (the required buffers: merged_dev, owner_dev), and a bias that is negative or NaN is
 * SVO_ERR_INVALID_ARG.  Asynchronous on `stream`; the model list lives in the model's scratch, the scene list (56 bytes per pixel) in
 * the scene's, and calls that share a world are ordered behind one another on the device. */
int svo_trace_instance_shadows(svo_world *scene, svo_world *model, const svo_camera *cam, const svo_trace_params *params,
                               const svo_instance *inst, int ninst, int64_t max_rays, float bias,
                               int x0, int y0, int w, int h,
                               svo_hit *merged_dev, const uint32_t *owner_dev, uint32_t *count_dev, void *stream);

/* ---- the edit cursor and the light markers: cubes over the finished image ----------------------------------
 * One overlay record, 48 bytes, on the device.  The reference has four: the cursor cube (ImagCube: translucent grey, black edges) and one
 * solid marker cube at each light (src/Main.cpp:223-225). */
enum { SVO_BOX_SOLID = 0, SVO_BOX_CURSOR = 1, SVO_BOX_HIDDEN = 1u << 8 };
#define SVO_MAX_BOXES 64
typedef struct svo_box {
    float    bmin[3];
    float    size;        /* cube edge (ImaginaryCube's scale is a vec3 with three equal components) */
    float    color[3];
    float    alpha;
    uint32_t style;       /* SVO_BOX_SOLID / SVO_BOX_CURSOR in bits 0-7, | SVO_BOX_HIDDEN */
    uint32_t _pad[3];
} svo_box;

/* computeTarget (src/Main.cpp:314-319) + ImaginaryCube::position (src/ImaginaryCube.cpp:59-62) without a read-back: one tiny launch.
 * record_dev is the record a march wrote for the ray (origin, dir): svo_trace_rays with one ray, or the address of a pixel's record
 * together with that pixel's ray.  If the record has SVO_HIT_FLAG and no SVO_ERR_FLAG - every operation separately rounded:
 *   sigma = origin + dir * t   per component (src/Traverse.cpp:161; under SVO_SEMANTICS_CPU svo_hit.t is that t),
 *   box_dev->bmin = sigma - size * 0.5f, box_dev->size = size, SVO_BOX_HIDDEN is cleared.
 * Otherwise SVO_BOX_HIDDEN is set (imag.real == false) and bmin / size are left alone.  color, alpha and the low style bits are never
 * written: the caller sets them once.  A NULL pointer or !(size > 0): SVO_ERR_INVALID_ARG before any device work.  Asynchronous on
 * `stream`: issue it behind the march on the same stream, and svo_shade_boxes behind it. */
int svo_cursor_place(const float origin[3], const float dir[3], const svo_hit *record_dev,
                     float size, svo_box *box_dev, void *stream);

/* The boxes over the shaded image, depth-tested against the world (ImaginaryCube::draw, src/ImaginaryCube.cpp:64-87,
 * shaders/Imag.Fragment.glsl; Light::draw, src/Light.cpp:141-155, shaders/Light.Fragment.glsl): over an image that svo_shade* has written
 * for the same rectangle, whose fourth float is the depth buffer.  If the frame has a sky, call it AFTER svo_shade_sky: that call picks
 * its pixels by the record's flag, not by depth, and would paint over a box drawn before it (the reference draws the sky at depth 1
 * with GL_LEQUAL for the same effect).
 * near_plane / far_plane of 0 mean 0.125 / 8192, as in svo_shade_params: pass the shade call's.  Per pixel, (o, d) is its ray exactly
 * as the march and svo_shade_sky form it, D its depth float.  The boxes go in list order (GL draws in call order); a box with
 * SVO_BOX_HIDDEN or !(size > 0) is skipped.  Every operation is in float and separately rounded, every division IEEE:
 *   slabs     bmax = bmin + size.  Per axis a with d.a != 0: t0 = (bmin.a - o.a) / d.a, t1 = (bmax.a - o.a) / d.a; the near value is the
 *             smaller and belongs to the min face if t0 <= t1 (to the max face otherwise), the far value is the other, on the other
 *             face.  With d.a == 0 the box is missed if o.a < bmin.a || o.a > bmax.a, and the axis bounds nothing otherwise.
 *             tnear = the largest near value, tfar = the smallest far value, in both the first axis in x, y, z order winning ties.
 *             The box is missed unless tnear <= tfar.
 *   fragments up to two: the entry face at tnear if tnear > 0, the exit face at tfar if tfar > 0 (culling is off,
 *             src/ImaginaryCube.cpp:71), processed in the face order of the reference's index buffer (CUBE_INDICES,
 *             src/Parallax.cpp:25-38): -Z, -X, +Z, +X, -Y, +Y.
 *   depth     a fragment at t has f = (1 / t - 1 / near) / (1 / far - 1 / near): gl_FragDepth's form in the world shader with the
 *             distance along the unit ray.  It passes iff f < D (GL_LESS; a NaN fails), and a passing fragment sets D = f (depth
 *             writes are on).  So an exit face drawn before its entry face shows through it, one drawn after its entry face is
 *             discarded - as in the reference.  There is no clipping against the planes.
 *   colour    SVO_BOX_SOLID (and every other value of the low style byte): {color, alpha}.  SVO_BOX_CURSOR (Imag.Fragment.glsl): with
 *             p = o + d * t the two in-face coordinates are c = (p - bmin) / size (the face axis' own coordinate is exactly 0 or 1 and
 *             always counts as an edge): {0, 0, 0, 1} if either is <= 1/64 or >= 1 - 1/64, {color, alpha} otherwise (the reference: 0.8
 *             and 0.2).
 *   blend     rgb = src * a + dst * (1 - a) per channel: GL_SRC_ALPHA, GL_ONE_MINUS_SRC_ALPHA, the state src/Text.cpp:135 leaves for
 *             every frame after the first; the reference's frame one has the GL default (GL_ONE, GL_ZERO) instead.
 *   stores    a pixel no fragment passed on is not written at all, neither is anything outside the w*h pixels; a pixel a fragment
 *             passed on gets all four floats (r, g, b, D) in one store.
 * Two departures from the reference: the direction is the pinhole ray's, not a rasteriser's interpolant (as svo_shade_sky); and the
 * rasterised cubes get GL's projective depth while the world shader writes the distance form - here both are in the world's form, so that
 * a box and the terrain are compared in one measure.
 * A NULL cam / rgba_dev, a NULL boxes_dev with nboxes > 0, nboxes < 0 or > SVO_MAX_BOXES, a negative rectangle, a camera without an
 * image size, a negative (or NaN) plane: SVO_ERR_INVALID_ARG, settled before any device work.  nboxes == 0 or w*h == 0: SVO_OK, nothing
 * written.  rgba_dev is 16-byte aligned, as for svo_shade.  Takes no world; asynchronous on `stream`. */
int svo_shade_boxes(const svo_camera *cam, const svo_box *boxes_dev, int nboxes, float near_plane, float far_plane,
                    int x0, int y0, int w, int h, float *rgba_dev, void *stream);

/* Number of rays the last launch on this world actually marched (primary + shadow, all frames of a
 * svo_trace_frames launch; a multi-frame call served by a kernel other than SVO_KERNEL_STACK is one launch per
 * frame and reports its last frame); synchronises `stream` internally — call it outside timed regions. */
int svo_trace_last_ray_count(svo_world *, void *stream, uint64_t *rays);

/* Light clearance: shadow rays of the directional light stop at the first empty cell with a clear way to the light.
 * A shadow ray adds one bit to its record, SVO_SHADOWED, and a lit one marches on through ever larger empty cells and out of the world
 * to report nothing.  Whether the way from an EMPTY node to the light is free depends only on the world and the light's direction, so
 * it is decided once, for every EMPTY node, by a sweep on the device (csrc/light_clearance.hip.h; DESIGN.md 6t has the rule and its
 * proof) and kept as one bit of the stack kernel's wide tree; a shadow ray of SVO_KERNEL_STACK that locates such a node ends there.
 * The records are the same bit for bit, svo_trace_last_ray_count too; only the steps taken differ.
 *   svo_world_prepare_light   decides the bits for light_dir (as svo_trace_params.light_dir: (0,0,0) or NULL = the default light).
 *                             Asynchronous on `stream`, ordered on the device behind every launch of the world issued before; launches
 *                             that use the bits wait for it.  One light at a time: a second call replaces the first.  Costs a sweep over
 *                             the wide pool per call (README quotes it beside the world build).
 *   automatic                 the first svo_trace / svo_trace_frames / svo_trace_rows(_frames) launch with shadow rays on a world that has
 *                             not changed since its upload (or its generation on the device) prepares the bits for its own light_dir.
 *   dropped by                every change to the pools (svo_world_update / _edit_* / _shift / _compact / _coarsen / _chunk_from_grid /
 *                             _chunk_from_mesh / _upload).  After a change only svo_world_prepare_light brings them back: a caller who edits every frame
 *                             never pays a sweep per frame.
 *   used by                   camera launches of SVO_SEMANTICS_CPU with shadow rays whose light_dir equals the prepared one bit for bit and
 *                             whose eps is a power of two of at least twice the float spacing at the world's largest coordinate.  Ray lists,
 *                             segments, local lights, reflections, see_through, tile_cost_dev, SVO_SEMANTICS_GLSL, the literal kernel and
 *                             SVO_SHADOW_NO_CLEARANCE march every step as before.  A direction with a non-zero component below 1/64 in
 *                             magnitude is accepted and never used (a ray that grazes a chunk face defeats the proof).
 *   svo_world_prepared_light  the prepared shadow direction, normalize(-light_dir) ((0,0,0) if none is), and the number of EMPTY reference
 *                             nodes found clear (0 if the direction is never used); waits for `stream` and for the pass, whichever stream
 *                             it was issued on.
 *   svo_world_prepared_bricks the number of bricks that carry the clear flag (0 if the flags are never used).  Behind the sweep the pass
 *                             decides one flag per brick, bit 15 of its 16-bit material word: every EMPTY cell of the brick has a clear way
 *                             to the light, bricks seen cell by cell.  A primary hit in a cell of such a brick whose shadow
 *                             origin lies in an empty cell of the same brick is lit without a step of its shadow ray; the record and
 *                             svo_trace_last_ray_count are what they were.  Same lifecycle and the same launches as the bits; in addition
 *                             the world must have no negative coordinate and no voxel below the float spacing at its largest coordinate,
 *                             and a brick of several materials, or of one material of 0x8000 and above, carries no flag.
 *                             SVO_SHADOW_NO_BRICK_CLEARANCE switches the flags off alone, SVO_SHADOW_NO_CLEARANCE both.
 *   dark at birth             needs none of the above: a primary hit in a brick cell whose shadow origin the hit block locates
 *                             in an OCCUPIED cell of the same brick is shadowed - the reference's shadow march finds that cell in its first
 *                             chunk step, tree step and brick cell - and the record is written once, with SVO_SHADOWED.  No prepared light,
 *                             no bit of the pools: it holds after edits and for every finite light_dir.  The same launches as the bits
 *                             (camera launches of SVO_SEMANTICS_CPU on the stack kernel, no see_through, no tile_cost_dev), on a world
 *                             without a negative coordinate.  By default it is also left off where eps is below twice the float spacing
 *                             at the world's largest coordinate: that is no premise of the rule, only a default that
 *                             keeps such launches step for step what they were.  SVO_SHADOW_NO_DARK_BIRTH switches it off alone,
 *                             SVO_SHADOW_NO_BRICK_CLEARANCE with the flags (no shadow ray is then settled at its primary hit),
 *                             SVO_SHADOW_NO_CLEARANCE with everything.
 * The pass keeps 16 bytes of scratch per wide node (41 MB on the 4x1x4 depth-12 world; svo_world_info does not count it) until the next change
 * to the pools, so that a second light costs no allocation.  A launch prepares a world on its own only while wide entries x chunks <= 1e10
 * (four times that world: a few seconds for the bits; the brick flags take seventeen times as long, 15 s on that world and 0.8 s at depth 10);
 * larger worlds are prepared by the call alone.
 * SVO_ERR_INVALID_ARG (NULL world / outputs), SVO_ERR_NOT_UPLOADED, SVO_ERR_OUT_OF_MEMORY (the scratch). */
int svo_world_prepare_light(svo_world *, const float light_dir[3], void *stream);
int svo_world_prepared_light(svo_world *, void *stream, float shadow_dir[3], uint64_t *clear_nodes);
int svo_world_prepared_bricks(svo_world *, void *stream, uint64_t *flagged);

/* ---- small device helpers so that C/C++ callers need no HIP headers --------------------- */
int   svo_device_count(void);
void *svo_device_alloc(size_t bytes);
void  svo_device_free(void *p_dev);
/* The library keeps the large device buffers of a world that is destroyed or re-packed (tree, brick, mask, material and wide
 * pools: at most 8 buffers of 1 MiB and more per process) and hands them to the next world whose pools they fit - a caller that
 * replaces its world pays no hipFree / hipMalloc of multi-GB buffers.  This returns them to the driver (also done by itself when
 * an allocation fails). */
void  svo_device_cache_trim(void);
int   svo_memcpy_h2d(void *dst_dev, const void *src, size_t bytes);
int   svo_memcpy_d2h(void *dst, const void *src_dev, size_t bytes);
int   svo_stream_synchronize(void *stream);

const char *svo_last_error(void);   /* thread-local message of the last failing call */
int         svo_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SVO_H */
