// svo_world.hpp — C++ host-side mirror of the reference's World / Traverse surface, over the C ABI.
//
// The reference is a C++ program whose hot path sits behind two in-process surfaces
// (src/World.h:44-68, src/Traverse.h:27-30).  This header gives a maintainer the same names, argument
// meaning and hit/miss behaviour, implemented by libsvo_amd.so (include/svo.h) — header-only, no HIP
// headers needed, plain float[3] instead of glm::vec3 so it compiles without GLM:
//
//   svo::World::init(w,h,d,s)        <- World::init            src/World.cpp:19-43
//   svo::World::load_gpu()           <- World::load_gpu        src/World.cpp:57-94
//   svo::World::draw(camera, ...)    <- World::draw (+ draw_shadowmap as the fused shadow ray)  src/World.cpp:162-266
//   svo::World::local_shadows(...)   <- (none: per-light shadows of the point light and the spotlight, svo_trace_local_shadows)
//   svo::World::lights / shade_lights  <- (none: the reference has three lights) up to 32 point lights with a reach, svo_trace_lights, svo_shade_lights
//   svo::World::instances / instance_shadows  <- (none: the reference's one moving object is a rasterised mesh, src/Worm.cpp) up to 32 placements
//                                       of a model world in the frame and their shadows, svo_trace_instances, svo_trace_instance_shadows
//   svo::World::shadowmap_fit / shadowmap_render / shadowmap_apply  <- the OrthoCamera, World::draw_shadowmap and computeShadow (svo_shadowmap_*):
//                                       the directional light rendered once, looked up per frame   src/World.cpp:162-203, shaders/World.Fragment.glsl:140-155
//   svo::World::modify(i, ...)       <- World::modify          src/World.cpp:268-274
//   svo::World::index / index_float  <- src/World.cpp:288-293,323-332
//   svo::World::locate(points, ...)  <- traverse over a point list (svo_world_locate)   src/Traverse.cpp:34-48
//   svo::World::chunk_from_mesh  <- (none) a chunk from triangle meshes without the dense grid, to depth 16 (svo_world_chunk_from_mesh),
//   svo::World::chunk_fill_enclosed / svo::chunk_fill_enclosed  <- (none) the voxels a chunk encloses filled on its tree, without a dense grid, to
//                                       depth 16 (svo_world_chunk_fill_enclosed on the device, svo_chunk_fill_enclosed on host pools)
//   svo::World::chunk_combine / svo::chunk_combine  <- (none) two chunks of one depth combined cell by cell on their trees (union, under / over,
//                                       subtraction, intersection), to depth 16 (svo_world_chunk_combine on the device, svo_chunk_combine on host pools)
//   svo::World::chunk_stamp / svo::chunk_stamp  <- (none) a chunk placed into another at a cell offset, in one of the 48 orientations of the cube, through a
//                                       SVO_COMBINE_* rule, to depth 16 (svo_world_chunk_stamp on the device, svo_chunk_stamp on host pools)
//   svo::World::chunk_extract / svo::chunk_extract  <- (none) the stamp's inverse: a cube of cells copied out of a chunk at a cell offset, in one of the 48
//                                       orientations of the cube, into a chunk of its own, to depth 16 (svo_world_chunk_extract on the device, svo_chunk_extract on host pools)
//   svo::World::chunk_from_grid / chunk_to_grid  <- grow() over a dense voxel grid instead of the height pyramid (svo_world_chunk_from_grid),
//                                       and the chunk's voxels back as a grid (svo_world_chunk_to_grid)   src/Octree.cpp:74-176
//   svo::grid_add_mesh / grid_fill_enclosed, svo::device_grid_add_mesh / device_grid_fill_enclosed  <- (none: the reference rasterises its
//                                       one mesh with GL) a triangle mesh voxelised into such a grid and its shell filled, on the host or in device memory
//   svo::World::hit_voxels(...)      <- hit.bmin / hit.size of fragment main (svo_hit_voxels)   shaders/World.Fragment.glsl:168-172
//   svo::World::hit_uv / shade_textured  <- leafUV, texture(Diffuse / Specular, uv) (svo_hit_uv, svo_shade_textured)   shaders/World.Fragment.glsl:5-15,178-182
//   svo::World::hit_ao / shade_ao    <- (none: the reference has no ambient occlusion) svo_hit_ao, svo_shade_ao
//   svo::World::trace_reflections / shade_reflections  <- (none: the reference has no reflections) svo_trace_reflections, svo_shade_reflections
//   svo::World::shade_sky / frame_rgba8  <- Skybox::draw and the RGBA8 colour attachment (svo_shade_sky, svo_frame_rgba8)   src/Skybox.cpp, src/GBuffer.cpp
//   svo::World::cursor_place / shade_boxes / edit_cube  <- computeTarget, ImaginaryCube::draw, modify() (svo_cursor_place, svo_shade_boxes,
//                                       svo_world_edit_cube)   src/Main.cpp:314-368, src/ImaginaryCube.cpp:59-87
//   svo::World::edit_ball / edit_ball_all  <- (none: the reference edits cubes only) svo_world_edit_ball, svo_world_edit_ball_all
//   svo::World::deinit()             <- World::deinit          src/World.cpp:129-151
//   svo::chunkmarch(alpha,beta,world,&sigma) <- chunkmarch     src/Traverse.cpp:127-171
//
// Errors: the reference asserts / die()s (src/Util.cpp:72-78); here every failure throws svo::Error
// carrying the svo_status and svo_last_error().  There is no CPU fallback.
#pragma once
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/svo.h"

namespace svo {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &where) : std::runtime_error(where + ": " + svo_last_error()), code(c) {}
};
inline void check(int rc, const char *where) { if (rc < 0) throw Error(rc, where); }

struct vec3 { float x, y, z; };
struct ivec3 { int x, y, z; };

// RAII HBM buffer of G-buffer records.
class GBuffer {
public:
    GBuffer() = default;
    GBuffer(int w, int h) { resize(w, h); }
    ~GBuffer() { svo_device_free(dev_); }
    GBuffer(const GBuffer &) = delete;
    GBuffer &operator=(const GBuffer &) = delete;
    void resize(int w, int h)
    {
        svo_device_free(dev_);
        width = w; height = h;
        dev_ = static_cast<svo_hit *>(svo_device_alloc(sizeof(svo_hit) * (size_t)w * h));
        if (!dev_) throw Error(SVO_ERR_OUT_OF_MEMORY, "GBuffer::resize");
    }
    svo_hit *device() const { return dev_; }
    std::vector<svo_hit> download() const
    {
        std::vector<svo_hit> host((size_t)width * height);
        check(svo_memcpy_d2h(host.data(), dev_, host.size() * sizeof(svo_hit)), "GBuffer::download");
        return host;
    }
    int width = 0, height = 0;
private:
    svo_hit *dev_ = nullptr;
};

// The directional light's view and its depth image in HBM (svo_shadowmap): World::shadowmap_fit places it, resize() sizes the image.
class ShadowMap : public svo_shadowmap {
public:
    ShadowMap() { std::memset(static_cast<svo_shadowmap *>(this), 0, sizeof(svo_shadowmap)); }
    ~ShadowMap() { svo_device_free(depth_dev); }
    ShadowMap(const ShadowMap &) = delete;
    ShadowMap &operator=(const ShadowMap &) = delete;
    void resize(int w, int h)
    {
        svo_device_free(depth_dev);
        width = w; height = h;
        depth_dev = static_cast<float *>(svo_device_alloc(sizeof(float) * (size_t)w * h));
        if (!depth_dev) throw Error(SVO_ERR_OUT_OF_MEMORY, "ShadowMap::resize");
    }
    std::vector<float> download() const
    {
        std::vector<float> host((size_t)width * height);
        check(svo_memcpy_d2h(host.data(), depth_dev, host.size() * sizeof(float)), "ShadowMap::download");
        return host;
    }
    float texel() const { return 2.0f * std::fmax(half_width / (float)width, half_height / (float)height); }    // world units: the scale of a good bias
};

struct Camera : svo_camera {
    // Camera::init-style construction (src/Camera.cpp): position, unit forward, up hint, vertical fov.
    Camera(vec3 eye_, vec3 fwd, vec3 up_hint, float vfov_deg, int w, int h)
    {
        auto norm = [](double v[3]) { double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); v[0] /= l; v[1] /= l; v[2] /= l; };
        double f[3] = { fwd.x, fwd.y, fwd.z }, u[3] = { up_hint.x, up_hint.y, up_hint.z };
        norm(f);
        double r[3] = { f[1] * u[2] - f[2] * u[1], f[2] * u[0] - f[0] * u[2], f[0] * u[1] - f[1] * u[0] };
        norm(r);
        double up2[3] = { r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0] };
        eye[0] = eye_.x; eye[1] = eye_.y; eye[2] = eye_.z;
        for (int i = 0; i < 3; ++i) { forward[i] = (float)f[i]; right[i] = (float)r[i]; up[i] = (float)up2[i]; }
        tan_half_y = (float)std::tan(vfov_deg * 3.14159265358979323846 / 360.0);
        tan_half_x = tan_half_y * (float)w / (float)h;
        width = w; height = h;
    }
};

class World {
public:
    World() = default;
    ~World() { deinit(); }
    World(const World &) = delete;
    World &operator=(const World &) = delete;

    // World::init(w, h, d, s) with the reference's terrain constants as defaults (src/World.cpp:296-321).
    void init(int w, int h, int d, int s, uint32_t tree_max_depth = 8, const int chunkcoordmin[3] = nullptr,
              const svo_terrain_params *terrain = nullptr)
    {
        deinit();
        svo_terrain_params tp;
        if (terrain) tp = *terrain;
        else {
            std::memset(&tp, 0, sizeof tp);
            tp.depth = tree_max_depth; tp.pyramid_resolution = 0; tp.amplitude = 64.0f; tp.yshift = 16.0f;
            tp.water = 1; tp.water_level = 6.0f; tp.water_material = 6;
        }
        check(svo_world_generate(w, h, d, s, chunkcoordmin, &tp, &world_), "World::init");
        width = w; height = h; depth = d; chunksize = s;
        plane = w * d; volume = plane * h;
    }
    // Adopt chunks the caller built itself (Ocroot arrays).
    void init(const std::vector<svo_chunk_desc> &chunks, int w, int h, int d, int s, const int chunkcoordmin[3] = nullptr)
    {
        deinit();
        check(svo_world_create(chunks.data(), (int)chunks.size(), w, h, d, s, chunkcoordmin, &world_), "World::init(chunks)");
        width = w; height = h; depth = d; chunksize = s;
        plane = w * d; volume = plane * h;
    }
    void deinit() { svo_world_destroy(world_); world_ = nullptr; }

    void load_gpu(int device = 0) { check(svo_world_upload(world_, device), "World::load_gpu"); }

    // Which of the reference's two marches draw() / draw_frames() follow: the CPU code's (src/Traverse.cpp; what computeTarget and the
    // edits use - the default) or the fragment shader's (shaders/Chunkmarch.glsl; what World::draw renders with).  SURVEY.md App. B.
    int semantics = SVO_SEMANTICS_CPU;

    // World::draw: march every pixel of the camera image into `out` (asynchronous on `stream`).
    // shadow = true also casts the shadow ray of draw_shadowmap's light direction from every hit.
    void draw(const Camera &cam, GBuffer &out, bool shadow = false, const float light_dir[3] = nullptr, void *stream = nullptr)
    {
        if (out.width != cam.width || out.height != cam.height) out.resize(cam.width, cam.height);
        svo_trace_params p;
        std::memset(&p, 0, sizeof p);
        p.semantics = semantics;
        p.shadow = shadow ? 1 : 0;
        if (light_dir) std::memcpy(p.light_dir, light_dir, sizeof p.light_dir);
        check(svo_trace(world_, &cam, &p, 0, 0, cam.width, cam.height, out.device(), stream), "World::draw");
    }

    // Several views in one launch (svo_trace_frames): `out` receives cams.size() rasters of cam size one after the
    // other (a GBuffer of height cams.size() * cam.height holds them).  All cameras share one image size.
    void draw_frames(const std::vector<Camera> &cams, GBuffer &out, bool shadow = false, const float light_dir[3] = nullptr, void *stream = nullptr)
    {
        if (cams.empty()) return;
        const int w = cams[0].width, h = cams[0].height;
        if (out.width != w || out.height != h * (int)cams.size()) out.resize(w, h * (int)cams.size());
        svo_trace_params p;
        std::memset(&p, 0, sizeof p);
        p.semantics = semantics;
        p.shadow = shadow ? 1 : 0;
        if (light_dir) std::memcpy(p.light_dir, light_dir, sizeof p.light_dir);
        std::vector<svo_camera> plain(cams.begin(), cams.end());
        check(svo_trace_frames(world_, plain.data(), (int)plain.size(), &p, 0, 0, w, h, out.device(), stream), "World::draw_frames");
    }

    // A fixed sun: decide once, for every empty node, whether its way to the light is clear (svo_world_prepare_light); the shadow rays of
    // draw() / draw_frames() with this light_dir then end at the first such node they locate - the same records in fewer steps.  A world
    // that has not changed since its upload is prepared by its first draw(shadow = true) on its own; after modify() or any other edit only
    // this call brings the bits back.  Asynchronous on `stream`.
    void prepare_light(const float light_dir[3] = nullptr, void *stream = nullptr) { check(svo_world_prepare_light(world_, light_dir, stream), "World::prepare_light"); }
    // ... and, with it, for every brick whether all its empty cells are (svo_world_prepared_bricks counts them): a hit whose shadow ray would
    // start in an empty cell of such a brick is lit without a step.  Waits for `stream` and for the pass.
    uint64_t prepared_bricks(void *stream = nullptr) { uint64_t n = 0; check(svo_world_prepared_bricks(world_, stream, &n), "World::prepared_bricks"); return n; }

    // Shadows from the point light and the spotlight on a G-buffer that draw() filled with the same camera, shadow flag and light
    // direction (svo_trace_local_shadows): one flag per light, a null position leaves that light with the directional light's term.
    // Not in the reference, whose three lights share one shadow term (shaders/World.Fragment.glsl:186-190).
    void local_shadows(const Camera &cam, GBuffer &gbuffer, const float point_position[3], const float spot_position[3],
                       bool shadow = false, const float light_dir[3] = nullptr, void *stream = nullptr)
    {
        svo_trace_params p;
        std::memset(&p, 0, sizeof p);
        p.semantics = semantics;
        p.shadow = shadow ? 1 : 0;
        if (light_dir) std::memcpy(p.light_dir, light_dir, sizeof p.light_dir);
        check(svo_trace_local_shadows(world_, &cam, &p, point_position, spot_position, 0, 0, cam.width, cam.height, gbuffer.device(), stream),
              "World::local_shadows");
    }

    // A list of up to SVO_MAX_LIGHTS point lights with a reach each (not in the reference, which has three lights).  lights() marches one
    // occlusion ray per hit of the G-buffer draw() filled and light that can reach it, all in one compacted list of max_rays slots (0 =
    // one per pixel; pairs beyond it count as lit), and writes one word per pixel: bit j set where light j reaches the hit unoccluded
    // (svo_trace_lights; count_dev, optional: the number of pairs, for the next frame's max_rays).  shade_lights adds the lights, windowed
    // to their reach, to the image a shade call wrote (svo_shade_lights: behind svo_shade*, before shade_ao; visible_dev null = unshadowed).
    void lights(const Camera &cam, const GBuffer &gbuffer, const svo_light *list, int nlights, uint32_t *visible_dev, int64_t max_rays = 0,
                uint32_t *count_dev = nullptr, uint32_t see_through = 0, void *stream = nullptr)
    {
        svo_trace_params p;
        std::memset(&p, 0, sizeof p);
        p.semantics = semantics;
        p.see_through = see_through;
        check(svo_trace_lights(world_, &cam, &p, list, nlights, max_rays, 0, 0, cam.width, cam.height, gbuffer.device(), visible_dev, count_dev, stream),
              "World::lights");
    }
    void shade_lights(const svo_camera &cam, const svo_shade_params &p, const svo_light *list, int nlights, int x0, int y0, int w, int h,
                      const svo_hit *gbuffer_dev, const uint32_t *visible_dev, float *rgba_dev, void *stream = nullptr) const
    {
        check(svo_shade_lights(&cam, &p, list, nlights, x0, y0, w, h, gbuffer_dev, visible_dev, rgba_dev, stream), "World::shade_lights");
    }

    // Up to SVO_MAX_INSTANCES placements (rotation, position, uniform scale) of `model`, another resident world - in practice one chunk
    // from a grid -, in front of the G-buffer draw() filled (not in the reference, whose worm is a rasterised mesh).  instances() marches
    // the pixels' rays in each placement's own space, bounded by what the frame holds, and writes the merged frame (merged_dev may be the
    // G-buffer itself) and per pixel 0 or 1 + the instance that owns it (svo_trace_instances); the chunk / node / cell of an owned pixel
    // belong to `model`.  instance_shadows() then gives every record not yet shadowed its SVO_SHADOW_TRACED / SVO_SHADOWED from the
    // instances and, for owned pixels, from this world (svo_trace_instance_shadows; bias 0 = the march's eps, a rotated instance wants 1/256).
    // max_rays: the slots of the compacted ray list (0 = one per pixel; pairs beyond it count as no hit); count_dev, optional: the pairs.
    void instances(World &model, const Camera &cam, const svo_instance *list, int ninst, const svo_hit *gbuffer_dev, svo_hit *merged_dev, uint32_t *owner_dev,
                   int64_t max_rays = 0, uint32_t *count_dev = nullptr, bool shadow = false, const float light_dir[3] = nullptr, void *stream = nullptr)
    {
        const svo_trace_params p = instance_params(shadow, light_dir);
        check(svo_trace_instances(world_, model.world_, &cam, &p, list, ninst, max_rays, 0, 0, cam.width, cam.height, gbuffer_dev, merged_dev, owner_dev, count_dev,
                                  stream), "World::instances");
    }
    void instance_shadows(World &model, const Camera &cam, const svo_instance *list, int ninst, svo_hit *merged_dev, const uint32_t *owner_dev,
                          int64_t max_rays = 0, float bias = 0.0f, uint32_t *count_dev = nullptr, const float light_dir[3] = nullptr, void *stream = nullptr)
    {
        const svo_trace_params p = instance_params(true, light_dir);
        check(svo_trace_instance_shadows(world_, model.world_, &cam, &p, list, ninst, max_rays, bias, 0, 0, cam.width, cam.height, merged_dev, owner_dev, count_dev,
                                         stream), "World::instance_shadows");
    }

    // The shadow map of a fixed sun (svo_shadowmap_fit / _render / _apply; the reference's World::draw_shadowmap and computeShadow,
    // src/World.cpp:162-203, shaders/World.Fragment.glsl:140-155): fit a width x height map around the world along `direction`, render it
    // once - and again after every edit, a rendered map is stale behind one -, then per frame draw(cam, out, false) and shadowmap_apply:
    // one lookup per hit in the place of one shadow ray.  bias in world units along the light, one to two ShadowMap::texel() is a good start.
    void shadowmap_fit(const float direction[3], int width, int height, ShadowMap &map) const
    {
        if (map.width != width || map.height != height || !map.depth_dev) map.resize(width, height);
        check(svo_shadowmap_fit(world_, direction, width, height, &map), "World::shadowmap_fit");
    }
    void shadowmap_render(const ShadowMap &map, uint32_t see_through = 0, void *stream = nullptr)
    {
        svo_trace_params p;
        std::memset(&p, 0, sizeof p);
        p.semantics = semantics;
        p.see_through = see_through;
        check(svo_shadowmap_render(world_, &map, &p, stream), "World::shadowmap_render");
    }
    void shadowmap_apply(const Camera &cam, GBuffer &gbuffer, const ShadowMap &map, float bias, void *stream = nullptr) const
    {
        check(svo_shadowmap_apply(&cam, &map, semantics == SVO_SEMANTICS_GLSL ? 1.0f / 4096.0f : 0.0f, bias, 0, 0, cam.width, cam.height, gbuffer.device(), stream),
              "World::shadowmap_apply");
    }

    // Rays with a far end (svo_trace_segments): n rays (origins / dirs [n][3], tmax [n], all on the device) into out_dev; a hit counts only
    // if its t < tmax and the march ends there.  Line of sight, picking with a reach, short occlusion rays.  Not in the reference.
    void segments(const float *origins_dev, const float *dirs_dev, const float *tmax_dev, int64_t n, svo_hit *out_dev,
                  bool shadow = false, const float light_dir[3] = nullptr, void *stream = nullptr)
    {
        svo_trace_params p;
        std::memset(&p, 0, sizeof p);
        p.semantics = semantics;
        p.shadow = shadow ? 1 : 0;
        if (light_dir) std::memcpy(p.light_dir, light_dir, sizeof p.light_dir);
        check(svo_trace_segments(world_, origins_dev, dirs_dev, tmax_dev, n, &p, out_dev, stream), "World::segments");
    }

    // traverse(p, root) over a point list (svo_world_locate; src/Traverse.cpp:34-48): the node, the voxel box and the material under each
    // of n points ([n][3] float on the device) into out_dev.  see_through: a material reported as empty (0 = off).
    void locate(const float *points_dev, int64_t n, svo_voxel *out_dev, uint32_t see_through = 0, void *stream = nullptr)
    {
        svo_trace_params p;
        std::memset(&p, 0, sizeof p);
        p.semantics = semantics;
        p.see_through = see_through;
        check(svo_world_locate(world_, points_dev, n, &p, out_dev, stream), "World::locate");
    }

    // Chunk i replaced by the tree of a dense grid in device memory ((2^depth)^3 uint16 materials, x fastest, 0 = empty; svo.h states the
    // rule), and the chunk's voxels back as such a grid of any depth in [2, 10] (asynchronous on `stream`).
    int chunk_from_grid(int i, const uint16_t *grid_dev, uint32_t depth)
    {
        const int rc = svo_world_chunk_from_grid(world_, i, grid_dev, depth);
        check(rc, "World::chunk_from_grid");
        return rc;                                          // SVO_OK, or SVO_OK_LITERAL_ONLY
    }
    void chunk_to_grid(int i, uint32_t depth, uint16_t *grid_dev, void *stream = nullptr)
    {
        check(svo_world_chunk_to_grid(world_, i, depth, grid_dev, stream), "World::chunk_to_grid");
    }
    // Chunk i replaced by the tree of the shell of nmeshes triangle meshes (their arrays in device memory), depth in [2, 16], built
    // without the dense grid (svo_world_chunk_from_mesh; svo.h states the rule).  The shell only: an edit that cuts it open finds it hollow.
    int chunk_from_mesh(int i, const svo_mesh *meshes, int nmeshes, uint32_t depth)
    {
        const int rc = svo_world_chunk_from_mesh(world_, i, meshes, nmeshes, depth);
        check(rc, "World::chunk_from_mesh");
        return rc;                                          // SVO_OK, or SVO_OK_LITERAL_ONLY
    }
    // Chunk i replaced by its filled form: every empty voxel that no path of empty voxels connects to the chunk's own six faces becomes
    // `material`, on the tree, chunk depth in [2, 16] (svo_world_chunk_fill_enclosed; svo.h states the rule).  What makes the shell of
    // chunk_from_mesh solid.  *filled_out (may be null) receives how many voxels were filled.
    int chunk_fill_enclosed(int i, uint16_t material, uint64_t *filled_out = nullptr)
    {
        const int rc = svo_world_chunk_fill_enclosed(world_, i, material, filled_out);
        check(rc, "World::chunk_fill_enclosed");
        return rc;                                          // SVO_OK, or SVO_OK_LITERAL_ONLY
    }
    // Chunk i replaced by its cell-wise combination (SVO_COMBINE_*) with chunk src_chunk of `src` - an uploaded world on the same device,
    // which may be this one -, on the two trees, one chunk depth in [2, 16] (svo_world_chunk_combine; svo.h states the rule).  What puts
    // a voxelised mesh into a terrain chunk or carves its shape out.  *changed_out (may be null) receives how many voxels changed.
    int chunk_combine(int i, World &src, int src_chunk, int op, uint64_t *changed_out = nullptr)
    {
        const int rc = svo_world_chunk_combine(world_, i, src.world_, src_chunk, op, changed_out);
        check(rc, "World::chunk_combine");
        return rc;                                          // SVO_OK, or SVO_OK_LITERAL_ONLY
    }
    // Chunk i with chunk src_chunk of `src` - an uploaded world on the same device, which may be this one; its depth at most chunk i's -
    // placed into it: its cube starts at cell pl.offset, in orientation pl.orient, through SVO_COMBINE_* op (svo_world_chunk_stamp; svo.h
    // states the rule).  What puts a small model into a deep terrain chunk, any number of times.  *changed_out (may be null) receives how
    // many voxels changed.
    int chunk_stamp(int i, World &src, int src_chunk, const svo_placement &pl, int op, uint64_t *changed_out = nullptr)
    {
        const int rc = svo_world_chunk_stamp(world_, i, src.world_, src_chunk, &pl, op, changed_out);
        check(rc, "World::chunk_stamp");
        return rc;                                          // SVO_OK, or SVO_OK_LITERAL_ONLY
    }
    // Chunk i replaced by the cube of its own number of cells that starts at cell pl.offset of chunk src_chunk of `src` - an uploaded
    // world on the same device, which may be this one, and the chunk may be chunk i; its depth at least chunk i's -, oriented so that
    // chunk_stamp with the same placement puts every cell back where it came from (svo_world_chunk_extract; svo.h states the rule).  What
    // lifts a piece of a deep terrain chunk out as a model.  *occupied_out (may be null) receives how many of its voxels are not empty.
    int chunk_extract(int i, World &src, int src_chunk, const svo_placement &pl, uint64_t *occupied_out = nullptr)
    {
        const int rc = svo_world_chunk_extract(world_, i, src.world_, src_chunk, &pl, occupied_out);
        check(rc, "World::chunk_extract");
        return rc;                                          // SVO_OK, or SVO_OK_LITERAL_ONLY
    }

    // The voxel box of each of n G-buffer records (svo_hit_voxels: hit.bmin / hit.size, shaders/World.Fragment.glsl:168-172) into out_dev;
    // all zero for a record without a usable hit.  What the edit cursor is placed from (src/Main.cpp:317,340-367) and what leafUV needs.
    void hit_voxels(const svo_hit *gbuffer_dev, int64_t n, svo_voxel *out_dev, void *stream = nullptr)
    {
        check(svo_hit_voxels(world_, gbuffer_dev, n, out_dev, stream), "World::hit_voxels");
    }

    // leafUV (svo_hit_uv; shaders/World.Fragment.glsl:5-15) of the rectangle draw() filled, from its records and their boxes; uv_dev is [w*h][2].
    void hit_uv(const svo_camera &cam, int x0, int y0, int w, int h, const svo_hit *gbuffer_dev, const svo_voxel *voxels_dev, float *uv_dev,
                void *stream = nullptr) const
    {
        check(svo_hit_uv(&cam, semantics == SVO_SEMANTICS_GLSL ? 1.0f / 4096.0f : 0.0f, x0, y0, w, h, gbuffer_dev, voxels_dev, uv_dev, stream), "World::hit_uv");
    }

    // The fragment shader's colour with the caller's atlas as albedo (svo_shade_textured; shaders/World.Fragment.glsl:178-190).
    void shade_textured(const svo_camera &cam, const svo_shade_params &p, const svo_atlas &atlas, int x0, int y0, int w, int h,
                        const svo_hit *gbuffer_dev, const svo_voxel *voxels_dev, float *rgba_dev, void *stream = nullptr) const
    {
        check(svo_shade_textured(&cam, &p, &atlas, x0, y0, w, h, gbuffer_dev, voxels_dev, rgba_dev, stream), "World::shade_textured");
    }

    // Voxel ambient occlusion of the rectangle draw() filled (svo_hit_ao: w*h floats in [0, 1], 1 = open, from the eight lattice cells around
    // the open cell in front of each hit's face; cell 0 = the finest voxel of the hit's chunk), and its factor on the shaded image
    // (svo_shade_ao: behind a shade call, before shade_sky, shade_boxes and frame_rgba8).
    void hit_ao(const svo_camera &cam, int x0, int y0, int w, int h, const svo_hit *gbuffer_dev, const svo_voxel *voxels_dev, float *ao_dev,
                float cell = 0.0f, uint32_t see_through = 0, void *stream = nullptr)
    {
        svo_trace_params p;
        std::memset(&p, 0, sizeof p);
        p.semantics = semantics;
        p.see_through = see_through;
        check(svo_hit_ao(world_, &cam, &p, cell, x0, y0, w, h, gbuffer_dev, voxels_dev, ao_dev, stream), "World::hit_ao");
    }
    void shade_ao(const float *ao_dev, float strength, int64_t n, float *rgba_dev, void *stream = nullptr) const
    {
        check(svo_shade_ao(ao_dev, strength, n, rgba_dev, stream), "World::shade_ao");
    }

    // Mirror reflections off the axis-aligned faces of the voxels that were hit (not in the reference).  trace_reflections marches the
    // mirror ray of every usable hit of `material` (0 = any) of the rectangle draw() filled - params: that frame's -, reflect_dev gets
    // w*h records (svo_trace_reflections); shade_reflections blends what they saw over the image a shade call wrote, by mirror's Fresnel
    // term (svo_shade_reflections: behind shade_ao, before shade_boxes and frame_rgba8; p.eps is the launch's).
    void trace_reflections(const svo_camera &cam, const svo_trace_params &params, uint32_t material, int x0, int y0, int w, int h,
                           const svo_hit *gbuffer_dev, const svo_voxel *voxels_dev, svo_hit *reflect_dev, void *stream = nullptr)
    {
        check(svo_trace_reflections(world_, &cam, &params, material, x0, y0, w, h, gbuffer_dev, voxels_dev, reflect_dev, stream), "World::trace_reflections");
    }
    void shade_reflections(const svo_camera &cam, const svo_shade_params &p, const svo_mirror &mirror, int x0, int y0, int w, int h,
                           const svo_hit *gbuffer_dev, const svo_voxel *voxels_dev, const svo_hit *reflect_dev, float *rgba_dev, void *stream = nullptr) const
    {
        check(svo_shade_reflections(&cam, &p, &mirror, x0, y0, w, h, gbuffer_dev, voxels_dev, reflect_dev, rgba_dev, stream), "World::shade_reflections");
    }

    // The skybox behind the misses (svo_shade_sky; src/Skybox.cpp, src/Main.cpp:227) over an image a shade call has written for the same
    // rectangle: exactly one of gbuffer_dev and packed_dev names the rectangle's records.  Hit pixels and every depth are left alone.
    void shade_sky(const svo_camera &cam, const svo_sky &sky, int x0, int y0, int w, int h, const svo_hit *gbuffer_dev, const uint64_t *packed_dev,
                   float *rgba_dev, void *stream = nullptr) const
    {
        check(svo_shade_sky(&cam, &sky, x0, y0, w, h, gbuffer_dev, packed_dev, rgba_dev, stream), "World::shade_sky");
    }

    // n float4 pixels to the RGBA8 of the reference's colour attachment (svo_frame_rgba8; src/GBuffer.cpp, alpha 255).
    void frame_rgba8(const float *rgba_dev, int64_t n, uint32_t *out_dev, void *stream = nullptr) const
    {
        check(svo_frame_rgba8(rgba_dev, n, out_dev, stream), "World::frame_rgba8");
    }

    // computeTarget + imag.position(sigma) (src/Main.cpp:314-319) from the record a march wrote for the ray (alpha, beta), on the device.
    void cursor_place(vec3 alpha, vec3 beta, const svo_hit *record_dev, float size, svo_box *box_dev, void *stream = nullptr) const
    {
        const float a[3] = { alpha.x, alpha.y, alpha.z }, b[3] = { beta.x, beta.y, beta.z };
        check(svo_cursor_place(a, b, record_dev, size, box_dev, stream), "World::cursor_place");
    }
    // imag.draw(mvp) and the lights' marker cubes (src/Main.cpp:223-225) over the shaded image, behind shade_sky.
    void shade_boxes(const svo_camera &cam, const svo_box *boxes_dev, int nboxes, float near_plane, float far_plane, int x0, int y0, int w, int h,
                     float *rgba_dev, void *stream = nullptr) const
    {
        check(svo_shade_boxes(&cam, boxes_dev, nboxes, near_plane, far_plane, x0, y0, w, h, rgba_dev, stream), "World::shade_boxes");
    }

    // World::modify(i, tree delta, twig delta): re-send an edited chunk (Ocdelta ranges, src/Octree.h:47-54).
    void modify(int i, const svo_chunk_desc &edited, uint64_t tree_left, uint64_t tree_right, uint64_t twig_left, uint64_t twig_right, bool realloc_)
    {
        check(svo_world_update(world_, i, &edited, tree_left, tree_right, twig_left, twig_right, realloc_ ? 1 : 0), "World::modify");
    }

    // world.chunk[i].build / destroy / replace(cmin, cmax, ...) followed by world.modify(i, ...) (src/Main.cpp:340-367) in one
    // call, on the device the world is uploaded to (svo_world_edit_box).
    void build(int i, vec3 cmin, vec3 cmax, uint16_t material) { edit(i, SVO_EDIT_BUILD, cmin, cmax, material, "World::build"); }
    void destroy(int i, vec3 cmin, vec3 cmax) { edit(i, SVO_EDIT_DESTROY, cmin, cmax, 0, "World::destroy"); }
    void replace(int i, vec3 cmin, vec3 cmax, uint16_t material) { edit(i, SVO_EDIT_REPLACE, cmin, cmax, material, "World::replace"); }

    // destroy() / build() / replace() of src/Main.cpp:340-367 through modify() (:321-338): the cursor cube to every chunk that holds one of
    // its corners (svo_world_edit_cube).  Returns the chunks edited.
    std::vector<int> edit_cube(int op, vec3 bmin, float size, uint16_t material)
    {
        const float lo[3] = { bmin.x, bmin.y, bmin.z };
        int chunks[8], n = 0;
        check(svo_world_edit_cube(world_, op, lo, size, material, chunks, &n), "World::edit_cube");
        return std::vector<int>(chunks, chunks + n);
    }

    // No counterpart in the reference, which edits cubes only: the closed ball |p - centre| <= radius built into / destroyed in / replaced
    // in chunk i (svo_world_edit_ball), or in every chunk whose box it touches (svo_world_edit_ball_all; returns the chunks edited).
    void edit_ball(int i, int op, vec3 centre, float radius, uint16_t material)
    {
        const float c[3] = { centre.x, centre.y, centre.z };
        check(svo_world_edit_ball(world_, i, op, c, radius, material), "World::edit_ball");
    }
    std::vector<int> edit_ball_all(int op, vec3 centre, float radius, uint16_t material)
    {
        const float c[3] = { centre.x, centre.y, centre.z };
        std::vector<int> chunks((size_t)(volume > 0 ? volume : 1));
        int n = 0;
        check(svo_world_edit_ball_all(world_, op, c, radius, material, chunks.data(), (int)chunks.size(), &n), "World::edit_ball_all");
        chunks.resize((size_t)n);
        return chunks;
    }

    // World::shift(offset): slide the grid by one chunk (src/World.cpp:334-378).
    void shift(ivec3 offset)
    {
        const int o[3] = { offset.x, offset.y, offset.z };
        check(svo_world_shift(world_, o), "World::shift");
    }

    ivec3 index_float(vec3 p) const
    {
        const float pp[3] = { p.x, p.y, p.z };
        int q[3];
        check(svo_world_index_float(world_, pp, q), "World::index_float");
        return { q[0], q[1], q[2] };
    }
    int index(int x, int y, int z) const { return svo_world_index(world_, x, y, z); }
    svo_chunk_desc chunk(int i) const { svo_chunk_desc d; check(svo_world_chunk(world_, i, &d), "World::chunk"); return d; }
    svo_world *handle() const { return world_; }
private:
    void edit(int i, int op, vec3 cmin, vec3 cmax, uint16_t material, const char *where)
    {
        const float lo[3] = { cmin.x, cmin.y, cmin.z }, hi[3] = { cmax.x, cmax.y, cmax.z };
        check(svo_world_edit_box(world_, i, op, lo, hi, material), where);
    }
public:

    int width = 0, height = 0, depth = 0, plane = 0, volume = 0, chunksize = 0;
    svo_trace_params instance_params(bool shadow, const float light_dir[3]) const
    {
        svo_trace_params p;
        std::memset(&p, 0, sizeof p);
        p.semantics = semantics;
        p.shadow = shadow ? 1 : 0;
        if (light_dir) std::memcpy(p.light_dir, light_dir, sizeof p.light_dir);
        return p;
    }

private:
    svo_world *world_ = nullptr;
};

// bool chunkmarch(vec3 alpha, vec3 beta, const World *world, vec3 *sigma) — src/Traverse.cpp:127-171.
// One ray through the device kernel (the reference uses this for the edit cursor, src/Main.cpp:314-319).
// sigma is written only on a hit, exactly like the reference; `hit_out` optionally receives the voxel record.
// `reach` (not in the reference): the ray ends there - a hit counts only if its t < reach (svo_trace_segments); the default is chunkmarch itself.
inline bool chunkmarch(vec3 alpha, vec3 beta, const World *world, vec3 *sigma, svo_hit *hit_out = nullptr, float reach = INFINITY)
{
    struct Scratch {
        float *o = nullptr, *d = nullptr, *far = nullptr; svo_hit *h = nullptr;
        Scratch() { o = (float *)svo_device_alloc(12); d = (float *)svo_device_alloc(12); far = (float *)svo_device_alloc(4); h = (svo_hit *)svo_device_alloc(sizeof(svo_hit)); }
        ~Scratch() { svo_device_free(o); svo_device_free(d); svo_device_free(far); svo_device_free(h); }
    };
    static thread_local Scratch s;
    const float a[3] = { alpha.x, alpha.y, alpha.z }, b[3] = { beta.x, beta.y, beta.z };
    check(svo_memcpy_h2d(s.o, a, sizeof a), "chunkmarch"); check(svo_memcpy_h2d(s.d, b, sizeof b), "chunkmarch");
    if (reach == INFINITY) check(svo_trace_rays(world->handle(), s.o, s.d, 1, nullptr, s.h, nullptr), "chunkmarch");
    else {
        check(svo_memcpy_h2d(s.far, &reach, sizeof reach), "chunkmarch");
        check(svo_trace_segments(world->handle(), s.o, s.d, s.far, 1, nullptr, s.h, nullptr), "chunkmarch");
    }
    svo_hit h;
    check(svo_memcpy_d2h(&h, s.h, sizeof h), "chunkmarch");
    if (hit_out) *hit_out = h;
    if (!(h.flags & SVO_HIT_FLAG)) return false;
    if (sigma) *sigma = { alpha.x + beta.x * h.t, alpha.y + beta.y * h.t, alpha.z + beta.z * h.t };   // src/Traverse.cpp:161
    return true;
}

// A triangle mesh into a dense grid ((2^depth)^3 uint16 materials, x fastest; the caller clears it first), and the cells its shell
// encloses filled - world-less, like the shading stages; svo.h states both rules.  grid_add_mesh / grid_fill_enclosed: every pointer host
// memory.  device_grid_add_mesh / device_grid_fill_enclosed: the mesh's three arrays and the grid in device memory (the grid 16-byte
// aligned), on the calling thread's current device and on `stream`, complete at the return.  The fills return how many cells they filled.
// From the grid on: World::chunk_from_grid, then World::instances; or svo_chunk_from_grid and a world created from it.
inline void grid_add_mesh(const svo_mesh &mesh, uint32_t depth, uint16_t *grid) { check(svo_grid_add_mesh(&mesh, depth, grid), "grid_add_mesh"); }
inline void device_grid_add_mesh(const svo_mesh &mesh, uint32_t depth, uint16_t *grid_dev, void *stream = nullptr)
{
    check(svo_device_grid_add_mesh(&mesh, depth, grid_dev, stream), "device_grid_add_mesh");
}
inline uint64_t grid_fill_enclosed(uint16_t *grid, uint32_t depth, uint16_t material)
{
    uint64_t filled = 0;
    check(svo_grid_fill_enclosed(grid, depth, material, &filled), "grid_fill_enclosed");
    return filled;
}
inline uint64_t device_grid_fill_enclosed(uint16_t *grid_dev, uint32_t depth, uint16_t material, void *stream = nullptr)
{
    uint64_t filled = 0;
    check(svo_device_grid_fill_enclosed(grid_dev, depth, material, &filled, stream), "device_grid_fill_enclosed");
    return filled;
}
// The same fill on a chunk's host pools, without the grid, chunk depth in [2, 16]: *out receives malloc'ed pools (svo_chunk_free), `in`
// stays as it is.  Returns how many voxels were filled.
inline uint64_t chunk_fill_enclosed(const svo_chunk_desc &in, uint16_t material, svo_chunk_desc *out)
{
    uint64_t filled = 0;
    check(svo_chunk_fill_enclosed(&in, material, out, &filled), "chunk_fill_enclosed");
    return filled;
}
// Two chunks' host pools of one depth in [2, 16] combined cell by cell on their trees (SVO_COMBINE_*), without a grid: *out receives
// malloc'ed pools in a's frame (svo_chunk_free), `a` and `b` stay as they are.  Returns how many voxels differ from a's.
inline uint64_t chunk_combine(const svo_chunk_desc &a, const svo_chunk_desc &b, int op, svo_chunk_desc *out)
{
    uint64_t changed = 0;
    check(svo_chunk_combine(&a, &b, op, out, &changed), "chunk_combine");
    return changed;
}
// Host pools b (depth at most a's, both in [2, 16]) placed into host pools a at cell pl.offset in orientation pl.orient through
// SVO_COMBINE_* op, without a grid: *out receives malloc'ed pools in a's frame (svo_chunk_free).  Returns how many voxels differ from a's.
inline uint64_t chunk_stamp(const svo_chunk_desc &a, const svo_chunk_desc &b, const svo_placement &pl, int op, svo_chunk_desc *out)
{
    uint64_t changed = 0;
    check(svo_chunk_stamp(&a, &b, &pl, op, out, &changed), "chunk_stamp");
    return changed;
}
// The cube of (2^depth)^3 cells of host pools a (depth at most a's, both in [2, 16]) that starts at cell pl.offset, in orientation
// pl.orient - the stamp's inverse -, without a grid: *out receives malloc'ed pools in the frame position / size (svo_chunk_free).
// Returns how many of its voxels are not empty.
inline uint64_t chunk_extract(const svo_chunk_desc &a, const svo_placement &pl, uint32_t depth, const float position[3], float size, svo_chunk_desc *out)
{
    uint64_t occupied = 0;
    check(svo_chunk_extract(&a, &pl, depth, position, size, out, &occupied), "chunk_extract");
    return occupied;
}

} // namespace svo
