// shadowmap.hip.h — the directional light's shadow map (svo_shadowmap_render, svo_shadowmap_apply).
//
// The reference marches the world once per frame from the directional light into a depth image (World::draw_shadowmap,
// src/World.cpp:162-203, shaders/ShadowmapWorld.Fragment.glsl, under an OrthoCamera, src/Main.cpp:149,190-198) and computeShadow looks
// every hit point up in it (shaders/World.Fragment.glsl:140-155,186).  Here the light's view is a true orthographic raster of parallel
// rays, the depth is the march's own t, and a point outside the map is lit (the reference's sampler wraps, src/Light.cpp:176-179).  The
// march kernels are not changed for it (the pattern of see_through.hip.h and local_shadows.hip.h): a kernel writes the ray list, ONE
// ray-list launch marches it into scratch records, a kernel folds those into the caller's depth image; the lookup is one gather per
// hit pixel of a G-buffer and needs no world.
#pragma once
#include "image_stage.hip.h"
#include "local_shadows.hip.h"

namespace svo {

// svo_shadowmap without its pointer
struct MapFrame {
    float origin[3], dir[3], right[3], up[3];
    float half_w, half_h;
    int32_t width, height;
    __host__ __device__ int64_t count() const { return (int64_t)width * height; }
};

// The ray list treats 64 consecutive rays as one tile (device.hip trace_list): slot r = tile * 64 + jj * 8 + ii holds texel
// (8 * (tile % (width / 8)) + ii, 8 * (tile / (width / 8)) + jj), so that a wave marches an 8 x 8 block of neighbouring parallel rays
// as the image path's waves do, not a 64 x 1 strip.  width and height are multiples of 8: every slot below count() names a texel.
__device__ __forceinline__ void map_slot_texel(const MapFrame &M, int64_t r, int &i, int &j)
{
    const int64_t tile = r >> 6;
    const int per_row = M.width >> 3, in_tile = (int)(r & 63);
    i = 8 * (int)(tile % per_row) + (in_tile & 7);
    j = 8 * (int)(tile / per_row) + (in_tile >> 3);
}

// the ray of texel (i, j): the shape of camera_ray's u and v, every operation separately rounded
__global__ __launch_bounds__(256) void k_shadowmap_rays(MapFrame M, float *origins, float *dirs)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= M.count()) return;
    int i, j;
    map_slot_texel(M, r, i, j);
    const float fx = (float)i + 0.5f, fy = (float)j + 0.5f;
    const float u = ((fx / (float)M.width) * 2.0f - 1.0f) * M.half_w;
    const float v = (1.0f - (fy / (float)M.height) * 2.0f) * M.half_h;
    const V3 o = (ld3(M.origin) + ld3(M.right) * u) + ld3(M.up) * v;
    origins[3 * r] = o.x; origins[3 * r + 1] = o.y; origins[3 * r + 2] = o.z;
    dirs[3 * r] = M.dir[0]; dirs[3 * r + 1] = M.dir[1]; dirs[3 * r + 2] = M.dir[2];
}

// depth[j * width + i] = t of slot r's record where it is a usable hit, +inf elsewhere: the permutation undone
__global__ __launch_bounds__(256) void k_shadowmap_depth(MapFrame M, const uint4 *records, float *depth)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= M.count()) return;
    int i, j;
    map_slot_texel(M, r, i, j);
    depth[(int64_t)j * M.width + i] = usable_hit(record_flags(records, r)) ? __uint_as_float(records[2 * r].x) : INFINITY;
}

// The lookup.  Only the flag half-word of a usable hit's record is rewritten: SVO_SHADOW_TRACED set, SVO_SHADOWED written.
__global__ __launch_bounds__(256) void k_shadowmap_apply(PixelFrame F, float eps, MapFrame M, const float *depth, float bias, uint4 *gbuffer)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= F.count()) return;
    const uint32_t word = gbuffer[2 * k + 1].x;
    uint32_t flags = word >> 16;
    if (!usable_hit(flags)) return;
    const V3 p = local_sample_point(F, k, __uint_as_float(gbuffer[2 * k].x), eps);
    const V3 q = p - ld3(M.origin);
    const float s = q.x * M.dir[0] + q.y * M.dir[1] + q.z * M.dir[2];
    const float a = q.x * M.right[0] + q.y * M.right[1] + q.z * M.right[2];
    const float b = q.x * M.up[0] + q.y * M.up[1] + q.z * M.up[2];
    const float w = (float)M.width, h = (float)M.height;
    const float fu = (a / M.half_w + 1.0f) * 0.5f * w;
    const float fv = (1.0f - b / M.half_h) * 0.5f * h;
    bool occluded = false;
    if (fu >= 0.0f && fu < w && fv >= 0.0f && fv < h) {                 // (NaN fails: lit)
        const int i = (int)floorf(fu), j = (int)floorf(fv);
        occluded = depth[(int64_t)j * M.width + i] < s - bias;
    }
    flags = (flags & ~(uint32_t)SVO_SHADOWED) | SVO_SHADOW_TRACED | (occluded ? (uint32_t)SVO_SHADOWED : 0u);
    reinterpret_cast<uint32_t *>(gbuffer + 2 * k + 1)[0] = (word & 0xFFFFu) | (flags << 16);
}

} // namespace svo
