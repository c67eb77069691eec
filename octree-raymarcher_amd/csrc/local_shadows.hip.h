// local_shadows.hip.h — shadows from the point light and the spotlight (svo_trace_local_shadows).
//
// The reference hands the directional light's shadow-map term to all three light functions (shaders/World.Fragment.glsl:186-190);
// this is the opt-in departure from it: one occlusion ray per hit and local light, from the sample point the existing shadow ray
// starts from towards the light's position, occluded only by what lies in front of the light.  The march kernels are not changed
// for it (the pattern of see_through.hip.h): a kernel writes the ray list, ONE ray-list launch marches the rays of every light
// asked for into scratch records, a kernel folds those into the flag word of the caller's G-buffer.
#pragma once
#include "image_stage.hip.h"

namespace svo {

constexpr int LOCAL_LIGHTS = 2;         // point, spot
struct LocalLights {
    float pos[LOCAL_LIGHTS][3];         // the lights asked for, in list-segment order
    uint32_t bit[LOCAL_LIGHTS];         // SVO_SHADOWED_POINT / SVO_SHADOWED_SPOT of each
    int32_t count;
};

// P = o + d * (t - eps) of pixel k's record: where the directional shadow ray starts (kernel_literal.hip.h; oracle trace_one)
__device__ __forceinline__ V3 local_sample_point(const PixelFrame &F, int64_t k, float t, float eps)
{
    V3 o, d;
    F.ray(k, o, d);
    return o + d * (t - eps);
}
// v = L - P, q = |v|^2 summed left to right; false where there is no ray (the light sits on P, or q is not finite).  Both kernels
// go through this, so the distance the resolve compares with is the one the direction was made from.
__device__ __forceinline__ bool local_light_vector(V3 p, const float *light, V3 &v, float &q)
{
    v = ld3(light) - p;
    q = v.x * v.x + v.y * v.y + v.z * v.z;
    return q > 0.0f && q < INFINITY;
}

// The ray list in pixel order, one segment of n rays per light.  A pixel without a usable hit, or whose light has no ray, gets
// k_continuation's ray: one whose line misses the world box, so its record is a miss.
__global__ __launch_bounds__(256) void k_local_rays(PixelFrame F, float eps, LocalLights L, V3 miss, const uint4 *gbuffer, float *origins, float *dirs)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x, n = F.count();
    if (k >= n) return;
    const bool hit = usable_hit(record_flags(gbuffer, k));
    V3 p = mk(0.0f, 0.0f, 0.0f);
    if (hit) p = local_sample_point(F, k, __uint_as_float(gbuffer[2 * k].x), eps);
    for (int j = 0; j < L.count; ++j) {
        V3 o = miss, d = mk(-1.0f, 0.0f, 0.0f), v;
        float q;
        if (hit && local_light_vector(p, L.pos[j], v, q)) { o = p; d = v * (1.0f / sqrtf(q)); }        // normalize3's expression
        const int64_t r = (int64_t)j * n + k;
        origins[3 * r] = o.x; origins[3 * r + 1] = o.y; origins[3 * r + 2] = o.z;
        dirs[3 * r] = d.x; dirs[3 * r + 1] = d.y; dirs[3 * r + 2] = d.z;
    }
}

// A light is occluded iff its ray's record is a usable hit in front of the light (t < dist): terrain behind the light does not
// shadow it, a runaway ray is "traced, not occluded".  Only the flag word of a usable hit's record is rewritten: SVO_LOCAL_SHADOWS,
// the bits of the lights asked for, and a copy of SVO_SHADOWED for a light that was not.
__global__ __launch_bounds__(256) void k_local_resolve(PixelFrame F, float eps, LocalLights L, const uint4 *rays, uint4 *gbuffer)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x, n = F.count();
    if (k >= n) return;
    const uint32_t word = gbuffer[2 * k + 1].x;
    uint32_t flags = word >> 16;
    if (!usable_hit(flags)) return;
    const V3 p = local_sample_point(F, k, __uint_as_float(gbuffer[2 * k].x), eps);
    const uint32_t both = SVO_SHADOWED_POINT | SVO_SHADOWED_SPOT;
    flags = (flags & ~both) | SVO_LOCAL_SHADOWS | ((flags & SVO_SHADOWED) ? both : 0u);
    for (int j = 0; j < L.count; ++j) {
        const int64_t r = (int64_t)j * n + k;
        V3 v;
        float q;
        bool occluded = false;
        if (local_light_vector(p, L.pos[j], v, q) && usable_hit(record_flags(rays, r))) occluded = __uint_as_float(rays[2 * r].x) < sqrtf(q);
        flags = (flags & ~L.bit[j]) | (occluded ? L.bit[j] : 0u);
    }
    reinterpret_cast<uint32_t *>(gbuffer + 2 * k + 1)[0] = (word & 0xFFFFu) | (flags << 16);
}

} // namespace svo
