// reflect.hip.h — mirror reflections off axis-aligned voxel faces (svo_trace_reflections, svo_shade_reflections).
//
// Not in the reference.  The pattern of see_through.hip.h and local_shadows.hip.h: a kernel writes the ray list, ONE ray-list launch
// marches it, a per-pixel kernel (shade.hip k_shade_reflections) uses the records; the march kernels are not changed.  The mirror ray
// of an axis-aligned face is the incoming ray with one sign flipped.  It starts on the face plane of the voxel that was hit, pushed
// out by eps, not at the shadow ray's point P = o + d * (t - eps): P lies on or inside the closed box of its voxel, and a ray from
// there hits that voxel again at t = 0 (DESIGN.md 6s has the figures).  That needs the voxel's box: voxels_dev, svo_hit_voxels'.
// Both stages form the ray through mirror_ray(), so the shade stage rebuilds exactly the ray that was marched.  Like march.hip.h this
// is compiled with -ffp-contract=off: every float operation below is separately rounded.
#pragma once
#include "image_stage.hip.h"

namespace svo {

// A pixel reflects iff its record is a usable hit of `material` (0: of any material) and its voxel record has a box
__device__ __forceinline__ bool mirror_pixel(uint32_t material, uint4 r1, uint4 v1)
{
    return usable_hit(r1.x >> 16) && (material == 0u || (r1.x & 0xFFFFu) == material) && ((v1.x >> 16) & SVO_LOCATE_INSIDE);
}

// The mirror ray (O, R) of pixel k, include/svo.h steps 1-4, and c = |d[axis]|, the cosine of the angle of incidence; false where
// the pixel is no mirror pixel
__device__ __forceinline__ bool mirror_ray(const PixelFrame &F, int64_t k, float eps, uint32_t material, const uint4 *gbuffer, const uint4 *voxels,
                                           V3 &O, V3 &R, float &c)
{
    if (!mirror_pixel(material, gbuffer[2 * k + 1], voxels[2 * k + 1])) return false;
    const float t = __uint_as_float(gbuffer[2 * k].x);
    V3 o, d;
    F.ray(k, o, d);
    const V3 P = o + d * (t - eps);                                             // 1.
    const HitFace face = hit_face(P, voxels[2 * k], d);                         // 2.
    const int ax = face.axis;
    const float sgn = face.sgn;
    O = with_axis(P, ax, (sgn > 0.0f ? axis_of(face.hi, ax) : axis_of(face.lo, ax)) + sgn * eps);     // 3.
    c = fabsf(axis_of(d, ax));
    R = with_axis(d, ax, sgn * c);                                              // 4.
    return true;
}

// svo_trace_reflections: the ray list in pixel order.  A pixel that does not reflect gets k_continuation's ray, whose line misses the
// world box: its record is the all-zero miss.  (static: shade.hip includes this header for mirror_ray() and launches no such kernel)
[[maybe_unused]] static __global__ __launch_bounds__(256) void k_mirror_rays(PixelFrame F, float eps, uint32_t material, V3 miss, const uint4 *gbuffer, const uint4 *voxels,
                                                     float *origins, float *dirs)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= F.count()) return;
    V3 o, d;
    float c;
    if (!mirror_ray(F, k, eps, material, gbuffer, voxels, o, d, c)) { o = miss; d = mk(-1.0f, 0.0f, 0.0f); }
    origins[3 * k] = o.x; origins[3 * k + 1] = o.y; origins[3 * k + 2] = o.z;
    dirs[3 * k] = d.x; dirs[3 * k + 1] = d.y; dirs[3 * k + 2] = d.z;
}

} // namespace svo
