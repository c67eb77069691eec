// image_stage.hip.h — what the per-pixel stages behind the march share (shade.hip, sky.hip, boxes.hip, see_through.hip.h,
// local_shadows.hip.h): the rectangle of the camera image a launch covers and the ray of each of its pixels, the decode of a G-buffer
// record in its two forms, leafUV from both, the entered face of a hit's voxel, and on the host the rectangle's validity test (the
// launch itself: hip_own.h, launch_per_element).
#pragma once
#include <cstring>
#include <string>

#include "march.hip.h"
#include "hip_own.h"

namespace svo {

// ---- device: which pixel a thread is, and its ray -----------------------------------------------------------------------------------
// Pixel k of the launch, k in [0, count()), is (x0 + k % w, y0 + k / w) of the cam's imgw x imgh image.
struct PixelFrame {
    FrameCam cam;
    int32_t imgw, imgh, x0, y0, w, h;
    __host__ __device__ int64_t count() const { return (int64_t)w * h; }
    __device__ __forceinline__ void pixel(int64_t k, int &px, int &py) const { px = x0 + (int)(k % w); py = y0 + (int)(k / w); }
    __device__ __forceinline__ void ray(int64_t k, V3 &o, V3 &d) const
    {
        int px, py;
        pixel(k, px, py);
        camera_ray(cam, imgw, imgh, px, py, o, d);
    }
};

// ---- device: a G-buffer record ------------------------------------------------------------------------------------------------------
struct HitRecord { float t; V3 n; uint32_t material, flags; };

__device__ __forceinline__ bool usable_hit(uint32_t flags) { return (flags & SVO_HIT_FLAG) && !(flags & SVO_ERR_FLAG); }

// normalize(ivec3 in {-1,0,1}^3) from the packed record's 2-bit-per-axis code (bit 6: NaN): the same constants as the march kernels
__device__ __forceinline__ V3 normal_from_code(uint32_t code)
{
    if (code & (1u << 6)) { const float q = __uint_as_float(0x7FC00000u); return mk(q, q, q); }
    const float ix = (float)((int)(code & 3u) - 1), iy = (float)((int)((code >> 2) & 3u) - 1), iz = (float)((int)((code >> 4) & 3u) - 1);
    const float dot = ix * ix + iy * iy + iz * iz;
    const float inv = dot == 1.0f ? 1.0f : dot == 2.0f ? __uint_as_float(0x3F3504F3u) : dot == 3.0f ? __uint_as_float(0x3F13CD3Au) : __uint_as_float(0x7FC00000u);
    return mk(ix * inv, iy * inv, iz * inv);
}

// the flags alone (one 4-byte load): all 16 of a 32-byte record, the low 8 of a packed one (bit 31, SVO_ERR_FLAG: k_gbuffer_unpack's)
__device__ __forceinline__ uint32_t record_flags(const uint4 *gbuffer, int64_t k) { return gbuffer[2 * k + 1].x >> 16; }
__device__ __forceinline__ uint32_t record_flags(const uint2 *packed, int64_t k) { return (packed[k].y >> 16) & 0xFFu; }

__device__ __forceinline__ HitRecord load_hit(const uint4 *gbuffer, int64_t k)
{
    const uint4 r0 = gbuffer[2 * k], r1 = gbuffer[2 * k + 1];
    HitRecord r;
    r.t = __uint_as_float(r0.x);
    r.n = mk(__uint_as_float(r0.y), __uint_as_float(r0.z), __uint_as_float(r0.w));
    r.material = r1.x & 0xFFFFu; r.flags = r1.x >> 16;
    return r;
}
__device__ __forceinline__ HitRecord load_packed(const uint2 *packed, int64_t k)
{
    const uint2 p = packed[k];
    HitRecord r;
    r.t = __uint_as_float(p.x);
    r.n = normal_from_code((p.y >> 24) & 0x7Fu);
    r.material = p.y & 0xFFFFu; r.flags = (p.y >> 16) & 0xFFu;
    return r;
}

// leafUV of pixel k from its record h and its voxel record (v0, v1: svo_hit_voxels); false, and (0, 0), where there is none: no usable
// hit, or a voxel record without SVO_LOCATE_INSIDE
__device__ __forceinline__ bool hit_uv(const PixelFrame &F, int64_t k, float eps, const HitRecord &h, uint4 v0, uint4 v1, float &u, float &v)
{
    u = v = 0.0f;
    if (!usable_hit(h.flags) || !((v1.x >> 16) & SVO_LOCATE_INSIDE)) return false;
    V3 o, d;
    F.ray(k, o, d);
    const V3 p = o + d * (h.t - eps);           // the point cubeNormal is taken at, shaders/World.Fragment.glsl:174
    leaf_uv(p, mk(__uint_as_float(v0.x), __uint_as_float(v0.y), __uint_as_float(v0.z)), __uint_as_float(v0.w), h.material, eps, u, v);
    return true;
}

// ---- device: the face of its voxel a hit entered (ao.hip.h, reflect.hip.h) ----------------------------------------------------------
__device__ __forceinline__ float axis_of(V3 v, int k) { return k == 0 ? v.x : k == 1 ? v.y : v.z; }
__device__ __forceinline__ V3 with_axis(V3 v, int k, float s) { return mk(k == 0 ? s : v.x, k == 1 ? s : v.y, k == 2 ? s : v.z); }

// The box [lo, hi] of a voxel record's first half (v0: bmin, size) and the face of it that the sample point P of a ray along d lies on:
// the SVO_NORMAL_FACE rule (march.hip.h face_normal; include/svo.h svo_hit_ao step 2) as an axis and a sign of +1 or -1
struct HitFace { V3 lo, hi; int axis; float sgn; };
__device__ __forceinline__ HitFace hit_face(V3 P, uint4 v0, V3 d)
{
    HitFace f;
    f.lo = mk(__uint_as_float(v0.x), __uint_as_float(v0.y), __uint_as_float(v0.z));
    f.hi = f.lo + __uint_as_float(v0.w);
    const V3 n = face_normal(P, f.lo, f.hi, d);
    f.axis = n.x != 0.0f ? 0 : n.y != 0.0f ? 1 : 2;
    f.sgn = axis_of(n, f.axis);
    return f;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
inline FrameCam frame_cam(const svo_camera &c)
{
    FrameCam d;
    std::memcpy(d.eye, c.eye, sizeof d.eye); std::memcpy(d.fwd, c.forward, sizeof d.fwd);
    std::memcpy(d.right, c.right, sizeof d.right); std::memcpy(d.up, c.up, sizeof d.up);
    d.tanx = c.tan_half_x; d.tany = c.tan_half_y;
    return d;
}

// a rectangle a stage accepts: it may be empty and may reach past the image, but neither starts nor extends backwards
inline bool rect_ok(const svo_camera *cam, int x0, int y0, int w, int h)
{
    return cam && w >= 0 && h >= 0 && x0 >= 0 && y0 >= 0 && cam->width > 0 && cam->height > 0;
}

inline PixelFrame make_frame(const svo_camera &cam, int x0, int y0, int w, int h)
{
    PixelFrame F;
    F.cam = frame_cam(cam);
    F.imgw = cam.width; F.imgh = cam.height; F.x0 = x0; F.y0 = y0; F.w = w; F.h = h;
    return F;
}

} // namespace svo
