// sky.hip — what stands between the shaded float4 image and the frame the reference shows: the skybox behind the misses
// (svo_shade_sky; src/Skybox.cpp, shaders/Skybox.*.glsl) and the RGBA8 colour attachment (svo_frame_rgba8; src/GBuffer.cpp,
// shaders/GBuffer.Fragment.glsl:10).  One thread per pixel each; the arithmetic is the one include/svo.h writes out, every operation
// in float and separately rounded (IEEE divisions, no hardware reciprocals: the face chosen at a cube edge must not hang on 1 ulp).
#include <hip/hip_runtime.h>

#include <cmath>

#include "image_stage.hip.h"

namespace svo {
namespace {

struct SkyArgs {
    PixelFrame frame;
    const uint8_t *faces[6];
    int32_t size, filter;
    const void *records;                        // the 32-byte records or the packed ones (image_stage.hip.h record_flags)
    float *rgba;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
// (int)v of a floor()ed texel coordinate; a NaN (a NaN camera) reads texel 0, never out of range
__device__ __forceinline__ int texel_int(float v) { return v == v ? (int)v : 0; }

struct Texel { float r, g, b; };
__device__ __forceinline__ Texel texel(const uint8_t *image, int size, int x, int y)
{
    const uint8_t *px = image + ((size_t)y * (size_t)size + (size_t)x) * 3;
    Texel t;
    t.r = (float)px[0] / 255.0f; t.g = (float)px[1] / 255.0f; t.b = (float)px[2] / 255.0f;
    return t;
}
__device__ __forceinline__ float lerp(float p, float q, float a) { return p + (q - p) * a; }

// PACKED: the records are svo_gbuffer_pack's.  A hit pixel ends after its one load; a sky pixel writes r, g, b and leaves its depth.
template <bool PACKED>
__global__ __launch_bounds__(256) void k_shade_sky(SkyArgs A)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= A.frame.count()) return;
    const uint32_t flags = PACKED ? record_flags(static_cast<const uint2 *>(A.records), k) : record_flags(static_cast<const uint4 *>(A.records), k);
    if (flags & SVO_HIT_FLAG) return;
    V3 o, d;
    A.frame.ray(k, o, d);
    // the OpenGL cube-map table: major axis (X before Y before Z on ties), face, (sc, tc)
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    int face;
    float ma, sc, tc;
    if (ax >= ay && ax >= az) { ma = ax; face = d.x < 0.0f ? 1 : 0; sc = d.x < 0.0f ? d.z : -d.z; tc = -d.y; }
    else if (ay >= az) { ma = ay; face = d.y < 0.0f ? 3 : 2; sc = d.x; tc = d.y < 0.0f ? -d.z : d.z; }
    else { ma = az; face = d.z < 0.0f ? 5 : 4; sc = d.z < 0.0f ? -d.x : d.x; tc = -d.y; }
    if (!(ma > 0.0f)) return;
    const float s = (sc / ma + 1.0f) * 0.5f, t = (tc / ma + 1.0f) * 0.5f;
    const uint8_t *image = A.faces[face];
    const int size = A.size;
    Texel c;
    if (A.filter == SVO_SKY_NEAREST) {
        c = texel(image, size, clampi(texel_int(floorf(s * (float)size)), 0, size - 1), clampi(texel_int(floorf(t * (float)size)), 0, size - 1));
    } else {                                    // GL_LINEAR, CLAMP_TO_EDGE within the face
        const float u = s * (float)size - 0.5f, v = t * (float)size - 0.5f;
        const float i = floorf(u), j = floorf(v);
        const float a = u - i, b = v - j;
        const int xi = texel_int(i), yj = texel_int(j);
        const int xl = clampi(xi, 0, size - 1), xr = clampi(xi + 1, 0, size - 1);
        const int yl = clampi(yj, 0, size - 1), yr = clampi(yj + 1, 0, size - 1);
        const Texel t00 = texel(image, size, xl, yl), t10 = texel(image, size, xr, yl);
        const Texel t01 = texel(image, size, xl, yr), t11 = texel(image, size, xr, yr);
        c.r = lerp(lerp(t00.r, t10.r, a), lerp(t01.r, t11.r, a), b);
        c.g = lerp(lerp(t00.g, t10.g, a), lerp(t01.g, t11.g, a), b);
        c.b = lerp(lerp(t00.b, t10.b, a), lerp(t01.b, t11.b, a), b);
    }
    float *out = A.rgba + 4 * k;
    out[0] = c.r; out[1] = c.g; out[2] = c.b;
}

__device__ __forceinline__ uint32_t unorm8(float c)
{
    if (!(c > 0.0f)) return 0u;                 // NaN, -0.0 and everything below
    if (c >= 1.0f) return 255u;
    return (uint32_t)(int)(c * 255.0f + 0.5f);
}

__global__ __launch_bounds__(256) void k_frame_rgba8(const float4 *rgba, uint32_t *out, int64_t n)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const float4 c = rgba[k];
    out[k] = unorm8(c.x) | (unorm8(c.y) << 8) | (unorm8(c.z) << 16) | 0xFF000000u;
}

} // namespace
} // namespace svo

using namespace svo;

extern "C" {

int svo_shade_sky(const svo_camera *cam, const svo_sky *sky, int x0, int y0, int w, int h,
                  const svo_hit *gbuffer_dev, const uint64_t *packed_dev, float *rgba_dev, void *stream)
{
    bool ok = sky && rgba_dev && (gbuffer_dev != nullptr) != (packed_dev != nullptr) && rect_ok(cam, x0, y0, w, h);
    ok = ok && sky->size > 0 && (sky->filter == SVO_SKY_LINEAR || sky->filter == SVO_SKY_NEAREST);
    for (int f = 0; ok && f < 6; ++f) ok = sky->faces_dev[f] != nullptr;
    if (!ok) { set_error("svo_shade_sky: bad argument"); return SVO_ERR_INVALID_ARG; }
    SkyArgs A;
    A.frame = make_frame(*cam, x0, y0, w, h);
    for (int f = 0; f < 6; ++f) A.faces[f] = sky->faces_dev[f];
    A.size = sky->size; A.filter = sky->filter;
    A.records = gbuffer_dev ? static_cast<const void *>(gbuffer_dev) : packed_dev;
    A.rgba = rgba_dev;
    return launch_per_element("svo_shade_sky", A.frame.count(), (hipStream_t)stream, packed_dev ? k_shade_sky<true> : k_shade_sky<false>, A);
}

int svo_frame_rgba8(const float *rgba_dev, int64_t n, uint32_t *out_dev, void *stream)
{
    if (n < 0 || (n > 0 && (!rgba_dev || !out_dev))) { set_error("svo_frame_rgba8: bad argument"); return SVO_ERR_INVALID_ARG; }
    return launch_per_element("svo_frame_rgba8", n, (hipStream_t)stream, k_frame_rgba8, reinterpret_cast<const float4 *>(rgba_dev), out_dev, n);
}

} // extern "C"
