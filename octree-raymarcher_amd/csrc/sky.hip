// sky.hip — what stands between the shaded float4 image and the frame the reference shows: the skybox behind the misses
// (svo_shade_sky; src/Skybox.cpp, shaders/Skybox.*.glsl) and the RGBA8 colour attachment (svo_frame_rgba8; src/GBuffer.cpp,
// shaders/GBuffer.Fragment.glsl:10).  One thread per pixel each; the arithmetic is the one include/svo.h writes out, every operation
// in float and separately rounded; the cube-map lookup itself is sky_lookup.hip.h's, shared with svo_shade_reflections (shade.hip).
#include <hip/hip_runtime.h>

#include <cmath>

#include "image_stage.hip.h"
#include "sky_lookup.hip.h"

namespace svo {
namespace {

struct SkyArgs {
    PixelFrame frame;
    SkyMap map;
    const void *records;                        // the 32-byte records or the packed ones (image_stage.hip.h record_flags)
    float *rgba;
};

// PACKED: the records are svo_gbuffer_pack's.  A hit pixel ends after its one load; a sky pixel writes r, g, b and leaves its depth.
template <bool PACKED>
__global__ __launch_bounds__(256) void k_shade_sky(SkyArgs A)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= A.frame.count()) return;
    const uint32_t flags = PACKED ? record_flags(static_cast<const uint2 *>(A.records), k) : record_flags(static_cast<const uint4 *>(A.records), k);
    if (flags & SVO_HIT_FLAG) return;
    V3 o, d, c;
    A.frame.ray(k, o, d);
    if (!sky_lookup(A.map, d, c)) return;       // (sky_lookup.hip.h)
    float *out = A.rgba + 4 * k;
    out[0] = c.x; out[1] = c.y; out[2] = c.z;
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
    if (!sky_ok(sky) || !rgba_dev || (gbuffer_dev != nullptr) == (packed_dev != nullptr) || !rect_ok(cam, x0, y0, w, h)) { set_error("svo_shade_sky: bad argument"); return SVO_ERR_INVALID_ARG; }
    SkyArgs A;
    A.frame = make_frame(*cam, x0, y0, w, h);
    A.map = sky_map(*sky);
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
