// sky_lookup.hip.h — the cube map of svo_sky looked up along a direction, as include/svo.h writes it out under svo_shade_sky: every
// operation in float and separately rounded (IEEE divisions, no hardware reciprocals: the face chosen at a cube edge must not hang on
// 1 ulp).  sky.hip looks along the pixel's own ray (k_shade_sky), shade.hip along a mirror ray (k_shade_reflections).
#pragma once
#include "image_stage.hip.h"

namespace svo {

struct SkyMap {
    const uint8_t *faces[6];
    int32_t size, filter;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
// (int)v of a floor()ed texel coordinate; a NaN (a NaN camera) reads texel 0, never out of range
__device__ __forceinline__ int texel_int(float v) { return v == v ? (int)v : 0; }

__device__ __forceinline__ V3 sky_texel(const uint8_t *image, int size, int x, int y)
{
    const uint8_t *px = image + ((size_t)y * (size_t)size + (size_t)x) * 3;
    return mk((float)px[0] / 255.0f, (float)px[1] / 255.0f, (float)px[2] / 255.0f);
}
__device__ __forceinline__ float sky_lerp(float p, float q, float a) { return p + (q - p) * a; }

// The colour of the sky along d; false, and c untouched, where there is none: !(ma > 0), a zero or NaN direction
__device__ __forceinline__ bool sky_lookup(const SkyMap &S, V3 d, V3 &c)
{
    // the OpenGL cube-map table: major axis (X before Y before Z on ties), face, (sc, tc)
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    int face;
    float ma, sc, tc;
    if (ax >= ay && ax >= az) { ma = ax; face = d.x < 0.0f ? 1 : 0; sc = d.x < 0.0f ? d.z : -d.z; tc = -d.y; }
    else if (ay >= az) { ma = ay; face = d.y < 0.0f ? 3 : 2; sc = d.x; tc = d.y < 0.0f ? -d.z : d.z; }
    else { ma = az; face = d.z < 0.0f ? 5 : 4; sc = d.z < 0.0f ? -d.x : d.x; tc = -d.y; }
    if (!(ma > 0.0f)) return false;
    const float s = (sc / ma + 1.0f) * 0.5f, t = (tc / ma + 1.0f) * 0.5f;
    const uint8_t *image = S.faces[face];
    const int size = S.size;
    if (S.filter == SVO_SKY_NEAREST) {
        c = sky_texel(image, size, clampi(texel_int(floorf(s * (float)size)), 0, size - 1), clampi(texel_int(floorf(t * (float)size)), 0, size - 1));
    } else {                                    // GL_LINEAR, CLAMP_TO_EDGE within the face
        const float u = s * (float)size - 0.5f, v = t * (float)size - 0.5f;
        const float i = floorf(u), j = floorf(v);
        const float a = u - i, b = v - j;
        const int xi = texel_int(i), yj = texel_int(j);
        const int xl = clampi(xi, 0, size - 1), xr = clampi(xi + 1, 0, size - 1);
        const int yl = clampi(yj, 0, size - 1), yr = clampi(yj + 1, 0, size - 1);
        const V3 t00 = sky_texel(image, size, xl, yl), t10 = sky_texel(image, size, xr, yl);
        const V3 t01 = sky_texel(image, size, xl, yr), t11 = sky_texel(image, size, xr, yr);
        c.x = sky_lerp(sky_lerp(t00.x, t10.x, a), sky_lerp(t01.x, t11.x, a), b);
        c.y = sky_lerp(sky_lerp(t00.y, t10.y, a), sky_lerp(t01.y, t11.y, a), b);
        c.z = sky_lerp(sky_lerp(t00.z, t10.z, a), sky_lerp(t01.z, t11.z, a), b);
    }
    return true;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// a sky a lookup accepts: six faces, a size, a known filter
inline bool sky_ok(const svo_sky *sky)
{
    bool ok = sky && sky->size > 0 && (sky->filter == SVO_SKY_LINEAR || sky->filter == SVO_SKY_NEAREST);
    for (int f = 0; ok && f < 6; ++f) ok = sky->faces_dev[f] != nullptr;
    return ok;
}

inline SkyMap sky_map(const svo_sky &sky)
{
    SkyMap S;
    for (int f = 0; f < 6; ++f) S.faces[f] = sky.faces_dev[f];
    S.size = sky.size; S.filter = sky.filter;
    return S;
}

} // namespace svo
