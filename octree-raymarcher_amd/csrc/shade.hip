// shade.hip — the shading stage over the G-buffer: Blinn-Phong x 3 lights,
// shaders/World.Fragment.glsl:63-138,180-197, as one coalesced kernel (32 B read + 16 B written per pixel:
// HBM-bound).  Albedo from the material table (svo_shade) or from the caller's texture atlas at the hit's leafUV
// (svo_shade_textured, :5-15,178-182; svo_hit_uv hands that leafUV to callers with a sampler of their own) — see include/svo.h.
// svo_shade_reflections blends what the mirror rays of svo_trace_reflections saw into the image (reflect.hip.h; not in the reference).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "image_stage.hip.h"
#include "reflect.hip.h"
#include "sky_lookup.hip.h"

namespace svo {
namespace {

struct ShadeArgs {
    svo_shade_params P;
    PixelFrame frame;
    const uint4 *gbuffer;                       // (svo_shade_packed: svo_gbuffer_pack's uint2 records)
    float4 *rgba;
    // per-launch constants worked out once on the host with the same float expressions the per-pixel code used:
    float gdiffuse[8][3], gspecular[8][3];      // pow(material.diffuse / .specular, gamma), :183-184
    float dir_l[3], spot_axis[3];               // normalize(-directional.direction), normalize(-spot.direction)
    float inv_imgw, inv_imgh, inv_spot_delta, inv_near, inv_depth_range;    // 1/width, 1/height, 1/(cos_phi - cos_gamma), 1/near, 1/(1/far - 1/near)
};

__device__ __forceinline__ float dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// The shading stage is compared with a float64 model to 1e-6 + 2e-5 relative + 8 * 2^-23 * shininess * |specular term|
// (tests/test_shading_synthetic.py; the correctly rounded float32 oracle needs 1.76 in place of the 8), not bit for bit (powf
// already differs between glibc and the device), so reciprocals and inverse square roots are the hardware's 1-ulp instructions
// instead of IEEE division sequences: ~20 VALU less per normalisation, seven normalisations per pixel.
__device__ __forceinline__ float rcp_fast(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ V3 normalize_fast(V3 v) { return v * __builtin_amdgcn_rsqf(dot3(v, v)); }
__device__ __forceinline__ float maxf0(float x) { return (x < 0.0f) ? 0.0f : x; }          // max(x, 0.0)
__device__ __forceinline__ float attenuation(float kc, float kl, float kq, float d) { return rcp_fast(kc + kl * d + kq * d * d); }   // :75-78
// pow(x, y) for x in [0, 1], y >= 0 as exp2(y * log2(x)).  The exponent y * log2(x) must be good to ~1e-5 absolute
// wherever the result is not negligible, i.e. for |y * log2(x)| < 20: near x = 1 (the only place a shininess of 10000
// leaves anything) log2(x) comes from the series of ln(1 - d), d = 1 - x exact, relative error ~1e-7; elsewhere from the
// hardware's 1-ulp log2, whose absolute error (~1e-7) times y stays below 1e-5 for y <= 100 and is irrelevant above
// (the result underflows).  No library powf: three of them were a third of the kernel.
__device__ __forceinline__ float pow_shiny(float x, float y)
{
    if (y == 0.0f) return 1.0f;                                     // pow(x, 0) = 1, also for x = 0
    if (!(x > 0.0f)) return 0.0f;
    const float d = 1.0f - x;
    const float series = -(d + d * d * (0.5f + d * (0.33333334f + d * 0.25f))) * 1.44269504f;       // log2(1 - d), d < 1/64
    const float l2 = d < 0.015625f ? series : __builtin_amdgcn_logf(x);
    return __builtin_amdgcn_exp2f(y * l2);
}
__device__ __forceinline__ int material_index(uint32_t material) { return material < 8 ? (int)material : 0; }

// {r, g, b, depth} of the record h (a hit: SVO_HIT_FLAG) of a ray from `eye` along the unit vector `beta`, with its gamma-decoded
// albedo (:181-182) - the body of every shading kernel.  The shaded point is alpha + beta * (sigma - EPS), :174.
// MIRROR: the ray is a mirror ray (k_shade_reflections): the view vector is -beta whatever sigma is, and there is no depth.
template <bool MIRROR>
__device__ __forceinline__ float4 shade_ray(const ShadeArgs &A, V3 eye, V3 beta, const HitRecord &h, V3 diffuse, V3 specular)
{
    const svo_shade_params &P = A.P;
    const float sdist = h.t - P.eps;
    const V3 p = eye + beta * sdist;
    const float shininess = P.materials[material_index(h.material)].shininess;
    // (1.0 - shadow): the directional light's term for all three (:186-190), unless svo_trace_local_shadows gave each local light its own
    const float lit = (h.flags & SVO_SHADOWED) ? 0.0f : 1.0f;
    const bool local = (h.flags & SVO_LOCAL_SHADOWS) != 0u;
    const float lit_point = local ? ((h.flags & SVO_SHADOWED_POINT) ? 0.0f : 1.0f) : lit;
    const float lit_spot = local ? ((h.flags & SVO_SHADOWED_SPOT) ? 0.0f : 1.0f) : lit;
    // normalize(eye - p) = -beta and |p - eye| = sigma - EPS (beta is a unit vector) while the hit lies in front of the eye
    const bool front = MIRROR || sdist > 1.0e-3f;
    const V3 vdir = front ? mk(-beta.x, -beta.y, -beta.z) : normalize_fast(eye - p);
    const float zdist = front ? sdist : sqrtf(dot3(p - eye, p - eye));
    V3 color = mk(0.0f, 0.0f, 0.0f);
    {   // computePointLight_BlinnPhong, :80-97
        const V3 lv = ld3(P.point.position) - p;
        const float l2 = dot3(lv, lv), il = __builtin_amdgcn_rsqf(l2);
        const V3 l = lv * il;
        const V3 hv = normalize_fast(l + vdir);
        const float d = maxf0(dot3(h.n, l));
        const float s = pow_shiny(maxf0(dot3(vdir, hv)), shininess);
        const float att = attenuation(P.point.constant, P.point.linear, P.point.quadratic, l2 * il);     // |p - position| = l2 / sqrt(l2)
        const V3 amb = ld3(P.point.ambient) * diffuse;
        const V3 dif = ((ld3(P.point.diffuse) * d) * diffuse) * lit_point;
        const V3 spe = ((ld3(P.point.specular) * s) * specular) * lit_point;
        color = color + ((amb + dif) + spe) * att;
    }
    {   // computeDirectionalLight_BlinnPhong, :99-114
        const V3 l = ld3(A.dir_l);
        const V3 hv = normalize_fast(l + vdir);
        const float d = maxf0(dot3(h.n, l));
        const float s = pow_shiny(maxf0(dot3(vdir, hv)), shininess);
        const V3 amb = ld3(P.directional.ambient) * diffuse;
        const V3 dif = ((ld3(P.directional.diffuse) * d) * diffuse) * lit;
        const V3 spe = ((ld3(P.directional.specular) * s) * specular) * lit;
        color = color + ((amb + dif) + spe);
    }
    {   // computeSpotlight_BlinnPhong, :116-138
        const V3 lv = ld3(P.spot.position) - p;
        const float l2 = dot3(lv, lv), il = __builtin_amdgcn_rsqf(l2);
        const V3 l = lv * il;
        const V3 hv = normalize_fast(l + vdir);
        const float d = maxf0(dot3(h.n, l));
        const float s = pow_shiny(maxf0(dot3(vdir, hv)), shininess);
        const float att = attenuation(P.spot.constant, P.spot.linear, P.spot.quadratic, l2 * il);
        const float theta = dot3(l, ld3(A.spot_axis));
        float intensity = (theta - P.spot.cos_gamma) * A.inv_spot_delta;
        intensity = (intensity < 0.0f) ? 0.0f : intensity;                      // clamp = min(max(x, 0), 1)
        intensity = (1.0f < intensity) ? 1.0f : intensity;
        const V3 amb = ld3(P.spot.ambient) * diffuse;
        const V3 dif = ((ld3(P.spot.diffuse) * d) * diffuse) * lit_spot;
        const V3 spe = ((ld3(P.spot.specular) * s) * specular) * lit_spot;
        color = color + (amb + (dif + spe) * intensity) * att;
    }
    return make_float4(color.x, color.y, color.z, MIRROR ? 0.0f : (rcp_fast(zdist) - A.inv_near) * A.inv_depth_range);     // :193-197
}

// One pixel's {r, g, b, depth} from its record: shade_ray along the ray of this pixel (same generation as the march)
__device__ __forceinline__ float4 shade_hit(const ShadeArgs &A, int64_t k, const HitRecord &h, V3 diffuse, V3 specular)
{
    const FrameCam &cam = A.frame.cam;
    // (not PixelFrame::ray: the host-made reciprocals and normalize_fast above, within this stage's tolerance and not bit for bit)
    int px, py;
    A.frame.pixel(k, px, py);
    const float fx = (float)px + 0.5f, fy = (float)py + 0.5f;
    const float u = ((fx * A.inv_imgw) * 2.0f - 1.0f) * cam.tanx;
    const float v = (1.0f - (fy * A.inv_imgh) * 2.0f) * cam.tany;
    const V3 beta = normalize_fast((ld3(cam.fwd) + ld3(cam.right) * u) + ld3(cam.up) * v);
    return shade_ray<false>(A, ld3(cam.eye), beta, h, diffuse, specular);
}

// svo_shade's albedo: the material table's (:183-184 with the table in the atlas's place)
__device__ __forceinline__ float4 shade_hit(const ShadeArgs &A, int64_t k, const HitRecord &h)
{
    const int mi = material_index(h.material);
    return shade_hit(A, k, h, ld3(A.gdiffuse[mi]), ld3(A.gspecular[mi]));
}

// PACKED: the G-buffer is the 8-byte form of svo_gbuffer_pack (8 B read + 16 B written per pixel instead of 32 + 16)
template <bool PACKED>
__global__ __launch_bounds__(256) void k_shade(ShadeArgs A)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= A.frame.count()) return;
    const HitRecord h = PACKED ? load_packed(reinterpret_cast<const uint2 *>(A.gbuffer), k) : load_hit(A.gbuffer, k);
    if (!(h.flags & SVO_HIT_FLAG)) { A.rgba[k] = make_float4(0.0f, 0.0f, 0.0f, 1.0f); return; }     // discard
    A.rgba[k] = shade_hit(A, k, h);
}

// svo_shade_translucent (shaders/ParallaxAlpha.Fragment.glsl:315-323): surface colour C_s, colour C_b of the behind record at the
// eye distance t1 + t2, blended by s = clamp(t2 * absorption, 0, 1); depth is C_b's.  A.gbuffer is the surface, `behind` the
// continuation records.
__global__ __launch_bounds__(256) void k_shade_translucent(ShadeArgs A, const uint4 *behind, float absorption)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= A.frame.count()) return;
    const HitRecord hs = load_hit(A.gbuffer, k);
    if (!(hs.flags & SVO_HIT_FLAG)) { A.rgba[k] = make_float4(0.0f, 0.0f, 0.0f, 1.0f); return; }
    const float4 cs = shade_hit(A, k, hs);
    HitRecord hb = load_hit(behind, k);
    if (!(hs.flags & SVO_SEE_THROUGH) || !(hb.flags & SVO_HIT_FLAG)) { A.rgba[k] = cs; return; }
    const float t2 = hb.t;
    hb.t = hs.t + t2;
    const float4 cb = shade_hit(A, k, hb);
    float s = t2 * absorption;
    s = (s < 0.0f) ? 0.0f : s;
    s = (1.0f < s) ? 1.0f : s;
    const float r = 1.0f - s;
    A.rgba[k] = make_float4(cb.x * r + cs.x * s, cb.y * r + cs.y * s, cb.z * r + cs.z * s, cb.w);
}

// svo_shade_textured: the caller's atlas (RGB8, rows tightly packed, row 0 at v = 0) and the 256 values a texel byte decodes to
struct AtlasArgs {
    const uint8_t *diffuse, *specular;
    int32_t width, height;
    float decode[256];                          // pow(byte / 255, gamma), made on the host like gdiffuse
};

// texture(sampler, uv) of a GL_NEAREST, GL_REPEAT sampler
__device__ __forceinline__ V3 atlas_texel(const AtlasArgs &T, const uint8_t *image, float u, float v)
{
    const int x = max(min((int)floorf((u - floorf(u)) * (float)T.width), T.width - 1), 0);       // (the max: a NaN uv reads texel 0, never out of range)
    const int y = max(min((int)floorf((v - floorf(v)) * (float)T.height), T.height - 1), 0);
    const uint8_t *px = image + ((size_t)y * (size_t)T.width + (size_t)x) * 3;
    return mk(T.decode[px[0]], T.decode[px[1]], T.decode[px[2]]);
}

// k_shade with the albedo of :178-182: the two atlases sampled at the hit's leafUV (image_stage.hip.h hit_uv, separately rounded IEEE
// operations: the texel is the reference's).  `voxels`: the records svo_hit_voxels wrote for A.gbuffer; a hit without a box gets
// the material table's albedo.
__global__ __launch_bounds__(256) void k_shade_textured(ShadeArgs A, const uint4 *voxels, AtlasArgs T)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= A.frame.count()) return;
    const HitRecord h = load_hit(A.gbuffer, k);
    if (!(h.flags & SVO_HIT_FLAG)) { A.rgba[k] = make_float4(0.0f, 0.0f, 0.0f, 1.0f); return; }
    float u, v;
    if (!hit_uv(A.frame, k, A.P.eps, h, voxels[2 * k], voxels[2 * k + 1], u, v)) { A.rgba[k] = shade_hit(A, k, h); return; }
    A.rgba[k] = shade_hit(A, k, h, atlas_texel(T, T.diffuse, u, v), atlas_texel(T, T.specular, u, v));
}

// svo_hit_uv: that leafUV per pixel, (0, 0) where there is none
__global__ __launch_bounds__(256) void k_hit_uv(PixelFrame F, float eps, const uint4 *gbuffer, const uint4 *voxels, float2 *uv)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= F.count()) return;
    float u, v;
    hit_uv(F, k, eps, load_hit(gbuffer, k), voxels[2 * k], voxels[2 * k + 1], u, v);
    uv[k] = make_float2(u, v);
}

// ---- packed G-buffer -------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t axis_code(float v) { return v < 0.0f ? 0u : (v > 0.0f ? 2u : 1u); }

__global__ __launch_bounds__(256) void k_gbuffer_pack(const uint4 *in, uint2 *out, int64_t n)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const uint4 r0 = in[2 * k], r1 = in[2 * k + 1];
    const float nx = __uint_as_float(r0.y), ny = __uint_as_float(r0.z), nz = __uint_as_float(r0.w);
    const bool nan = (nx != nx) | (ny != ny) | (nz != nz);
    const uint32_t code = nan ? (1u << 6) : (axis_code(nx) | (axis_code(ny) << 2) | (axis_code(nz) << 4));
    uint2 o;
    o.x = r0.x;
    const uint32_t flags = r1.x >> 16;
    o.y = (r1.x & 0xFFFFu) | ((flags & 0xFFu) << 16) | (code << 24) | ((flags & SVO_ERR_FLAG) ? 1u << 31 : 0u);
    out[k] = o;
}

__global__ __launch_bounds__(256) void k_gbuffer_unpack(const uint2 *in, uint4 *out, int64_t n)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const uint2 p = in[k];
    const uint32_t code = (p.y >> 24) & 0x7Fu, flags = ((p.y >> 16) & 0xFFu) | ((p.y >> 31) ? (uint32_t)SVO_ERR_FLAG : 0u);
    const V3 nrm = (flags & SVO_HIT_FLAG) ? normal_from_code(code) : mk(0.0f, 0.0f, 0.0f);
    uint4 a, b;
    a.x = p.x; a.y = __float_as_uint(nrm.x); a.z = __float_as_uint(nrm.y); a.w = __float_as_uint(nrm.z);
    b.x = (p.y & 0xFFFFu) | (flags << 16); b.y = 0u; b.z = 0u; b.w = 0u;
    out[2 * k] = a;
    out[2 * k + 1] = b;
}

// svo_shade_ao: r, g and b scaled by f = 1 - strength * (1 - ao); the depth float is not written, and neither is a pixel whose f is
// exactly 1 (ao == 1, strength == 0) or NaN (a NaN ao)
__global__ __launch_bounds__(256) void k_shade_ao(const float *ao, float strength, int64_t n, float4 *rgba)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const float f = 1.0f - strength * (1.0f - ao[k]);
    if (f == 1.0f || f != f) return;
    float *px = reinterpret_cast<float *>(rgba + k);
    px[0] = px[0] * f; px[1] = px[1] * f; px[2] = px[2] * f;
}

// svo_shade_reflections: what a mirror pixel's ray saw, blended over the pixel by the reflectance F.  A.gbuffer and `voxels` are the
// records the ray list was made from - mirror_ray() rebuilds the ray that was marched -, `reflect` what the march wrote for it.
struct MirrorArgs {
    uint32_t material;
    float f0;
    int32_t fresnel, has_sky;
    float background[3];
    SkyMap sky;
};

__global__ __launch_bounds__(256) void k_shade_reflections(ShadeArgs A, MirrorArgs M, const uint4 *voxels, const uint4 *reflect)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= A.frame.count()) return;
    V3 O, R;
    float c;
    if (!mirror_ray(A.frame, k, A.P.eps, M.material, A.gbuffer, voxels, O, R, c)) return;
    const float x = 1.0f - c;
    const float F = M.fresnel ? M.f0 + (1.0f - M.f0) * (((x * x) * (x * x)) * x) : M.f0;        // Schlick
    if (F == 0.0f) return;
    const HitRecord h = load_hit(reflect, k);
    V3 C = ld3(M.background);
    if (h.flags & SVO_HIT_FLAG) {
        const int mi = material_index(h.material);
        const float4 s = shade_ray<true>(A, O, R, h, ld3(A.gdiffuse[mi]), ld3(A.gspecular[mi]));      // (R is d with one sign flipped: a unit vector)
        C = mk(s.x, s.y, s.z);
    } else if (M.has_sky) {
        sky_lookup(M.sky, R, C);                // (no answer: C stays the background)
    }
    const float keep = 1.0f - F;
    float *px = reinterpret_cast<float *>(A.rgba + k);
    px[0] = px[0] * keep + C.x * F; px[1] = px[1] * keep + C.y * F; px[2] = px[2] * keep + C.z * F;
}

// svo_shade_lights: computePointLight_BlinnPhong (:80-97, the point-light block of shade_ray) for every light of a list, each windowed
// to its reach and with its own bit of the pixel's word for the shadow factor, added to the pixel.  A pixel no light reaches is not written.
struct ListLights {
    svo_light light[SVO_MAX_LIGHTS];
    float inv_reach[SVO_MAX_LIGHTS];            // 1 / reach, made on the host
    int32_t count;
};

__global__ __launch_bounds__(256) void k_shade_lights(ShadeArgs A, ListLights L, const uint32_t *visible)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= A.frame.count()) return;
    const HitRecord h = load_hit(A.gbuffer, k);
    if (!(h.flags & SVO_HIT_FLAG)) return;
    const FrameCam &cam = A.frame.cam;
    int px, py;
    A.frame.pixel(k, px, py);                   // the ray as shade_hit makes it, the point and the view vector as shade_ray does
    const float fx = (float)px + 0.5f, fy = (float)py + 0.5f;
    const float u = ((fx * A.inv_imgw) * 2.0f - 1.0f) * cam.tanx;
    const float v = (1.0f - (fy * A.inv_imgh) * 2.0f) * cam.tany;
    const V3 eye = ld3(cam.eye), beta = normalize_fast((ld3(cam.fwd) + ld3(cam.right) * u) + ld3(cam.up) * v);
    const float sdist = h.t - A.P.eps;
    const V3 p = eye + beta * sdist;
    const V3 vdir = sdist > 1.0e-3f ? mk(-beta.x, -beta.y, -beta.z) : normalize_fast(eye - p);
    const int mi = material_index(h.material);
    const float shininess = A.P.materials[mi].shininess;
    const V3 diffuse = ld3(A.gdiffuse[mi]), specular = ld3(A.gspecular[mi]);
    const uint32_t word = visible ? visible[k] : 0xFFFFFFFFu;
    V3 sum = mk(0.0f, 0.0f, 0.0f);
    bool reached = false;
    for (int j = 0; j < L.count; ++j) {
        const svo_light &Lj = L.light[j];
        const V3 lv = ld3(Lj.position) - p;
        const float l2 = dot3(lv, lv), il = __builtin_amdgcn_rsqf(l2), dist = l2 * il;
        if (!(dist > 0.0f) || !(dist < Lj.reach)) continue;         // (l2 == 0 or inf: dist is NaN)
        reached = true;
        const V3 l = lv * il;
        const V3 hv = normalize_fast(l + vdir);
        const float d = maxf0(dot3(h.n, l));
        const float s = pow_shiny(maxf0(dot3(vdir, hv)), shininess);
        const float x = dist * L.inv_reach[j], x2 = x * x;
        float win = 1.0f - x2 * x2;
        win = (win < 0.0f) ? 0.0f : win;
        win = (1.0f < win) ? 1.0f : win;
        const float att = (win * win) * attenuation(Lj.constant, Lj.linear, Lj.quadratic, dist);
        const float vis = ((word >> j) & 1u) ? 1.0f : 0.0f;
        const V3 amb = ld3(Lj.ambient) * diffuse;
        const V3 dif = ((ld3(Lj.diffuse) * d) * diffuse) * vis;
        const V3 spe = ((ld3(Lj.specular) * s) * specular) * vis;
        sum = sum + ((amb + dif) + spe) * att;
    }
    if (!reached) return;
    float *out = reinterpret_cast<float *>(A.rgba + k);
    out[0] = out[0] + sum.x; out[1] = out[1] + sum.y; out[2] = out[2] + sum.z;
}

} // namespace
} // namespace svo

using namespace svo;

extern "C" {

void svo_shade_defaults(svo_shade_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    auto set3 = [](float *d, float x, float y, float z) { d[0] = x; d[1] = y; d[2] = z; };
    // src/Main.cpp:101-109
    set3(p->point.position, 50, 8, 65); set3(p->point.ambient, 0.1f, 0.1f, 0.1f); set3(p->point.diffuse, 0.5f, 0.5f, 0.5f); set3(p->point.specular, 1, 1, 1);
    p->point.constant = 1.0f; p->point.linear = 0.14f; p->point.quadratic = 0.09f;
    // :114-119
    const float inv = 1.0f / std::sqrt(2.0f);
    set3(p->directional.position, 250, 125, 250); set3(p->directional.direction, inv, -inv, 0.0f);
    set3(p->directional.ambient, 0.2f, 0.3f, 0.4f); set3(p->directional.diffuse, 0.3f, 0.3f, 0.6f); set3(p->directional.specular, 0, 0, 0);
    // :121-131
    const float sl = 1.0f / std::sqrt(0.01f + 1.0f + 0.01f);
    set3(p->spot.position, 50, 20, 70); set3(p->spot.direction, -0.1f * sl, -1.0f * sl, -0.1f * sl);
    set3(p->spot.ambient, 0.2f, 0.8f, 0.3f); set3(p->spot.diffuse, 0.2f, 0.8f, 0.3f); set3(p->spot.specular, 1, 1, 1);
    p->spot.cos_phi = (float)std::cos(25.0 * 3.14159265358979323846 / 180.0);
    p->spot.cos_gamma = (float)std::cos(35.0 * 3.14159265358979323846 / 180.0);
    p->spot.constant = 1.0f; p->spot.linear = 0.045f; p->spot.quadratic = 0.0075f;
    // ML[8], shaders/World.Fragment.glsl:63-73
    const float ml[8][10] = {
        { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 }, { .8f, .8f, .8f, .8f, .8f, .8f, .5f, .5f, .5f, 8 }, { .8f, .8f, .8f, .6f, .6f, .6f, .1f, .1f, .1f, 16 },
        { .8f, .8f, .8f, .7f, .7f, .7f, .15f, .15f, .15f, 32 }, { .8f, .8f, .8f, .9f, .9f, .9f, .7f, .7f, .7f, 10000 },
        { .8f, .8f, .8f, .5f, .5f, .5f, 0, 0, 0, 0 }, { .8f, .8f, .8f, .4f, .4f, .4f, 1, 1, 1, 100 }, { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 } };
    for (int i = 0; i < 8; ++i) {
        std::memcpy(p->materials[i].ambient, &ml[i][0], 12); std::memcpy(p->materials[i].diffuse, &ml[i][3], 12);
        std::memcpy(p->materials[i].specular, &ml[i][6], 12); p->materials[i].shininess = ml[i][9];
    }
    p->eps = 1.0f / 8192.0f; p->gamma = 2.2f; p->near_plane = 0.125f; p->far_plane = 8192.0f;
}

static int pack_common(const void *in, void *out, int64_t n, void *stream, bool pack)
{
    if (n < 0 || (n > 0 && (!in || !out))) { set_error("svo_gbuffer_pack/unpack: bad argument"); return SVO_ERR_INVALID_ARG; }
    const char *who = "svo_gbuffer_pack/unpack";
    if (pack) return launch_per_element(who, n, (hipStream_t)stream, k_gbuffer_pack, (const uint4 *)in, (uint2 *)out, n);
    return launch_per_element(who, n, (hipStream_t)stream, k_gbuffer_unpack, (const uint2 *)in, (uint4 *)out, n);
}

int svo_gbuffer_pack(const svo_hit *gbuffer_dev, uint64_t *packed_dev, int64_t n, void *stream) { return pack_common(gbuffer_dev, packed_dev, n, stream, true); }
int svo_gbuffer_unpack(const uint64_t *packed_dev, svo_hit *gbuffer_dev, int64_t n, void *stream) { return pack_common(packed_dev, gbuffer_dev, n, stream, false); }

// What every shade call shares: the argument check and A - the frame, the parameters with their defaults filled in, the per-launch
// constants, the records and the image.  The caller launches its own kernel over A.frame.count() pixels.
static int shade_args(const svo_camera *cam, const svo_shade_params *p, int x0, int y0, int w, int h, const void *gbuffer_dev, float *rgba_dev, ShadeArgs &A)
{
    if (!p || !gbuffer_dev || !rgba_dev || !rect_ok(cam, x0, y0, w, h)) { set_error("svo_shade: bad argument"); return SVO_ERR_INVALID_ARG; }
    A.P = *p;
    if (A.P.eps == 0.0f) A.P.eps = 1.0f / 8192.0f;
    if (A.P.gamma == 0.0f) A.P.gamma = 2.2f;
    if (A.P.near_plane == 0.0f) A.P.near_plane = 0.125f;
    if (A.P.far_plane == 0.0f) A.P.far_plane = 8192.0f;
    A.frame = make_frame(*cam, x0, y0, w, h);
    for (int m = 0; m < 8; ++m)
        for (int c = 0; c < 3; ++c) {
            A.gdiffuse[m][c] = std::pow(A.P.materials[m].diffuse[c], A.P.gamma);
            A.gspecular[m][c] = std::pow(A.P.materials[m].specular[c], A.P.gamma);
        }
    auto unit_neg = [](const float v[3], float out[3]) {          // glm::normalize(-v) = -v * (1 / sqrt(dot))
        const float x = -v[0], y = -v[1], z = -v[2];
        const float inv = 1.0f / std::sqrt(x * x + y * y + z * z);
        out[0] = x * inv; out[1] = y * inv; out[2] = z * inv;
    };
    unit_neg(A.P.directional.direction, A.dir_l);
    unit_neg(A.P.spot.direction, A.spot_axis);
    A.inv_imgw = 1.0f / (float)cam->width; A.inv_imgh = 1.0f / (float)cam->height;
    A.inv_spot_delta = 1.0f / (A.P.spot.cos_phi - A.P.spot.cos_gamma);
    A.inv_near = 1.0f / A.P.near_plane;
    A.inv_depth_range = 1.0f / (1.0f / A.P.far_plane - 1.0f / A.P.near_plane);
    A.gbuffer = reinterpret_cast<const uint4 *>(gbuffer_dev);
    A.rgba = reinterpret_cast<float4 *>(rgba_dev);
    return SVO_OK;
}

int svo_shade(const svo_camera *cam, const svo_shade_params *p, int x0, int y0, int w, int h,
              const svo_hit *gbuffer_dev, float *rgba_dev, void *stream)
{
    ShadeArgs A;
    if (const int rc = shade_args(cam, p, x0, y0, w, h, gbuffer_dev, rgba_dev, A)) return rc;
    return launch_per_element("svo_shade", A.frame.count(), (hipStream_t)stream, k_shade<false>, A);
}

int svo_shade_packed(const svo_camera *cam, const svo_shade_params *p, int x0, int y0, int w, int h,
                     const uint64_t *packed_dev, float *rgba_dev, void *stream)
{
    ShadeArgs A;
    if (const int rc = shade_args(cam, p, x0, y0, w, h, packed_dev, rgba_dev, A)) return rc;
    return launch_per_element("svo_shade", A.frame.count(), (hipStream_t)stream, k_shade<true>, A);
}

int svo_shade_translucent(const svo_camera *cam, const svo_shade_params *p, float absorption, int x0, int y0, int w, int h,
                          const svo_hit *surface_dev, const svo_hit *behind_dev, float *rgba_dev, void *stream)
{
    if (!behind_dev || !(absorption >= 0.0f)) { set_error("svo_shade_translucent: bad argument"); return SVO_ERR_INVALID_ARG; }
    ShadeArgs A;
    if (const int rc = shade_args(cam, p, x0, y0, w, h, surface_dev, rgba_dev, A)) return rc;
    return launch_per_element("svo_shade", A.frame.count(), (hipStream_t)stream, k_shade_translucent, A, reinterpret_cast<const uint4 *>(behind_dev),
                              absorption == 0.0f ? 0.5f : absorption);
}

int svo_shade_textured(const svo_camera *cam, const svo_shade_params *p, const svo_atlas *atlas, int x0, int y0, int w, int h,
                       const svo_hit *gbuffer_dev, const svo_voxel *voxels_dev, float *rgba_dev, void *stream)
{
    if (!atlas || !atlas->diffuse_dev || atlas->width <= 0 || atlas->height <= 0 || !voxels_dev) { set_error("svo_shade_textured: bad argument"); return SVO_ERR_INVALID_ARG; }
    ShadeArgs A;
    if (const int rc = shade_args(cam, p, x0, y0, w, h, gbuffer_dev, rgba_dev, A)) return rc;
    AtlasArgs T;
    T.diffuse = atlas->diffuse_dev; T.specular = atlas->specular_dev ? atlas->specular_dev : atlas->diffuse_dev;      // src/Atlas.cpp:31-32
    T.width = atlas->width; T.height = atlas->height;
    for (int v = 0; v < 256; ++v) T.decode[v] = std::pow((float)v / 255.0f, A.P.gamma);
    return launch_per_element("svo_shade", A.frame.count(), (hipStream_t)stream, k_shade_textured, A, reinterpret_cast<const uint4 *>(voxels_dev), T);
}

// leafUV per pixel (image_stage.hip.h hit_uv) from the G-buffer and the records svo_hit_voxels wrote for it
int svo_hit_uv(const svo_camera *cam, float eps, int x0, int y0, int rw, int rh, const svo_hit *gbuffer_dev, const svo_voxel *voxels_dev,
               float *uv_dev, void *stream)
{
    if (!gbuffer_dev || !voxels_dev || !uv_dev || !rect_ok(cam, x0, y0, rw, rh) || !(eps >= 0.0f)) { set_error("svo_hit_uv: bad argument"); return SVO_ERR_INVALID_ARG; }
    return launch_per_element("svo_hit_uv", (int64_t)rw * rh, (hipStream_t)stream, k_hit_uv, make_frame(*cam, x0, y0, rw, rh),
                              eps == 0.0f ? 1.0f / 8192.0f : eps, reinterpret_cast<const uint4 *>(gbuffer_dev), reinterpret_cast<const uint4 *>(voxels_dev),
                              reinterpret_cast<float2 *>(uv_dev));
}

// The ambient-occlusion factor of svo_hit_ao over an image a shade call has written
int svo_shade_ao(const float *ao_dev, float strength, int64_t n, float *rgba_dev, void *stream)
{
    if (!(strength >= 0.0f && strength <= 1.0f) || n < 0 || (n > 0 && (!ao_dev || !rgba_dev))) { set_error("svo_shade_ao: bad argument"); return SVO_ERR_INVALID_ARG; }
    return launch_per_element("svo_shade_ao", n, (hipStream_t)stream, k_shade_ao, ao_dev, strength, n, reinterpret_cast<float4 *>(rgba_dev));
}

// Mirror reflections over an image a shade call has written: svo_trace_reflections' records shaded along their mirror rays
int svo_shade_reflections(const svo_camera *cam, const svo_shade_params *p, const svo_mirror *mirror, int x0, int y0, int w, int h,
                          const svo_hit *gbuffer_dev, const svo_voxel *voxels_dev, const svo_hit *reflect_dev, float *rgba_dev, void *stream)
{
    const auto refuse = [](const char *what) { set_error(std::string("svo_shade_reflections: ") + what); return SVO_ERR_INVALID_ARG; };
    if (!p || !mirror || !rect_ok(cam, x0, y0, w, h)) return refuse("bad camera, params, mirror or rectangle");
    const int64_t n = (int64_t)w * h;
    if (n > 0 && (!gbuffer_dev || !voxels_dev || !reflect_dev || !rgba_dev)) return refuse("NULL buffer");
    if (!(mirror->f0 >= 0.0f && mirror->f0 <= 1.0f) || mirror->material > 0xFFFFu) return refuse("f0 is in [0, 1], material a 16-bit material");
    for (int c = 0; c < 3; ++c) if (!std::isfinite(mirror->background[c])) return refuse("the background is not finite");
    if (mirror->sky && !sky_ok(mirror->sky)) return refuse("bad sky");
    if (n == 0) return SVO_OK;
    ShadeArgs A;
    if (const int rc = shade_args(cam, p, x0, y0, w, h, gbuffer_dev, rgba_dev, A)) return rc;
    MirrorArgs M;
    std::memset(&M, 0, sizeof M);
    M.material = mirror->material; M.f0 = mirror->f0; M.fresnel = mirror->fresnel != 0;
    std::memcpy(M.background, mirror->background, sizeof M.background);
    if (mirror->sky) { M.has_sky = 1; M.sky = sky_map(*mirror->sky); }
    return launch_per_element("svo_shade_reflections", n, (hipStream_t)stream, k_shade_reflections, A, M, reinterpret_cast<const uint4 *>(voxels_dev),
                              reinterpret_cast<const uint4 *>(reflect_dev));
}

// The lights of a list (svo_trace_lights' words for their shadow factors) added to an image a shade call has written
int svo_shade_lights(const svo_camera *cam, const svo_shade_params *p, const svo_light *lights, int nlights, int x0, int y0, int w, int h,
                     const svo_hit *gbuffer_dev, const uint32_t *visible_dev, float *rgba_dev, void *stream)
{
    if (!lights || nlights < 1 || nlights > SVO_MAX_LIGHTS) { set_error("svo_shade_lights: between 1 and 32 lights"); return SVO_ERR_INVALID_ARG; }
    ShadeArgs A;
    if (const int rc = shade_args(cam, p, x0, y0, w, h, gbuffer_dev, rgba_dev, A)) return rc;
    ListLights L;
    std::memset(&L, 0, sizeof L);
    std::memcpy(L.light, lights, (size_t)nlights * sizeof(svo_light));
    for (int j = 0; j < nlights; ++j) L.inv_reach[j] = 1.0f / lights[j].reach;
    L.count = nlights;
    return launch_per_element("svo_shade_lights", A.frame.count(), (hipStream_t)stream, k_shade_lights, A, L, visible_dev);
}

} // extern "C"
