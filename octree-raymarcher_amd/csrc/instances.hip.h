// instances.hip.h — up to 32 placements of one voxel model in a frame (svo_trace_instances) and their shadows
// (svo_trace_instance_shadows).
//
// Not in the reference, whose only moving object is a rasterised mesh (src/Worm.cpp).  The pattern of light_list.hip.h with another
// item: a pixel and an instance are a PAIR where the pixel's ray, taken into the instance's space, meets the model world's box in
// front of what the frame already holds.  The pairs are ranked instance-major by light_list.hip.h's ballot ranking (an instance
// takes a light's place: one bit of the pixel's mask), so nothing per pair is stored:
//   k_inst_cull      per pixel the 32-bit pair mask, per block of 256 pixels and instance the number of pairs
//   (device scan)    exclusive sum over the [instance][block] counts; k_light_total: how many pairs there are
//   k_inst_emit      the rank of every pair again; its ray in MODEL space (and, stage 1, its far end) into its slot
//   (ray-list march) ONE launch of `cap` rays on the MODEL world
//   k_inst_resolve   stage 1: the nearest usable record of a pixel's pairs, taken back to the world, into merged / owner
//   k_inst_fold      stage 2: SVO_SHADOW_TRACED / SVO_SHADOWED from the model list's records and the scene list's
// The march kernels are not changed.  Like march.hip.h this is compiled with -ffp-contract=off: every float operation below is
// separately rounded, and tests/instances_model.py repeats them in numpy float32.
#pragma once
#include "light_list.hip.h"

namespace svo {

constexpr int MAX_INSTANCES = 32;       // SVO_MAX_INSTANCES: one bit of the mask each
static_assert(MAX_INSTANCES == MAX_LIGHTS, "the ranking's shared words are sized for MAX_LIGHTS items");
struct InstanceList {
    float rot[MAX_INSTANCES][9];        // R, row-major, model -> world
    float pos[MAX_INSTANCES][3];
    float scale[MAX_INSTANCES], inv[MAX_INSTANCES];    // inv = 1.0f / scale, rounded once on the host
    float bmin[3], bmax[3];             // the model world's box
    int32_t count;
};

// (o, d) in instance j's space: om = R^T (o - pos) * inv, dm = R^T d, each sum left to right; dm is not re-normalised, so a
// distance along the model ray is the world's times inv
__device__ __forceinline__ void to_model(const InstanceList &I, int j, V3 o, V3 d, V3 &om, V3 &dm)
{
    const float *R = I.rot[j];
    const V3 u = o - ld3(I.pos[j]);
    const float inv = I.inv[j];
    om = mk((R[0] * u.x + R[3] * u.y + R[6] * u.z) * inv, (R[1] * u.x + R[4] * u.y + R[7] * u.z) * inv, (R[2] * u.x + R[5] * u.y + R[8] * u.z) * inv);
    dm = mk(R[0] * d.x + R[3] * d.y + R[6] * d.z, R[1] * d.x + R[4] * d.y + R[7] * d.z, R[2] * d.x + R[5] * d.y + R[8] * d.z);
}

// The box rule (include/svo.h, svo_trace_instances step 2): true where the ray misses the model's box, else tn = where it enters
// (0 from inside).  A NaN compares false and bounds nothing.
__device__ __forceinline__ bool box_missed(const InstanceList &I, V3 om, V3 dm, float &tn)
{
    tn = 0.0f;
    float tf = INFINITY;
    for (int a = 0; a < 3; ++a) {
        const float o = axis_of(om, a), g = axis_of(dm, a), lo = I.bmin[a], hi = I.bmax[a];
        if (g == 0.0f) {
            if (!(lo <= o && o <= hi)) return true;
            continue;
        }
        const float r = 1.0f / g;
        float t0 = (lo - o) * r, t1 = (hi - o) * r;
        if (t1 < t0) { const float s = t0; t0 = t1; t1 = s; }
        if (t0 > tn) tn = t0;
        if (t1 < tf) tf = t1;
    }
    return tn > tf;
}

// The world ray a stage takes into the instances' spaces for pixel k, and whether a world distance `end` ends it; false where the
// pixel has none.  Stage 1 (SHADOW = false): the camera ray, ended by a usable record of `records` (the G-buffer).
// Stage 2: (P, S) of a CONSIDERED pixel - a usable record of `records` (merged) without SVO_SHADOWED -, P = o + d * (t - bias).
template <bool SHADOW>
__device__ __forceinline__ bool instance_ray(const PixelFrame &F, int64_t k, float bias, V3 S, const uint4 *records, V3 &o, V3 &d, bool &ended, float &end)
{
    const uint32_t flags = record_flags(records, k);
    ended = false; end = 0.0f;
    if (SHADOW) {
        if (!usable_hit(flags) || (flags & SVO_SHADOWED)) return false;
        o = local_sample_point(F, k, __uint_as_float(records[2 * k].x), bias);
        d = S;
        return true;
    }
    F.ray(k, o, d);
    if (usable_hit(flags)) { ended = true; end = __uint_as_float(records[2 * k].x); }
    return true;
}

// Pixel k's pair mask: bit j where the ray does not miss instance j's box and enters it before its far end, far = end * inv or +inf
template <bool SHADOW>
__device__ __forceinline__ uint32_t instance_pairs(const InstanceList &I, V3 o, V3 d, bool ended, float end)
{
    uint32_t mask = 0u;
#pragma unroll 1                                             // (unrolled, stage 1's cull takes 163 VGPRs: 3 waves per SIMD instead of 8)
    for (int j = 0; j < I.count; ++j) {
        V3 om, dm;
        float tn;
        to_model(I, j, o, d, om, dm);
        if (box_missed(I, om, dm, tn)) continue;
        if (SHADOW || tn < (ended ? end * I.inv[j] : INFINITY)) mask |= 1u << j;
    }
    return mask;
}

// Stage 2 writes the SCENE list here as well, one ray per pixel: (P, S) for a considered pixel that an instance owns, the ray that
// misses the scene for every other (svo_trace_reflections' padding).  Stage 1 passes no owner and no scene list.
template <bool SHADOW>
__global__ __launch_bounds__(256) void k_inst_cull(PixelFrame F, float bias, V3 S, InstanceList I, const uint4 *records, uint32_t *masks, uint32_t *counts, uint32_t nblocks,
                                                   const uint32_t *owner, V3 scene_miss, float *scene_origins, float *scene_dirs)
{
    __shared__ uint32_t sh[MAX_LIGHTS][LIGHT_WAVES];
    const int64_t k = (int64_t)blockIdx.x * LIGHT_BLOCK + threadIdx.x, n = F.count();
    uint32_t mask = 0u;
    if (k < n) {
        V3 o, d;
        float end;
        bool ended;
        const bool has = instance_ray<SHADOW>(F, k, bias, S, records, o, d, ended, end);
        if (has) mask = instance_pairs<SHADOW>(I, o, d, ended, end);
        masks[k] = mask;
        if (SHADOW) {
            if (!(has && owner[k] != 0u)) { o = scene_miss; d = mk(-1.0f, 0.0f, 0.0f); }
            scene_origins[3 * k] = o.x; scene_origins[3 * k + 1] = o.y; scene_origins[3 * k + 2] = o.z;
            scene_dirs[3 * k] = d.x; scene_dirs[3 * k + 1] = d.y; scene_dirs[3 * k + 2] = d.z;
        }
    }
    light_wave_counts(mask, I.count, sh);
    if ((int)threadIdx.x < I.count) {
        uint32_t tot = 0u;
        for (unsigned w = 0; w < LIGHT_WAVES; ++w) tot += sh[threadIdx.x][w];
        counts[(size_t)threadIdx.x * nblocks + blockIdx.x] = tot;
    }
}

// The model ray of every pair into its slot - stage 1 with its far end (tmax != null) -, and the ray that misses the MODEL, with a
// far end of 0, into the slots [total, cap)
template <bool SHADOW>
__global__ __launch_bounds__(256) void k_inst_emit(PixelFrame F, float bias, V3 S, InstanceList I, V3 miss, const uint4 *records, const uint32_t *masks, const uint32_t *base,
                                                   uint32_t nblocks, const uint32_t *total, uint32_t cap, float *origins, float *dirs, float *tmax)
{
    __shared__ uint32_t sh[MAX_LIGHTS][LIGHT_WAVES];
    const int64_t k = (int64_t)blockIdx.x * LIGHT_BLOCK + threadIdx.x, n = F.count();
    const uint32_t mask = k < n ? masks[k] : 0u;
    V3 o = mk(0.0f, 0.0f, 0.0f), d = o;
    float end = 0.0f;
    bool ended = false;
    if (mask) (void)instance_ray<SHADOW>(F, k, bias, S, records, o, d, ended, end);
    light_pairs(mask, I.count, base, nblocks, sh, [&](int j, uint32_t r) {
        if (r >= cap) return;                               // dropped
        V3 om, dm;
        to_model(I, j, o, d, om, dm);
        origins[3 * (size_t)r] = om.x; origins[3 * (size_t)r + 1] = om.y; origins[3 * (size_t)r + 2] = om.z;
        dirs[3 * (size_t)r] = dm.x; dirs[3 * (size_t)r + 1] = dm.y; dirs[3 * (size_t)r + 2] = dm.z;
        if (!SHADOW) tmax[r] = ended ? end * I.inv[j] : INFINITY;
    });
    const uint64_t stride = (uint64_t)nblocks * LIGHT_BLOCK;
    for (uint64_t r = (uint64_t)total[0] + (uint64_t)k; r < cap; r += stride) {
        origins[3 * r] = miss.x; origins[3 * r + 1] = miss.y; origins[3 * r + 2] = miss.z;
        dirs[3 * r] = -1.0f; dirs[3 * r + 1] = 0.0f; dirs[3 * r + 2] = 0.0f;
        if (!SHADOW) tmax[r] = 0.0f;
    }
}

// Stage 1's fold.  A pair HITS iff it has a slot and its record M is usable (the bounded march has applied M.t < far); its world
// distance is M.t * scale; the smallest wins, the lowest j among equals.  The winner's record goes to merged[k] with its normal
// taken to the world (R n, summed left to right) and owner[k] = j + 1; without one merged[k] = gbuffer[k] and owner[k] = 0.
__global__ __launch_bounds__(256) void k_inst_resolve(PixelFrame F, InstanceList I, const uint4 *gbuffer, const uint32_t *masks, const uint32_t *base, uint32_t nblocks,
                                                      uint32_t cap, const uint4 *rays, uint4 *merged, uint32_t *owner)
{
    __shared__ uint32_t sh[MAX_LIGHTS][LIGHT_WAVES];
    const int64_t k = (int64_t)blockIdx.x * LIGHT_BLOCK + threadIdx.x, n = F.count();
    const uint32_t mask = k < n ? masks[k] : 0u;
    int win = -1;
    uint32_t slot = 0u;
    float best = 0.0f;
    light_pairs(mask, I.count, base, nblocks, sh, [&](int j, uint32_t r) {
        if (r >= cap || !usable_hit(record_flags(rays, r))) return;
        const float tw = __uint_as_float(rays[2 * (size_t)r].x) * I.scale[j];
        if (win < 0 || tw < best) { win = j; slot = r; best = tw; }
    });
    if (k >= n) return;
    if (win < 0) {
        if (merged != gbuffer) { merged[2 * k] = gbuffer[2 * k]; merged[2 * k + 1] = gbuffer[2 * k + 1]; }
        owner[k] = 0u;
        return;
    }
    const uint4 m0 = rays[2 * (size_t)slot], m1 = rays[2 * (size_t)slot + 1];
    const float *R = I.rot[win];
    const V3 nm = mk(__uint_as_float(m0.y), __uint_as_float(m0.z), __uint_as_float(m0.w));
    const V3 nw = mk(R[0] * nm.x + R[1] * nm.y + R[2] * nm.z, R[3] * nm.x + R[4] * nm.y + R[5] * nm.z, R[6] * nm.x + R[7] * nm.y + R[8] * nm.z);
    const uint32_t flags = SVO_HIT_FLAG | ((m1.x >> 16) & SVO_FACE_NORMAL);
    merged[2 * k] = make_uint4(__float_as_uint(best), __float_as_uint(nw.x), __float_as_uint(nw.y), __float_as_uint(nw.z));
    merged[2 * k + 1] = make_uint4((m1.x & 0xFFFFu) | (flags << 16), m1.y, m1.z, m1.w);
    owner[k] = (uint32_t)win + 1u;
}

// Stage 2's fold.  A considered pixel gets SVO_SHADOW_TRACED, and SVO_SHADOWED where a pair of its has a slot and a usable record
// or its record of the scene list is usable; no other byte of merged changes.  (Its mask is 0 where it is not considered.)
__global__ __launch_bounds__(256) void k_inst_fold(PixelFrame F, InstanceList I, const uint32_t *masks, const uint32_t *base, uint32_t nblocks, uint32_t cap,
                                                   const uint4 *rays, const uint4 *scene_rays, uint4 *merged)
{
    __shared__ uint32_t sh[MAX_LIGHTS][LIGHT_WAVES];
    const int64_t k = (int64_t)blockIdx.x * LIGHT_BLOCK + threadIdx.x, n = F.count();
    const uint32_t mask = k < n ? masks[k] : 0u;
    bool occluded = false;
    light_pairs(mask, I.count, base, nblocks, sh, [&](int j, uint32_t r) {
        if (r < cap && usable_hit(record_flags(rays, r))) occluded = true;
    });
    if (k >= n) return;
    const uint32_t word = merged[2 * k + 1].x, flags = word >> 16;
    if (!usable_hit(flags) || (flags & SVO_SHADOWED)) return;
    if (usable_hit(record_flags(scene_rays, k))) occluded = true;
    reinterpret_cast<uint32_t *>(merged + 2 * k + 1)[0] = word | ((SVO_SHADOW_TRACED | (occluded ? SVO_SHADOWED : 0u)) << 16);
}

} // namespace svo
