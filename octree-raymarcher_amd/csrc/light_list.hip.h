// light_list.hip.h — a list of up to 32 point lights, each with a reach (svo_trace_lights): one occlusion ray per hit pixel and light
// that can reach it, in ONE compacted ray list, and one bit per light in a word per pixel.
//
// Not in the reference.  The pattern of local_shadows.hip.h with the padding taken out: a pixel and a light are a PAIR where the hit
// is usable, lies within the light's reach and faces it.  The pairs are ranked light-major (all of light 0 in pixel order, then
// light 1, ...), so that the 64 rays of a wave converge on one light.  Nothing per pair is stored for that:
//   k_light_cull     per pixel the 32-bit candidate mask, per block of 256 pixels and light the number of candidates
//   (device scan)    exclusive sum over the [light][block] counts: where a block's pairs of a light begin; k_light_total: how many there are
//   k_light_emit     rank of every pair from the block's base, the waves before it and the lanes below it; the ray into its slot
//   (ray-list march) ONE svo_trace_rays launch of `cap` rays
//   k_light_resolve  the same ranks again; bit j of the pixel's word is set iff (pixel, j) is a pair and its ray was not occluded
// A pair whose rank is not below `cap` has no slot: it is not marched and counts as not occluded.
#pragma once
#include "local_shadows.hip.h"

namespace svo {

constexpr int MAX_LIGHTS = 32;          // SVO_MAX_LIGHTS: one bit of the word each
constexpr unsigned LIGHT_BLOCK = 256, LIGHT_WAVES = LIGHT_BLOCK / 64;
struct LightList {
    float pos[MAX_LIGHTS][3];
    float reach2[MAX_LIGHTS];           // reach * reach, rounded once on the host (+inf: everything is in reach)
    int32_t count;
};

// Pixel k's candidate mask: bit j where the hit is usable, v = L_j - P has a length (local_light_vector), q <= reach^2 and the hit
// faces the light - !(n . v <= 0), summed left to right, so that a NaN normal faces every light
__device__ __forceinline__ uint32_t light_candidates(const PixelFrame &F, int64_t k, float eps, const LightList &L, const uint4 *gbuffer)
{
    if (!usable_hit(record_flags(gbuffer, k))) return 0u;
    const uint4 r0 = gbuffer[2 * k];
    const V3 n = mk(__uint_as_float(r0.y), __uint_as_float(r0.z), __uint_as_float(r0.w));
    const V3 p = local_sample_point(F, k, __uint_as_float(r0.x), eps);
    uint32_t mask = 0u;
    for (int j = 0; j < L.count; ++j) {
        V3 v;
        float q;
        if (!local_light_vector(p, L.pos[j], v, q) || !(q <= L.reach2[j])) continue;
        const float s = n.x * v.x + n.y * v.y + n.z * v.z;
        if (!(s <= 0.0f)) mask |= 1u << j;
    }
    return mask;
}

// The wave's votes per light, and in sh[j][wave] how many of them there are.  Every thread of the block calls this.
__device__ __forceinline__ void light_wave_counts(uint32_t mask, int count, uint32_t (*sh)[LIGHT_WAVES])
{
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (int j = 0; j < count; ++j) {
        const unsigned long long m = __ballot((mask >> j) & 1u);
        if (lane == 0u) sh[j][wv] = (uint32_t)__popcll(m);
    }
    __syncthreads();                                        // one for all lights
}

// pair(j, rank) for every light j of this thread's mask: base[j][block] + the waves before this one + the lanes below this one
// (block_take's in-block part, hip_own.h).  Every thread of the block calls this; sh holds [MAX_LIGHTS][LIGHT_WAVES] words.
template <typename Pair>
__device__ __forceinline__ void light_pairs(uint32_t mask, int count, const uint32_t *base, uint32_t nblocks, uint32_t (*sh)[LIGHT_WAVES], Pair &&pair)
{
    light_wave_counts(mask, count, sh);
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (int j = 0; j < count; ++j) {
        const unsigned long long m = __ballot((mask >> j) & 1u);
        if (!((mask >> j) & 1u)) continue;
        uint32_t r = base[(size_t)j * nblocks + blockIdx.x];
        for (unsigned w = 0; w < wv; ++w) r += sh[j][w];
        pair(j, r + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)));
    }
}

__global__ __launch_bounds__(256) void k_light_cull(PixelFrame F, float eps, LightList L, const uint4 *gbuffer, uint32_t *masks, uint32_t *counts, uint32_t nblocks)
{
    __shared__ uint32_t sh[MAX_LIGHTS][LIGHT_WAVES];
    const int64_t k = (int64_t)blockIdx.x * LIGHT_BLOCK + threadIdx.x, n = F.count();
    const uint32_t mask = k < n ? light_candidates(F, k, eps, L, gbuffer) : 0u;
    if (k < n) masks[k] = mask;
    light_wave_counts(mask, L.count, sh);
    if ((int)threadIdx.x < L.count) {
        uint32_t tot = 0u;
        for (unsigned w = 0; w < LIGHT_WAVES; ++w) tot += sh[threadIdx.x][w];
        counts[(size_t)threadIdx.x * nblocks + blockIdx.x] = tot;
    }
}

// total[0] = the number of pairs, total[1] = min(pairs, cap); a copy for the caller where it asked for one
__global__ void k_light_total(const uint32_t *counts, const uint32_t *base, uint32_t items, uint32_t cap, uint32_t *total, uint32_t *count_out)
{
    const uint32_t pairs = base[items - 1] + counts[items - 1];
    total[0] = pairs; total[1] = pairs < cap ? pairs : cap;
    if (count_out) { count_out[0] = total[0]; count_out[1] = total[1]; }
}

// The ray (P, v * (1 / sqrt(q))) of every pair into its slot, and k_continuation's miss ray into the slots [total, cap)
__global__ __launch_bounds__(256) void k_light_emit(PixelFrame F, float eps, LightList L, V3 miss, const uint4 *gbuffer, const uint32_t *masks, const uint32_t *base,
                                                    uint32_t nblocks, const uint32_t *total, uint32_t cap, float *origins, float *dirs)
{
    __shared__ uint32_t sh[MAX_LIGHTS][LIGHT_WAVES];
    const int64_t k = (int64_t)blockIdx.x * LIGHT_BLOCK + threadIdx.x, n = F.count();
    const uint32_t mask = k < n ? masks[k] : 0u;
    V3 p = mk(0.0f, 0.0f, 0.0f);
    if (mask) p = local_sample_point(F, k, __uint_as_float(gbuffer[2 * k].x), eps);
    light_pairs(mask, L.count, base, nblocks, sh, [&](int j, uint32_t r) {
        if (r >= cap) return;                               // dropped
        V3 v;
        float q;
        (void)local_light_vector(p, L.pos[j], v, q);        // (a candidate: q has a length)
        const V3 d = v * (1.0f / sqrtf(q));                 // normalize3's expression
        origins[3 * (size_t)r] = p.x; origins[3 * (size_t)r + 1] = p.y; origins[3 * (size_t)r + 2] = p.z;
        dirs[3 * (size_t)r] = d.x; dirs[3 * (size_t)r + 1] = d.y; dirs[3 * (size_t)r + 2] = d.z;
    });
    const uint64_t stride = (uint64_t)nblocks * LIGHT_BLOCK;
    for (uint64_t r = (uint64_t)total[0] + (uint64_t)k; r < cap; r += stride) {
        origins[3 * r] = miss.x; origins[3 * r + 1] = miss.y; origins[3 * r + 2] = miss.z;
        dirs[3 * r] = -1.0f; dirs[3 * r + 1] = 0.0f; dirs[3 * r + 2] = 0.0f;
    }
}

// A pair is occluded iff its ray's record is a usable hit in front of the light (t < dist, svo_trace_local_shadows' rule), with the
// distance remade through local_light_vector: the one the direction was made from.  `words` holds the masks and receives the result.
__global__ __launch_bounds__(256) void k_light_resolve(PixelFrame F, float eps, LightList L, const uint4 *gbuffer, const uint32_t *base, uint32_t nblocks, uint32_t cap,
                                                       const uint4 *rays, uint32_t *words)
{
    __shared__ uint32_t sh[MAX_LIGHTS][LIGHT_WAVES];
    const int64_t k = (int64_t)blockIdx.x * LIGHT_BLOCK + threadIdx.x, n = F.count();
    const uint32_t mask = k < n ? words[k] : 0u;
    V3 p = mk(0.0f, 0.0f, 0.0f);
    if (mask) p = local_sample_point(F, k, __uint_as_float(gbuffer[2 * k].x), eps);
    uint32_t visible = mask;
    light_pairs(mask, L.count, base, nblocks, sh, [&](int j, uint32_t r) {
        if (r >= cap) return;                               // dropped: not marched, not occluded
        V3 v;
        float q;
        (void)local_light_vector(p, L.pos[j], v, q);
        if (usable_hit(record_flags(rays, r)) && __uint_as_float(rays[2 * (size_t)r].x) < sqrtf(q)) visible &= ~(1u << j);
    });
    if (k < n && visible != mask) words[k] = visible;
}

} // namespace svo
