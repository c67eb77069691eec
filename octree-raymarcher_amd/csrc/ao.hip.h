// ao.hip.h — svo_hit_ao: voxel ambient occlusion of every hit of a G-buffer, from the eight lattice cells around the open cell in
// front of the face that was hit (include/svo.h states the rule, steps 1-7; tests/ao_model.py restates it in numpy).
//
// Not in the reference.  "Is this cell solid" is svo_world_locate's question, so the kernel calls locate.hip.h's walks
// (walk_literal / walk_wide, terminal_solid) on eight points per pixel and folds their solid bits; no point list and no records
// pass through memory.  Eight lanes per pixel: lane j of an octet walks neighbour j, a wave holds 8 pixels, a block of 256 holds 32.
// The lanes of an octet load the same records and the same upper tree levels (one request each), the eight solid bits come back as
// byte lane >> 3 of a 64-bit __ballot, lane 0 of the octet folds and stores.  EVERY lane reaches the ballot: pixels beyond w*h, misses
// and the last partial wave skip their walk by predicate, never by an early return.  (One lane per pixel with the eight walks in a loop
// was built and measured, 1.55 - 1.66 times slower on the benchmark world, and deleted: DESIGN.md 6q.)
// No LDS.  Like march.hip.h this is compiled with -ffp-contract=off: every float operation below is separately rounded.
#pragma once
#include "image_stage.hip.h"
#include "locate.hip.h"

namespace svo {

// Steps 1-4 for pixel k: false where the pixel gets 1.0f without a walk.  Q: the centre of the open cell, (u, v): the face's two
// other axes, e: the lattice pitch, (fu, fv): where the sample point lies in its lattice cell.
template <bool WIDE>
__device__ __forceinline__ bool ao_cell(const TraceArgs &A, const PixelFrame &F, float cell, uint32_t k, const uint4 *gbuffer, const uint4 *voxels,
                                        V3 &Q, int &u, int &v, float &e, float &fu, float &fv)
{
    const uint4 r1 = gbuffer[2 * (size_t)k + 1], v1 = voxels[2 * (size_t)k + 1];
    if (!usable_hit(r1.x >> 16) || !((v1.x >> 16) & SVO_LOCATE_INSIDE) || v1.y >= (uint32_t)(A.dimw * A.dimh * A.dimd)) return false;
    const float t = __uint_as_float(gbuffer[2 * (size_t)k].x);
    const uint4 v0 = voxels[2 * (size_t)k];
    V3 o, d;
    camera_ray(F.cam, F.imgw, F.imgh, F.x0 + (int)(k % (uint32_t)F.w), F.y0 + (int)(k / (uint32_t)F.w), o, d);     // (PixelFrame::ray; k < 2^31)
    const V3 P = o + d * (t - A.eps);                                           // 1.
    const HitFace face = hit_face(P, v0, d);                                    // 2. (image_stage.hip.h)
    const int ax = face.axis;
    const float sgn = face.sgn;
    e = cell;                                                                   // 3.
    if (!(cell > 0.0f)) {
        const uint32_t levels = WIDE ? A.wchunks[v1.y].levels : A.chunks[v1.y].levels;
        e = ldexpf(A.chunksize, -(int)(levels + TWIG_LEVELS));
    }
    u = ax == 0 ? 1 : 0; v = ax == 2 ? 1 : 2;                                   // 4.
    const float ru = axis_of(P, u) / e, rv = axis_of(P, v) / e;
    const float gu = floorf(ru), gv = floorf(rv);
    fu = ru - gu; fv = rv - gv;
    Q = mk(0.0f, 0.0f, 0.0f);
    Q = with_axis(Q, u, (gu + 0.5f) * e);
    Q = with_axis(Q, v, (gv + 0.5f) * e);
    Q = with_axis(Q, ax, (sgn > 0.0f ? axis_of(face.hi, ax) : axis_of(face.lo, ax)) + sgn * (e * 0.5f));
    return isfinite(ru) && isfinite(rv);
}

// Step 5 for neighbour j: occ of the lattice cell (a, b) = (-1,-1), (0,-1), (1,-1), (-1,0), (1,0), (-1,1), (0,1), (1,1) beside Q
template <bool WIDE>
__device__ __forceinline__ bool ao_occupied(const TraceArgs &A, uint32_t see, V3 Q, int u, int v, float e, int j)
{
    const int g = j < 4 ? j : j + 1;
    V3 N = Q;
    N = with_axis(N, u, axis_of(Q, u) + (float)(g % 3 - 1) * e);
    N = with_axis(N, v, axis_of(Q, v) + (float)(g / 3 - 1) * e);
    Terminal T;
    if (!(WIDE ? walk_wide<false>(A, N, T) : walk_literal(A, N, T))) return false;
    uint32_t material, cell;
    return terminal_solid(N, T, A.glsl != 0, see, material, cell);
}

// Steps 6 and 7 from the eight occ bits (bit j: neighbour j)
__device__ __forceinline__ float ao_fold(uint32_t occ, float fu, float fv)
{
    auto corner = [occ](int s1, int s2, int cn) {
        const uint32_t a = (occ >> s1) & 1u, b = (occ >> s2) & 1u, c = (occ >> cn) & 1u;
        return (float)((a & b) ? 0u : 3u - (a + b + c)) / 3.0f;
    };
    const float a00 = corner(3, 1, 0), a10 = corner(4, 1, 2), a01 = corner(3, 6, 5), a11 = corner(4, 6, 7);
    const float l0 = a00 + (a10 - a00) * fu;
    const float l1 = a01 + (a11 - a01) * fu;
    return l0 + (l1 - l0) * fv;
}

// A: the world (fill_common), A.n = w*h < 2^31.  8 n lanes, blocks of 256 = 32 pixels.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_hit_ao(TraceArgs A, PixelFrame F, float cell, uint32_t see, const uint4 *gbuffer, const uint4 *voxels, float *ao)
{
    const uint64_t k = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 3;
    const bool live = k < (uint64_t)A.n;
    V3 Q = mk(0.0f, 0.0f, 0.0f);
    int u = 0, v = 0;
    float e = 0.0f, fu = 0.0f, fv = 0.0f;
    const bool walks = live && ao_cell<WIDE>(A, F, cell, (uint32_t)k, gbuffer, voxels, Q, u, v, e, fu, fv);
    const bool solid = walks && ao_occupied<WIDE>(A, see, Q, u, v, e, (int)(threadIdx.x & 7u));
    const unsigned long long all = __ballot(solid);                             // (every lane of the wave is here)
    const uint32_t occ = (uint32_t)(all >> (threadIdx.x & 56u)) & 0xFFu;        // byte (lane >> 3) of the wave's mask
    if (live && !(threadIdx.x & 7u)) ao[k] = walks ? ao_fold(occ, fu, fv) : 1.0f;
}

} // namespace svo
