// see_through.hip.h — see-through materials (svo_trace_params.see_through, svo_trace_translucent).
//
// The reference's shader march threads an `ignore` material through treemarch / twigmarch (shaders/Chunkmarch.glsl:190-191,
// 240-241,280) and ParallaxAlpha.Fragment.glsl marches a second time from a water hit with water ignored (:141-199,276-335).
// The stack kernel is not changed for it: it marches a see-through VIEW of the world instead, i.e. the two pools it reads
// derived once more with material m taken out -
//   wide pool   a terminal LEAF entry of payload m becomes EMPTY at the same level (wide_tree.hip.h: what the builder makes of
//               the node word 0 that replaces LEAF(m) in the rewritten tree); wbase is shared, node indices do not move;
//   mask pool   the bits of cells holding m are cleared.
// Everything else is shared.  bmat (device.hip k_brick_masks) holds a brick's one material, 0 or 0xFFFF: a brick of m alone
// has bmat = m but no mask bit left, so it is never hit; a brick that mixes m with another material has 0xFFFF, so the hit
// block reads the real cell, which is never m once its mask bit is clear.  The chunk table holds wide-node and brick indices
// relative to the pools (DevWide.wide_off / twig_off), so the view reuses it too.  The records of a launch on the view equal,
// bit for bit, those of the world with LEAF(m) -> 0 and cell m -> 0.
#pragma once
#include "image_stage.hip.h"
#include "wide_tree.hip.h"

namespace svo {

// wide entries [0, n4 * 4): LEAF(m) -> EMPTY at its level
__global__ __launch_bounds__(256) void k_view_wide(const uint4 *wide, uint4 *out, uint64_t n4, uint32_t m)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const uint32_t leaf_m = (LEAF << 30) | m, keep = ((1u << WIDE_LEVEL_BITS) - 1u) << WIDE_LEVEL_SHIFT;
    uint4 v = wide[i];
    // (type and payload without the level bits: a LEAF's payload is its 16-bit material)
    v.x = (v.x & ~keep) == leaf_m ? v.x & keep : v.x;
    v.y = (v.y & ~keep) == leaf_m ? v.y & keep : v.y;
    v.z = (v.z & ~keep) == leaf_m ? v.z & keep : v.z;
    v.w = (v.w & ~keep) == leaf_m ? v.w & keep : v.w;
    out[i] = v;
}

// masks of bricks [0, count): one thread per 16-byte eighth of a brick (8 cells -> one mask byte), as k_brick_masks
__global__ __launch_bounds__(256) void k_view_mask(const uint16_t *twig, const uint64_t *mask, uint64_t *out, uint64_t count, uint32_t m)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count * 8) return;
    const uint4 v = reinterpret_cast<const uint4 *>(twig)[i];
    const uint32_t w[4] = { v.x, v.y, v.z, v.w };
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        bits |= ((w[k] & 0xFFFFu) == m ? 1u : 0u) << (2 * k);
        bits |= ((w[k] >> 16) == m ? 1u : 0u) << (2 * k + 1);
    }
    reinterpret_cast<uint8_t *>(out)[i] = (uint8_t)(reinterpret_cast<const uint8_t *>(mask)[i] & ~bits);
}

// svo_trace_translucent: the continuation list in pixel order.  A surface hit of material m (not a runaway) continues from
// p1 = o + d * t1 along its primary direction d and gets SVO_SEE_THROUGH; every other pixel gets the ray from `miss` (device.hip
// miss_ray_origin) along -x, whose line misses the world box (both marches' entry tests refuse it), so its record is the all-zero miss.
__global__ __launch_bounds__(256) void k_continuation(PixelFrame F, uint32_t m, V3 miss, uint4 *surface, float *origins, float *dirs)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= F.count()) return;
    uint4 r1 = surface[2 * k + 1];
    V3 o = miss, d = mk(-1.0f, 0.0f, 0.0f);
    if (usable_hit(r1.x >> 16) && (r1.x & 0xFFFFu) == m) {
        V3 eye;
        F.ray(k, eye, d);
        const float t1 = __uint_as_float(surface[2 * k].x);
        o = mk(__fadd_rn(eye.x, __fmul_rn(d.x, t1)), __fadd_rn(eye.y, __fmul_rn(d.y, t1)), __fadd_rn(eye.z, __fmul_rn(d.z, t1)));
        r1.x |= (uint32_t)SVO_SEE_THROUGH << 16;
        surface[2 * k + 1] = r1;
    }
    origins[3 * k] = o.x; origins[3 * k + 1] = o.y; origins[3 * k + 2] = o.z;
    dirs[3 * k] = d.x; dirs[3 * k + 1] = d.y; dirs[3 * k + 2] = d.z;
}

} // namespace svo
