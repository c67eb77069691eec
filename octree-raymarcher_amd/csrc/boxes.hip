// boxes.hip — the edit cursor and the light markers: what the reference draws over the finished image (ImagCube::draw,
// src/ImaginaryCube.cpp:64-87, shaders/Imag.Fragment.glsl; Light::draw, src/Light.cpp:141-155, shaders/Light.Fragment.glsl) and how it
// places the cursor (computeTarget, src/Main.cpp:314-319; ImaginaryCube::position, src/ImaginaryCube.cpp:59-62).  svo_cursor_place is
// one thread; svo_shade_boxes one thread per pixel over the float4 image a shade call wrote, its depth float the depth buffer.  The
// arithmetic is the one include/svo.h writes out, every operation in float and separately rounded (IEEE divisions, no hardware
// reciprocals: the face chosen at a box edge must not hang on 1 ulp).
#include <hip/hip_runtime.h>

#include "image_stage.hip.h"

static_assert(sizeof(svo_box) == 48, "svo_box is 48 bytes");

namespace svo {
namespace {

constexpr int BOX_WORDS = sizeof(svo_box) / 4;

struct BoxArgs {
    PixelFrame frame;
    const uint32_t *boxes;                      // nboxes svo_box records
    int32_t nboxes;
    float inv_near, depth_range;                // 1 / near, 1 / far - 1 / near
    float4 *rgba;
};

// CUBE_INDICES (src/Parallax.cpp:25-38) draws the faces in the order -Z, -X, +Z, +X, -Y, +Y: the place of face (axis, max side) in it
__device__ __forceinline__ int draw_order(int axis, bool max_side)
{
    return axis == 2 ? (max_side ? 2 : 0) : axis == 0 ? (max_side ? 3 : 1) : (max_side ? 5 : 4);
}

// isEdge of shaders/Imag.Fragment.glsl on one in-face coordinate
__device__ __forceinline__ bool is_edge(float c) { return c <= 0.015625f || c >= 0.984375f; }

// The box list is staged in LDS by the whole block (wave-uniform reads from there on).  A pixel loads its float4 once and stores
// it once, only where a fragment passed.
__global__ __launch_bounds__(256) void k_shade_boxes(BoxArgs A)
{
    __shared__ uint32_t list[SVO_MAX_BOXES * BOX_WORDS];
    for (int i = (int)threadIdx.x; i < A.nboxes * BOX_WORDS; i += 256) list[i] = A.boxes[i];
    __syncthreads();
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= A.frame.count()) return;
    V3 o, d;
    A.frame.ray(k, o, d);
    float4 px = A.rgba[k];
    bool written = false;
    const float oa[3] = { o.x, o.y, o.z }, da[3] = { d.x, d.y, d.z };
    for (int b = 0; b < A.nboxes; ++b) {
        const uint32_t *rec = list + b * BOX_WORDS;
        const float size = __uint_as_float(rec[3]);
        const uint32_t style = rec[8];
        if ((style & SVO_BOX_HIDDEN) || !(size > 0.0f)) continue;
        const float lo[3] = { __uint_as_float(rec[0]), __uint_as_float(rec[1]), __uint_as_float(rec[2]) };
        // slabs: the largest near value and the smallest far value, the first axis winning ties
        float tnear = -INFINITY, tfar = INFINITY;
        int fnear = -1, ffar = -1;
        bool missed = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float hi = lo[a] + size;
            if (da[a] != 0.0f) {
                const float t0 = (lo[a] - oa[a]) / da[a], t1 = (hi - oa[a]) / da[a];
                const bool min_first = t0 <= t1;
                const float n = min_first ? t0 : t1, f = min_first ? t1 : t0;
                if (n > tnear) { tnear = n; fnear = draw_order(a, !min_first); }
                if (f < tfar) { tfar = f; ffar = draw_order(a, min_first); }
            } else if (oa[a] < lo[a] || oa[a] > hi) missed = true;
        }
        if (missed || fnear < 0 || ffar < 0 || !(tnear <= tfar)) continue;
        // up to two fragments, in the order the reference's index buffer draws their faces
        const bool entry = tnear > 0.0f, leave = tfar > 0.0f;
        const bool entry_first = fnear < ffar;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const bool is_entry = (pass == 0) == entry_first;
            if (!(is_entry ? entry : leave)) continue;
            const float t = is_entry ? tnear : tfar;
            const int face = is_entry ? fnear : ffar;
            const float f = (1.0f / t - A.inv_near) / A.depth_range;
            if (!(f < px.w)) continue;          // GL_LESS; a NaN fails
            float r = __uint_as_float(rec[4]), g = __uint_as_float(rec[5]), bl = __uint_as_float(rec[6]), al = __uint_as_float(rec[7]);
            if ((style & 0xFFu) == SVO_BOX_CURSOR) {
                const float cx = ((oa[0] + da[0] * t) - lo[0]) / size, cy = ((oa[1] + da[1] * t) - lo[1]) / size, cz = ((oa[2] + da[2] * t) - lo[2]) / size;
                // the face axis' own coordinate counts as an edge: black where one of the two in-face coordinates is one too
                const bool edge = face == 0 || face == 2 ? is_edge(cx) || is_edge(cy) : face == 1 || face == 3 ? is_edge(cy) || is_edge(cz) : is_edge(cx) || is_edge(cz);
                if (edge) { r = g = bl = 0.0f; al = 1.0f; }
            }
            const float keep = 1.0f - al;       // GL_SRC_ALPHA, GL_ONE_MINUS_SRC_ALPHA
            px.x = r * al + px.x * keep;
            px.y = g * al + px.y * keep;
            px.z = bl * al + px.z * keep;
            px.w = f;
            written = true;
        }
    }
    if (written) A.rgba[k] = px;
}

// computeTarget + ImaginaryCube::position from the record the march wrote for the ray (o, d)
__global__ void k_cursor_place(V3 o, V3 d, float size, const uint32_t *record, uint32_t *box)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t style = box[8];
    if (usable_hit(record[4] >> 16)) {
        const V3 sigma = o + d * __uint_as_float(record[0]);        // src/Traverse.cpp:161
        const float half = size * 0.5f;
        box[0] = __float_as_uint(sigma.x - half);
        box[1] = __float_as_uint(sigma.y - half);
        box[2] = __float_as_uint(sigma.z - half);
        box[3] = __float_as_uint(size);
        style &= ~(uint32_t)SVO_BOX_HIDDEN;
    } else style |= SVO_BOX_HIDDEN;                                 // imag.real == false
    box[8] = style;
}

} // namespace
} // namespace svo

using namespace svo;

extern "C" {

int svo_cursor_place(const float origin[3], const float dir[3], const svo_hit *record_dev, float size, svo_box *box_dev, void *stream)
{
    if (!origin || !dir || !record_dev || !box_dev || !(size > 0.0f)) { set_error("svo_cursor_place: bad argument"); return SVO_ERR_INVALID_ARG; }
    V3 o, d;
    o.x = origin[0]; o.y = origin[1]; o.z = origin[2]; d.x = dir[0]; d.y = dir[1]; d.z = dir[2];
    hipLaunchKernelGGL(k_cursor_place, dim3(1), dim3(64), 0, (hipStream_t)stream, o, d, size,
                       reinterpret_cast<const uint32_t *>(record_dev), reinterpret_cast<uint32_t *>(box_dev));
    return launch_status("svo_cursor_place");
}

int svo_shade_boxes(const svo_camera *cam, const svo_box *boxes_dev, int nboxes, float near_plane, float far_plane,
                    int x0, int y0, int w, int h, float *rgba_dev, void *stream)
{
    bool ok = rgba_dev && nboxes >= 0 && nboxes <= SVO_MAX_BOXES && (boxes_dev || nboxes == 0) && rect_ok(cam, x0, y0, w, h);
    ok = ok && near_plane >= 0.0f && far_plane >= 0.0f;       // (a NaN plane fails the compare)
    if (!ok) { set_error("svo_shade_boxes: bad argument"); return SVO_ERR_INVALID_ARG; }
    if (nboxes == 0) return SVO_OK;
    if (near_plane == 0.0f) near_plane = 0.125f;
    if (far_plane == 0.0f) far_plane = 8192.0f;
    BoxArgs A;
    A.frame = make_frame(*cam, x0, y0, w, h);
    A.boxes = reinterpret_cast<const uint32_t *>(boxes_dev); A.nboxes = nboxes;
    A.inv_near = 1.0f / near_plane;
    A.depth_range = 1.0f / far_plane - A.inv_near;
    A.rgba = reinterpret_cast<float4 *>(rgba_dev);
    return launch_per_element("svo_shade_boxes", A.frame.count(), (hipStream_t)stream, k_shade_boxes, A);
}

} // extern "C"
