// mesh_rule.h — the voxelisation rule of svo_grid_add_mesh (include/svo.h states it), once, for the host twin (mesh.cpp, plain g++) and
// the kernels (mesh.hip).  Every operation is a separately rounded float operation written in the header's order (both files are
// compiled without contraction), every comparison is written the way the header writes it (NaN compares false), so the two sides
// agree bit for bit.  No HIP include: the sanitizer program compiles this with g++.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/svo.h"

#if defined(__HIPCC__)
#define SVO_MESH_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SVO_MESH_HD inline
#endif

namespace svo {

// mesh.cpp: the refusals of both add_mesh twins that do not depend on where the grid lives; *inv receives 1 / cell
bool mesh_args_ok(const svo_mesh *m, uint32_t depth, const void *grid, float *inv);
bool mesh_frame_ok(const svo_mesh *m, float *inv);          // its part about the mesh alone: the arrays, cell, inv, origin

// What the cell test needs of one triangle, in grid units: 48 words, the record the setup kernel leaves per triangle.
struct MeshTri {
    float n[3], d1, d2;                 // plane: (dot(p, n) + d1) * (dot(p, n) + d2) <= 0
    float lo[3], hi[3];                 // box:   p[k] <= hi[k] && p[k] + 1 >= lo[k]
    float e[9][3];                      // edge functions, e[3 * plane + k] = { a, b, de }: (a * p[i] + b * p[j]) + de >= 0
    int32_t c0[3], c1[3];               // the clamped cell box [c0, c1] that is visited (a superset of the Box test's cells inside the grid)
    uint32_t material;                  // 0: dropped, or nothing to write - c0 / c1 are not valid then
    uint32_t pad_[3];
};
static_assert(sizeof(MeshTri) == 48 * 4, "the setup record is 48 words");

SVO_MESH_HD float mesh_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
SVO_MESH_HD float mesh_max0(float t) { return t > 0.0f ? t : 0.0f; }
SVO_MESH_HD float mesh_min(float a, float b) { return b < a ? b : a; }        // (finite operands only: the callers have dropped the rest)
SVO_MESH_HD float mesh_max(float a, float b) { return b > a ? b : a; }
SVO_MESH_HD bool mesh_finite(float v) { return v - v == 0.0f; }               // false for NaN and +-inf

// The record of the triangle (a, b, c) of the mesh's coordinates, `material` its material, N = 2^depth.  Returns false (T.material = 0)
// when the triangle is dropped, carries material 0 or misses the grid's box.
SVO_MESH_HD bool mesh_setup(const float a[3], const float b[3], const float c[3], const float origin[3], float inv, uint32_t material,
                            int32_t N, MeshTri &T)
{
    T.material = 0;
    T.pad_[0] = T.pad_[1] = T.pad_[2] = 0;
    float v[3][3];
    bool finite = true;
    for (int k = 0; k < 3; ++k) {
        v[0][k] = (a[k] - origin[k]) * inv;
        v[1][k] = (b[k] - origin[k]) * inv;
        v[2][k] = (c[k] - origin[k]) * inv;
        finite = finite && mesh_finite(v[0][k]) && mesh_finite(v[1][k]) && mesh_finite(v[2][k]);
    }
    if (!finite || material == 0) return false;
    float e[3][3];                                          // e0 = v1 - v0, e1 = v2 - v1, e2 = v0 - v2
    for (int k = 0; k < 3; ++k) { e[0][k] = v[1][k] - v[0][k]; e[1][k] = v[2][k] - v[1][k]; e[2][k] = v[0][k] - v[2][k]; }
    float n[3];
    n[0] = e[0][1] * e[1][2] - e[0][2] * e[1][1];
    n[1] = e[0][2] * e[1][0] - e[0][0] * e[1][2];
    n[2] = e[0][0] * e[1][1] - e[0][1] * e[1][0];
    if (n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f) return false;
    float c1[3], c2[3];
    for (int k = 0; k < 3; ++k) {
        const float ck = n[k] > 0.0f ? 1.0f : 0.0f;
        c1[k] = ck - v[0][k];
        c2[k] = (1.0f - ck) - v[0][k];
        T.n[k] = n[k];
        T.lo[k] = mesh_min(mesh_min(v[0][k], v[1][k]), v[2][k]);
        T.hi[k] = mesh_max(mesh_max(v[0][k], v[1][k]), v[2][k]);
    }
    T.d1 = mesh_dot(c1, n);
    T.d2 = mesh_dot(c2, n);
    for (int plane = 0; plane < 3; ++plane) {               // (i, j, w) = (x, y, z), (y, z, x), (z, x, y)
        const int i = plane, j = (plane + 1) % 3, w = (plane + 2) % 3;
        const float s = n[w] >= 0.0f ? 1.0f : -1.0f;
        for (int k = 0; k < 3; ++k) {
            const float ea = -e[k][j] * s, eb = e[k][i] * s;
            float *out = T.e[3 * plane + k];
            out[0] = ea;
            out[1] = eb;
            out[2] = ((-(ea * v[k][i] + eb * v[k][j])) + mesh_max0(ea)) + mesh_max0(eb);
        }
    }
    // the cells to visit: p <= hi and p + 1 >= lo give floor(lo) - 1 <= p <= floor(hi), clamped to the grid (p + 1 is exact there)
    const float last = (float)(N - 1);
    for (int k = 0; k < 3; ++k) {
        const float flo = floorf(T.lo[k]) - 1.0f, fhi = floorf(T.hi[k]);
        if (!(fhi >= 0.0f) || !(flo <= last)) return false;
        T.c0[k] = flo < 0.0f ? 0 : (int32_t)flo;
        T.c1[k] = fhi > last ? N - 1 : (int32_t)fhi;
    }
    T.material = material;
    return true;
}

// Tile job `local` of a triangle whose cell box is nx x ny x nz tiles of 4^3 cells, x fastest: the tile (ox, oy, oz) within the box.
// local < nx * ny * nz, which is up to 2^24 for a grid of depth 10 and up to 2^42 at depth 16: jobs below 2^32 - every job of a grid up
// to depth 10 - are decoded in 32-bit divisions, the others in 64-bit ones (on the device the branch is wave-uniform).
SVO_MESH_HD void mesh_tile_of_job(unsigned long long local, uint32_t nx, uint32_t ny, uint32_t &ox, uint32_t &oy, uint32_t &oz)
{
    if ((local >> 32) == 0ull) {
        const uint32_t l = (uint32_t)local, row = l / nx;
        ox = l - row * nx; oy = row % ny; oz = row / ny;
    } else {
        const unsigned long long row = local / nx, slab = row / ny;
        ox = (uint32_t)(local - row * nx); oy = (uint32_t)(row - slab * ny); oz = (uint32_t)slab;
    }
}

// Does the triangle overlap the cell whose integer min corner is p (as floats)?
SVO_MESH_HD bool mesh_overlaps(const MeshTri &T, const float p[3])
{
    for (int k = 0; k < 3; ++k)
        if (!(p[k] <= T.hi[k] && p[k] + 1.0f >= T.lo[k])) return false;
    const float q = mesh_dot(p, T.n);
    if (!((q + T.d1) * (q + T.d2) <= 0.0f)) return false;
    for (int plane = 0; plane < 3; ++plane) {
        const int i = plane, j = (plane + 1) % 3;
        for (int k = 0; k < 3; ++k) {
            const float *f = T.e[3 * plane + k];
            if (!((f[0] * p[i] + f[1] * p[j]) + f[2] >= 0.0f)) return false;
        }
    }
    return true;
}

} // namespace svo
