// mesh.cpp — svo_grid_add_mesh / svo_grid_fill_enclosed: a triangle mesh rasterised into a dense voxel grid and the shell made
// solid, on the host.  The readable statement of both rules (include/svo.h; mesh_rule.h has the float arithmetic), the twin of
// mesh.hip, and what gives a caller without a device a grid for svo_chunk_from_grid + svo_world_create.
//   add_mesh   per triangle: its record (mesh_setup), then every cell of its clamped cell box is tested (mesh_overlaps) and raised to
//              the triangle's material if that is larger - a maximum, so neither the order of the triangles nor a second call matters
//   fill       a queue flood over the empty cells from the empty cells of the grid's six faces; what it did not reach is enclosed
// mesh_args_ok is shared with mesh.hip: one statement of the refusals.  No HIP include: plain g++ compiles this file
// (host/mesh_check.cpp runs it under the sanitizers).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "mesh_rule.h"
#include "world.h"

namespace svo {

// the refusals of both add_mesh twins that do not depend on where the grid lives; *inv receives 1 / cell
bool mesh_args_ok(const svo_mesh *m, uint32_t depth, const void *grid, float *inv)
{
    if (!grid || depth < SVO_GRID_MIN_DEPTH || depth > SVO_GRID_MAX_DEPTH) return false;
    return mesh_frame_ok(m, inv);
}

// the part of them that is about the mesh alone (sparse_mesh.cpp has no grid and a depth range of its own)
bool mesh_frame_ok(const svo_mesh *m, float *inv)
{
    if (!m || (m->nvertices && !m->vertices) || (m->ntriangles && !m->indices)) return false;
    if (!std::isfinite(m->cell) || !(m->cell > 0.0f)) return false;
    *inv = 1.0f / m->cell;
    if (!std::isfinite(*inv)) return false;
    return std::isfinite(m->origin[0]) && std::isfinite(m->origin[1]) && std::isfinite(m->origin[2]);
}

} // namespace svo

extern "C" {

int svo_grid_add_mesh(const svo_mesh *mesh, uint32_t depth, uint16_t *grid)
{
    using namespace svo;
    float inv = 0.0f;
    if (!mesh_args_ok(mesh, depth, grid, &inv)) {
        set_error("svo_grid_add_mesh: bad argument (a mesh with its arrays, depth in [2, 10], a grid, cell positive and finite with a finite 1 / cell, a finite origin)");
        return SVO_ERR_INVALID_ARG;
    }
    const int32_t N = 1 << depth;
    for (uint32_t t = 0; t < mesh->ntriangles; ++t) {
        const uint32_t *ix = mesh->indices + 3 * (size_t)t;
        if (ix[0] >= mesh->nvertices || ix[1] >= mesh->nvertices || ix[2] >= mesh->nvertices) continue;
        MeshTri T;
        if (!mesh_setup(mesh->vertices + 3 * (size_t)ix[0], mesh->vertices + 3 * (size_t)ix[1], mesh->vertices + 3 * (size_t)ix[2], mesh->origin, inv,
                        mesh->materials ? mesh->materials[t] : mesh->material, N, T)) continue;
        for (int32_t z = T.c0[2]; z <= T.c1[2]; ++z)
            for (int32_t y = T.c0[1]; y <= T.c1[1]; ++y)
                for (int32_t x = T.c0[0]; x <= T.c1[0]; ++x) {
                    const float p[3] = { (float)x, (float)y, (float)z };
                    if (!mesh_overlaps(T, p)) continue;
                    uint16_t &cell = grid[((((size_t)z << depth) + (size_t)y) << depth) + (size_t)x];
                    if (T.material > cell) cell = (uint16_t)T.material;
                }
    }
    return SVO_OK;
}

int svo_grid_fill_enclosed(uint16_t *grid, uint32_t depth, uint16_t material, uint64_t *filled_out)
{
    using namespace svo;
    if (!grid || depth < SVO_GRID_MIN_DEPTH || depth > SVO_GRID_MAX_DEPTH || material == 0) {
        set_error("svo_grid_fill_enclosed: bad argument (a grid, depth in [2, 10], a material that is not 0)");
        return SVO_ERR_INVALID_ARG;
    }
    try {
        const uint32_t N = 1u << depth, last = N - 1;
        const size_t cells = (size_t)1 << (3 * depth);
        std::vector<uint8_t> outside(cells, 0);
        std::vector<uint32_t> queue;                        // cell indices (< 2^30)
        auto visit = [&](size_t i) { if (grid[i] == 0 && !outside[i]) { outside[i] = 1; queue.push_back((uint32_t)i); } };
        for (uint32_t z = 0; z < N; ++z)
            for (uint32_t y = 0; y < N; ++y) {
                const bool face = z == 0 || z == last || y == 0 || y == last;
                const size_t row = (((size_t)z << depth) + y) << depth;
                if (face) for (uint32_t x = 0; x < N; ++x) visit(row + x);
                else { visit(row); visit(row + last); }
            }
        const size_t sy = N, sz = (size_t)N * N;
        for (size_t head = 0; head < queue.size(); ++head) {
            const size_t i = queue[head];
            const uint32_t x = (uint32_t)i & last, y = (uint32_t)(i >> depth) & last, z = (uint32_t)(i >> (2 * depth));
            if (x > 0) visit(i - 1);
            if (x < last) visit(i + 1);
            if (y > 0) visit(i - sy);
            if (y < last) visit(i + sy);
            if (z > 0) visit(i - sz);
            if (z < last) visit(i + sz);
        }
        uint64_t filled = 0;
        for (size_t i = 0; i < cells; ++i)
            if (grid[i] == 0 && !outside[i]) { grid[i] = material; ++filled; }
        if (filled_out) *filled_out = filled;
        return SVO_OK;
    } catch (const std::bad_alloc &) {
        set_error("svo_grid_fill_enclosed: out of host memory");
        return SVO_ERR_OUT_OF_MEMORY;
    }
}

} // extern "C"
