// mesh_tiles.hip.h — what the two device voxelisers share (mesh.hip: into a dense grid; sparse_mesh.hip: into a list of cells): the
// setup kernel, the decode of a tile job, and the host-side helpers of a world-less call (its working memory is an Arena of
// hip_own.h).  Everything sits in an unnamed namespace: each of the two files compiles its own copy.
//   k_mesh_setup     one thread per triangle: the record of mesh_setup (48 words: plane, box, nine edge functions, the clamped cell
//                    box) and the number of 4x4x4-cell tiles its cell box touches; 0 for a dropped triangle
//   tile_job_cell    one wave per tile job: the triangle by binary search in the scan of those counts, its record through the scalar
//                    cache (everything about the job is wave-uniform), one cell per lane
#pragma once
#include <hip/hip_runtime.h>

#include "hip_own.h"
#include "mesh_rule.h"

namespace svo {

namespace {

constexpr unsigned long long TILE_JOBS_PER_LAUNCH = 1ull << 30;

struct MeshArgs {
    const float *vertices; const uint32_t *indices; const uint16_t *materials;
    uint32_t nvertices, ntriangles;
    float origin[3], inv;
    uint32_t material; int32_t N;
};

__device__ __forceinline__ uint32_t tiles_of(const MeshTri &T, int k) { return (uint32_t)((T.c1[k] >> 2) - (T.c0[k] >> 2) + 1); }

// tri[t] and count[t] of triangle t; count[ntriangles] = 0 is the scan's last item, whose sum is the total
__global__ __launch_bounds__(256) void k_mesh_setup(MeshArgs A, MeshTri *tri, unsigned long long *count)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t > A.ntriangles) return;
    if (t == A.ntriangles) { count[t] = 0ull; return; }
    const uint32_t i0 = A.indices[3ull * t], i1 = A.indices[3ull * t + 1], i2 = A.indices[3ull * t + 2];
    MeshTri T = {};
    bool live = false;
    if (i0 < A.nvertices && i1 < A.nvertices && i2 < A.nvertices) {
        const float *pa = A.vertices + 3ull * i0, *pb = A.vertices + 3ull * i1, *pc = A.vertices + 3ull * i2;
        const float a[3] = { pa[0], pa[1], pa[2] }, b[3] = { pb[0], pb[1], pb[2] }, c[3] = { pc[0], pc[1], pc[2] };
        live = mesh_setup(a, b, c, A.origin, A.inv, A.materials ? (uint32_t)A.materials[t] : A.material, A.N, T);
    }
    if (!live) T.material = 0u;
    tri[t] = T;
    count[t] = live ? (unsigned long long)tiles_of(T, 0) * tiles_of(T, 1) * tiles_of(T, 2) : 0ull;
}

// The cell (x, y, z) of lane `lane` in tile job `job` and the job's triangle; start[t] = the first job of triangle t,
// start[ntriangles] = the total, job below it
__device__ __forceinline__ const MeshTri &tile_job_cell(const MeshTri *__restrict__ tri, const unsigned long long *__restrict__ start, uint32_t ntriangles,
                                                        unsigned long long job, uint32_t lane, uint32_t &x, uint32_t &y, uint32_t &z)
{
    uint32_t lo = 0u, hi = ntriangles;                      // start[lo] <= job < start[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (start[mid] <= job) lo = mid; else hi = mid;
    }
    const MeshTri &T = tri[lo];
    const unsigned long long local = job - start[lo];       // below nx * ny * nz: up to 2^24 at depth 10, 2^42 at depth 16
    const uint32_t nx = tiles_of(T, 0), ny = tiles_of(T, 1);
    uint32_t ox, oy, oz;
    mesh_tile_of_job(local, nx, ny, ox, oy, oz);
    const uint32_t tx = (uint32_t)(T.c0[0] >> 2) + ox, ty = (uint32_t)(T.c0[1] >> 2) + oy, tz = (uint32_t)(T.c0[2] >> 2) + oz;
    x = tx * 4u + (lane & 3u); y = ty * 4u + ((lane >> 2) & 3u); z = tz * 4u + (lane >> 4);
    return T;
}

// ---- the host side --------------------------------------------------------------------------------------------------------------
inline int current_device(const char *who, int *device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { set_error(std::string(who) + ": no HIP device"); return SVO_ERR_NO_DEVICE; }
    HIP_TRY(hipGetDevice(device));
    return SVO_OK;
}

inline MeshArgs mesh_kernel_args(const svo_mesh &m, float inv, uint32_t depth)
{
    MeshArgs K;
    K.vertices = m.vertices; K.indices = m.indices; K.materials = m.materials;
    K.nvertices = m.nvertices; K.ntriangles = m.ntriangles;
    std::memcpy(K.origin, m.origin, sizeof K.origin);
    K.inv = inv; K.material = m.material; K.N = 1 << depth;
    return K;
}

} // namespace

} // namespace svo
