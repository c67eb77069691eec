// mesh.hip — svo_device_grid_add_mesh / svo_device_grid_fill_enclosed: a triangle mesh in device memory rasterised into a dense voxel
// grid in device memory, and the shell made solid.  mesh.cpp is the host twin of both; mesh_rule.h holds the float arithmetic that
// the two share.  World-less: the calling thread's current device, the caller's stream, one arena from the device buffer cache per
// call (at least 1 MiB, so that it goes back to the cache and not to hipFree, which would drain the device), complete at the return.
//
// The voxeliser - the same three launches for thousands of sub-cell triangles and for one triangle across a 1024^3 grid (the setup
// kernel and the decode of a tile job live in mesh_tiles.hip.h, which sparse_mesh.hip shares):
//   k_mesh_setup     one thread per triangle: the record of mesh_setup (48 words: plane, box, nine edge functions, the clamped cell
//                    box) and the number of 4x4x4-cell tiles its cell box touches; 0 for a dropped triangle
//   hipcub scan      exclusive sum of the counts, 64-bit: where each triangle's tile jobs begin, and their total for the host
//   k_mesh_tiles     one wave per tile job, in launches of at most 2^30 jobs: the triangle by binary search in the scan, its record
//                    through the scalar cache (everything about the job is wave-uniform), one cell per lane through mesh_overlaps;
//                    the lanes of an x pair share a 32-bit word of the grid, the even lane raises both halves with a compare-and-swap
//                    loop - a maximum, so the order in which jobs arrive does not matter
// There is no wave-uniform early rejection of a tile by the plane test: in float it would need an error bound to stay a superset of
// the cells' own tests, and it saves 60 VALU operations behind a job lookup that costs more.
//
// The fill - one bit per cell, 64-bit words along x (a row of N < 64 cells is one word of N bits):
//   k_fill_init      one thread per cell, a ballot per wave: the "empty" words, and the "outside" words seeded with the empty cells
//                    of the grid's six faces
//   k_fill_sweep     one thread per word: the outside bits of the four y / z neighbour words and the end bits of the two x
//                    neighbours come in, masked by empty; a Kogge-Stone fill floods them along the word's runs of empty bits in 12
//                    shifts; a word that changed raises the sweep's flag.  Words are only ever raised towards the fixed point, so
//                    a neighbour read while it is being written (old or new value) is harmless
//   the host         FILL_BATCH sweeps, then the last sweep's flag is read: 0 ends the loop.  Any number of sweeps is reached
//   k_fill_count / k_fill_write   empty & ~outside: counted per word (one atomic per block), written per cell
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "hip_own.h"
#include "mesh_rule.h"
#include "mesh_tiles.hip.h"

namespace svo {

namespace {

constexpr unsigned FILL_BATCH = 16;                 // sweeps between two reads of the flag

// Tile job first + 4 * block + wave of `total`; start[t] = the first job of triangle t, start[ntriangles] = total
__global__ __launch_bounds__(256) void k_mesh_tiles(const MeshTri *__restrict__ tri, const unsigned long long *__restrict__ start, uint32_t ntriangles,
                                                    unsigned long long first, unsigned long long total, uint32_t depth, uint32_t *grid)
{
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const unsigned long long job = first + (unsigned long long)blockIdx.x * 4ull + wave;
    if (job >= total) return;
    uint32_t x, y, z;
    const MeshTri &T = tile_job_cell(tri, start, ntriangles, job, lane, x, y, z);
    const float p[3] = { (float)x, (float)y, (float)z };
    const uint32_t m = mesh_overlaps(T, p) ? T.material : 0u;
    const uint32_t other = (uint32_t)__shfl_xor((int)m, 1, 64);
    const uint32_t want = m | (other << 16);                // even lane: its cell in the low half, the odd lane's in the high half
    if ((lane & 1u) != 0u || want == 0u) return;
    uint32_t *word = grid + ((((((size_t)z << depth) + y) << depth) + x) >> 1);
    uint32_t old = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        const uint32_t a = old & 0xFFFFu, b = old >> 16, wa = want & 0xFFFFu, wb = want >> 16;
        const uint32_t raised = (wa > a ? wa : a) | ((wb > b ? wb : b) << 16);
        if (raised == old) break;
        const uint32_t seen = atomicCAS(word, old, raised);
        if (seen == old) break;
        old = seen;
    }
}

// ---- the fill -------------------------------------------------------------------------------------------------------------------
// Cell (x, y, z) is bit x & 63 of word (((z << depth) + y) << wshift) + (x >> 6), wshift = log2 of the words per row.
struct FillDims {
    uint32_t depth, wshift, bshift;                         // bshift: log2 of the cells per word (6, or depth below 6)
    unsigned long long cells, words;
    explicit FillDims(uint32_t d) : depth(d), wshift(d > 6 ? d - 6 : 0), bshift(d < 6 ? d : 6), cells(1ull << (3 * d)), words(cells >> bshift) {}
};

__global__ __launch_bounds__(256) void k_fill_init(const uint16_t *grid, FillDims D, unsigned long long *empty, unsigned long long *outside)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (i >= D.cells) return;                               // (whole waves: the cell count is a multiple of 64)
    const uint32_t last = (1u << D.depth) - 1u, lane = threadIdx.x & 63u;
    const uint32_t x = (uint32_t)i & last, y = (uint32_t)(i >> D.depth) & last, z = (uint32_t)(i >> (2 * D.depth));
    const bool e = grid[i] == 0;
    const bool face = x == 0u || x == last || y == 0u || y == last || z == 0u || z == last;
    const unsigned long long me = __ballot(e), mo = __ballot(e && face);
    const uint32_t per = 1u << D.bshift;
    if ((lane & (per - 1u)) != 0u) return;
    const unsigned long long keep = per == 64u ? ~0ull : (1ull << per) - 1ull;
    empty[i >> D.bshift] = (me >> lane) & keep;
    outside[i >> D.bshift] = (mo >> lane) & keep;
}

// g flooded along the runs of set bits of p (g is a subset of p): Kogge-Stone, towards the high bits and towards the low bits
__device__ __forceinline__ unsigned long long flood_word(unsigned long long g, unsigned long long e)
{
    unsigned long long p = e;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { g |= p & (g << s); p &= p << s; }
    p = e;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { g |= p & (g >> s); p &= p >> s; }
    return g;
}

__global__ __launch_bounds__(256) void k_fill_sweep(FillDims D, const unsigned long long *__restrict__ empty, unsigned long long *outside, uint32_t *changed)
{
    const unsigned long long w = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (w >= D.words) return;
    const unsigned long long e = empty[w], o = outside[w];
    if (e == o) return;                                     // nothing left to gain (no empty cell, or all of them outside)
    const uint32_t last = (1u << D.depth) - 1u, perrow = 1u << D.wshift;
    const uint32_t wx = (uint32_t)w & (perrow - 1u);
    const unsigned long long r = w >> D.wshift;
    const uint32_t y = (uint32_t)r & last, z = (uint32_t)(r >> D.depth);
    const unsigned long long sy = perrow, sz = (unsigned long long)perrow << D.depth;
    unsigned long long in = o;
    if (y > 0u) in |= outside[w - sy];
    if (y < last) in |= outside[w + sy];
    if (z > 0u) in |= outside[w - sz];
    if (z < last) in |= outside[w + sz];
    if (wx > 0u) in |= outside[w - 1] >> 63;
    if (wx + 1u < perrow) in |= outside[w + 1] << 63;
    in = flood_word(in & e, e);
    if (in != o) { outside[w] = in; *changed = 1u; }
}

__global__ __launch_bounds__(256) void k_fill_count(FillDims D, const unsigned long long *__restrict__ empty, const unsigned long long *__restrict__ outside,
                                                    unsigned long long *filled)
{
    __shared__ uint32_t sh[4];
    const unsigned long long w = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    uint32_t c = w < D.words ? (uint32_t)__popcll(empty[w] & ~outside[w]) : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += (uint32_t)__shfl_xor((int)c, d, 64);
    if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0u) {
        const uint32_t tot = sh[0] + sh[1] + sh[2] + sh[3];
        if (tot) atomicAdd(filled, (unsigned long long)tot);
    }
}

__global__ __launch_bounds__(256) void k_fill_write(uint16_t *grid, FillDims D, const unsigned long long *__restrict__ empty,
                                                    const unsigned long long *__restrict__ outside, uint16_t material)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (i >= D.cells) return;
    const unsigned long long w = i >> D.bshift;
    const uint32_t bit = (uint32_t)i & ((1u << D.bshift) - 1u);
    if (((empty[w] & ~outside[w]) >> bit) & 1ull) grid[i] = material;
}

// ---- the host side (mesh_tiles.hip.h: current_device; hip_own.h: Arena, SyncAtExit) ------------------------------------------------
int add_mesh_device(const svo_mesh &m, float inv, uint32_t depth, uint16_t *grid, hipStream_t s)
{
    const char *who = "svo_device_grid_add_mesh";
    int device = 0;
    if (const int rc = current_device(who, &device)) return rc;
    const uint32_t n = m.ntriangles;
    size_t need = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)(n + 1), s));
    Arena A;
    const size_t k_tri = A.add((size_t)n * sizeof(MeshTri)), k_count = A.add(((size_t)n + 1) * 8), k_start = A.add(((size_t)n + 1) * 8), k_tmp = A.add(need + 16);
    if (const int rc = A.alloc(who, device)) return rc;
    SyncAtExit sync{ s };
    MeshTri *tri = A.at<MeshTri>(k_tri);
    unsigned long long *count = A.at<unsigned long long>(k_count), *start = A.at<unsigned long long>(k_start);
    const MeshArgs K = mesh_kernel_args(m, inv, depth);
    hipLaunchKernelGGL(k_mesh_setup, dim3(blocks_for((uint64_t)n + 1, 256)), dim3(256), 0, s, K, tri, count);
    if (const int rc = launch_status(who)) return rc;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(A.at<unsigned char>(k_tmp), need, count, start, (int)(n + 1), s));
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, start + n, sizeof total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (unsigned long long first = 0; first < total; first += TILE_JOBS_PER_LAUNCH) {
        const unsigned long long jobs = std::min(total - first, TILE_JOBS_PER_LAUNCH);
        hipLaunchKernelGGL(k_mesh_tiles, dim3(blocks_for(jobs, 4)), dim3(256), 0, s, tri, start, n, first, total, depth, reinterpret_cast<uint32_t *>(grid));
        if (const int rc = launch_status(who)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(s));
    return SVO_OK;
}

int fill_device(uint16_t *grid, uint32_t depth, uint16_t material, uint64_t *filled_out, hipStream_t s)
{
    const char *who = "svo_device_grid_fill_enclosed";
    int device = 0;
    if (const int rc = current_device(who, &device)) return rc;
    const FillDims D(depth);
    Arena A;
    const size_t k_empty = A.add(D.words * 8), k_outside = A.add(D.words * 8), k_flags = A.add(FILL_BATCH * sizeof(uint32_t)), k_filled = A.add(8);
    if (const int rc = A.alloc(who, device)) return rc;
    SyncAtExit sync{ s };
    unsigned long long *empty = A.at<unsigned long long>(k_empty), *outside = A.at<unsigned long long>(k_outside), *filled = A.at<unsigned long long>(k_filled);
    uint32_t *flags = A.at<uint32_t>(k_flags);
    const unsigned cell_blocks = blocks_for(D.cells, 256), word_blocks = blocks_for(D.words, 256);
    hipLaunchKernelGGL(k_fill_init, dim3(cell_blocks), dim3(256), 0, s, grid, D, empty, outside);
    if (const int rc = launch_status(who)) return rc;
    for (;;) {
        HIP_TRY(hipMemsetAsync(flags, 0, FILL_BATCH * sizeof(uint32_t), s));
        for (unsigned k = 0; k < FILL_BATCH; ++k) hipLaunchKernelGGL(k_fill_sweep, dim3(word_blocks), dim3(256), 0, s, D, empty, outside, flags + k);
        if (const int rc = launch_status(who)) return rc;
        uint32_t changed = 0;
        HIP_TRY(hipMemcpyAsync(&changed, flags + (FILL_BATCH - 1), sizeof changed, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (!changed) break;                                // the batch's last sweep raised no word: the fixed point
    }
    HIP_TRY(hipMemsetAsync(filled, 0, 8, s));
    hipLaunchKernelGGL(k_fill_count, dim3(word_blocks), dim3(256), 0, s, D, empty, outside, filled);
    hipLaunchKernelGGL(k_fill_write, dim3(cell_blocks), dim3(256), 0, s, grid, D, empty, outside, material);
    if (const int rc = launch_status(who)) return rc;
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, filled, sizeof total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (filled_out) *filled_out = total;
    return SVO_OK;
}

} // namespace

} // namespace svo

using namespace svo;

extern "C" {

int svo_device_grid_add_mesh(const svo_mesh *mesh, uint32_t depth, uint16_t *grid_dev, void *stream)
{
    float inv = 0.0f;
    if (!mesh_args_ok(mesh, depth, grid_dev, &inv) || ((uintptr_t)grid_dev & 15u) != 0) {
        set_error("svo_device_grid_add_mesh: bad argument (a mesh with its arrays, depth in [2, 10], a 16-byte aligned grid, cell positive and finite with a finite 1 / cell, a finite origin)");
        return SVO_ERR_INVALID_ARG;
    }
    if (mesh->ntriangles == 0) return SVO_OK;
    if (mesh->ntriangles >= 0x7FFFFFFFu) { set_error("svo_device_grid_add_mesh: too many triangles for one scan"); return SVO_ERR_UNSUPPORTED; }
    return fenced("svo_device_grid_add_mesh", [&] { return add_mesh_device(*mesh, inv, depth, grid_dev, (hipStream_t)stream); });
}

int svo_device_grid_fill_enclosed(uint16_t *grid_dev, uint32_t depth, uint16_t material, uint64_t *filled_out, void *stream)
{
    if (!grid_dev || depth < SVO_GRID_MIN_DEPTH || depth > SVO_GRID_MAX_DEPTH || material == 0 || ((uintptr_t)grid_dev & 15u) != 0) {
        set_error("svo_device_grid_fill_enclosed: bad argument (a 16-byte aligned grid, depth in [2, 10], a material that is not 0)");
        return SVO_ERR_INVALID_ARG;
    }
    return fenced("svo_device_grid_fill_enclosed", [&] { return fill_device(grid_dev, depth, material, filled_out, (hipStream_t)stream); });
}

} // extern "C"
