// bfs.hip.h — what every level-synchronous grow() shares (builder.hip: the terrain, float corners; grid.hip: a voxel grid, integer
// corners): the level's totals taken from the scan, the emit that appends children in parent order (== the reference's FIFO queue
// order, src/Octree.cpp:155-174), and bfs_grow, the host loop around them.  A frontier entry is 16 B: { x, y, z, slot } with x, y, z of
// type T.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "hip_own.h"

namespace svo {

template <typename T> struct BfsCell { T x, y, z; uint32_t slot; };

// the level's totals, from the scan instead of a counter: exclusive rank of the last node + its own flags
static __global__ void k_level_totals(const unsigned long long *flags, const unsigned long long *rank, uint32_t n, uint32_t *totals /* [0] BRANCH, [1] TWIG */)
{
    const unsigned long long t = rank[n - 1] + flags[n - 1];
    totals[0] = (uint32_t)t;
    totals[1] = (uint32_t)(t >> 32);
}

// node words; children of every BRANCH appended to the next frontier in parent order (== FIFO queue order);
// brick jobs listed in TWIG order.  A child's corner is the parent's plus `half` on the axes of its slot bits.
template <typename T>
__global__ __launch_bounds__(256) void k_emit(const BfsCell<T> *frontier, uint32_t n, T half, const uint32_t *word,
                                              const unsigned long long *rank /* BRANCH rank | TWIG rank << 32 */,
                                              uint32_t trees, uint32_t twigs, uint32_t *tree, BfsCell<T> *next, BfsCell<T> *brick_jobs)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const BfsCell<T> e = frontier[i];
    uint32_t w = word[i];
    const uint32_t type = node_type(w);
    if (type == BRANCH) {
        const uint32_t branch_rank = (uint32_t)rank[i];
        const uint32_t first = trees + 8 * branch_rank;
        w = node_make(BRANCH, first);
#pragma unroll
        for (uint32_t c = 0; c < 8; ++c) {
            const T ox = (c & 1) ? T(1) : T(0), oy = (c & 2) ? T(1) : T(0), oz = (c & 4) ? T(1) : T(0);
            BfsCell<T> ch; ch.x = e.x + ox * half; ch.y = e.y + oy * half; ch.z = e.z + oz * half; ch.slot = first + c;
            next[8 * (uint64_t)branch_rank + c] = ch;
        }
    } else if (type == TWIG) {
        const uint32_t twig_rank = (uint32_t)(rank[i] >> 32);
        const uint32_t brick = twigs + twig_rank;
        w = node_make(TWIG, brick);
        BfsCell<T> job = e; job.slot = brick;
        brick_jobs[twig_rank] = job;
    }
    tree[e.slot] = w;
}

// The arrays of the loop, one set per world (its builder context owns them: bfs_arrays, builder.hip) that the terrain and the grid
// both use: BfsCell<float> and BfsCell<uint32_t> are 16 bytes of the same alignment, so the cell arrays are kept as the integer kind
// and bfs_grow<T> reads them as BfsCell<T>; no call leaves anything in them for the next one.
struct BfsArrays {
    DevBuf<BfsCell<uint32_t>> frontier, next, jobs;
    DevBuf<uint32_t> word, totals;
    DevBuf<unsigned long long> flags, rank;
    DevBuf<unsigned char> scan_tmp;
    Pinned<uint32_t> h_totals;                  // the level's two totals read back (a pageable destination stages every 4-byte copy)
};
BfsArrays &bfs_arrays(svo_world &w);

// grow() from `root` (edge `edge`, slot 0) into the pool at `tree`, level by level; trees / twigs count what has been appended.
//   classify(level, edge, frontier, n, word, flags) -> status   launches the caller's classify kernel over the level's n nodes
//   room(nb, nt) -> status     before the level's nb BRANCHes and nt TWIGs are written: the pools come to hold trees + 8 * nb node
//                              words and twigs + nt bricks (`tree` is read after it: the caller may have moved the pool), or it refuses
//   bricks(jobs, nt)           launches the caller's brick kernel over the level's nt brick jobs
template <typename T, class Classify, class Room, class Bricks>
int bfs_grow(BfsArrays &B, const BfsCell<T> &root, T edge, uint64_t &trees, uint64_t &twigs, uint32_t *const &tree, hipStream_t s,
             Classify classify, Room room, Bricks bricks)
{
    static_assert(sizeof(BfsCell<T>) == sizeof(BfsCell<uint32_t>) && alignof(BfsCell<T>) == alignof(BfsCell<uint32_t>), "one set of cell arrays serves every T");
    auto cells = [](DevBuf<BfsCell<uint32_t>> &b) { return reinterpret_cast<BfsCell<T> *>(b.p); };
    int rc;
    if ((rc = B.frontier.reserve(1, false, s)) != SVO_OK || (rc = B.totals.reserve(2, false, s)) != SVO_OK || (rc = B.h_totals.alloc(2)) != SVO_OK) return rc;
    HIP_TRY(hipMemcpyAsync(B.frontier.p, &root, sizeof root, hipMemcpyHostToDevice, s));
    trees = 1; twigs = 0;
    for (uint32_t level = 0, n = 1; n > 0; ++level, edge = edge / 2) {
        if ((rc = B.word.reserve(n, false, s)) != SVO_OK || (rc = B.flags.reserve(n, false, s)) != SVO_OK || (rc = B.rank.reserve(n, false, s)) != SVO_OK) return rc;
        if ((rc = classify(level, edge, cells(B.frontier), n, B.word.p, B.flags.p)) != SVO_OK) return rc;
        size_t need = 0;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need, B.flags.p, B.rank.p, (int)n, s));
        if ((rc = B.scan_tmp.reserve(need + 16, false, s)) != SVO_OK) return rc;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(B.scan_tmp.p, need, B.flags.p, B.rank.p, (int)n, s));
        hipLaunchKernelGGL(k_level_totals, dim3(1), dim3(1), 0, s, B.flags.p, B.rank.p, n, B.totals.p);
        HIP_TRY(hipMemcpyAsync(B.h_totals.p, B.totals.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const uint64_t nb = B.h_totals.p[0], nt = B.h_totals.p[1];
        if ((rc = room(nb, nt)) != SVO_OK || (rc = B.next.reserve(std::max<uint64_t>(8 * nb, 1), false, s)) != SVO_OK ||
            (rc = B.jobs.reserve(std::max<uint64_t>(nt, 1), false, s)) != SVO_OK) return rc;
        hipLaunchKernelGGL(k_emit<T>, dim3(blocks_for(n, 256)), dim3(256), 0, s, cells(B.frontier), n, (T)(edge / 2), B.word.p, B.rank.p,
                           (uint32_t)trees, (uint32_t)twigs, tree, cells(B.next), cells(B.jobs));
        if (nt) bricks(cells(B.jobs), (uint32_t)nt);
        HIP_TRY(hipGetLastError());
        trees += 8 * nb; twigs += nt;
        std::swap(B.frontier, B.next);
        n = (uint32_t)(8 * nb);
    }
    return SVO_OK;
}

} // namespace svo
