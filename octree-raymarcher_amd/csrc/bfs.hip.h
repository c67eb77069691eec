// bfs.hip.h — the two kernels every level-synchronous grow() shares (builder.hip: the terrain, float corners; grid.hip: a voxel grid,
// integer corners): the level's totals taken from the scan, and the emit that appends children in parent order (== the reference's
// FIFO queue order, src/Octree.cpp:155-174).  A frontier entry is 16 B: { x, y, z, slot } with x, y, z of type T.
#pragma once
#include <hip/hip_runtime.h>

#include "svo_format.h"

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

} // namespace svo
