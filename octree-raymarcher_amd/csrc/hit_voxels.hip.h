// hit_voxels.hip.h — svo_hit_voxels: the voxel box of every hit of a G-buffer (svo_hit_uv, the reference's leafUV on it: shade.hip).
//
//   traverse (the box it holds on arriving at a node)   src/Traverse.cpp:34-48
//   the brick cell's leafmin / leafsize                 src/Traverse.cpp:58-66
//   cubeUV / leafUV                                     shaders/Chunkmarch.glsl:138-149, shaders/World.Fragment.glsl:5-15 (march.hip.h leaf_uv, image_stage.hip.h hit_uv)
//
// svo_hit has no room for the box and the summed t does not give the point traverse() saw, but (chunk, node, cell) name the voxel:
// children live in 8-blocks at 1 + 8k, every BRANCH points forward and no reachable block is referenced twice (validate_chunk), so
// the node's ancestors follow from a PARENT INDEX - per 8-block of the tree pool the chunk-relative index of the BRANCH that owns it
// and the block's level, 0 = not reachable - and the box from replaying traverse()'s float arithmetic from the root down.
// The index is validate_chunk's forward pass as kernels: the roots mark level 1, sweep L visits the blocks of level L and marks
// level L + 1.  Only reachable blocks are ever visited, so a BRANCH word in an orphan block (Ocroot::destroy leaves them) never
// writes.  Nothing is read back.  Like march.hip.h this is compiled with -ffp-contract=off: every float operation below is
// separately rounded, the box and the UV are bit for bit what the reference's expressions give.
#pragma once
#include "image_stage.hip.h"

namespace svo {

// pool block of chunk-relative node `node` >= 1 (tree_off % 8 == 7: the 8-blocks behind a root are 8-aligned in the pool)
__device__ __forceinline__ uint64_t pool_block(uint64_t tree_off, uint32_t node) { return (tree_off + node) >> 3; }

// a BRANCH at chunk-relative index `at` names a forward 8-block inside its chunk's `trees` node words (what validate_chunk asks)
__device__ __forceinline__ bool child_block_ok(uint32_t off, uint32_t at, uint32_t trees)
{
    return off > at && ((off - 1u) & 7u) == 0u && (uint64_t)off + 8u <= trees;
}

// level 1: the child block of every chunk's root
__global__ __launch_bounds__(256) void k_parent_roots(const DevChunk *chunks, const uint32_t *trees, uint32_t nchunks, const uint32_t *tree,
                                                      uint32_t *parent, uint8_t *level)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= nchunks) return;
    const uint64_t base = chunks[c].tree_off;
    const uint32_t word = tree[base];
    if (node_type(word) != BRANCH || !child_block_ok(node_offset(word), 0u, trees[c])) return;
    const uint64_t cb = pool_block(base, node_offset(word));
    parent[cb] = 0u;
    level[cb] = 1u;
}

// sweep L: thread (x, chunk) looks at the chunk's block x (nodes 1 + 8x .. 8 + 8x) and, if the sweep before marked it, marks the
// child block of each of its BRANCH words.  Blocks marked in this sweep read as 0 or L + 1, never as L.
__global__ __launch_bounds__(256) void k_parent_sweep(const DevChunk *chunks, const uint32_t *trees, uint32_t nchunks, const uint32_t *tree,
                                                      uint32_t *parent, uint8_t *level, uint32_t L)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    for (uint32_t c = blockIdx.y; c < nchunks; c += gridDim.y) {
        const uint32_t n = trees[c];
        if (x >= (n - 1u) / 8u) continue;
        const uint64_t base = chunks[c].tree_off;
        const uint32_t first = 1u + 8u * x;
        if (level[pool_block(base, first)] != L) continue;
        const uint4 *blk = reinterpret_cast<const uint4 *>(tree + base + first);      // 32-byte aligned
        const uint4 a = blk[0], b = blk[1];
        const uint32_t words[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            const uint32_t off = node_offset(words[j]);
            if (node_type(words[j]) != BRANCH || !child_block_ok(off, first + j, n)) continue;
            const uint64_t cb = pool_block(base, off);
            parent[cb] = first + j;
            level[cb] = (uint8_t)(L + 1u);
        }
    }
}

constexpr uint32_t HIT_PATH_LEVELS = 28;    // depth <= 30 (validate_chunk): at most 28 BRANCH levels above a node, 84 slot bits

// One lane per record: the walk up from `node` through the parent index pushes 3-bit child slots onto a 128-bit stack (a chain of
// dependent 4-byte loads: the cost of this call), the replay pops them from the root down.
__global__ __launch_bounds__(256) void k_hit_voxels(const uint4 *gbuffer, void *out, int64_t n, const DevChunk *chunks, const uint32_t *trees,
                                                    uint32_t nchunks, const uint32_t *tree, const uint32_t *parent, const uint8_t *level, float chunksize)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const uint4 r1 = gbuffer[2 * k + 1];
    const uint32_t chunk = r1.y, node = r1.z, cell = r1.w;
    if (!usable_hit(r1.x >> 16) || chunk >= nchunks || node >= trees[chunk]) { store_miss(out, k, 0u); return; }
    const DevChunk ch = chunks[chunk];
    const uint32_t type = node_type(tree[ch.tree_off + node]);
    const bool named = (type == LEAF && cell == SVO_CELL_NONE) || (type == TWIG && cell < TWIG_WORDS);
    const uint32_t lv = node == 0u ? 0u : level[pool_block(ch.tree_off, node)];
    if (!named || (node != 0u && lv == 0u) || lv > HIT_PATH_LEVELS) { store_miss(out, k, 0u); return; }
    uint64_t lo_bits = 0u, hi_bits = 0u;
    uint32_t cur = node;
    for (uint32_t i = 0; i < lv; ++i) {                     // (a block of level lv has lv ancestors: cur ends at the root)
        hi_bits = (hi_bits << 3) | (lo_bits >> 61);
        lo_bits = (lo_bits << 3) | ((cur - 1u) & 7u);
        cur = parent[pool_block(ch.tree_off, cur)];
    }
    V3 lo = ld3(ch.bmin);
    float size = chunksize;
    for (uint32_t i = 0; i < lv; ++i) {                     // src/Traverse.cpp:39-45
        const uint32_t slot = (uint32_t)lo_bits & 7u;
        lo_bits = (lo_bits >> 3) | (hi_bits << 61);
        hi_bits >>= 3;
        const float half = size * 0.5f;
        lo = lo + mk((slot & 1u) ? 1.0f : 0.0f, (slot & 2u) ? 1.0f : 0.0f, (slot & 4u) ? 1.0f : 0.0f) * half;
        size = half;
    }
    if (type == TWIG) {                                     // :58-66
        const float voxel = size / 4.0f;
        lo = lo + mk((float)(cell & 3u), (float)((cell >> 2) & 3u), (float)(cell >> 4)) * voxel;
        size = voxel;
    }
    store_hit(out, k, lo.x, mk(lo.y, lo.z, size), r1.x & 0xFFFFu, SVO_LOCATE_INSIDE | SVO_LOCATE_SOLID, chunk, node, cell);
}

} // namespace svo
