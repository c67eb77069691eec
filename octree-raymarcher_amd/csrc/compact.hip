// compact.hip — svo_world_compact / svo_world_coarsen on an uploaded world: Ocroot::defragcopy / Ocroot::lodmm
// (src/Octree.cpp:445-614, 626-765; compact.cpp states both as the host recursion) without the host.
//
// The recursion numbers what it keeps in depth-first preorder: a block's index is 1 + 8 x (kept BRANCHes before it), a brick's the
// number of kept bricks before it; a folded subtree gives its blocks and bricks back.  Three level-synchronous sweeps over the
// nodes the root reaches give exactly that (the same plan as builder.hip's DeviceFiller):
//   A (top-down)   k_lod_gather: the reachable nodes of each level listed (the 8 children of every BRANCH the recursion descends
//                  into, appended to the next level's list); EMPTY / LEAF nodes get their result at once, every BRANCH / TWIG is
//                  listed again as a candidate for sweep B
//   B (bottom-up)  k_lod_reduce, one wave per candidate: the node's result (the word it becomes, the depth defragcopy returns, or
//                  "kept brick" with where its cells come from) and the kept blocks / bricks of its subtree.  A brick's 64 cells are
//                  one per lane - the one-value test is a ballot; a resampled brick reads the results of the two levels below
//   C (top-down)   k_lod_number: preorder prefix of the counts = each kept block's / brick's index, node words written to the new
//                  pool (children of a node that is not kept are marked dead); k_lod_bricks writes the kept bricks' cells, one
//                  lane per cell, recomputed from their sources (the old brick, the children's results, or the old subtree)
// The chunk's pools are read in place in the world's pools; the new ones are written to the edits' resident scratch and installed
// through install_resident_chunk (device.hip), which also rebuilds the chunk's masks and wide tree.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "hip_own.h"

namespace svo {

namespace {

constexpr unsigned LOD_BLOCK = 256;                 // 4 waves: sweep B / C brick kernels give one wave to each candidate
constexpr uint32_t NO_KIDS = 0xFFFFFFFFu, DEAD = 0xFFFFFFFFu;

// result word .y: the depth defragcopy returns (bits 0-7) and what the node becomes (bits 8-)
enum LodKind : uint32_t {
    KIND_NODE = 0,          // .x is the final word (EMPTY / LEAF), or a kept BRANCH (type BRANCH)
    KIND_COPY = 1,          // kept brick, cells of the old brick .x (the old TWIG word)
    KIND_RESAMPLE = 2,      // kept brick, cells from the children's results (two levels of EMPTY / LEAF)
    KIND_COARSEN = 3,       // kept brick, majority cells of the old BRANCH .x (lodmm's new brick)
    KIND_CANDIDATE = 4,     // sweep A -> B: .x is the node's old word
};
__device__ __forceinline__ uint2 result(uint32_t word, uint32_t depth, uint32_t kind) { return make_uint2(word, depth | (kind << 8)); }
__device__ __forceinline__ uint32_t res_depth(uint2 r) { return r.y & 0xFFu; }
__device__ __forceinline__ uint32_t res_kind(uint2 r) { return r.y >> 8; }
__device__ __forceinline__ uint32_t leaf_value(uint32_t word) { return node_type(word) == LEAF ? node_offset(word) & 0xFFFFu : 0u; }
__device__ __forceinline__ uint32_t octant(uint32_t x, uint32_t y, uint32_t z) { return (x & 1u) | (y & 1u) << 1 | (z & 1u) << 2; }

// One level's arrays (hip_own.h: LodScratch::Level owns them).  old: the node's index in the old pool; kids: index of its child block in the next level's
// list (NO_KIDS unless the recursion descends into it); res / cnt: sweep B's result and {blocks, bricks} of the subtree - in sweep
// C cnt becomes the {blocks, bricks} that precede the node in preorder; slot: the node's index in the new pool (or DEAD); cand:
// the BRANCH / TWIG nodes of the level (indices into this level's list).
struct LodLevel {
    uint32_t *old, *kids, *slot, *cand;
    uint2 *res, *cnt;
    uint32_t n = 0, ncand = 0;
};

struct LodArgs {
    const uint32_t *tree;       // the chunk's old node words (in the world's tree pool)
    const uint16_t *twig;       // its old bricks
    uint32_t coarse_level;      // coarsen: the level whose BRANCHes become bricks (UINT32_MAX: compact)
};

__global__ __launch_bounds__(LOD_BLOCK) void k_lod_gather(LodArgs A, uint32_t level, LodLevel L, uint32_t *next_old, uint32_t *ctr /* [0] child blocks, [1] candidates */)
{
    __shared__ uint32_t sh[LOD_BLOCK / 64 + 1];
    const uint32_t i = blockIdx.x * LOD_BLOCK + threadIdx.x;
    const bool live = i < L.n;
    const uint32_t word = live ? A.tree[L.old[i]] : node_make(EMPTY, 0);
    const uint32_t type = node_type(word);
    const bool descend = live && type == BRANCH && level != A.coarse_level;
    const bool cand = live && (type == BRANCH || type == TWIG);
    const uint32_t kids = block_take<LOD_BLOCK>(&ctr[0], descend, sh);
    const uint32_t c = block_take<LOD_BLOCK>(&ctr[1], cand, sh);
    if (!live) return;
    if (descend)
        for (uint32_t k = 0; k < 8; ++k) next_old[8 * (uint64_t)kids + k] = node_offset(word) + k;
    L.kids[i] = descend ? kids : NO_KIDS;
    if (cand) { L.cand[c] = i; L.res[i] = result(word, 0, KIND_CANDIDATE); }
    else { L.res[i] = result(type == LEAF ? word : node_make(EMPTY, 0), 1, KIND_NODE); L.cnt[i] = make_uint2(0, 0); }
}

// The cell `lane` of a resampled brick (defragcopy's descend at the cell centres of the copied children): child node, then - if it
// stayed a BRANCH - grandchild node, whose value the cell takes.
__device__ __forceinline__ uint32_t resample_cell(uint32_t lane, uint32_t kids, const uint2 *res1, const uint32_t *kids1, const uint2 *res2)
{
    const uint32_t x = lane & 3u, y = (lane >> 2) & 3u, z = lane >> 4;
    const uint64_t ci = 8 * (uint64_t)kids + octant(x >> 1, y >> 1, z >> 1);
    const uint2 r = res1[ci];
    if (res_kind(r) == KIND_NODE && node_type(r.x) == BRANCH)
        return leaf_value(res2[8 * (uint64_t)kids1[ci] + octant(x, y, z)].x);
    return leaf_value(r.x);
}

// The cell `lane` of lodmm's new brick under the old BRANCH `word`: the majority of the 8 old cells under it (one child: that node's
// value; a child brick: the most frequent of its 2x2x2 cells, ties to the first in z, y, x order - compact.cpp says why this is
// MisraGriesCounter<8>'s answer).
__device__ __forceinline__ uint32_t coarsen_cell(uint32_t lane, uint32_t word, const LodArgs &A)
{
    const uint32_t x = lane & 3u, y = (lane >> 2) & 3u, z = lane >> 4;
    const uint32_t child = A.tree[node_offset(word) + octant(x >> 1, y >> 1, z >> 1)];
    if (node_type(child) != TWIG) return leaf_value(child);
    const uint16_t *b = A.twig + (uint64_t)node_offset(child) * TWIG_WORDS + ((z & 1u) * 2) * 16 + ((y & 1u) * 2) * 4 + (x & 1u) * 2;
    uint32_t v[8];
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) v[k] = b[(k >> 2) * 16 + ((k >> 1) & 1u) * 4 + (k & 1u)];
    uint32_t best = v[0], best_count = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
        uint32_t n = 0;
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) n += v[j] == v[k] ? 1u : 0u;
        if (n > best_count) { best = v[k]; best_count = n; }
    }
    return best;
}

__device__ __forceinline__ uint32_t brick_cell(uint32_t lane, uint2 r, uint32_t kids, const LodArgs &A, const uint2 *res1, const uint32_t *kids1, const uint2 *res2)
{
    switch (res_kind(r)) {
    case KIND_COPY: return A.twig[(uint64_t)node_offset(r.x) * TWIG_WORDS + lane];
    case KIND_RESAMPLE: return resample_cell(lane, kids, res1, kids1, res2);
    default: return coarsen_cell(lane, r.x, A);
    }
}

// one wave per candidate of level L (N: level L+1, res2: level L+2's results)
__global__ __launch_bounds__(LOD_BLOCK) void k_lod_reduce(LodArgs A, uint32_t level, LodLevel L, LodLevel N, const uint2 *res2)
{
    const uint32_t w = blockIdx.x * (LOD_BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (w >= L.ncand) return;
    const uint32_t i = L.cand[w];
    const uint32_t word = L.res[i].x, kids = L.kids[i];
    uint2 out, cnt = make_uint2(0, 1);
    if (node_type(word) == TWIG || kids == NO_KIDS) {
        if (node_type(word) == TWIG) {
            const uint32_t v = A.twig[(uint64_t)node_offset(word) * TWIG_WORDS + lane];
            const uint32_t v0 = __shfl(v, 0);
            if (__ballot(v != v0) == 0ull) { out = result(v0 ? node_make(LEAF, v0) : node_make(EMPTY, 0), 1, KIND_NODE); cnt = make_uint2(0, 0); }
            else out = result(word, TWIG_LEVELS + 1, KIND_COPY);
        } else out = result(word, TWIG_LEVELS + 1, KIND_COARSEN);       // (always kept: lodmm does not fold its new bricks)
    } else {
        // a BRANCH the recursion descended into: lanes 0-7 hold its children's results
        const uint64_t ci = 8 * (uint64_t)kids + (lane & 7u);
        const uint2 r = N.res[ci], k = N.cnt[ci];
        uint32_t d = res_depth(r), blocks = k.x, bricks = k.y;
        const bool same = r.x == __shfl(r.x, 0) && res_kind(r) == KIND_NODE;
        for (uint32_t s = 1; s < 8; s <<= 1) {
            d = max(d, (uint32_t)__shfl_xor(d, s));
            blocks += __shfl_xor(blocks, s);
            bricks += __shfl_xor(bricks, s);
        }
        const bool mono = (__ballot(!same) & 0xFFull) == 0ull;
        if (A.coarse_level != UINT32_MAX) {
            out = result(node_make(BRANCH, 0), 0, KIND_NODE);            // lodmm copies the BRANCHes above coarse_level as they are
            cnt = make_uint2(1 + blocks, bricks);
        } else if (d == 1 && mono) {
            const uint32_t x = node_offset(__shfl(r.x, 0));
            out = result(x ? node_make(LEAF, x) : node_make(EMPTY, 0), 1, KIND_NODE);
            cnt = make_uint2(0, 0);
        } else if (d == TWIG_LEVELS) {
            const uint32_t v = resample_cell(lane, kids, N.res, N.kids, res2);
            const uint32_t v0 = __shfl(v, 0);
            if (__ballot(v != v0) == 0ull) { out = result(v0 ? node_make(LEAF, v0) : node_make(EMPTY, 0), 1, KIND_NODE); cnt = make_uint2(0, 0); }
            else out = result(node_make(TWIG, 0), TWIG_LEVELS + 1, KIND_RESAMPLE);
        } else {
            out = result(node_make(BRANCH, 0), d + 1, KIND_NODE);
            cnt = make_uint2(1 + blocks, bricks);
        }
    }
    if (lane == 0) { L.res[i] = out; L.cnt[i] = cnt; }
}

// one thread per node of level L: its word in the new pool, its children's slots and preorder bases
__global__ __launch_bounds__(LOD_BLOCK) void k_lod_number(LodLevel L, LodLevel N, uint32_t *tree, uint64_t trees)
{
    const uint32_t i = blockIdx.x * LOD_BLOCK + threadIdx.x;
    if (i >= L.n) return;
    const uint32_t s = L.slot[i], kids = L.kids[i];
    const uint2 r = L.res[i];
    const bool kept_branch = s != DEAD && res_kind(r) == KIND_NODE && node_type(r.x) == BRANCH;
    if (s != DEAD && s < trees) {
        const uint2 base = L.cnt[i];
        if (kept_branch) tree[s] = node_make(BRANCH, 1 + 8 * base.x);
        else if (res_kind(r) == KIND_NODE) tree[s] = r.x;
        else tree[s] = node_make(TWIG, base.y);
    }
    if (kids == NO_KIDS) return;
    const uint2 base = kept_branch ? L.cnt[i] : make_uint2(0, 0);
    uint2 run = make_uint2(base.x + 1, base.y);
    for (uint32_t c = 0; c < 8; ++c) {
        const uint64_t k = 8 * (uint64_t)kids + c;
        if (!kept_branch) { N.slot[k] = DEAD; continue; }
        N.slot[k] = 1 + 8 * base.x + c;
        const uint2 sub = N.cnt[k];
        N.cnt[k] = run;
        run.x += sub.x; run.y += sub.y;
    }
}

// one wave per candidate of level L that ended as a kept brick: its 64 cells into the new pool
__global__ __launch_bounds__(LOD_BLOCK) void k_lod_bricks(LodArgs A, LodLevel L, LodLevel N, const uint2 *res2, uint16_t *twig, uint64_t twigs)
{
    const uint32_t w = blockIdx.x * (LOD_BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (w >= L.ncand) return;
    const uint32_t i = L.cand[w];
    const uint2 r = L.res[i];
    if (L.slot[i] == DEAD || res_kind(r) == KIND_NODE) return;
    const uint32_t dst = L.cnt[i].y;
    if (dst >= twigs) return;
    twig[(uint64_t)dst * TWIG_WORDS + lane] = (uint16_t)brick_cell(lane, r, L.kids[i], A, N.res, N.kids, res2);
}

int rebuild_resident_impl(svo_world &w, int chunk, bool lod)
{
    HIP_TRY(hipSetDevice(w.device));
    HIP_TRY(hipDeviceSynchronize());                    // ordered behind every launch issued before it, like svo_world_edit_box
    hipStream_t s = nullptr;
    const ChunkPools &c = w.chunks[(size_t)chunk];
    const DevChunk &e = w.table[(size_t)chunk];
    const uint32_t maxlevel = c.depth - TWIG_LEVELS;
    LodArgs A;
    A.tree = w.hbm->tree.p + e.tree_off;
    A.twig = w.hbm->twig.p + e.twig_off * TWIG_WORDS;
    A.coarse_level = lod ? c.depth - 1 - TWIG_LEVELS : UINT32_MAX;
    const uint32_t last_level = lod ? A.coarse_level : maxlevel;        // no BRANCH below it is descended into
    int rc;
    LodScratch &S = lod_scratch(w);
    if (S.lv.size() < last_level + 2) S.lv.resize(last_level + 2);
    auto level_arrays = [&](uint32_t l, uint32_t n, LodLevel &L) -> int {
        LodScratch::Level &B = S.lv[l];
        const size_t m = std::max<size_t>(n, 1);
        if ((rc = B.old.reserve(m, false, s)) != SVO_OK || (rc = B.kids.reserve(m, false, s)) != SVO_OK || (rc = B.slot.reserve(m, false, s)) != SVO_OK ||
            (rc = B.cand.reserve(m, false, s)) != SVO_OK || (rc = B.res.reserve(m, false, s)) != SVO_OK || (rc = B.cnt.reserve(m, false, s)) != SVO_OK) return rc;
        L.old = B.old.p; L.kids = B.kids.p; L.slot = B.slot.p; L.cand = B.cand.p; L.res = B.res.p; L.cnt = B.cnt.p; L.n = n; L.ncand = 0;
        return SVO_OK;
    };
    if ((rc = S.ctr.reserve(2 * 32, false, s)) != SVO_OK) return rc;
    uint32_t *const ctr = S.ctr.p;
    HIP_TRY(hipMemsetAsync(ctr, 0, 2 * 32 * sizeof(uint32_t), s));
    std::vector<LodLevel> lv(last_level + 2);
    if ((rc = level_arrays(0, 1, lv[0])) != SVO_OK) return rc;
    const uint32_t zero = 0;
    HIP_TRY(hipMemcpyAsync(lv[0].old, &zero, sizeof zero, hipMemcpyHostToDevice, s));
    // sweep A
    uint32_t last = 0;
    for (uint32_t level = 0;; ++level) {
        LodLevel &L = lv[level];
        last = level;
        // the children's list, written before the next level's arrays are sized (level_arrays then finds `old` large enough and leaves it
        // alone); level last_level descends into nothing: its list is never written, a one-entry dummy stands in
        DevBuf<uint32_t> &next_old = S.lv[level + 1].old;
        if ((rc = next_old.reserve(level < last_level ? (size_t)L.n * 8 : 1, false, s)) != SVO_OK) return rc;
        hipLaunchKernelGGL(k_lod_gather, dim3(blocks_for(L.n, LOD_BLOCK)), dim3(LOD_BLOCK), 0, s, A, level, L, next_old.p, ctr + 2 * level);
        HIP_TRY(hipGetLastError());
        uint32_t h[2];
        HIP_TRY(hipMemcpyAsync(h, ctr + 2 * level, sizeof h, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        L.ncand = h[1];
        if (h[0] == 0) break;
        if (level >= last_level || (uint64_t)h[0] * 8 >= (1ull << 31)) {
            set_error("svo_world_compact: BRANCH below level depth-2, or a level of more than 2^31 nodes");
            return SVO_ERR_MALFORMED_TREE;
        }
        if ((rc = level_arrays(level + 1, h[0] * 8, lv[level + 1])) != SVO_OK) return rc;
    }
    // sweep B
    for (int level = (int)last; level >= 0; --level) {
        LodLevel &L = lv[(size_t)level];
        const LodLevel &N = lv[(size_t)level + 1];
        const uint2 *res2 = (size_t)level + 2 < lv.size() ? lv[(size_t)level + 2].res : nullptr;
        if (L.ncand) hipLaunchKernelGGL(k_lod_reduce, dim3(blocks_for(L.ncand, LOD_BLOCK / 64)), dim3(LOD_BLOCK), 0, s, A, (uint32_t)level, L, N, res2);
    }
    HIP_TRY(hipGetLastError());
    uint32_t total[2];
    HIP_TRY(hipMemcpyAsync(total, lv[0].cnt, sizeof total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t trees = 1 + 8ull * total[0], twigs = total[1];
    if (trees >= (1ull << 30) || twigs >= (1ull << 30)) { set_error("svo_world_compact: chunk exceeds the 30-bit node offset"); return SVO_ERR_UNSUPPORTED; }
    uint32_t *tree = nullptr;
    uint16_t *twig = nullptr;
    if ((rc = edit_scratch(w, trees, twigs, &tree, &twig)) != SVO_OK) return rc;
    // sweep C: the root sits at slot 0 with nothing before it
    const uint32_t root[3] = { 0u, 0u, 0u };
    HIP_TRY(hipMemcpyAsync(lv[0].slot, &root[0], sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(lv[0].cnt, &root[1], sizeof(uint2), hipMemcpyHostToDevice, s));
    for (uint32_t level = 0; level <= last; ++level) {
        const LodLevel &L = lv[level], &N = lv[level + 1];
        const uint2 *res2 = level + 2 < lv.size() ? lv[level + 2].res : nullptr;
        hipLaunchKernelGGL(k_lod_number, dim3(blocks_for(L.n, LOD_BLOCK)), dim3(LOD_BLOCK), 0, s, L, N, tree, trees);
        if (L.ncand) hipLaunchKernelGGL(k_lod_bricks, dim3(blocks_for(L.ncand, LOD_BLOCK / 64)), dim3(LOD_BLOCK), 0, s, A, L, N, res2, twig, twigs);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return install_rebuilt(w, chunk, lod ? c.depth - 1 : c.depth, nullptr, trees, twigs, tree, twig);
}

} // namespace

int rebuild_resident(svo_world &w, int chunk, bool lod) { return rebuild_resident_impl(w, chunk, lod); }

} // namespace svo
