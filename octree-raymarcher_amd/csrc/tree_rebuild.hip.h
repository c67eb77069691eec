// tree_rebuild.hip.h — what the level-synchronous tree rebuilders share (sparse_fill.hip: the interior fill; combine.hip: chunk CSG).
// Both walk from the root(s) level by level into per-level lists in visiting order - the FIFO walk's order -, work on the lists, and
// then rebuild the chunk from a result word per entry (BRANCH / TWIG without an offset):
//   walk     the caller's k_walk flags the entries to descend and reports a word it refuses; walk_level_tail ranks the flags, reads
//            { how many, the error } back and refuses; the caller's k_children appends the children in parent order
//   fold     bottom-up (fold_and_rank): the caller's k_fold gives every entry of a level its result from its children's and flags
//            what stays a BRANCH / TWIG; one scan per level ranks them.  The lists are in visiting order and what stays is
//            reachable, so these ranks are the FIFO walk's numbers: BRANCH k of the tree owns block 1 + 8k, TWIG k brick k
//   emit     top-down (emit_levels): k_emit writes an entry whose parent stays a BRANCH to first + slot; the caller's k_write_bricks
//            follows.  Every index written is checked against the pool it goes to
// The entry layouts, the walk and fold kernels and everything between walk and fold are the callers'.  Everything sits in an unnamed
// namespace: each of the two files compiles its own copy, as with mesh_tiles.hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "hip_own.h"
#include "chunk_pools.h"

namespace svo {

namespace {

// what a k_walk writes to its error word
enum : uint32_t { ERR_MALFORMED = 1, ERR_SHALLOW_TWIG = 2 };

// one call's name, stream and scan scratch (need_scan bytes at tmp: enough for the longest level's n + 1 items)
struct Rebuild { const char *who; hipStream_t s; unsigned char *tmp; size_t need_scan; };

// The tail of one walk level of n entries: the exclusive scan of its n + 1 descend flags in place, { the total, *err } read back
// behind one synchronise, the two refusals.  `subject` says whose pools ("a chunk's", "the chunk's"); `used` of `cap` entries are
// taken.  *total: the entries to descend, whose 8 * total children fit; the caller launches its k_children
inline int walk_level_tail(const Rebuild &R, const char *subject, uint32_t *flags, uint32_t n, const uint32_t *err, size_t used, size_t cap, uint32_t *total)
{
    size_t bytes = R.need_scan;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(R.tmp, bytes, flags, flags, (int)n + 1, R.s));
    uint32_t back[2] = { 0, 0 };
    HIP_TRY(hipMemcpyAsync(&back[0], flags + n, 4, hipMemcpyDeviceToHost, R.s));
    HIP_TRY(hipMemcpyAsync(&back[1], err, 4, hipMemcpyDeviceToHost, R.s));
    HIP_TRY(hipStreamSynchronize(R.s));
    if (back[1] == ERR_SHALLOW_TWIG) { set_error(std::string(R.who) + ": " + SHALLOW_TWIG_WHY); return SVO_ERR_UNSUPPORTED; }
    if (back[1] != 0 || back[0] > n || used + 8ull * back[0] > cap) { set_error(std::string(R.who) + ": " + subject + " pools are malformed"); return SVO_ERR_MALFORMED_TREE; }
    *total = back[0];
    return SVO_OK;
}

// what the fold leaves: above[L] = the BRANCHes that stay above level L, and the output's node words and bricks
struct Ranks { std::vector<uint32_t> above; uint64_t otrees = 1, twigs = 0; };

// Bottom-up over the levels lv (each with .rank of n + 1 items and .n): fold(L) launches the caller's fold kernel of level L, which
// leaves the level's "stays a BRANCH / TWIG" flags in .rank; they are scanned in place, the totals read back behind one synchronise
// at the end.  What stays at level `maxlevel` are TWIGs, above it BRANCHes
template <class Level, class Fold> int fold_and_rank(const Rebuild &R, const std::vector<Level> &lv, uint32_t maxlevel, Fold &&fold, Ranks &K)
{
    const uint32_t levels = (uint32_t)lv.size();
    std::vector<uint32_t> stay(levels, 0);
    for (uint32_t L = levels; L-- > 0;) {
        fold(L);
        if (const int rc = launch_status(R.who)) return rc;
        size_t bytes = R.need_scan;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(R.tmp, bytes, lv[L].rank, lv[L].rank, (int)lv[L].n + 1, R.s));
        HIP_TRY(hipMemcpyAsync(&stay[L], lv[L].rank + lv[L].n, 4, hipMemcpyDeviceToHost, R.s));
    }
    HIP_TRY(hipStreamSynchronize(R.s));
    uint64_t branches = 0;
    K.above.assign(levels, 0);
    K.twigs = 0;
    for (uint32_t L = 0; L < levels; ++L) {
        K.above[L] = (uint32_t)branches;
        if (L == maxlevel) K.twigs = stay[L]; else branches += stay[L];
    }
    K.otrees = 1 + 8 * branches;
    return SVO_OK;
}

// One level as k_emit reads it: entry i's result word is res[i], or res[index[i]] where the results are indexed by something else
// than the entry (the fill: by the old pool); its parent's entry in the level above; its rank among what stays
struct EmitLevel { const uint32_t *res; const uint32_t *index; const uint32_t *parent; const uint32_t *rank; uint32_t n; };
__device__ __forceinline__ uint32_t emit_result(const EmitLevel &L, uint32_t i) { return L.res[L.index ? L.index[i] : i]; }

// level C into the blocks of its parents' level V; above_v / above_c = the BRANCHes that stay above V / above C.  V.res == null: C is
// level 0 and its one entry the root.  (sparse_mesh.hip's k_write_nodes stays its own: its levels are sparse, a child's slot is key & 7.)
__global__ __launch_bounds__(256) void k_emit(EmitLevel C, EmitLevel V, uint32_t above_v, uint32_t above_c, uint32_t *tree, uint32_t trees)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= C.n) return;
    uint32_t at = 0u;
    if (V.res) {
        const uint32_t p = C.parent[i];
        if (node_type(emit_result(V, p)) != BRANCH) return;
        at = 1u + 8u * (above_v + V.rank[p]) + (i & 7u);
    }
    const uint32_t r = emit_result(C, i), type = node_type(r);
    const uint32_t w = type == BRANCH ? node_make(BRANCH, 1u + 8u * (above_c + C.rank[i])) : type == TWIG ? node_make(TWIG, C.rank[i]) : r;
    if (at < trees) tree[at] = w;
}

// The output pools in the edits' resident scratch of `w`, sized from the fold's totals, the tree cleared, and the levels emitted
// top-down; view(L) is level L as an EmitLevel.  The caller writes its bricks, synchronises and installs
template <class View> int emit_levels(const Rebuild &R, svo_world &w, uint32_t levels, View &&view, const Ranks &K, uint32_t **otree, uint16_t **otwig)
{
    if (const int rc = edit_scratch(w, K.otrees, K.twigs, otree, otwig)) return rc;
    HIP_TRY(hipMemsetAsync(*otree, 0, K.otrees * sizeof(uint32_t), R.s));
    for (uint32_t L = 0; L < levels; ++L) {
        const EmitLevel C = view(L), V = L ? view(L - 1) : EmitLevel{ nullptr, nullptr, nullptr, nullptr, 0 };
        hipLaunchKernelGGL(k_emit, dim3(blocks_for(C.n, 256)), dim3(256), 0, R.s, C, V, L ? K.above[L - 1] : 0u, K.above[L], *otree, (uint32_t)K.otrees);
        if (const int rc = launch_status(R.who)) return rc;
    }
    return SVO_OK;
}

} // namespace

} // namespace svo
