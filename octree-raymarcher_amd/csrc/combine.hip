// combine.hip — svo_world_chunk_combine: two chunks of one depth combined cell by cell on their trees, on the device the two worlds live
// on, without a dense grid, depth 2 .. 16.  combine.cpp is the host twin and states the combination as a recursive pair walk, a fold and
// a FIFO emit; combine_rule.h holds the cell function.  On the null stream, behind a hipDeviceSynchronize like
// svo_world_chunk_fill_enclosed; complete at the return.  tree_rebuild.hip.h holds the frame of the rebuild (the walk's tail, the
// fold's ranks, the emit); this file's own:
//   walk              An entry is the pair of node WORDS (w_A, w_B) and its parent's entry; the rule has no geometry, so there is no
//                     corner.  k_walk flags the entries to descend (either side a BRANCH; every offset is checked against its pool),
//                     gives every other entry above the bricks its result word f(a, b) and counts its edge^3 cells if that differs
//                     from a; k_children, one thread per child: a side that is EMPTY or LEAF hands its own word down, a BRANCH hands
//                     down tree[offset + c]
//   bricks            at level depth-2 an entry with a TWIG on either side is a brick candidate.  k_bricks, one wave per entry of that
//                     level, sixteen entries a wave: lane l reads cell l of each side (the brick's, or the side's one value), applies f, one ballot compare
//                     decides "one value", one ballot of r != a gives the changed cells
//   count             64 bits, one atomic per block (hip_own.h: block_sum64)
//   fold, bricks out  k_fold: a descended entry whose eight results are one EMPTY / LEAF word is that word, else BRANCH | 0;
//                     k_write_bricks one wave per surviving brick, the cells computed again
// The output is sized from the fold's totals (it can exceed either input) and installed by install_rebuilt.  B is read completely
// before A is replaced.  Plain C++ and vector stores; integer arithmetic only.
#include <cstdio>
#include <cstdlib>

#include "tree_rebuild.hip.h"
#include "combine_rule.h"

namespace svo {

namespace {

// One level's entries in visiting order: [n] of each; kids and rank have n + 1 entries (a scan's last item is the total)
struct LevelList {
    uint32_t *wa, *wb;              // the pair of node words
    uint32_t *parent;               // the parent's entry in the level above
    uint32_t *kids;                 // rank among the level's descended entries: the children are entries [8 * kids, 8 * kids + 8) below
    uint32_t *res;                  // the result word (BRANCH / TWIG without an offset)
    uint32_t *rank;                 // after the fold: rank among the entries that stay a BRANCH / TWIG
    uint32_t n;
};

struct Pools { const uint32_t *tree; const uint16_t *twig; uint32_t trees, twigs; };

// a BRANCH the walk follows: above the last level, an 8-block inside the pool behind the root.  off >= 1, where sparse_fill.hip asks
// off > node: the entries here carry words, not pool indices, so "forward" cannot be asked - and need not be: the walk ends at level
// depth-2 and at the arrays' capacity whatever the offsets say
__device__ __forceinline__ bool walk_branch(const Pools &P, uint32_t w, bool last)
{
    const uint32_t off = node_offset(w);
    return node_type(w) == BRANCH && !last && off >= 1u && (uint64_t)off + 8u <= P.trees;
}
// what the walk refuses in one side's word
__device__ __forceinline__ uint32_t walk_error(const Pools &P, uint32_t w, bool last)
{
    if (node_type(w) == BRANCH && !walk_branch(P, w, last)) return ERR_MALFORMED;
    if (node_type(w) == TWIG) return node_offset(w) >= P.twigs ? ERR_MALFORMED : last ? 0u : ERR_SHALLOW_TWIG;
    return 0u;
}

// entry i of level V (edge `edge` cells): descended (kids flag 1), a brick candidate (left to k_bricks), or settled here
__global__ __launch_bounds__(256) void k_walk(Pools A, Pools B, LevelList V, uint32_t last, uint32_t op, uint32_t edge, uint32_t *err, unsigned long long *total)
{
    __shared__ unsigned long long sh[256];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    unsigned long long v = 0ull;
    if (i == V.n) V.kids[i] = 0u;
    if (i < V.n) {
        const uint32_t wa = V.wa[i], wb = V.wb[i];
        const uint32_t bad = max(walk_error(A, wa, last != 0u), walk_error(B, wb, last != 0u));     // (the shallow TWIG outranks the malformed word: both refuse)
        if (bad) *err = bad;
        const bool descend = !bad && (walk_branch(A, wa, last != 0u) || walk_branch(B, wb, last != 0u));
        V.kids[i] = descend ? 1u : 0u;
        if (combine_uniform(wa) && combine_uniform(wb)) {
            const uint32_t a = combine_value(wa), r = combine_cell(op, a, combine_value(wb));
            V.res[i] = combine_word(r);
            if (r != a) v = (unsigned long long)edge * edge * edge;
        } else V.res[i] = node_make(BRANCH, 0);             // (the fold and k_bricks write what it is)
    }
    block_sum64<256>(v, sh, total);
}

// thread t: child t & 7 of entry t >> 3 of level V, into C, whose capacity is `room` entries
__global__ __launch_bounds__(256) void k_children(Pools A, Pools B, LevelList V, LevelList C, uint32_t room)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t i = (uint32_t)(t >> 3), c = (uint32_t)t & 7u;
    if (i >= V.n) return;
    const uint32_t r = V.kids[i];
    if (V.kids[i + 1] == r) return;                         // not descended
    const uint64_t at = 8ull * r + c;
    if (at >= room) return;
    const uint32_t wa = V.wa[i], wb = V.wb[i];
    C.wa[at] = walk_branch(A, wa, false) ? A.tree[node_offset(wa) + c] : wa;
    C.wb[at] = walk_branch(B, wb, false) ? B.tree[node_offset(wb) + c] : wb;
    C.parent[at] = i;
}

// cell `lane` of one side of a brick candidate: the brick's, or the side's one value
__device__ __forceinline__ uint32_t brick_cell(const Pools &P, uint32_t w, uint32_t lane)
{
    if (node_type(w) != TWIG) return combine_value(w);
    const uint32_t off = node_offset(w);
    return off < P.twigs ? P.twig[(size_t)off * TWIG_WORDS + lane] : 0u;
}

// one wave per entry of level depth-2, BRICKS_PER_WAVE entries one after the other: a candidate's result word and its changed cells.
// (With four entries a block, and so one of the count's same-address atomics per four entries, 70 000 entries took 167 us; so 26 us.)
constexpr uint32_t BRICKS_PER_WAVE = 16;
__global__ __launch_bounds__(256) void k_bricks(Pools A, Pools B, LevelList V, uint32_t op, unsigned long long *total)
{
    __shared__ unsigned long long sh[256];
    const uint32_t first = (blockIdx.x * 4u + (threadIdx.x >> 6)) * BRICKS_PER_WAVE, lane = threadIdx.x & 63u;
    unsigned long long v = 0ull;
    for (uint32_t j = 0; j < BRICKS_PER_WAVE; ++j) {
        const uint32_t k = first + j;
        if (k >= V.n) break;
        const uint32_t wa = V.wa[k], wb = V.wb[k];
        if (node_type(wa) != TWIG && node_type(wb) != TWIG) continue;
        const uint32_t a = brick_cell(A, wa, lane), r = combine_cell(op, a, brick_cell(B, wb, lane)), r0 = (uint32_t)__shfl((int)r, 0);
        const bool one = __ballot(r != r0) == 0ull;
        if (r != a) v += 1ull;
        if (lane == 0u) V.res[k] = one ? combine_word(r0) : node_make(TWIG, 0);
    }
    block_sum64<256>(v, sh, total);
}

// the result of every descended entry of level V from its children in C (V.res of the others stands), and the flags of what stays;
// C.n == 0: V is the deepest level, nothing in it is descended
__global__ __launch_bounds__(256) void k_fold(LevelList V, LevelList C)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > V.n) return;
    if (i == V.n) { V.rank[i] = 0u; return; }
    uint32_t r = V.res[i];
    const uint32_t k = V.kids[i];
    if (V.kids[i + 1] != k && 8ull * k + 8ull <= C.n) {
        const uint32_t first = C.res[8u * k];
        bool one = combine_uniform(first);
#pragma unroll
        for (uint32_t c = 1; c < 8u; ++c) one = one && C.res[8u * k + c] == first;
        r = one ? first : node_make(BRANCH, 0);
        V.res[i] = r;
    }
    V.rank[i] = node_type(r) == BRANCH || node_type(r) == TWIG ? 1u : 0u;
}

// one wave per entry of level depth-2: one that stays a TWIG is written as brick V.rank[entry], its cells computed again
__global__ __launch_bounds__(256) void k_write_bricks(Pools A, Pools B, LevelList V, uint32_t op, uint16_t *twig, uint32_t twigs)
{
    const uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (k >= V.n || node_type(V.res[k]) != TWIG) return;
    const uint32_t to = V.rank[k];
    if (to >= twigs) return;
    twig[(size_t)to * TWIG_WORDS + lane] = (uint16_t)combine_cell(op, brick_cell(A, V.wa[k], lane), brick_cell(B, V.wb[k], lane));
}

Pools pools_of(const svo_world &w, int chunk)
{
    const ChunkPools &c = w.chunks[(size_t)chunk];
    const DevChunk &entry = w.table[(size_t)chunk];
    return Pools{ w.hbm->tree.p + entry.tree_off, w.hbm->twig.p + entry.twig_off * TWIG_WORDS, (uint32_t)c.tree_count(), (uint32_t)c.twig_count() };    // (< 2^30: offsets are 30-bit)
}

int combine_resident(svo_world &w, int chunk, const svo_world &src, int src_chunk, uint32_t op, uint64_t *changed_out)
{
    const char *who = "svo_world_chunk_combine";
    HIP_TRY(hipSetDevice(w.device));
    HIP_TRY(hipDeviceSynchronize());                    // ordered behind every launch issued before it, on either world
    hipStream_t s = nullptr;
    const Pools A = pools_of(w, chunk), B = pools_of(src, src_chunk);
    const uint32_t depth = w.chunks[(size_t)chunk].depth, maxlevel = depth - TWIG_LEVELS;
    if (A.trees == 0 || B.trees == 0) { set_error(std::string(who) + ": a chunk has no node words"); return SVO_ERR_INVALID_ARG; }

    // every descended entry holds a BRANCH of A or of B that no other entry holds, and has eight children: at most trees_A + trees_B
    // entries.  Level L's part of each array starts at the entries of the levels above it (kids and rank one entry further per
    // level: every level's scan has n + 1 items)
    const size_t cap = (size_t)A.trees + B.trees;
    size_t need_scan = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need_scan, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)cap + 1, s));
    Arena M;                                            // (declared before `sync`: it outlives the work)
    const size_t k_wa = M.add(cap * 4), k_wb = M.add(cap * 4), k_parent = M.add(cap * 4), k_kids = M.add((cap + maxlevel + 2) * 4), k_res = M.add(cap * 4),
                 k_rank = M.add((cap + maxlevel + 2) * 4), k_tmp = M.add(need_scan + 16), k_words = M.add(256);
    if (const int rc = M.alloc(who, w.device)) return rc;
    SyncAtExit sync{ s };
    const Rebuild R{ who, s, M.at<unsigned char>(k_tmp), need_scan };
    // words: [0] the walk's error, [2, 3] the cells changed (64 bits)
    uint32_t *const words = M.at<uint32_t>(k_words), *const err = words;
    unsigned long long *const total = reinterpret_cast<unsigned long long *>(words + 2);
    HIP_TRY(hipMemsetAsync(words, 0, 256, s));
    auto level_at = [&](size_t first, uint32_t L, uint32_t n) {
        return LevelList{ M.at<uint32_t>(k_wa) + first, M.at<uint32_t>(k_wb) + first, M.at<uint32_t>(k_parent) + first, M.at<uint32_t>(k_kids) + first + L,
                          M.at<uint32_t>(k_res) + first, M.at<uint32_t>(k_rank) + first + L, n };
    };

    // 1. the walk; it settles every entry that is neither descended nor a brick candidate
    std::vector<LevelList> lv;
    lv.push_back(level_at(0, 0, 1));
    HIP_TRY(hipMemcpyAsync(lv[0].wa, A.tree, 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(lv[0].wb, B.tree, 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemsetAsync(lv[0].parent, 0, 4, s));
    size_t used = 1;
    for (uint32_t L = 0;; ++L) {
        const LevelList &V = lv[L];
        hipLaunchKernelGGL(k_walk, dim3(blocks_for((uint64_t)V.n + 1, 256)), dim3(256), 0, s, A, B, V, L == maxlevel ? 1u : 0u, op, (1u << depth) >> L, err, total);
        if (const int rc = launch_status(who)) return rc;
        uint32_t descended = 0;
        if (const int rc = walk_level_tail(R, "a chunk's", V.kids, V.n, err, used, cap, &descended)) return rc;
        if (descended == 0) break;
        LevelList C = level_at(used, L + 1, 8 * descended);
        hipLaunchKernelGGL(k_children, dim3(blocks_for(8ull * V.n, 256)), dim3(256), 0, s, A, B, V, C, C.n);
        if (const int rc = launch_status(who)) return rc;
        used += C.n;
        lv.push_back(C);
    }
    const uint32_t levels = (uint32_t)lv.size();        // (<= maxlevel + 1: k_walk descends no entry of the last level)

    // 2. the brick candidates
    if (levels == maxlevel + 1) {
        hipLaunchKernelGGL(k_bricks, dim3(blocks_for(lv[maxlevel].n, 4 * BRICKS_PER_WAVE)), dim3(256), 0, s, A, B, lv[maxlevel], op, total);
        if (const int rc = launch_status(who)) return rc;
    }
    unsigned long long changed = 0;
    HIP_TRY(hipMemcpyAsync(&changed, total, 8, hipMemcpyDeviceToHost, s));

    // 3. the fold, bottom-up, and the ranks of what stays
    Ranks ranks;
    if (const int rc = fold_and_rank(R, lv, maxlevel, [&](uint32_t L) {
            const LevelList C = L + 1 < levels ? lv[L + 1] : LevelList{ nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0 };
            hipLaunchKernelGGL(k_fold, dim3(blocks_for((uint64_t)lv[L].n + 1, 256)), dim3(256), 0, s, lv[L], C);
        }, ranks)) return rc;
    const uint64_t otrees = ranks.otrees, twigs = ranks.twigs;
    if (otrees > used || (levels == maxlevel + 1 ? twigs > lv[maxlevel].n : twigs != 0)) { set_error(std::string(who) + ": the fold disagrees with the walk"); return SVO_ERR_HIP; }
    if (otrees > (1ull << 30) || twigs > (1ull << 30)) { set_error(std::string(who) + ": 2^30 nodes or bricks"); return SVO_ERR_UNSUPPORTED; }

    // 4. the emit, top-down, into the edits' resident scratch of the destination: sized from the fold's totals, not from A
    uint32_t *otree = nullptr;
    uint16_t *otwig = nullptr;
    if (const int rc = emit_levels(R, w, levels, [&](uint32_t L) { return EmitLevel{ lv[L].res, nullptr, lv[L].parent, lv[L].rank, lv[L].n }; }, ranks, &otree, &otwig)) return rc;
    if (twigs) {
        hipLaunchKernelGGL(k_write_bricks, dim3(blocks_for(lv[maxlevel].n, 4)), dim3(256), 0, s, A, B, lv[maxlevel], op, otwig, (uint32_t)twigs);
        if (const int rc = launch_status(who)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(s));                   // B has been read completely: from here on A is replaced
    if (std::getenv("SVO_BUILD_TIMING"))
        std::fprintf(stderr, "[svo combine] depth %u, op %u: %u + %u node words, %zu entries, %llu node words and %llu bricks out, %llu cells changed, %llu working bytes\n", depth, op,
                     A.trees, B.trees, used, (unsigned long long)otrees, (unsigned long long)twigs, changed, (unsigned long long)M.bytes);
    const int rc = install_rebuilt(w, chunk, depth, nullptr, otrees, twigs, otree, otwig);
    if (rc >= 0 && changed_out) *changed_out = changed;
    return rc;
}

} // namespace

} // namespace svo

using namespace svo;

extern "C" {

int svo_world_chunk_combine(svo_world *dst, int chunk, svo_world *src, int src_chunk, int op, uint64_t *changed_out)
{
    const char *who = "svo_world_chunk_combine";
    if (!dst || !src || chunk < 0 || chunk >= (int)dst->chunks.size() || src_chunk < 0 || src_chunk >= (int)src->chunks.size() || op < 0 || op >= (int)COMBINE_OPS ||
        (dst->device >= 0 && src->device >= 0 && dst->device != src->device)) {
        set_error(std::string(who) + ": bad argument (two worlds, on one device if both are uploaded; a chunk in range in each; a known op)");
        return SVO_ERR_INVALID_ARG;
    }
    if (dst->device < 0 || src->device < 0) { set_error(std::string(who) + ": a world is not uploaded (svo_chunk_combine combines host pools)"); return SVO_ERR_NOT_UPLOADED; }
    const uint32_t depth = dst->chunks[(size_t)chunk].depth;
    if (depth != src->chunks[(size_t)src_chunk].depth) { set_error(std::string(who) + ": the two chunks differ in depth"); return SVO_ERR_UNSUPPORTED; }
    if (depth < SVO_COMBINE_MIN_DEPTH || depth > SVO_COMBINE_MAX_DEPTH) { set_error(std::string(who) + ": the chunks' depth is outside [2, 16]"); return SVO_ERR_UNSUPPORTED; }
    return fenced(who, [&] { return combine_resident(*dst, chunk, *src, src_chunk, (uint32_t)op, changed_out); });
}

} // extern "C"
