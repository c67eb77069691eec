// extract.hip — svo_world_chunk_extract: a cube of N_C^3 cells copied out of chunk A at an integer cell offset, in one of the 48
// orientations of the cube, into chunk C of depth D_C <= D_A, on the device the two worlds live on, without a dense grid, depth
// 2 .. 16.  The inverse of svo_world_chunk_stamp (stamp.hip).  extract.cpp is the host twin and states the extract as a recursive walk
// over entries, a fold and a FIFO emit; extract_rule.h holds the window.  On the null stream, behind a hipDeviceSynchronize like
// svo_world_chunk_stamp; complete at the return.  tree_rebuild.hip.h holds the frame of the rebuild (the walk's tail, the fold's
// ranks, the emit); this file's own:
//   root              k_root, one lane per neighbour of C's root: the node of A at level D_A - D_C and index floor(offset / N_C) + j,
//                     by a descent from A's root that checks every offset before it follows it; an index outside A is EMPTY.  Its
//                     error word is read back with the first level's
//   walk              An entry is a node of C: its corner (3 x 16 bits; its edge is its level's) and the 2x2x2 neighbourhood of A's
//                     node words of the same edge that its image can overlap: eight words.  There is no destination word and no cell
//                     function: k_walk settles an entry whose overlapped neighbours are uniform with one value - that value's word,
//                     edge^3 cells counted if it is not 0 -, flags every other entry above edge 4 to descend and checks every offset
//                     against A's pool; k_children, one thread per child in C's slot order: each neighbour from one of the parent's
//                     eight, in A's frame (stamp_step, extract_hand_down).  The orientation enters only through the image's corner
//   capacity          the entries follow the RESULT: every level's arrays are taken from the pool cache when the level above has
//                     been counted, 8 x its descended entries; 2^30 entries are refused
//   bricks            at edge 4 an entry that is not settled is a brick candidate.  k_bricks, one wave per candidate, sixteen entries
//                     a wave: lane l is C's cell l and reads the neighbour its image falls into and the cell in it (extract_cell)
//   count             64 bits, one atomic per block (hip_own.h: block_sum64)
//   fold, bricks out  as stamp.hip's: k_fold; k_write_bricks one wave per surviving brick, the cells computed again
// The walk visits only what the window reaches.  A is read completely before C is installed, so C may be A.  Plain C++ and vector
// stores; integer arithmetic only.
#include <cstdio>
#include <cstdlib>

#include "tree_rebuild.hip.h"
#include "extract_rule.h"

namespace svo {

namespace {

// One level's entries in visiting order: [n] of each, nb [8][n]; kids and rank have n + 1 entries (a scan's last item is the total)
struct LevelList {
    uint32_t *nb;                   // neighbour j of entry i: nb[j * n + i]
    uint32_t *xy;                   // the corner in C: x | y << 16
    uint16_t *z;
    uint32_t *parent;               // the parent's entry in the level above
    uint32_t *kids;                 // rank among the level's descended entries: the children are entries [8 * kids, 8 * kids + 8) below
    uint32_t *res;                  // the result word (BRANCH / TWIG without an offset)
    uint32_t *rank;                 // after the fold: rank among the entries that stay a BRANCH / TWIG
    uint32_t n;
};

struct Pools { const uint32_t *tree; const uint16_t *twig; uint32_t trees, twigs; };

// a BRANCH the walk follows, as stamp.hip's: above the last level, an 8-block inside the pool behind the root
__device__ __forceinline__ bool walk_branch(const Pools &P, uint32_t w, bool last)
{
    const uint32_t off = node_offset(w);
    return node_type(w) == BRANCH && !last && off >= 1u && (uint64_t)off + 8u <= P.trees;
}
// what the walk refuses in a word of A
__device__ __forceinline__ uint32_t walk_error(const Pools &P, uint32_t w, bool last)
{
    if (node_type(w) == BRANCH && !walk_branch(P, w, last)) return ERR_MALFORMED;
    if (node_type(w) == TWIG) return node_offset(w) >= P.twigs ? ERR_MALFORMED : last ? 0u : ERR_SHALLOW_TWIG;
    return 0u;
}

__device__ __forceinline__ void corner_of(const LevelList &V, uint32_t i, uint32_t x[3])
{
    const uint32_t xy = V.xy[i];
    x[0] = xy & 0xFFFFu; x[1] = xy >> 16; x[2] = V.z[i];
}

// lane j < 8: neighbour j of C's root into V (one entry, corner 0).  A BRANCH whose block lies outside the pool is not followed
__global__ __launch_bounds__(64) void k_root(Pools A, LevelList V, ExtractPlace E, uint32_t depth_a, uint32_t *err)
{
    const uint32_t j = threadIdx.x;
    if (j >= 8u) return;
    uint32_t left = 0u, bad = 0u;
    const uint32_t w = extract_root_word(E, depth_a, j, A.tree[0], &left, [&](uint32_t at, uint32_t slot) {
        if (walk_branch(A, at, false)) return A.tree[node_offset(at) + slot];
        bad = ERR_MALFORMED;
        return node_make(EMPTY, 0);
    });
    if (!bad && left > 0u && node_type(w) == TWIG) bad = ERR_SHALLOW_TWIG;
    if (bad) *err = bad;
    V.nb[j] = w;                                            // (n = 1: nb[j * n + 0])
    if (j == 0u) { V.xy[0] = 0u; V.z[0] = 0; V.parent[0] = 0u; }
}

// entry i of level V (edge 2^shift cells): settled here, descended (kids flag 1), or - at the last level - a brick candidate (res TWIG | 0, left to k_bricks)
__global__ __launch_bounds__(256) void k_walk(Pools A, LevelList V, ExtractPlace E, uint32_t last, uint32_t shift, uint32_t *err, unsigned long long *total)
{
    __shared__ unsigned long long sh[256];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    unsigned long long count = 0ull;
    if (i == V.n) V.kids[i] = 0u;
    if (i < V.n) {
        uint32_t nb[8], x[3];
        uint32_t bad = 0u;
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            nb[j] = V.nb[(size_t)j * V.n + i];
            bad = max(bad, walk_error(A, nb[j], last != 0u));                           // (the shallow TWIG outranks the malformed word: both refuse)
        }
        if (bad) *err = bad;
        corner_of(V, i, x);
        const StampHood H = extract_hood(E, x, shift);
        uint32_t v = 0u;
        const bool settled = extract_settled(nb, H.unaligned, &v);
        V.kids[i] = !bad && !settled && !last ? 1u : 0u;
        if (settled) {
            V.res[i] = combine_word(v);
            if (v != 0u) count = 1ull << (3u * shift);
        } else V.res[i] = node_make(last ? TWIG : BRANCH, 0);      // (the fold and k_bricks write what it is)
    }
    block_sum64<256>(count, sh, total);
}

// thread t: child t & 7 of entry t >> 3 of level V (edge 2^shift), into C, whose capacity is its n
__global__ __launch_bounds__(256) void k_children(Pools A, LevelList V, LevelList C, ExtractPlace E, uint32_t shift)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t i = (uint32_t)(t >> 3), c = (uint32_t)t & 7u;
    if (i >= V.n) return;
    const uint32_t r = V.kids[i];
    if (V.kids[i + 1] == r) return;                         // not descended
    const uint64_t at = 8ull * r + c;
    if (at >= C.n) return;
    const uint32_t h = 1u << (shift - 1u);
    uint32_t x[3];
    corner_of(V, i, x);
    const StampHood H = extract_hood(E, x, shift);
    x[0] += (c & 1u) * h; x[1] += ((c >> 1) & 1u) * h; x[2] += (c >> 2) * h;
    const StampHood Hc = extract_hood(E, x, shift - 1u);
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) {
        const StampStep S = stamp_step(H, Hc, j);
        const uint32_t w = V.nb[(size_t)S.from * V.n + i];                              // (k_walk has checked it: a BRANCH's block lies inside the pool)
        C.nb[(size_t)j * C.n + at] = extract_hand_down(walk_branch(A, w, false) || node_type(w) != BRANCH ? w : node_make(EMPTY, 0), S.slot,
                                                       [&](uint32_t k) { return A.tree[k]; });
    }
    C.xy[at] = x[0] | x[1] << 16;
    C.z[at] = (uint16_t)x[2];
    C.parent[at] = i;
}

// cell `lane` of C's candidate k: A's cell from the neighbour the lane's image falls into
__device__ __forceinline__ uint32_t cell_out(const Pools &A, const LevelList &V, const ExtractPlace &E, uint32_t k, uint32_t lane)
{
    uint32_t x[3];
    corner_of(V, k, x);
    const StampCell at = extract_cell(E, extract_hood(E, x, TWIG_LEVELS), x, lane & 3u, (lane >> 2) & 3u, lane >> 4);
    const uint32_t wa = V.nb[(size_t)at.from * V.n + k], off = node_offset(wa);
    return node_type(wa) != TWIG ? combine_value(wa) : off < A.twigs ? A.twig[(size_t)off * TWIG_WORDS + at.index] : 0u;
}

// one wave per entry of the last level, BRICKS_PER_WAVE entries one after the other: a candidate's result word and its occupied cells
constexpr uint32_t BRICKS_PER_WAVE = 16;
__global__ __launch_bounds__(256) void k_bricks(Pools A, LevelList V, ExtractPlace E, unsigned long long *total)
{
    __shared__ unsigned long long sh[256];
    const uint32_t first = (blockIdx.x * 4u + (threadIdx.x >> 6)) * BRICKS_PER_WAVE, lane = threadIdx.x & 63u;
    unsigned long long count = 0ull;
    for (uint32_t j = 0; j < BRICKS_PER_WAVE; ++j) {
        const uint32_t k = first + j;
        if (k >= V.n) break;
        if (node_type(V.res[k]) != TWIG) continue;          // settled by k_walk
        const uint32_t r = cell_out(A, V, E, k, lane), r0 = (uint32_t)__shfl((int)r, 0);
        const bool one = __ballot(r != r0) == 0ull;
        if (r != 0u) count += 1ull;
        if (lane == 0u && one) V.res[k] = combine_word(r0);
    }
    block_sum64<256>(count, sh, total);
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

// one wave per entry of the last level: one that stays a TWIG is written as brick V.rank[entry], its cells computed again
__global__ __launch_bounds__(256) void k_write_bricks(Pools A, LevelList V, ExtractPlace E, uint16_t *twig, uint32_t twigs)
{
    const uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (k >= V.n || node_type(V.res[k]) != TWIG) return;
    const uint32_t to = V.rank[k];
    if (to >= twigs) return;
    twig[(size_t)to * TWIG_WORDS + lane] = (uint16_t)cell_out(A, V, E, k, lane);
}

Pools pools_of(const svo_world &w, int chunk)
{
    const ChunkPools &c = w.chunks[(size_t)chunk];
    const DevChunk &entry = w.table[(size_t)chunk];
    return Pools{ w.hbm->tree.p + entry.tree_off, w.hbm->twig.p + entry.twig_off * TWIG_WORDS, (uint32_t)c.tree_count(), (uint32_t)c.twig_count() };    // (< 2^30: offsets are 30-bit)
}

// One level's arrays and the scratch of its scans, n entries, as one buffer of the pool cache
struct Level { Arena M; LevelList V; unsigned char *tmp; size_t need_scan; };
int level_take(const char *who, int device, hipStream_t s, uint32_t n, Level &L)
{
    L.need_scan = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, L.need_scan, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)n + 1, s));
    Arena &M = L.M;
    const size_t words = (size_t)n * 4, k_nb = M.add(8 * words), k_xy = M.add(words), k_z = M.add((size_t)n * 2), k_parent = M.add(words), k_kids = M.add(words + 4),
                 k_res = M.add(words), k_rank = M.add(words + 4), k_tmp = M.add(L.need_scan + 16);
    if (const int rc = M.alloc(who, device)) return rc;
    L.V = LevelList{ M.at<uint32_t>(k_nb), M.at<uint32_t>(k_xy), M.at<uint16_t>(k_z), M.at<uint32_t>(k_parent), M.at<uint32_t>(k_kids), M.at<uint32_t>(k_res),
                     M.at<uint32_t>(k_rank), n };
    L.tmp = M.at<unsigned char>(k_tmp);
    return SVO_OK;
}

int extract_resident(svo_world &w, int chunk, const svo_world &src, int src_chunk, const svo_placement &pl, uint64_t *occupied_out)
{
    const char *who = "svo_world_chunk_extract";
    HIP_TRY(hipSetDevice(w.device));
    HIP_TRY(hipDeviceSynchronize());                    // ordered behind every launch issued before it, on either world
    hipStream_t s = nullptr;
    const Pools A = pools_of(src, src_chunk);
    const uint32_t depth = w.chunks[(size_t)chunk].depth, depth_a = src.chunks[(size_t)src_chunk].depth, maxlevel = depth - TWIG_LEVELS;
    const ExtractPlace E{ stamp_place(pl.offset, pl.orient), depth };
    if (A.trees == 0) { set_error(std::string(who) + ": the source chunk has no node words"); return SVO_ERR_INVALID_ARG; }

    std::vector<Level> mem(maxlevel + 1);               // (declared before `sync`: the arenas outlive the work)
    Arena M;
    const size_t k_words = M.add(256);
    if (const int rc = M.alloc(who, w.device)) return rc;
    SyncAtExit sync{ s };
    // words: [0] the walk's error, [2, 3] the occupied cells (64 bits)
    uint32_t *const words = M.at<uint32_t>(k_words), *const err = words;
    unsigned long long *const total = reinterpret_cast<unsigned long long *>(words + 2);
    HIP_TRY(hipMemsetAsync(words, 0, 256, s));

    // 1. the root's neighbourhood, by a descent of its own, and the walk; it settles every entry that is neither descended nor a
    //    brick candidate
    if (const int rc = level_take(who, w.device, s, 1, mem[0])) return rc;
    std::vector<LevelList> lv(1, mem[0].V);
    hipLaunchKernelGGL(k_root, dim3(1), dim3(64), 0, s, A, lv[0], E, depth_a, err);
    if (const int rc = launch_status(who)) return rc;
    size_t used = 1, bytes = M.bytes + mem[0].M.bytes, longest = 0;
    for (uint32_t L = 0;; ++L) {
        const LevelList &V = lv[L];
        hipLaunchKernelGGL(k_walk, dim3(blocks_for((uint64_t)V.n + 1, 256)), dim3(256), 0, s, A, V, E, L == maxlevel ? 1u : 0u, depth - L, err, total);
        if (const int rc = launch_status(who)) return rc;
        uint32_t descended = 0;
        const Rebuild R{ who, s, mem[L].tmp, mem[L].need_scan };
        if (const int rc = walk_level_tail(R, "the source chunk's", V.kids, V.n, err, 0, ~(size_t)0, &descended)) return rc;    // (no capacity to run out of: the next level is sized from the total)
        if (descended == 0) break;
        if (L == maxlevel) { set_error(std::string(who) + ": the walk descended below the bricks"); return SVO_ERR_HIP; }
        if (used + 8ull * descended > (1ull << 30)) { set_error(std::string(who) + ": 2^30 entries"); return SVO_ERR_UNSUPPORTED; }
        if (const int rc = level_take(who, w.device, s, 8 * descended, mem[L + 1])) return rc;
        const LevelList C = mem[L + 1].V;
        hipLaunchKernelGGL(k_children, dim3(blocks_for(8ull * V.n, 256)), dim3(256), 0, s, A, V, C, E, depth - L);
        if (const int rc = launch_status(who)) return rc;
        used += C.n;
        bytes += mem[L + 1].M.bytes;
        if (C.n > lv[longest].n) longest = L + 1;
        lv.push_back(C);
    }
    const uint32_t levels = (uint32_t)lv.size();        // (<= maxlevel + 1)
    const Rebuild R{ who, s, mem[longest].tmp, mem[longest].need_scan };

    // 2. the brick candidates
    if (levels == maxlevel + 1) {
        hipLaunchKernelGGL(k_bricks, dim3(blocks_for(lv[maxlevel].n, 4 * BRICKS_PER_WAVE)), dim3(256), 0, s, A, lv[maxlevel], E, total);
        if (const int rc = launch_status(who)) return rc;
    }
    unsigned long long occupied = 0;
    HIP_TRY(hipMemcpyAsync(&occupied, total, 8, hipMemcpyDeviceToHost, s));

    // 3. the fold, bottom-up, and the ranks of what stays
    Ranks ranks;
    if (const int rc = fold_and_rank(R, lv, maxlevel, [&](uint32_t L) {
            const LevelList C = L + 1 < levels ? lv[L + 1] : LevelList{ nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0 };
            hipLaunchKernelGGL(k_fold, dim3(blocks_for((uint64_t)lv[L].n + 1, 256)), dim3(256), 0, s, lv[L], C);
        }, ranks)) return rc;
    const uint64_t otrees = ranks.otrees, twigs = ranks.twigs;
    if (otrees > used || (levels == maxlevel + 1 ? twigs > lv[maxlevel].n : twigs != 0)) { set_error(std::string(who) + ": the fold disagrees with the walk"); return SVO_ERR_HIP; }
    if (otrees > (1ull << 30) || twigs > (1ull << 30)) { set_error(std::string(who) + ": 2^30 nodes or bricks"); return SVO_ERR_UNSUPPORTED; }

    // 4. the emit, top-down, into the edits' resident scratch of the destination: sized from the fold's totals
    uint32_t *otree = nullptr;
    uint16_t *otwig = nullptr;
    if (const int rc = emit_levels(R, w, levels, [&](uint32_t L) { return EmitLevel{ lv[L].res, nullptr, lv[L].parent, lv[L].rank, lv[L].n }; }, ranks, &otree, &otwig)) return rc;
    if (twigs) {
        hipLaunchKernelGGL(k_write_bricks, dim3(blocks_for(lv[maxlevel].n, 4)), dim3(256), 0, s, A, lv[maxlevel], E, otwig, (uint32_t)twigs);
        if (const int rc = launch_status(who)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(s));                   // A has been read completely: from here on C is installed
    if (std::getenv("SVO_BUILD_TIMING"))
        std::fprintf(stderr, "[svo extract] depth %u <- %u, orient %u: %u node words, %zu entries, %llu node words and %llu bricks out, %llu cells occupied, %llu working bytes\n",
                     depth, depth_a, pl.orient, A.trees, used, (unsigned long long)otrees, (unsigned long long)twigs, occupied, (unsigned long long)bytes);
    const int rc = install_rebuilt(w, chunk, depth, nullptr, otrees, twigs, otree, otwig);
    if (rc >= 0 && occupied_out) *occupied_out = occupied;
    return rc;
}

} // namespace

} // namespace svo

using namespace svo;

extern "C" {

int svo_world_chunk_extract(svo_world *dst, int chunk, svo_world *src, int src_chunk, const svo_placement *pl, uint64_t *occupied_out)
{
    const char *who = "svo_world_chunk_extract";
    if (!dst || !src || chunk < 0 || chunk >= (int)dst->chunks.size() || src_chunk < 0 || src_chunk >= (int)src->chunks.size() ||
        (dst->device >= 0 && src->device >= 0 && dst->device != src->device) || !pl || !stamp_placement_ok(pl->offset, pl->orient)) {
        set_error(std::string(who) + ": bad argument (two worlds, on one device if both are uploaded; a chunk in range in each; a placement with orient <= 47 and offsets in "
                                     "[-65536, 65536])");
        return SVO_ERR_INVALID_ARG;
    }
    if (dst->device < 0 || src->device < 0) { set_error(std::string(who) + ": a world is not uploaded (svo_chunk_extract extracts from host pools)"); return SVO_ERR_NOT_UPLOADED; }
    const uint32_t dc = dst->chunks[(size_t)chunk].depth, da = src->chunks[(size_t)src_chunk].depth;
    if (dc > da) { set_error(std::string(who) + ": the destination chunk is deeper than the source (that direction is the stamp into an empty chunk)"); return SVO_ERR_UNSUPPORTED; }
    if (dc < EXTRACT_MIN_DEPTH || da > EXTRACT_MAX_DEPTH) { set_error(std::string(who) + ": a chunk's depth is outside [2, 16]"); return SVO_ERR_UNSUPPORTED; }
    return fenced(who, [&] { return extract_resident(*dst, chunk, *src, src_chunk, *pl, occupied_out); });
}

} // extern "C"
