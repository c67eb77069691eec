// sparse_fill.hip — svo_world_chunk_fill_enclosed: svo_grid_fill_enclosed's rule applied to a chunk of an uploaded world on its tree,
// without the dense grid, depth 2 .. 16.  sparse_fill.cpp is the host twin and states the fill as a walk, a queue flood, a fold and a
// FIFO emit; sparse_fill_rule.h holds the bit arithmetic of a brick's 64-bit mask.  On the world's device, on the null stream, behind
// a hipDeviceSynchronize like svo_world_chunk_from_mesh; complete at the return.  tree_rebuild.hip.h holds the frame of the rebuild
// (the walk's tail, the fold's ranks, the emit); this file's own:
//   walk              An entry is { old pool index, corner in cells, parent's entry }.  k_walk flags the BRANCHes of the level's list
//                     (and checks every offset against the pools), k_children appends their eight children to the next level's list
//   state             one byte per node word ("the EMPTY node here is OUTSIDE") and two 64-bit masks per brick (its empty cells, its
//                     OUTSIDE cells).  k_seed_nodes lists the EMPTY nodes (block_take: one atomic per block) and raises those that touch
//                     a face of the chunk; k_brick_slots / k_seed_bricks number the TWIGs of the last level and seed their border cells
//   sweeps            every adjacency is served by its smaller side, the brick at equal size.  k_sweep_bricks, one thread per brick:
//                     across each face the neighbour block by integer descent from the root; a TWIG's facing bits and an EMPTY node's
//                     flag are pulled, the brick floods inside its own word (shifts by 1, 4, 16 in registers), its outside face cells
//                     raise an EMPTY neighbour.  k_sweep_nodes, one thread per EMPTY node: the descent stops at the node's own level;
//                     two EMPTY nodes exchange in both directions.  The state only ever moves towards the fixed point, so the plain racy
//                     stores are harmless (the argument of mesh.hip's k_fill_sweep).  The host launches SWEEP_BATCH sweeps, reads the
//                     last one's "something changed" word and stops at 0: no number of sweeps is assumed
//   count             edge^3 per EMPTY node that is not outside + a popcount per brick, 64 bits, one atomic per block (block_sum64)
//   fold, bricks out  k_fold writes every reached node's result word into an array indexed by the old pool (k_emit reads it through
//                     the entries' pool indices); k_write_bricks one wave per surviving brick with the fill applied
// The install is svo_world_chunk_from_grid's (install_rebuilt).  Plain C++ and vector stores; integer arithmetic only.
#include <cstdio>
#include <cstdlib>

#include "tree_rebuild.hip.h"
#include "sparse_fill_rule.h"

namespace svo {

namespace {

constexpr uint32_t SWEEP_BATCH = 8;
constexpr uint32_t NONE = 0xFFFFFFFFu;

// One level's reached nodes in visiting order: [n] of each, rank has n + 1 entries (a scan's last item is the total)
struct LevelList {
    uint32_t *node;                 // index of the node word in the chunk's (old) pool
    uint32_t *xy, *z;               // its corner in cells: x | y << 16, z
    uint32_t *parent;               // its parent's entry in the level above
    uint32_t *rank;                 // the walk: rank among the level's BRANCHes; after the fold: among the BRANCHes / TWIGs that stay
    uint32_t n;
};

struct Pools { const uint32_t *tree; const uint16_t *twig; uint32_t trees, twigs, depth; };

// a BRANCH the walk follows: above the last level, a forward 8-block inside the pool (what validate_chunk asks).  off > node, where
// combine.hip can only ask off >= 1: the entries here carry pool indices, so a back edge is seen where it is met
__device__ __forceinline__ bool walk_branch(const Pools &P, uint32_t node, uint32_t w, bool last)
{
    const uint32_t off = node_offset(w);
    return node_type(w) == BRANCH && !last && off > node && (uint64_t)off + 8u <= P.trees;
}

__global__ __launch_bounds__(256) void k_walk(Pools P, LevelList V, uint32_t last, uint32_t *err)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > V.n) return;
    if (i == V.n) { V.rank[i] = 0u; return; }
    const uint32_t node = V.node[i], w = P.tree[node], type = node_type(w);
    const bool follow = walk_branch(P, node, w, last != 0u);
    if (type == BRANCH && !follow) *err = ERR_MALFORMED;
    if (type == TWIG && node_offset(w) >= P.twigs) *err = ERR_MALFORMED;
    else if (type == TWIG && !last) *err = ERR_SHALLOW_TWIG;
    V.rank[i] = follow ? 1u : 0u;
}

// the eight children of every BRANCH of level V (edge `half` cells each) into C, whose capacity is `room` entries
__global__ __launch_bounds__(256) void k_children(Pools P, LevelList V, uint32_t half, LevelList C, uint32_t room)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= V.n) return;
    const uint32_t node = V.node[i], w = P.tree[node];
    if (!walk_branch(P, node, w, false)) return;
    const uint32_t r = V.rank[i], xy = V.xy[i], z = V.z[i];
    if (8ull * r + 8ull > room) return;
#pragma unroll
    for (uint32_t c = 0; c < 8u; ++c) {
        const uint32_t at = 8u * r + c;
        C.node[at] = node_offset(w) + c;
        C.xy[at] = xy + (c & 1u) * half + (((c >> 1) & 1u) * half << 16);
        C.z[at] = z + (c >> 2) * half;
        C.parent[at] = i;
    }
}

// the EMPTY nodes of level V (edge `edge` cells) join `elist` { node, xy, z, edge }; one that touches a face of the chunk is OUTSIDE
__global__ __launch_bounds__(256) void k_seed_nodes(Pools P, LevelList V, uint32_t edge, uint8_t *outside, uint4 *elist, uint32_t *ecount, uint32_t room)
{
    __shared__ uint32_t sh[256 / 64 + 1];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, N = 1u << P.depth;
    uint32_t node = 0u;
    bool hollow = false;
    if (i < V.n) { node = V.node[i]; hollow = fill_is_empty(P.tree[node]); }
    const uint32_t at = block_take<256>(ecount, hollow, sh);
    if (!hollow || at >= room) return;
    const uint32_t xy = V.xy[i], x = xy & 0xFFFFu, y = xy >> 16, z = V.z[i];
    elist[at] = make_uint4(node, xy, z, edge);
    if (x == 0u || y == 0u || z == 0u || x + edge == N || y + edge == N || z + edge == N) outside[node] = 1;
}

// the TWIGs of the last level, numbered in visiting order (V.rank holds the scan of their flags): slot[node] and where[slot] = entry
__global__ __launch_bounds__(256) void k_twig_flags(Pools P, LevelList V)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > V.n) return;
    V.rank[i] = i < V.n && node_type(P.tree[V.node[i]]) == TWIG ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_brick_slots(Pools P, LevelList V, uint32_t *slot, uint32_t *where, uint32_t nbricks)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= V.n) return;
    const uint32_t node = V.node[i];
    if (node_type(P.tree[node]) != TWIG) return;
    const uint32_t k = V.rank[i];
    if (k >= nbricks) return;
    slot[node] = k;
    where[k] = i;
}

struct Bricks { const uint32_t *where; unsigned long long *empty, *out; uint32_t n; };

// one wave per brick: its empty cells (one ballot) and, flooded from them, those with a coordinate of 0 or N - 1
__global__ __launch_bounds__(256) void k_seed_bricks(Pools P, LevelList V, Bricks B)
{
    const uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (k >= B.n) return;
    const uint32_t i = B.where[k], off = node_offset(P.tree[V.node[i]]);
    const unsigned long long empty = __ballot(off < P.twigs && P.twig[(size_t)off * TWIG_WORDS + lane] == 0);
    if (lane != 0u) return;
    const uint32_t xy = V.xy[i];
    B.empty[k] = empty;
    B.out[k] = fill_flood_brick(fill_border_cells(xy & 0xFFFFu, xy >> 16, V.z[i], 1u << P.depth), empty);
}

struct Found { uint32_t node, w; };
// the node that holds cell (x, y, z): the descent from the root, stopped at level `stop` or at the first node that is no BRANCH
__device__ __forceinline__ Found fill_descend(const Pools &P, uint32_t x, uint32_t y, uint32_t z, uint32_t stop)
{
    Found f{ 0u, P.tree[0] };
    for (uint32_t level = 0; level < stop && node_type(f.w) == BRANCH;) {
        ++level;
        const uint32_t lg = P.depth - level;
        f.node = node_offset(f.w) + (((x >> lg) & 1u) | ((y >> lg) & 1u) << 1 | ((z >> lg) & 1u) << 2);
        if (f.node >= P.trees) { f.node = 0u; f.w = node_make(LEAF, 1); break; }       // (no validated pool: it gives nothing)
        f.w = P.tree[f.node];
    }
    return f;
}
// the cell behind face f of the cube (x, y, z) of `edge` cells; false at a face of the chunk
__device__ __forceinline__ bool fill_behind(uint32_t f, uint32_t edge, uint32_t N, uint32_t &x, uint32_t &y, uint32_t &z)
{
    uint32_t &c = f < 2u ? x : f < 4u ? y : z;
    if (f & 1u) { if (c + edge == N) return false; c += edge; }
    else { if (c == 0u) return false; c -= 1u; }
    return true;
}

__global__ __launch_bounds__(256) void k_sweep_bricks(Pools P, LevelList V, Bricks B, const uint32_t *__restrict__ slot, uint8_t *outside, uint32_t *changed)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= B.n) return;
    const uint32_t i = B.where[k], xy = V.xy[i], N = 1u << P.depth, maxlevel = P.depth - TWIG_LEVELS;
    const unsigned long long empty = B.empty[k], old = B.out[k];
    unsigned long long o = old;
    uint32_t hollow[6];
#pragma unroll
    for (uint32_t f = 0; f < 6u; ++f) {
        hollow[f] = NONE;
        uint32_t x = xy & 0xFFFFu, y = xy >> 16, z = V.z[i];
        if (!fill_behind(f, TWIG_SIZE, N, x, y, z)) continue;
        const Found nb = fill_descend(P, x, y, z, maxlevel);
        if (node_type(nb.w) == TWIG) {
            const uint32_t s = slot[nb.node];
            if (s < B.n) o |= fill_face_pull(B.out[s], f ^ 1u) & empty;
        } else if (fill_is_empty(nb.w)) {
            hollow[f] = nb.node;
            if (outside[nb.node]) o |= fill_face(f) & empty;
        }
    }
    o = fill_flood_brick(o, empty);
    bool moved = o != old;
    if (moved) B.out[k] = o;
#pragma unroll
    for (uint32_t f = 0; f < 6u; ++f)
        if (hollow[f] != NONE && (o & fill_face(f)) != 0ull && !outside[hollow[f]]) { outside[hollow[f]] = 1; moved = true; }
    if (moved) *changed = 1u;
}

__global__ __launch_bounds__(256) void k_sweep_nodes(Pools P, const uint4 *__restrict__ elist, uint32_t n, uint8_t *outside, uint32_t *changed)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint4 e = elist[j];                               // { node, xy, z, edge }
    const uint32_t N = 1u << P.depth, level = P.depth - (31u - (uint32_t)__clz((int)e.w));
    bool me = outside[e.x] != 0, moved = false;
#pragma unroll
    for (uint32_t f = 0; f < 6u; ++f) {
        uint32_t x = e.y & 0xFFFFu, y = e.y >> 16, z = e.z;
        if (!fill_behind(f, e.w, N, x, y, z)) continue;
        const Found nb = fill_descend(P, x, y, z, level);
        if (!fill_is_empty(nb.w)) continue;                 // a BRANCH or a TWIG: the smaller side serves the adjacency; a LEAF gives nothing
        const bool other = outside[nb.node] != 0;
        if (other == me) continue;
        outside[e.x] = 1; outside[nb.node] = 1;
        me = true; moved = true;
    }
    if (moved) *changed = 1u;
}

// thread t < ne: EMPTY node t; ne <= t < ne + B.n: brick t - ne
__global__ __launch_bounds__(256) void k_count(const uint4 *__restrict__ elist, uint32_t ne, const uint8_t *__restrict__ outside, Bricks B, unsigned long long *total)
{
    __shared__ unsigned long long sh[256];
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    unsigned long long v = 0ull;
    if (t < ne) {
        const uint4 e = elist[t];
        if (!outside[e.x]) v = (unsigned long long)e.w * e.w * e.w;
    } else if (t - ne < B.n) v = (unsigned long long)__popcll(B.empty[t - ne] & ~B.out[t - ne]);
    block_sum64<256>(v, sh, total);
}

// res[node] of every node of level V (the levels below are done): BRANCH | 0 and TWIG | 0 for what stays one; V.rank flags those
__global__ __launch_bounds__(256) void k_fold(Pools P, LevelList V, uint32_t last, const uint8_t *__restrict__ outside, const uint32_t *__restrict__ slot, Bricks B,
                                              uint32_t material, uint32_t *res)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > V.n) return;
    if (i == V.n) { V.rank[i] = 0u; return; }
    const uint32_t node = V.node[i], w = P.tree[node], type = node_type(w);
    uint32_t r;
    if (walk_branch(P, node, w, last != 0u)) {
        const uint32_t first = res[node_offset(w)];
        bool one = node_type(first) != BRANCH && node_type(first) != TWIG;
#pragma unroll
        for (uint32_t c = 1; c < 8u; ++c) one = one && res[node_offset(w) + c] == first;
        r = one ? first : node_make(BRANCH, 0);
    } else if (type == TWIG) {
        const uint32_t s = slot[node], off = node_offset(w);
        r = s < B.n && off < P.twigs ? fill_brick_result(P.twig + (size_t)off * TWIG_WORDS, B.empty[s] & ~B.out[s], material) : node_make(EMPTY, 0);
    } else if (fill_is_empty(w)) r = outside[node] ? node_make(EMPTY, 0) : node_make(LEAF, material);
    else r = type == LEAF ? node_make(LEAF, node_offset(w) & 0xFFFFu) : node_make(EMPTY, 0);
    res[node] = r;
    V.rank[i] = node_type(r) == BRANCH || node_type(r) == TWIG ? 1u : 0u;
}

// one wave per brick of the input: one that stays is written, the fill applied, as brick V.rank[its entry]
__global__ __launch_bounds__(256) void k_write_bricks(Pools P, LevelList V, Bricks B, const uint32_t *__restrict__ res, uint32_t material, uint16_t *twig, uint32_t twigs)
{
    const uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (k >= B.n) return;
    const uint32_t i = B.where[k], node = V.node[i], off = node_offset(P.tree[node]), to = V.rank[i];
    if (node_type(res[node]) != TWIG || to >= twigs || off >= P.twigs) return;
    const bool in = (((B.empty[k] & ~B.out[k]) >> lane) & 1ull) != 0ull;
    twig[(size_t)to * TWIG_WORDS + lane] = in ? (uint16_t)material : P.twig[(size_t)off * TWIG_WORDS + lane];
}

int fill_resident(svo_world &w, int chunk, uint32_t material, uint64_t *filled_out)
{
    const char *who = "svo_world_chunk_fill_enclosed";
    HIP_TRY(hipSetDevice(w.device));
    HIP_TRY(hipDeviceSynchronize());                    // ordered behind every launch issued before it, like svo_world_chunk_from_mesh
    hipStream_t s = nullptr;
    const ChunkPools &c = w.chunks[(size_t)chunk];
    const DevChunk &entry = w.table[(size_t)chunk];
    Pools P;
    P.tree = w.hbm->tree.p + entry.tree_off;
    P.twig = w.hbm->twig.p + entry.twig_off * TWIG_WORDS;
    P.trees = (uint32_t)c.tree_count(); P.twigs = (uint32_t)c.twig_count();    // (< 2^30: offsets are 30-bit)
    P.depth = c.depth;
    const uint32_t depth = c.depth, maxlevel = depth - TWIG_LEVELS, trees = P.trees;
    if (trees == 0) { set_error(std::string(who) + ": the chunk has no node words"); return SVO_ERR_INVALID_ARG; }

    // the arrays that are proportional to the node words: level L's part of each starts at the nodes of the levels above it
    // (its ranks one entry further per level: every level's scan has n + 1 items)
    size_t need_scan = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need_scan, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)trees + 1, s));
    Arena A, K;                                         // per node word, per brick (declared before `sync`: they outlive the work)
    const size_t cap = trees, k_node = A.add(cap * 4), k_xy = A.add(cap * 4), k_z = A.add(cap * 4), k_parent = A.add(cap * 4), k_rank = A.add((cap + maxlevel + 2) * 4),
                 k_res = A.add(cap * 4), k_slot = A.add(cap * 4), k_outside = A.add(cap), k_elist = A.add(cap * 16), k_tmp = A.add(need_scan + 16), k_words = A.add(256);
    if (const int rc = A.alloc(who, w.device)) return rc;
    SyncAtExit sync{ s };
    uint32_t *const res = A.at<uint32_t>(k_res), *const slot = A.at<uint32_t>(k_slot), *const words = A.at<uint32_t>(k_words);
    uint8_t *const outside = A.at<uint8_t>(k_outside);
    uint4 *const elist = A.at<uint4>(k_elist);
    unsigned char *const tmp = A.at<unsigned char>(k_tmp);
    const Rebuild R{ who, s, tmp, need_scan };
    // words: [0] the walk's error, [1] the EMPTY nodes listed, [2, 3] the cells filled (64 bits), [8 .. 8 + SWEEP_BATCH) a batch's "changed"
    uint32_t *const err = words, *const ecount = words + 1, *const changed = words + 8;
    unsigned long long *const total = reinterpret_cast<unsigned long long *>(words + 2);
    HIP_TRY(hipMemsetAsync(words, 0, 256, s));
    HIP_TRY(hipMemsetAsync(outside, 0, cap, s));
    HIP_TRY(hipMemsetAsync(slot, 0xFF, cap * 4, s));
    auto level_at = [&](size_t first, uint32_t L, uint32_t n) {
        return LevelList{ A.at<uint32_t>(k_node) + first, A.at<uint32_t>(k_xy) + first, A.at<uint32_t>(k_z) + first, A.at<uint32_t>(k_parent) + first,
                          A.at<uint32_t>(k_rank) + first + L, n };
    };

    // 1. the walk
    std::vector<LevelList> lv;
    lv.push_back(level_at(0, 0, 1));
    HIP_TRY(hipMemsetAsync(lv[0].node, 0, 4, s));
    HIP_TRY(hipMemsetAsync(lv[0].xy, 0, 4, s));
    HIP_TRY(hipMemsetAsync(lv[0].z, 0, 4, s));
    HIP_TRY(hipMemsetAsync(lv[0].parent, 0, 4, s));
    size_t used = 1;
    for (uint32_t L = 0;; ++L) {
        const LevelList &V = lv[L];
        hipLaunchKernelGGL(k_walk, dim3(blocks_for((uint64_t)V.n + 1, 256)), dim3(256), 0, s, P, V, L == maxlevel ? 1u : 0u, err);
        if (const int rc = launch_status(who)) return rc;
        uint32_t branches = 0;
        if (const int rc = walk_level_tail(R, "the chunk's", V.rank, V.n, err, used, cap, &branches)) return rc;
        if (branches == 0) break;
        LevelList C = level_at(used, L + 1, 8 * branches);
        hipLaunchKernelGGL(k_children, dim3(blocks_for(V.n, 256)), dim3(256), 0, s, P, V, (1u << depth) >> (L + 1), C, C.n);
        if (const int rc = launch_status(who)) return rc;
        used += C.n;
        lv.push_back(C);
    }
    const uint32_t levels = (uint32_t)lv.size();        // (<= maxlevel + 1: k_walk follows no BRANCH of the last level)

    // 2. the state and its seeds
    for (uint32_t L = 0; L < levels; ++L) {
        hipLaunchKernelGGL(k_seed_nodes, dim3(blocks_for(lv[L].n, 256)), dim3(256), 0, s, P, lv[L], (1u << depth) >> L, outside, elist, ecount, (uint32_t)cap);
        if (const int rc = launch_status(who)) return rc;
    }
    uint32_t ne = 0, nbricks = 0;
    const LevelList &Last = lv[levels - 1];
    if (levels == maxlevel + 1) {
        hipLaunchKernelGGL(k_twig_flags, dim3(blocks_for((uint64_t)Last.n + 1, 256)), dim3(256), 0, s, P, Last);
        if (const int rc = launch_status(who)) return rc;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, need_scan, Last.rank, Last.rank, (int)Last.n + 1, s));
        HIP_TRY(hipMemcpyAsync(&nbricks, Last.rank + Last.n, 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipMemcpyAsync(&ne, ecount, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (ne > cap || nbricks > Last.n) { set_error(std::string(who) + ": the lists disagree with the walk"); return SVO_ERR_HIP; }
    const size_t k_where = K.add(((size_t)nbricks + 1) * 4), k_empty = K.add(((size_t)nbricks + 1) * 8), k_out = K.add(((size_t)nbricks + 1) * 8);
    if (const int rc = K.alloc(who, w.device)) return rc;
    uint32_t *const where = K.at<uint32_t>(k_where);
    const Bricks B{ where, K.at<unsigned long long>(k_empty), K.at<unsigned long long>(k_out), nbricks };
    if (nbricks) {
        hipLaunchKernelGGL(k_brick_slots, dim3(blocks_for(Last.n, 256)), dim3(256), 0, s, P, Last, slot, where, nbricks);
        if (const int rc = launch_status(who)) return rc;
        hipLaunchKernelGGL(k_seed_bricks, dim3(blocks_for(nbricks, 4)), dim3(256), 0, s, P, Last, B);
        if (const int rc = launch_status(who)) return rc;
    }

    // 3. the sweeps, to the fixed point
    uint64_t sweeps = 0;
    for (bool moving = ne + nbricks > 0; moving;) {
        HIP_TRY(hipMemsetAsync(changed, 0, SWEEP_BATCH * 4, s));
        for (uint32_t k = 0; k < SWEEP_BATCH; ++k, ++sweeps) {
            if (nbricks) hipLaunchKernelGGL(k_sweep_bricks, dim3(blocks_for(nbricks, 256)), dim3(256), 0, s, P, Last, B, slot, outside, changed + k);
            if (ne) hipLaunchKernelGGL(k_sweep_nodes, dim3(blocks_for(ne, 256)), dim3(256), 0, s, P, elist, ne, outside, changed + k);
            if (const int rc = launch_status(who)) return rc;
        }
        uint32_t last_changed = 0;
        HIP_TRY(hipMemcpyAsync(&last_changed, changed + SWEEP_BATCH - 1, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        moving = last_changed != 0;
    }

    // 4. the count
    if (ne + (uint64_t)nbricks > 0) {
        hipLaunchKernelGGL(k_count, dim3(blocks_for((uint64_t)ne + nbricks, 256)), dim3(256), 0, s, elist, ne, outside, B, total);
        if (const int rc = launch_status(who)) return rc;
    }
    unsigned long long filled = 0;
    HIP_TRY(hipMemcpyAsync(&filled, total, 8, hipMemcpyDeviceToHost, s));

    // 5. the fold, bottom-up, and the ranks of what stays
    Ranks ranks;
    if (const int rc = fold_and_rank(R, lv, maxlevel, [&](uint32_t L) {
            hipLaunchKernelGGL(k_fold, dim3(blocks_for((uint64_t)lv[L].n + 1, 256)), dim3(256), 0, s, P, lv[L], L == maxlevel ? 1u : 0u, outside, slot, B, material, res);
        }, ranks)) return rc;
    const uint64_t otrees = ranks.otrees, twigs = ranks.twigs;
    if (otrees > trees || twigs > nbricks) { set_error(std::string(who) + ": the fold disagrees with the walk"); return SVO_ERR_HIP; }

    // 6. the emit, top-down, into the edits' resident scratch
    uint32_t *otree = nullptr;
    uint16_t *otwig = nullptr;
    if (const int rc = emit_levels(R, w, levels, [&](uint32_t L) { return EmitLevel{ res, lv[L].node, lv[L].parent, lv[L].rank, lv[L].n }; }, ranks, &otree, &otwig)) return rc;
    if (twigs) {
        hipLaunchKernelGGL(k_write_bricks, dim3(blocks_for(nbricks, 4)), dim3(256), 0, s, P, Last, B, res, material, otwig, (uint32_t)twigs);
        if (const int rc = launch_status(who)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (std::getenv("SVO_BUILD_TIMING"))
        std::fprintf(stderr, "[svo sparse fill] depth %u: %u node words, %u EMPTY nodes, %u bricks, %llu sweeps, %llu cells filled, %llu working bytes\n", depth, trees, ne, nbricks,
                     (unsigned long long)sweeps, filled, (unsigned long long)(A.bytes + K.bytes));
    const int rc = install_rebuilt(w, chunk, depth, nullptr, otrees, twigs, otree, otwig);
    if (rc >= 0 && filled_out) *filled_out = filled;
    return rc;
}

} // namespace

} // namespace svo

using namespace svo;

extern "C" {

int svo_world_chunk_fill_enclosed(svo_world *w, int chunk, uint16_t material, uint64_t *filled_out)
{
    const char *who = "svo_world_chunk_fill_enclosed";
    if (!w || chunk < 0 || chunk >= (int)w->chunks.size() || material == 0) { set_error(std::string(who) + ": bad argument (a world, a chunk in range, a material other than 0)"); return SVO_ERR_INVALID_ARG; }
    if (w->device < 0) { set_error(std::string(who) + ": the world is not uploaded (svo_chunk_fill_enclosed fills host pools)"); return SVO_ERR_NOT_UPLOADED; }
    const uint32_t depth = w->chunks[(size_t)chunk].depth;
    if (depth < SVO_FILL_MIN_DEPTH || depth > SVO_FILL_MAX_DEPTH) { set_error(std::string(who) + ": the chunk's depth is outside [2, 16]"); return SVO_ERR_UNSUPPORTED; }
    return fenced(who, [&] { return fill_resident(*w, chunk, material, filled_out); });
}

} // extern "C"
