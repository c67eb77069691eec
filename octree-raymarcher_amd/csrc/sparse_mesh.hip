// sparse_mesh.hip — svo_world_chunk_from_mesh: a chunk of an uploaded world built from triangle meshes in device memory without the
// dense grid, depth 2 .. 16.  sparse_mesh.cpp is the host twin and states the builder as plain loops; mesh_rule.h holds the float
// arithmetic of the overlap test, sparse_mesh_rule.h the packed word (Morton key << 16 | material), mesh_tiles.hip.h what this file
// shares with mesh.hip (the setup kernel, the decode of a tile job, the arena).  On the world's device, on the null stream, behind
// a hipDeviceSynchronize like svo_world_chunk_from_grid; complete at the return.
//   k_mesh_setup      per mesh, into one record array and one count array for the whole list; one hipcub scan of the tile counts
//   k_sparse_tiles    one wave per 4^3-cell tile job, twice: COUNT adds the wave's overlaps to a counter (one ballot, one atomic per
//                     wave), EMIT reserves that many slots of the list the same way and writes the packed words; their order does
//                     not matter
//   hipcub sort       DeviceRadixSort::SortKeys on bits 0 .. 16 + 3 * depth: a cell's largest material is the last of its duplicates
//   k_last_of_key     flags the last word of every run of equal cell keys; hipcub DeviceSelect::Flagged keeps them: the cells
//   bottom-up         per level k_heads flags the first entry of every run of equal parents (at the bottom: the first cell of every
//                     4^3 block), DeviceSelect::Flagged over a counting iterator turns the flags into the runs' starts, and one
//                     thread per run folds it: k_fold_blocks (64 cells of one material: LEAF, else TWIG), k_fold_nodes (eight LEAF
//                     children of one material: LEAF, else BRANCH; the children learn their parent's index).  A hipcub exclusive scan
//                     of the BRANCH / TWIG flags ranks them; the host reads each level's size and rank total
//   top-down          k_write_nodes per level: a node whose parent is a BRANCH goes to first + slot, first = 1 + 8 * (BRANCHes of the
//                     levels above + the parent's rank); k_write_bricks: one wave per TWIG block, a cell per lane to
//                     k * 64 + cz * 16 + cy * 4 + cx.  Both pools are cleared first
// A level's entries are in ascending key order, which is the FIFO walk's visiting order, so the ranks are the walk's numbers and the
// pools equal the host twin's index for index.  Every index written is checked against the pool it goes to.  The install is
// svo_world_chunk_from_grid's (install_rebuilt).  Plain C++ and vector stores; no float arithmetic outside mesh_rule.h.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdio>
#include <cstdlib>

#include "hip_own.h"
#include "mesh_tiles.hip.h"
#include "sparse_mesh_rule.h"

namespace svo {

bool sparse_mesh_args_ok(const svo_mesh *meshes, int nmeshes, uint32_t depth, std::vector<float> &inv);     // sparse_mesh.cpp

namespace {

// Tile job first + 4 * block + wave of `total`.  list == null: *counter += the wave's overlaps; else the wave takes that many slots of
// list[capacity] at *counter and writes its cells' words
__global__ __launch_bounds__(256) void k_sparse_tiles(const MeshTri *__restrict__ tri, const unsigned long long *__restrict__ start, uint32_t ntriangles,
                                                      unsigned long long first, unsigned long long total, unsigned long long *counter,
                                                      unsigned long long *list, unsigned long long capacity)
{
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const unsigned long long job = first + (unsigned long long)blockIdx.x * 4ull + wave;
    if (job >= total) return;
    uint32_t x, y, z;
    const MeshTri &T = tile_job_cell(tri, start, ntriangles, job, lane, x, y, z);
    const float p[3] = { (float)x, (float)y, (float)z };
    const bool hit = mesh_overlaps(T, p);
    const unsigned long long m = __ballot(hit);
    if (m == 0ull) return;
    unsigned long long base = 0ull;
    if (lane == 0u) base = atomicAdd(counter, (unsigned long long)__popcll(m));
    if (!list) return;
    base = __shfl(base, 0, 64);
    const unsigned long long at = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
    if (hit && at < capacity) list[at] = sparse_word(x, y, z, T.material);
}

__global__ __launch_bounds__(256) void k_last_of_key(const unsigned long long *__restrict__ words, uint32_t n, uint8_t *flag)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    flag[i] = (i + 1u == n || sparse_word_key(words[i + 1u]) != sparse_word_key(words[i])) ? 1 : 0;
}

// flag[i] = entry i begins a run of equal key[i] >> shift
__global__ __launch_bounds__(256) void k_heads(const unsigned long long *__restrict__ key, uint32_t n, uint32_t shift, uint8_t *flag)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    flag[i] = (i == 0u || (key[i - 1u] >> shift) != (key[i] >> shift)) ? 1 : 0;
}

// One level's nodes that hold a cell, in visiting order: [n] of each, ranked has n + 1 entries (the scan's last item is the total)
struct LevelArrays {
    unsigned long long *key;        // the node's Morton prefix
    uint32_t *word;                 // LEAF | material, or BRANCH | 0 / TWIG | 0
    uint32_t *parent;               // its parent's index in the level above
    uint32_t *ranked;               // before the scan: 1 for a BRANCH / TWIG; after it: its rank among the level's
};

// block b = cells [start[b], start[b + 1]) (the last one ends at ncells)
__global__ __launch_bounds__(256) void k_fold_blocks(const unsigned long long *__restrict__ cells, uint32_t ncells, const uint32_t *__restrict__ start, uint32_t n, LevelArrays B)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b > n) return;
    if (b == n) { B.ranked[b] = 0u; return; }
    const uint32_t i0 = start[b], i1 = min(b + 1u < n ? start[b + 1u] : ncells, ncells);
    const unsigned long long w0 = cells[i0];
    bool one = true;
    for (uint32_t i = i0 + 1u; i < i1; ++i) one = one && sparse_word_material(cells[i]) == sparse_word_material(w0);
    const bool leaf = one && i1 - i0 == TWIG_WORDS;
    B.key[b] = sparse_word_block(w0);
    B.word[b] = leaf ? node_make(LEAF, sparse_word_material(w0)) : node_make(TWIG, 0);
    B.ranked[b] = leaf ? 0u : 1u;
}

// node p of the level above = children [start[p], start[p + 1]) of level C (the last one ends at nchildren)
__global__ __launch_bounds__(256) void k_fold_nodes(LevelArrays C, uint32_t nchildren, const uint32_t *__restrict__ start, uint32_t n, LevelArrays P)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p > n) return;
    if (p == n) { P.ranked[p] = 0u; return; }
    const uint32_t i0 = start[p], i1 = min(p + 1u < n ? start[p + 1u] : nchildren, nchildren);
    const uint32_t w0 = C.word[i0];
    bool one = node_type(w0) == LEAF;
    for (uint32_t i = i0; i < i1; ++i) { one = one && C.word[i] == w0; C.parent[i] = p; }
    const bool leaf = one && i1 - i0 == 8u;
    P.key[p] = C.key[i0] >> 3;
    P.word[p] = leaf ? w0 : node_make(BRANCH, 0);
    P.ranked[p] = leaf ? 0u : 1u;
}

// the node word as the pool holds it; above = the BRANCHes of the levels above the node's
__device__ __forceinline__ uint32_t final_word(const LevelArrays &V, uint32_t i, uint32_t above)
{
    const uint32_t w = V.word[i], type = node_type(w);
    return type == BRANCH ? node_make(BRANCH, 1u + 8u * (above + V.ranked[i])) : type == TWIG ? node_make(TWIG, V.ranked[i]) : w;
}

// level C (n nodes) into the blocks of its parents' level P; above_p / above_c = the BRANCHes above P / above C.  P.key == null: C is
// level 0 and its one node the root
__global__ __launch_bounds__(256) void k_write_nodes(LevelArrays C, uint32_t n, LevelArrays P, uint32_t above_p, uint32_t above_c, uint32_t *tree, uint32_t trees)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t at = 0u;
    if (P.key) {
        const uint32_t p = C.parent[i];
        if (node_type(P.word[p]) != BRANCH) return;
        at = 1u + 8u * (above_p + P.ranked[p]) + ((uint32_t)C.key[i] & 7u);
    } else if (i != 0u) return;
    if (at < trees) tree[at] = final_word(C, i, above_c);
}

// one wave per block of the last level: the cells of a TWIG into its brick
__global__ __launch_bounds__(256) void k_write_bricks(const unsigned long long *__restrict__ cells, uint32_t ncells, const uint32_t *__restrict__ start, LevelArrays B, uint32_t n,
                                                      uint16_t *twig, uint32_t twigs)
{
    const uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (b >= n || node_type(B.word[b]) != TWIG) return;
    const uint32_t k = B.ranked[b];
    const uint32_t i = start[b] + lane, i1 = min(b + 1u < n ? start[b + 1u] : ncells, ncells);
    if (i >= i1 || k >= twigs) return;
    const unsigned long long w = cells[i];
    twig[(size_t)k * TWIG_WORDS + sparse_brick_index(w)] = (uint16_t)sparse_word_material(w);
}

using Counting = hipcub::CountingInputIterator<uint32_t>;

int install_empty(svo_world &w, int chunk, uint32_t depth)
{
    uint32_t *tree = nullptr;
    uint16_t *twig = nullptr;
    if (const int rc = edit_scratch(w, 1, 0, &tree, &twig)) return rc;
    HIP_TRY(hipMemsetAsync(tree, 0, sizeof(uint32_t), nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return install_rebuilt(w, chunk, depth, nullptr, 1, 0, tree, twig);
}

int chunk_from_mesh_resident(svo_world &w, int chunk, const svo_mesh *meshes, int nmeshes, const std::vector<float> &inv, uint32_t depth)
{
    const char *who = "svo_world_chunk_from_mesh";
    HIP_TRY(hipSetDevice(w.device));
    HIP_TRY(hipDeviceSynchronize());                    // ordered behind every launch issued before it, like svo_world_chunk_from_grid
    hipStream_t s = nullptr;
    const int device = w.device;
    uint64_t ntri = 0;
    for (int m = 0; m < nmeshes; ++m) ntri += meshes[m].ntriangles;
    if (ntri == 0) return install_empty(w, chunk, depth);
    const uint32_t n = (uint32_t)ntri;                  // (< 2^31 - 1: the caller has refused the rest)

    // 1. the triangles' records and tile jobs
    size_t need = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)(n + 1), s));
    Arena A, W, V;                                      // the triangles' arrays, the list's, the levels' (declared before `sync`: they outlive the work)
    const size_t k_tri = A.add((size_t)n * sizeof(MeshTri)), k_count = A.add(((size_t)n + 1) * 8), k_start = A.add(((size_t)n + 1) * 8), k_tmp = A.add(need + 16),
                 k_counter = A.add(16);
    if (const int rc = A.alloc(who, device)) return rc;
    SyncAtExit sync{ s };                               // (the arenas go back to the cache behind the work, on every way out)
    MeshTri *tri = A.at<MeshTri>(k_tri);
    unsigned long long *count = A.at<unsigned long long>(k_count), *start = A.at<unsigned long long>(k_start), *counter = A.at<unsigned long long>(k_counter);
    uint32_t base = 0;
    for (int m = 0; m < nmeshes; ++m) {                 // mesh m's count[ntriangles] = 0 is overwritten by mesh m + 1's first count, the last one's stays
        if (meshes[m].ntriangles == 0) continue;
        hipLaunchKernelGGL(k_mesh_setup, dim3(blocks_for((uint64_t)meshes[m].ntriangles + 1, 256)), dim3(256), 0, s, mesh_kernel_args(meshes[m], inv[(size_t)m], depth),
                           tri + base, count + base);
        if (const int rc = launch_status(who)) return rc;
        base += meshes[m].ntriangles;
    }
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(A.at<unsigned char>(k_tmp), need, count, start, (int)(n + 1), s));
    HIP_TRY(hipMemsetAsync(counter, 0, 16, s));
    unsigned long long jobs = 0, overlaps = 0;
    HIP_TRY(hipMemcpyAsync(&jobs, start + n, sizeof jobs, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));

    // 2. count, then emit
    auto tiles = [&](unsigned long long *ctr, unsigned long long *list, unsigned long long capacity) -> int {
        for (unsigned long long first = 0; first < jobs; first += TILE_JOBS_PER_LAUNCH) {
            const unsigned long long some = std::min(jobs - first, TILE_JOBS_PER_LAUNCH);
            hipLaunchKernelGGL(k_sparse_tiles, dim3(blocks_for(some, 4)), dim3(256), 0, s, tri, start, n, first, jobs, ctr, list, capacity);
            if (const int rc = launch_status(who)) return rc;
        }
        return SVO_OK;
    };
    if (const int rc = tiles(counter, nullptr, 0)) return rc;
    HIP_TRY(hipMemcpyAsync(&overlaps, counter, sizeof overlaps, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (overlaps == 0) return install_empty(w, chunk, depth);
    if (overlaps >= SPARSE_MAX_WORDS) { set_error(std::string(who) + ": 2^31 - 1 overlaps or more"); return SVO_ERR_UNSUPPORTED; }
    const uint32_t nw = (uint32_t)overlaps;

    // 3. 4. the list, sorted, the last word of every cell kept
    size_t need_sort = 0, need_select = 0, need_starts = 0, need_rank = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, need_sort, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)nw, 0, (int)(SPARSE_MATERIAL_BITS + 3 * depth), s));
    HIP_TRY(hipcub::DeviceSelect::Flagged(nullptr, need_select, (unsigned long long *)nullptr, (uint8_t *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr, (int)nw, s));
    HIP_TRY(hipcub::DeviceSelect::Flagged(nullptr, need_starts, Counting(0u), (uint8_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)nw, s));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need_rank, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)nw + 1, s));
    const size_t k_a = W.add((size_t)nw * 8), k_b = W.add((size_t)nw * 8), k_flag = W.add(nw), k_runs = W.add((size_t)nw * 4), k_num = W.add(16),
                 k_wtmp = W.add(std::max(std::max(need_sort, need_select), std::max(need_starts, need_rank)) + 16);
    if (const int rc = W.alloc(who, device)) return rc;
    unsigned long long *list = W.at<unsigned long long>(k_a), *sorted = W.at<unsigned long long>(k_b), *cells = list;    // (the cells take the list's place)
    uint8_t *flag = W.at<uint8_t>(k_flag);
    uint32_t *runs = W.at<uint32_t>(k_runs), *num = W.at<uint32_t>(k_num);
    unsigned char *tmp = W.at<unsigned char>(k_wtmp);
    HIP_TRY(hipMemsetAsync(counter, 0, 16, s));
    if (const int rc = tiles(counter, list, nw)) return rc;
    unsigned long long emitted = 0;
    HIP_TRY(hipMemcpyAsync(&emitted, counter, sizeof emitted, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (emitted != overlaps) { set_error(std::string(who) + ": the emit pass disagrees with the count pass"); return SVO_ERR_HIP; }
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(tmp, need_sort, list, sorted, (int)nw, 0, (int)(SPARSE_MATERIAL_BITS + 3 * depth), s));
    hipLaunchKernelGGL(k_last_of_key, dim3(blocks_for(nw, 256)), dim3(256), 0, s, sorted, nw, flag);
    if (const int rc = launch_status(who)) return rc;
    HIP_TRY(hipcub::DeviceSelect::Flagged(tmp, need_select, sorted, flag, cells, num, (int)nw, s));
    uint32_t ncells = 0;
    HIP_TRY(hipMemcpyAsync(&ncells, num, sizeof ncells, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (ncells == 0 || ncells > nw) { set_error(std::string(who) + ": the selection disagrees with the list"); return SVO_ERR_HIP; }

    // 5. bottom-up.  The blocks first: their starts stay (k_write_bricks), so the upper levels' runs go behind them in `runs`
    const uint32_t maxlevel = depth - TWIG_LEVELS;
    hipLaunchKernelGGL(k_heads, dim3(blocks_for(ncells, 256)), dim3(256), 0, s, cells, ncells, SPARSE_MATERIAL_BITS + 6u, flag);
    if (const int rc = launch_status(who)) return rc;
    HIP_TRY(hipcub::DeviceSelect::Flagged(tmp, need_starts, Counting(0u), flag, runs, num, (int)ncells, s));
    uint32_t nblocks = 0;
    HIP_TRY(hipMemcpyAsync(&nblocks, num, sizeof nblocks, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (nblocks == 0 || nblocks > ncells || (3 * maxlevel < 32 && nblocks > (1ull << (3 * maxlevel)))) { set_error(std::string(who) + ": the selection disagrees with the cells"); return SVO_ERR_HIP; }
    // the levels' arrays: level L holds at most min(blocks, 8^L) nodes
    std::vector<uint32_t> cap(maxlevel + 1);
    for (uint32_t L = 0; L <= maxlevel; ++L) cap[L] = 3 * L >= 32 ? nblocks : (uint32_t)std::min<uint64_t>(nblocks, 1ull << (3 * L));
    std::vector<size_t> k_key(maxlevel + 1), k_word(maxlevel + 1), k_parent(maxlevel + 1), k_ranked(maxlevel + 1);
    for (uint32_t L = 0; L <= maxlevel; ++L) {
        k_key[L] = V.add((size_t)cap[L] * 8); k_word[L] = V.add((size_t)cap[L] * 4); k_parent[L] = V.add((size_t)cap[L] * 4); k_ranked[L] = V.add(((size_t)cap[L] + 1) * 4);
    }
    const size_t k_uruns = V.add((size_t)nblocks * 4);
    if (const int rc = V.alloc(who, device)) return rc;
    std::vector<LevelArrays> lv(maxlevel + 1);
    for (uint32_t L = 0; L <= maxlevel; ++L) lv[L] = LevelArrays{ V.at<unsigned long long>(k_key[L]), V.at<uint32_t>(k_word[L]), V.at<uint32_t>(k_parent[L]), V.at<uint32_t>(k_ranked[L]) };
    uint32_t *uruns = V.at<uint32_t>(k_uruns);
    std::vector<uint32_t> count_of(maxlevel + 1, 0), ranked_of(maxlevel + 1, 0);
    auto rank_level = [&](uint32_t L) -> int {          // the scan of the level's flags and its total
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, need_rank, lv[L].ranked, lv[L].ranked, (int)count_of[L] + 1, s));
        HIP_TRY(hipMemcpyAsync(&ranked_of[L], lv[L].ranked + count_of[L], sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        return SVO_OK;
    };
    count_of[maxlevel] = nblocks;
    hipLaunchKernelGGL(k_fold_blocks, dim3(blocks_for((uint64_t)nblocks + 1, 256)), dim3(256), 0, s, cells, ncells, runs, nblocks, lv[maxlevel]);
    if (const int rc = launch_status(who)) return rc;
    if (const int rc = rank_level(maxlevel)) return rc;
    for (uint32_t L = maxlevel; L-- > 0;) {
        const uint32_t nc = count_of[L + 1];
        hipLaunchKernelGGL(k_heads, dim3(blocks_for(nc, 256)), dim3(256), 0, s, lv[L + 1].key, nc, 3u, flag);
        if (const int rc = launch_status(who)) return rc;
        HIP_TRY(hipcub::DeviceSelect::Flagged(tmp, need_starts, Counting(0u), flag, uruns, num, (int)nc, s));
        uint32_t np = 0;
        HIP_TRY(hipMemcpyAsync(&np, num, sizeof np, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (np == 0 || np > cap[L]) { set_error(std::string(who) + ": a level holds more nodes than its bound"); return SVO_ERR_HIP; }
        count_of[L] = np;
        hipLaunchKernelGGL(k_fold_nodes, dim3(blocks_for((uint64_t)np + 1, 256)), dim3(256), 0, s, lv[L + 1], nc, uruns, np, lv[L]);
        if (const int rc = launch_status(who)) return rc;
        if (const int rc = rank_level(L)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(s));

    // 6. 7. 8. top-down: the pools' sizes, then the words and the bricks
    uint64_t branches = 0;
    std::vector<uint32_t> above(maxlevel + 1, 0);
    for (uint32_t L = 0; L < maxlevel; ++L) { above[L] = (uint32_t)branches; branches += ranked_of[L]; }
    above[maxlevel] = (uint32_t)branches;
    const uint64_t trees = 1 + 8 * branches, twigs = ranked_of[maxlevel];
    if (trees >= (1ull << 30) || twigs >= (1ull << 30)) { set_error(std::string(who) + ": chunk exceeds the 30-bit node offset"); return SVO_ERR_UNSUPPORTED; }
    uint32_t *tree = nullptr;
    uint16_t *twig = nullptr;
    if (const int rc = edit_scratch(w, trees, twigs, &tree, &twig)) return rc;
    HIP_TRY(hipMemsetAsync(tree, 0, trees * sizeof(uint32_t), s));
    if (twigs) HIP_TRY(hipMemsetAsync(twig, 0, twigs * TWIG_WORDS * sizeof(uint16_t), s));
    for (uint32_t L = 0; L <= maxlevel; ++L) {
        const LevelArrays P = L ? lv[L - 1] : LevelArrays{ nullptr, nullptr, nullptr, nullptr };
        hipLaunchKernelGGL(k_write_nodes, dim3(blocks_for(count_of[L], 256)), dim3(256), 0, s, lv[L], count_of[L], P, L ? above[L - 1] : 0u, above[L], tree, (uint32_t)trees);
        if (const int rc = launch_status(who)) return rc;
    }
    if (twigs) hipLaunchKernelGGL(k_write_bricks, dim3(blocks_for(nblocks, 4)), dim3(256), 0, s, cells, ncells, runs, lv[maxlevel], nblocks, twig, (uint32_t)twigs);
    if (const int rc = launch_status(who)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    if (std::getenv("SVO_BUILD_TIMING"))
        std::fprintf(stderr, "[svo sparse mesh] depth %u: %llu tile jobs, %llu overlaps, %u cells, %u blocks, %llu working bytes\n", depth, jobs, overlaps, ncells, nblocks,
                     (unsigned long long)(A.bytes + W.bytes + V.bytes));
    return install_rebuilt(w, chunk, depth, nullptr, trees, twigs, tree, twig);
}

} // namespace

} // namespace svo

using namespace svo;

extern "C" {

int svo_world_chunk_from_mesh(svo_world *w, int chunk, const svo_mesh *meshes, int nmeshes, uint32_t depth)
{
    const char *who = "svo_world_chunk_from_mesh";
    return fenced(who, [&]() -> int {                   // (the argument checks too: they fill a vector, one 1 / cell per mesh)
        std::vector<float> inv;
        if (!w || chunk < 0 || chunk >= (int)w->chunks.size() || !sparse_mesh_args_ok(meshes, nmeshes, depth, inv)) {
            set_error(std::string(who) + ": bad argument (chunk in range, meshes with their arrays, each cell positive and finite with a finite 1 / cell and a finite origin, depth in [2, 16])");
            return SVO_ERR_INVALID_ARG;
        }
        if (w->device < 0) { set_error(std::string(who) + ": the world is not uploaded (svo_chunk_from_mesh builds host pools)"); return SVO_ERR_NOT_UPLOADED; }
        uint64_t ntri = 0;
        for (int m = 0; m < nmeshes; ++m) ntri += meshes[m].ntriangles;
        if (ntri >= 0x7FFFFFFFull) { set_error(std::string(who) + ": too many triangles for one scan"); return SVO_ERR_UNSUPPORTED; }
        return chunk_from_mesh_resident(*w, chunk, meshes, nmeshes, inv, depth);
    });
}

} // extern "C"
