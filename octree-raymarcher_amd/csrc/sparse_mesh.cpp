// sparse_mesh.cpp — svo_chunk_from_mesh: the tree of the grid that svo_grid_add_mesh would leave of a list of meshes, built without
// that grid, on the host.  The readable statement of the sparse builder and the twin of sparse_mesh.hip; depth 2 .. 16.
//   cells      per mesh and triangle mesh.cpp's loops over the clamped cell box (mesh_rule.h has the float arithmetic); every overlap
//              is one packed word (sparse_mesh_rule.h) in a list instead of a write into the grid.  std::sort; the last word of every
//              run of equal keys is the cell with its largest material
//   bottom-up  runs of equal block keys: a 4^3 block of 64 cells of one material is a LEAF, any other a TWIG; then per level runs of
//              equal parents: eight LEAF children of one material are a LEAF, anything else a BRANCH.  What is absent is EMPTY
//   top-down   a level's nodes are in visiting order (ascending keys), so a BRANCH's first is 1 + 8 * (BRANCHes of the levels above +
//              its rank among its level's), a TWIG's brick its rank; a node whose parent is a BRANCH is written to first + slot
// A LEAF that was folded into its parent stays in its level's list and is skipped by the last step: its parent is no BRANCH.
// Working memory is proportional to the overlaps.  No HIP include: plain g++ compiles this file (host/sparse_mesh_check.cpp runs it
// under the sanitizers).
#include <algorithm>
#include <cmath>
#include <new>

#include "chunk_pools.h"
#include "sparse_mesh_rule.h"

namespace svo {

// the refusals of both chunk_from_mesh twins that are about the meshes and the depth; inv[m] receives 1 / cell of mesh m
bool sparse_mesh_args_ok(const svo_mesh *meshes, int nmeshes, uint32_t depth, std::vector<float> &inv)
{
    if (nmeshes < 0 || (nmeshes > 0 && !meshes) || depth < SVO_MESH_MIN_DEPTH || depth > SVO_MESH_MAX_DEPTH) return false;
    inv.assign((size_t)nmeshes, 0.0f);
    for (int m = 0; m < nmeshes; ++m)
        if (!mesh_frame_ok(meshes + m, &inv[(size_t)m])) return false;
    return true;
}

namespace {

struct Level {                                              // the nodes of one level that hold a cell, in visiting order
    std::vector<uint64_t> key;                              // the node's Morton prefix
    std::vector<uint32_t> word;                             // LEAF | material, or BRANCH / TWIG with its rank in the level
    std::vector<uint32_t> parent;                           // its parent's index in the level above
    uint32_t ranked = 0;                                    // BRANCHes (TWIGs at the last level) in it
};

int collect(const svo_mesh *meshes, int nmeshes, const std::vector<float> &inv, uint32_t depth, std::vector<uint64_t> &words)
{
    const int32_t N = 1 << depth;
    for (int k = 0; k < nmeshes; ++k) {
        const svo_mesh *mesh = meshes + k;
        for (uint32_t t = 0; t < mesh->ntriangles; ++t) {
            const uint32_t *ix = mesh->indices + 3 * (size_t)t;
            if (ix[0] >= mesh->nvertices || ix[1] >= mesh->nvertices || ix[2] >= mesh->nvertices) continue;
            MeshTri T;
            if (!mesh_setup(mesh->vertices + 3 * (size_t)ix[0], mesh->vertices + 3 * (size_t)ix[1], mesh->vertices + 3 * (size_t)ix[2], mesh->origin,
                            inv[(size_t)k], mesh->materials ? mesh->materials[t] : mesh->material, N, T)) continue;
            for (int32_t z = T.c0[2]; z <= T.c1[2]; ++z)
                for (int32_t y = T.c0[1]; y <= T.c1[1]; ++y)
                    for (int32_t x = T.c0[0]; x <= T.c1[0]; ++x) {
                        const float p[3] = { (float)x, (float)y, (float)z };
                        if (!mesh_overlaps(T, p)) continue;
                        if (words.size() + 1 >= SPARSE_MAX_WORDS) { set_error("svo_chunk_from_mesh: 2^31 - 1 overlaps or more"); return SVO_ERR_UNSUPPORTED; }
                        words.push_back(sparse_word((uint32_t)x, (uint32_t)y, (uint32_t)z, T.material));
                    }
        }
    }
    return SVO_OK;
}

int chunk_from_words(std::vector<uint64_t> &words, uint32_t depth, std::vector<uint32_t> &tree, std::vector<uint16_t> &twig)
{
    tree.assign(1, node_make(EMPTY, 0));
    twig.clear();
    if (words.empty()) return SVO_OK;
    std::sort(words.begin(), words.end());
    size_t cells = 0;                                       // the last word of every run of equal keys
    for (size_t i = 0; i < words.size(); ++i)
        if (i + 1 == words.size() || sparse_word_key(words[i + 1]) != sparse_word_key(words[i])) words[cells++] = words[i];
    words.resize(cells);

    const uint32_t maxlevel = depth - TWIG_LEVELS;
    std::vector<Level> lv(maxlevel + 1);
    std::vector<size_t> block_start;                        // the first cell of every block of the last level
    {   // the last level: runs of equal block keys
        Level &B = lv[maxlevel];
        for (size_t i = 0; i < cells;) {
            size_t j = i + 1;
            bool one = true;
            while (j < cells && sparse_word_block(words[j]) == sparse_word_block(words[i])) { one = one && sparse_word_material(words[j]) == sparse_word_material(words[i]); ++j; }
            B.key.push_back(sparse_word_block(words[i]));
            B.word.push_back(one && j - i == TWIG_WORDS ? node_make(LEAF, sparse_word_material(words[i])) : node_make(TWIG, B.ranked++));
            block_start.push_back(i);
            i = j;
        }
        block_start.push_back(cells);
    }
    for (uint32_t L = maxlevel; L-- > 0;) {                 // level L from level L + 1: runs of equal parents
        Level &C = lv[L + 1], &P = lv[L];
        C.parent.resize(C.key.size());
        for (size_t i = 0; i < C.key.size();) {
            size_t j = i + 1;
            bool one = node_type(C.word[i]) == LEAF;
            while (j < C.key.size() && (C.key[j] >> 3) == (C.key[i] >> 3)) { one = one && C.word[j] == C.word[i]; ++j; }
            for (size_t k = i; k < j; ++k) C.parent[k] = (uint32_t)P.key.size();
            P.key.push_back(C.key[i] >> 3);
            P.word.push_back(one && j - i == 8 ? C.word[i] : node_make(BRANCH, P.ranked++));
            i = j;
        }
    }
    uint64_t branches = 0;
    std::vector<uint64_t> above(maxlevel + 1, 0);           // BRANCHes of the levels above
    for (uint32_t L = 0; L < maxlevel; ++L) { above[L] = branches; branches += lv[L].ranked; }
    const uint64_t trees = 1 + 8 * branches, twigs = lv[maxlevel].ranked;
    if (trees >= (1ull << 30) || twigs >= (1ull << 30)) { set_error("svo_chunk_from_mesh: chunk exceeds the 30-bit node offset"); return SVO_ERR_UNSUPPORTED; }
    tree.assign(trees, node_make(EMPTY, 0));
    twig.assign(twigs * TWIG_WORDS, 0);
    auto final_word = [&](uint32_t L, size_t i) {           // the node word as the pool holds it
        const uint32_t w = lv[L].word[i];
        return node_type(w) == BRANCH ? node_make(BRANCH, (uint32_t)(1 + 8 * (above[L] + node_offset(w)))) : w;
    };
    tree[0] = final_word(0, 0);
    for (uint32_t L = 1; L <= maxlevel; ++L)
        for (size_t i = 0; i < lv[L].key.size(); ++i) {
            const uint32_t p = lv[L - 1].word[lv[L].parent[i]];
            if (node_type(p) != BRANCH) continue;
            tree[1 + 8 * (above[L - 1] + node_offset(p)) + (lv[L].key[i] & 7u)] = final_word(L, i);
        }
    const Level &B = lv[maxlevel];
    for (size_t b = 0; b < B.key.size(); ++b) {
        if (node_type(B.word[b]) != TWIG) continue;
        uint16_t *brick = twig.data() + (size_t)node_offset(B.word[b]) * TWIG_WORDS;
        for (size_t i = block_start[b]; i < block_start[b + 1]; ++i) brick[sparse_brick_index(words[i])] = (uint16_t)sparse_word_material(words[i]);
    }
    return SVO_OK;
}

} // namespace

} // namespace svo

extern "C" {

int svo_chunk_from_mesh(const svo_mesh *meshes, int nmeshes, uint32_t depth, const float position[3], float size, svo_chunk_desc *out)
{
    using namespace svo;
    try {
        std::vector<float> inv;
        if (!position || !out || !(size > 0.0f) || !std::isfinite(size) || !sparse_mesh_args_ok(meshes, nmeshes, depth, inv)) {
            set_error("svo_chunk_from_mesh: bad argument (meshes with their arrays, each cell positive and finite with a finite 1 / cell and a finite origin, depth in [2, 16], size positive and finite)");
            return SVO_ERR_INVALID_ARG;
        }
        std::vector<uint64_t> words;
        std::vector<uint32_t> tree;
        std::vector<uint16_t> twig;
        if (const int rc = collect(meshes, nmeshes, inv, depth, words)) return rc;
        if (const int rc = chunk_from_words(words, depth, tree, twig)) return rc;
        return chunk_desc_take(out, position, size, depth, tree, twig, "svo_chunk_from_mesh");
    } catch (const std::bad_alloc &) {
        set_error("svo_chunk_from_mesh: out of host memory");
        return SVO_ERR_OUT_OF_MEMORY;
    }
}

} // extern "C"
