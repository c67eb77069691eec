// sparse_fill_check.cpp — csrc/sparse_fill.cpp (svo_chunk_fill_enclosed) on its own, for the host sanitizers: compiled together with
// it, csrc/sparse_mesh.cpp, csrc/mesh.cpp and csrc/grid.cpp by tests/test_sparse_fill_host_sanitize.py (g++
// -fsanitize=address,undefined), no HIP and no libsvo_amd.so.  For built-in boxes and triangle soups at depths 2 to 6 the sparse fill of
// the sparse voxeliser's chunk is compared, index for index and count for count, with the dense composition svo_chunk_from_grid of
// svo_grid_fill_enclosed of svo_grid_add_mesh; one depth-16 cube is filled; the refusals are tried; everything is freed.  Exit status
// 1 when something differs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/svo.h"

namespace svo { void set_error(const std::string &) {} }        // (world.cpp's, which this program does not link)

struct Mesh {
    std::vector<float> v;
    std::vector<uint32_t> ix;
    void box(float lo, float hi)
    {
        const uint32_t base = (uint32_t)(v.size() / 3);
        for (int c = 0; c < 8; ++c)
            for (int k = 0; k < 3; ++k) v.push_back((c >> k) & 1 ? hi : lo);
        static const uint32_t quads[6][4] = { { 0, 1, 3, 2 }, { 4, 6, 7, 5 }, { 0, 4, 5, 1 }, { 2, 3, 7, 6 }, { 0, 2, 6, 4 }, { 1, 5, 7, 3 } };
        for (const auto &q : quads) for (uint32_t t : { q[0], q[1], q[2], q[0], q[2], q[3] }) ix.push_back(base + t);
    }
    void soup(uint32_t seed, int count, float n)
    {
        uint32_t s = seed;
        auto next = [&] { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; };
        for (int t = 0; t < count; ++t) {
            const float c[3] = { next() * n, next() * n, next() * n }, ext = 0.05f + next() * n / 3.0f;
            const uint32_t base = (uint32_t)(v.size() / 3);
            for (int k = 0; k < 9; ++k) v.push_back(c[k % 3] + (next() - 0.5f) * ext);
            for (uint32_t k = 0; k < 3; ++k) ix.push_back(base + k);
        }
    }
    svo_mesh desc(uint16_t material, float cell = 1.0f) const
    {
        svo_mesh m = {};
        m.vertices = v.data(); m.indices = ix.data();
        m.nvertices = (uint32_t)(v.size() / 3); m.ntriangles = (uint32_t)(ix.size() / 3);
        m.cell = cell; m.material = material;
        return m;
    }
};

static void free_chunk(svo_chunk_desc &c)
{
    std::free(const_cast<uint32_t *>(c.tree));                      // what svo_chunk_free does (world.cpp)
    std::free(const_cast<uint16_t *>(c.twig));
    c.tree = nullptr; c.twig = nullptr;
}

static int report(const char *name, bool ok) { std::printf("%s: %s\n", name, ok ? "ok" : "WRONG"); return ok ? 0 : 1; }

// mesh -> sparse chunk -> sparse fill equals mesh -> grid -> dense fill -> chunk; want_filled: the case must enclose something
static bool same_as_dense(const std::vector<svo_mesh> &meshes, uint32_t depth, uint16_t material, bool want_filled)
{
    const float pos[3] = { 1.0f, 2.0f, 3.0f };
    std::vector<uint16_t> grid((size_t)1 << (3 * depth), 0);
    for (const svo_mesh &m : meshes)
        if (svo_grid_add_mesh(&m, depth, grid.data()) != SVO_OK) return false;
    uint64_t dense_filled = 0, sparse_filled = 0;
    if (svo_grid_fill_enclosed(grid.data(), depth, material, &dense_filled) != SVO_OK) return false;
    svo_chunk_desc dense = {}, shell = {}, sparse = {};
    if (svo_chunk_from_grid(grid.data(), depth, pos, 64.0f, &dense) != SVO_OK) return false;
    if (svo_chunk_from_mesh(meshes.data(), (int)meshes.size(), depth, pos, 64.0f, &shell) != SVO_OK) { free_chunk(dense); return false; }
    if (svo_chunk_fill_enclosed(&shell, material, &sparse, &sparse_filled) != SVO_OK) { free_chunk(dense); free_chunk(shell); return false; }
    bool ok = dense.trees == sparse.trees && dense.twigs == sparse.twigs && sparse.depth == depth && sparse.size == 64.0f && sparse.position[2] == 3.0f;
    ok = ok && std::memcmp(dense.tree, sparse.tree, dense.trees * sizeof(uint32_t)) == 0;
    ok = ok && (dense.twigs == 0 || std::memcmp(dense.twig, sparse.twig, dense.twigs * 64 * sizeof(uint16_t)) == 0);
    ok = ok && dense_filled == sparse_filled && (!want_filled || dense_filled > 0);
    free_chunk(dense); free_chunk(shell); free_chunk(sparse);
    return ok;
}

int main()
{
    int bad = 0;
    for (uint32_t depth = 2; depth <= 6; ++depth) {
        const float n = (float)(1u << depth);
        char name[64];
        Mesh a; a.box(0.2f * n, 0.8f * n);                              // off the lattice; at depth >= 3 it encloses cells
        std::snprintf(name, sizeof name, "depth %u, box", depth);
        bad += report(name, same_as_dense({ a.desc(5) }, depth, 9, depth >= 3));
        Mesh s; s.soup(depth, 40, n);
        Mesh b; b.box(1.0f, n - 1.0f);                                  // on the lattice, the soup inside it: pockets between the triangles
        std::snprintf(name, sizeof name, "depth %u, soup in a lattice box", depth);
        bad += report(name, same_as_dense({ s.desc(1), b.desc(0xFFFF) }, depth, 0xFFFF, false));
        std::snprintf(name, sizeof name, "depth %u, soup alone", depth);
        bad += report(name, same_as_dense({ s.desc(3) }, depth, 4, false));
    }
    {   // depth 16: a cube of 256 cells far from the origin; 254^3 cells are enclosed, and a second fill finds none
        Mesh m; m.box(47104.0f * 0.25f, (47104.0f + 256.0f) * 0.25f);
        const svo_mesh d = m.desc(6, 0.25f);
        const float pos[3] = { 0, 0, 0 };
        svo_chunk_desc shell = {}, solid = {}, again = {};
        uint64_t filled = 0, none = 1;
        bool ok = svo_chunk_from_mesh(&d, 1, 16, pos, 128.0f, &shell) == SVO_OK && svo_chunk_fill_enclosed(&shell, 2, &solid, &filled) == SVO_OK &&
                  filled == 254ull * 254 * 254 && solid.trees <= shell.trees && solid.twigs <= shell.twigs;
        ok = ok && svo_chunk_fill_enclosed(&solid, 2, &again, &none) == SVO_OK && none == 0 && again.trees == solid.trees && again.twigs == solid.twigs &&
             std::memcmp(again.tree, solid.tree, solid.trees * sizeof(uint32_t)) == 0 && std::memcmp(again.twig, solid.twig, solid.twigs * 64 * sizeof(uint16_t)) == 0;
        free_chunk(shell); free_chunk(solid); free_chunk(again);
        bad += report("depth 16, a cube of 256 cells", ok);
    }
    {   // the refusals
        const uint32_t leaf[1] = { (1u << 30) | 3u }, back[9] = { 2u << 30, 0, 0, 0, 0, 0, 0, 0, 0 }, twig_node[1] = { 3u << 30 };
        const uint16_t brick[64] = { 0 };
        svo_chunk_desc in = {}, out = {};
        in.size = 1.0f; in.depth = 4; in.tree = leaf; in.trees = 1;
        bool ok = svo_chunk_fill_enclosed(nullptr, 1, &out, nullptr) == SVO_ERR_INVALID_ARG && svo_chunk_fill_enclosed(&in, 1, nullptr, nullptr) == SVO_ERR_INVALID_ARG &&
                  svo_chunk_fill_enclosed(&in, 0, &out, nullptr) == SVO_ERR_INVALID_ARG && svo_chunk_fill_enclosed(&in, 1, &in, nullptr) == SVO_ERR_INVALID_ARG;
        ok = ok && svo_chunk_fill_enclosed(&in, 1, &out, nullptr) == SVO_OK && out.trees == 1 && out.tree[0] == leaf[0];
        free_chunk(out);
        in.depth = 17;
        ok = ok && svo_chunk_fill_enclosed(&in, 1, &out, nullptr) == SVO_ERR_UNSUPPORTED;
        in.depth = 4; in.tree = back; in.trees = 9;                     // a BRANCH that points at itself
        ok = ok && svo_chunk_fill_enclosed(&in, 1, &out, nullptr) == SVO_ERR_INVALID_ARG;
        in.tree = twig_node; in.trees = 1; in.twig = brick; in.twigs = 1;   // a brick above level depth-2
        ok = ok && svo_chunk_fill_enclosed(&in, 1, &out, nullptr) == SVO_ERR_UNSUPPORTED && !out.tree && !out.twig;
        in.depth = 2;                                                   // ... and at it: one empty brick, which folds into EMPTY
        ok = ok && svo_chunk_fill_enclosed(&in, 1, &out, nullptr) == SVO_OK && out.trees == 1 && out.twigs == 0 && out.tree[0] == 0;
        free_chunk(out);
        bad += report("refusals", ok);
    }
    return bad ? 1 : 0;
}
