// sparse_mesh_check.cpp — csrc/sparse_mesh.cpp (svo_chunk_from_mesh) on its own, for the host sanitizers: compiled together with it,
// csrc/mesh.cpp and csrc/grid.cpp by tests/test_sparse_mesh_host_sanitize.py (g++ -fsanitize=address,undefined), no HIP and no
// libsvo_amd.so.  For a few built-in meshes at depths 2 to 6 the pools of the sparse builder are compared, index for index, with
// svo_chunk_from_grid of svo_grid_add_mesh of a cleared grid; the Morton spread is compared with the bit loop; everything is freed.
// Exit status 1 when something differs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/svo.h"
#include "../csrc/sparse_mesh_rule.h"

namespace svo { void set_error(const std::string &) {} }        // (world.cpp's, which this program does not link)

struct Mesh {
    std::vector<float> v;
    std::vector<uint32_t> ix;
    std::vector<uint16_t> mats;
    void box(float lo, float hi)
    {
        const uint32_t base = (uint32_t)(v.size() / 3);
        for (int c = 0; c < 8; ++c)
            for (int k = 0; k < 3; ++k) v.push_back((c >> k) & 1 ? hi : lo);
        static const uint32_t quads[6][4] = { { 0, 1, 3, 2 }, { 4, 6, 7, 5 }, { 0, 4, 5, 1 }, { 2, 3, 7, 6 }, { 0, 2, 6, 4 }, { 1, 5, 7, 3 } };
        for (const auto &q : quads) for (uint32_t t : { q[0], q[1], q[2], q[0], q[2], q[3] }) ix.push_back(base + t);
    }
    void soup(uint32_t seed, int count, float n)           // `count` triangles around a grid of n cells, some of them outside
    {
        uint32_t s = seed;
        auto next = [&] { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; };
        for (int t = 0; t < count; ++t) {
            const float c[3] = { (next() * 1.4f - 0.2f) * n, (next() * 1.4f - 0.2f) * n, (next() * 1.4f - 0.2f) * n }, ext = 0.05f + next() * n / 3.0f;
            for (int k = 0; k < 9; ++k) v.push_back(c[k % 3] + (next() - 0.5f) * ext);
            for (int k = 0; k < 3; ++k) ix.push_back((uint32_t)(3 * t + k));
            mats.push_back((uint16_t)(1 + (s >> 20) % 999));
        }
    }
    svo_mesh desc(uint16_t material) const
    {
        svo_mesh m = {};
        m.vertices = v.data(); m.indices = ix.data(); m.materials = mats.empty() ? nullptr : mats.data();
        m.nvertices = (uint32_t)(v.size() / 3); m.ntriangles = (uint32_t)(ix.size() / 3);
        m.cell = 1.0f; m.material = material;
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

// the sparse pools of the list equal the dense path's, index for index
static bool same_as_dense(const std::vector<svo_mesh> &meshes, uint32_t depth, bool want_empty = false)
{
    const float pos[3] = { 1.0f, 2.0f, 3.0f };
    std::vector<uint16_t> grid((size_t)1 << (3 * depth), 0);
    for (const svo_mesh &m : meshes)
        if (svo_grid_add_mesh(&m, depth, grid.data()) != SVO_OK) return false;
    svo_chunk_desc dense = {}, sparse = {};
    if (svo_chunk_from_grid(grid.data(), depth, pos, 64.0f, &dense) != SVO_OK) return false;
    if (svo_chunk_from_mesh(meshes.data(), (int)meshes.size(), depth, pos, 64.0f, &sparse) != SVO_OK) { free_chunk(dense); return false; }
    bool ok = dense.trees == sparse.trees && dense.twigs == sparse.twigs && sparse.depth == depth && sparse.size == 64.0f && sparse.position[2] == 3.0f;
    ok = ok && std::memcmp(dense.tree, sparse.tree, dense.trees * sizeof(uint32_t)) == 0;
    ok = ok && (dense.twigs == 0 || std::memcmp(dense.twig, sparse.twig, dense.twigs * 64 * sizeof(uint16_t)) == 0);
    ok = ok && (want_empty ? dense.trees == 1 && dense.tree[0] == 0 : dense.tree[0] != 0);     // a case that marks nothing where it should proves nothing
    free_chunk(dense); free_chunk(sparse);
    return ok;
}

int main()
{
    int bad = 0;
    {   // the spread of the Morton key against the bit loop
        bool ok = true;
        for (uint32_t v = 0; v < 65536u; ++v) {
            uint64_t want = 0;
            for (int b = 0; b < 16; ++b) want |= (uint64_t)((v >> b) & 1u) << (3 * b);
            ok = ok && svo::sparse_spread(v) == want;
        }
        ok = ok && svo::sparse_key(0xFFFFu, 0xFFFFu, 0xFFFFu) == 0xFFFFFFFFFFFFull && svo::sparse_brick_index(svo::sparse_word(1, 2, 3, 9)) == 3 * 16 + 2 * 4 + 1;
        bad += report("morton key", ok);
    }
    {   // the decode of a tile job (the device's, mesh_rule.h) on both sides of 2^32: boxes of up to (2^14)^3 tiles, depth 16
        bool ok = true;
        const uint32_t dims[4][3] = { { 1, 1, 1 }, { 7, 5, 3 }, { 2048, 2048, 2048 }, { 16384, 16384, 16384 } };
        for (const auto &d : dims) {
            const unsigned long long total = (unsigned long long)d[0] * d[1] * d[2];
            const unsigned long long some[] = { 0, 1, total / 3, total / 2 + 1, total - 1, 0xFFFFFFFFull, 0x100000000ull, 0x100000001ull, (1ull << 41) + 12345 };
            for (unsigned long long local : some) {
                if (local >= total) continue;
                uint32_t ox, oy, oz;
                svo::mesh_tile_of_job(local, d[0], d[1], ox, oy, oz);
                ok = ok && ox < d[0] && oy < d[1] && oz < d[2] && ox + (unsigned long long)d[0] * (oy + (unsigned long long)d[1] * oz) == local;
            }
        }
        bad += report("tile job decode", ok);
    }
    for (uint32_t depth = 2; depth <= 6; ++depth) {
        const float n = (float)(1u << depth);
        char name[64];
        Mesh a; a.box(0.27f * n, 0.77f * n);                            // off the lattice
        std::snprintf(name, sizeof name, "depth %u, box", depth);
        bad += report(name, same_as_dense({ a.desc(5) }, depth));
        Mesh s; s.soup(depth, 40, n);
        Mesh b; b.box(1.0f, n - 1.0f);                                  // on the lattice, and it shares cells with the soup
        std::snprintf(name, sizeof name, "depth %u, soup and lattice box", depth);
        bad += report(name, same_as_dense({ s.desc(1), b.desc(0xFFFF) }, depth));
    }
    {   // quads in lattice planes that cover the whole grid: the root is one LEAF
        Mesh q;
        for (float z : { 1.0f, 3.0f, 5.0f, 7.0f }) {
            const uint32_t base = (uint32_t)(q.v.size() / 3);
            for (float c : { 0.25f, 0.25f, z, 7.75f, 0.25f, z, 7.75f, 7.75f, z, 0.25f, 7.75f, z }) q.v.push_back(c);
            for (uint32_t t : { 0u, 1u, 2u, 0u, 2u, 3u }) q.ix.push_back(base + t);
        }
        const svo_mesh d = q.desc(7);
        const float pos[3] = { 0, 0, 0 };
        svo_chunk_desc c = {};
        bool ok = svo_chunk_from_mesh(&d, 1, 3, pos, 8.0f, &c) == SVO_OK && c.trees == 1 && c.twigs == 0 && c.tree[0] == ((1u << 30) | 7u);
        free_chunk(c);
        bad += report("depth 3, wholly covered", ok && same_as_dense({ d }, 3));
    }
    {   // nothing marked: no mesh, dropped triangles (indices out of range, vertices that are not finite, no area), material 0
        Mesh m;
        const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
        m.v = { 1, 1, 1, 2, 3, 1, 3, 1, 2, nan, 1, 1, 1, inf, 1 };
        m.ix = { 0, 1, 5, 0xFFFFFFFFu, 1, 2, 0, 1, 3, 0, 4, 2, 0, 0, 1 };
        bool ok = same_as_dense({ m.desc(9) }, 4, true) && same_as_dense({}, 2, true);
        m.ix = { 0, 1, 2 };
        ok = ok && same_as_dense({ m.desc(0) }, 4, true) && same_as_dense({ m.desc(9) }, 4);
        bad += report("nothing marked", ok);
    }
    {   // depth 16: the last cell of the grid
        Mesh m;
        m.v = { 65535.3f, 65535.3f, 65535.3f, 65535.6f, 65535.4f, 65535.35f, 65535.4f, 65535.7f, 65535.5f };
        m.ix = { 0, 1, 2 };
        const svo_mesh d = m.desc(0xFFFF);
        const float pos[3] = { 0, 0, 0 };
        svo_chunk_desc c = {};
        bool ok = svo_chunk_from_mesh(&d, 1, 16, pos, 128.0f, &c) == SVO_OK && c.trees == 1 + 8 * 14 && c.twigs == 1 && c.twig[63] == 0xFFFF;
        for (int k = 0; ok && k < 63; ++k) ok = c.twig[k] == 0;
        free_chunk(c);
        bad += report("depth 16, the last cell", ok);
    }
    {   // the refusals
        Mesh m; m.box(1.0f, 2.0f);
        svo_mesh d = m.desc(1);
        const float pos[3] = { 0, 0, 0 };
        svo_chunk_desc c = {};
        bool ok = svo_chunk_from_mesh(nullptr, 1, 4, pos, 1.0f, &c) == SVO_ERR_INVALID_ARG && svo_chunk_from_mesh(&d, -1, 4, pos, 1.0f, &c) == SVO_ERR_INVALID_ARG &&
                  svo_chunk_from_mesh(&d, 1, 1, pos, 1.0f, &c) == SVO_ERR_INVALID_ARG && svo_chunk_from_mesh(&d, 1, 17, pos, 1.0f, &c) == SVO_ERR_INVALID_ARG &&
                  svo_chunk_from_mesh(&d, 1, 4, nullptr, 1.0f, &c) == SVO_ERR_INVALID_ARG && svo_chunk_from_mesh(&d, 1, 4, pos, 0.0f, &c) == SVO_ERR_INVALID_ARG &&
                  svo_chunk_from_mesh(&d, 1, 4, pos, 1.0f, nullptr) == SVO_ERR_INVALID_ARG;
        d.cell = 0.0f;
        ok = ok && svo_chunk_from_mesh(&d, 1, 4, pos, 1.0f, &c) == SVO_ERR_INVALID_ARG;
        d.cell = 1.0f; d.indices = nullptr;
        ok = ok && svo_chunk_from_mesh(&d, 1, 4, pos, 1.0f, &c) == SVO_ERR_INVALID_ARG && !c.tree && !c.twig;
        bad += report("refusals", ok);
    }
    return bad ? 1 : 0;
}
