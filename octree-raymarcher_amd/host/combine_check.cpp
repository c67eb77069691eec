// combine_check.cpp — csrc/combine.cpp (svo_chunk_combine) on its own, for the host sanitizers: compiled together with it,
// csrc/grid.cpp, csrc/sparse_mesh.cpp, csrc/mesh.cpp and csrc/sparse_fill.cpp by tests/test_combine_host_sanitize.py (g++
// -fsanitize=address,undefined), no HIP and no libsvo_amd.so.  For built-in grids at depths 2 to 6 the five ops are compared, index for
// index and count for count, with a dense loop: svo_chunk_from_grid of f_op over the two grids; the two depth-16 cubes (sparse
// voxeliser, sparse fill) are combined and their counts compared with the closed form; the refusals are tried; everything is freed.
// Exit status 1 when something differs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/svo.h"

namespace svo { void set_error(const std::string &) {} }        // (world.cpp's, which this program does not link)

static void free_chunk(svo_chunk_desc &c)
{
    std::free(const_cast<uint32_t *>(c.tree));                      // what svo_chunk_free does (world.cpp)
    std::free(const_cast<uint16_t *>(c.twig));
    c.tree = nullptr; c.twig = nullptr;
}

static int report(const char *name, bool ok) { std::printf("%s: %s\n", name, ok ? "ok" : "WRONG"); return ok ? 0 : 1; }

static uint16_t cell_rule(int op, uint16_t a, uint16_t b)           // the header's table, restated
{
    switch (op) {
    case SVO_COMBINE_MAX:      return a > b ? a : b;
    case SVO_COMBINE_UNDER:    return a ? a : b;
    case SVO_COMBINE_OVER:     return b ? b : a;
    case SVO_COMBINE_SUBTRACT: return b ? (uint16_t)0 : a;
    default:                   return b ? a : (uint16_t)0;
    }
}

// boxes of a few materials over an empty background, and noise in one octant: EMPTY and LEAF nodes of every size beside bricks
static std::vector<uint16_t> test_grid(uint32_t depth, uint32_t seed)
{
    const uint32_t n = 1u << depth;
    std::vector<uint16_t> g((size_t)n * n * n, 0);
    uint32_t s = seed;
    auto next = [&](uint32_t m) { s = s * 1664525u + 1013904223u; return (s >> 8) % m; };
    static const uint16_t mats[4] = { 1, 5, 300, 0xFFFF };
    for (int k = 0; k < 6; ++k) {
        uint32_t lo[3], hi[3];
        for (int a = 0; a < 3; ++a) { lo[a] = next(n); hi[a] = lo[a] + 1 + next(n / 2 + 1); if (hi[a] > n) hi[a] = n; }
        const uint16_t m = mats[next(4)];
        for (uint32_t z = lo[2]; z < hi[2]; ++z)
            for (uint32_t y = lo[1]; y < hi[1]; ++y)
                for (uint32_t x = lo[0]; x < hi[0]; ++x) g[((size_t)z * n + y) * n + x] = m;
    }
    const uint32_t h = n / 2, oct = next(8);
    for (uint32_t z = 0; z < h; ++z)
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < h; ++x)
                if (next(3) == 0) g[((size_t)(z + (oct >> 2) * h) * n + y + ((oct >> 1) & 1) * h) * n + x + (oct & 1) * h] = mats[next(4)];
    return g;
}

static bool same_pools(const svo_chunk_desc &x, const svo_chunk_desc &y)
{
    return x.trees == y.trees && x.twigs == y.twigs && x.depth == y.depth && std::memcmp(x.tree, y.tree, x.trees * sizeof(uint32_t)) == 0 &&
           (x.twigs == 0 || std::memcmp(x.twig, y.twig, x.twigs * 64 * sizeof(uint16_t)) == 0);
}

static bool same_as_dense(uint32_t depth, int op)
{
    const float pa[3] = { 1.0f, 2.0f, 3.0f }, pb[3] = { -4.0f, 0.0f, 9.0f };
    const std::vector<uint16_t> ga = test_grid(depth, 11u * depth), gb = test_grid(depth, 7u * depth + 1u);
    std::vector<uint16_t> g(ga.size());
    uint64_t dense_changed = 0, changed = 0;
    for (size_t i = 0; i < g.size(); ++i) { g[i] = cell_rule(op, ga[i], gb[i]); dense_changed += g[i] != ga[i]; }
    svo_chunk_desc a = {}, b = {}, want = {}, got = {};
    bool ok = svo_chunk_from_grid(ga.data(), depth, pa, 64.0f, &a) == SVO_OK && svo_chunk_from_grid(gb.data(), depth, pb, 32.0f, &b) == SVO_OK &&
              svo_chunk_from_grid(g.data(), depth, pa, 64.0f, &want) == SVO_OK;
    ok = ok && svo_chunk_combine(&a, &b, op, &got, &changed) == SVO_OK && same_pools(got, want) && changed == dense_changed && got.size == 64.0f && got.position[2] == 3.0f;
    free_chunk(a); free_chunk(b); free_chunk(want); free_chunk(got);
    return ok;
}

struct Box {
    std::vector<float> v;
    std::vector<uint32_t> ix;
    Box(const float lo[3], float edge)
    {
        for (int c = 0; c < 8; ++c)
            for (int k = 0; k < 3; ++k) v.push_back(lo[k] + ((c >> k) & 1 ? edge : 0.0f));
        static const uint32_t quads[6][4] = { { 0, 1, 3, 2 }, { 4, 6, 7, 5 }, { 0, 4, 5, 1 }, { 2, 3, 7, 6 }, { 0, 2, 6, 4 }, { 1, 5, 7, 3 } };
        for (const auto &q : quads) for (uint32_t t : { q[0], q[1], q[2], q[0], q[2], q[3] }) ix.push_back(t);
    }
    // the solid cube: the shell of the closed rule (258 cells per axis) filled with its own material
    bool solid(uint16_t material, svo_chunk_desc *out) const
    {
        svo_mesh m = {};
        m.vertices = v.data(); m.indices = ix.data(); m.nvertices = 8; m.ntriangles = 12; m.cell = 0.25f; m.material = material;
        const float pos[3] = { 0, 0, 0 };
        svo_chunk_desc shell = {};
        uint64_t filled = 0;
        const bool ok = svo_chunk_from_mesh(&m, 1, 16, pos, 128.0f, &shell) == SVO_OK && svo_chunk_fill_enclosed(&shell, material, out, &filled) == SVO_OK && filled == 254ull * 254 * 254;
        free_chunk(shell);
        return ok;
    }
};

int main()
{
    int bad = 0;
    static const char *names[5] = { "MAX", "UNDER", "OVER", "SUBTRACT", "INTERSECT" };
    for (uint32_t depth = 2; depth <= 6; ++depth)
        for (int op = 0; op < 5; ++op) {
            char name[64];
            std::snprintf(name, sizeof name, "depth %u, %s", depth, names[op]);
            bad += report(name, same_as_dense(depth, op));
        }
    {   // depth 16: two solid cubes of 258 cells far from the origin, the second shifted by (128, 64, 32) cells
        const float c = 47104.0f * 0.25f, la[3] = { c, c, c }, lb[3] = { c + 32.0f, c + 16.0f, c + 8.0f };
        svo_chunk_desc a = {}, b = {};
        bool ok = Box(la, 64.0f).solid(3, &a) && Box(lb, 64.0f).solid(5, &b);
        const uint64_t cube = 258ull * 258 * 258, overlap = 130ull * 194 * 226;
        const uint64_t want[5] = { cube, cube - overlap, cube, overlap, cube - overlap };
        for (int op = 0; ok && op < 5; ++op) {
            svo_chunk_desc got = {};
            uint64_t changed = 0;
            ok = svo_chunk_combine(&a, &b, op, &got, &changed) == SVO_OK && changed == want[op] && got.depth == 16 && got.trees <= a.trees + b.trees && got.twigs <= a.twigs + b.twigs;
            free_chunk(got);
        }
        svo_chunk_desc none = {};
        uint64_t changed = 1;
        ok = ok && svo_chunk_combine(&a, &a, SVO_COMBINE_SUBTRACT, &none, &changed) == SVO_OK && none.trees == 1 && none.tree[0] == 0 && none.twigs == 0 && changed == cube;
        free_chunk(none); free_chunk(a); free_chunk(b);
        bad += report("depth 16, two cubes of 258 cells", ok);
    }
    {   // the refusals
        const uint32_t leaf[1] = { (1u << 30) | 3u }, back[9] = { 2u << 30, 0, 0, 0, 0, 0, 0, 0, 0 }, twig_node[1] = { 3u << 30 };
        const uint16_t brick[64] = { 0 };
        svo_chunk_desc a = {}, b = {}, out = {};
        a.size = 1.0f; a.depth = 4; a.tree = leaf; a.trees = 1;
        b = a;
        bool ok = svo_chunk_combine(nullptr, &b, 0, &out, nullptr) == SVO_ERR_INVALID_ARG && svo_chunk_combine(&a, nullptr, 0, &out, nullptr) == SVO_ERR_INVALID_ARG &&
                  svo_chunk_combine(&a, &b, 0, nullptr, nullptr) == SVO_ERR_INVALID_ARG && svo_chunk_combine(&a, &b, 0, &a, nullptr) == SVO_ERR_INVALID_ARG &&
                  svo_chunk_combine(&a, &b, 0, &b, nullptr) == SVO_ERR_INVALID_ARG && svo_chunk_combine(&a, &b, 5, &out, nullptr) == SVO_ERR_INVALID_ARG;
        ok = ok && svo_chunk_combine(&a, &a, SVO_COMBINE_MAX, &out, nullptr) == SVO_OK && out.trees == 1 && out.tree[0] == leaf[0];
        free_chunk(out);
        b.depth = 5;
        ok = ok && svo_chunk_combine(&a, &b, 0, &out, nullptr) == SVO_ERR_UNSUPPORTED;
        a.depth = b.depth = 17;
        ok = ok && svo_chunk_combine(&a, &b, 0, &out, nullptr) == SVO_ERR_UNSUPPORTED;
        a.depth = b.depth = 4; b.tree = back; b.trees = 9;             // a BRANCH that points at itself
        ok = ok && svo_chunk_combine(&a, &b, 0, &out, nullptr) == SVO_ERR_INVALID_ARG;
        b.tree = twig_node; b.trees = 1; b.twig = brick; b.twigs = 1;   // a brick above level depth-2
        ok = ok && svo_chunk_combine(&a, &b, 0, &out, nullptr) == SVO_ERR_UNSUPPORTED && !out.tree && !out.twig;
        a.depth = b.depth = 2;                                          // ... and at it: a LEAF over an empty brick
        ok = ok && svo_chunk_combine(&a, &b, SVO_COMBINE_INTERSECT, &out, nullptr) == SVO_OK && out.trees == 1 && out.twigs == 0 && out.tree[0] == 0;
        free_chunk(out);
        bad += report("refusals", ok);
    }
    return bad ? 1 : 0;
}
