// stamp_check.cpp — csrc/stamp.cpp (svo_chunk_stamp) on its own, for the host sanitizers: compiled together with it, csrc/grid.cpp,
// csrc/sparse_mesh.cpp, csrc/mesh.cpp and csrc/sparse_fill.cpp by tests/test_stamp_host_sanitize.py (g++ -fsanitize=address,undefined),
// no HIP and no libsvo_amd.so.  For built-in grids with D_A <= 5 and D_B <= D_A the five ops are compared, index for index and count for
// count, with a dense loop - the header's rule, cell by cell - at offsets in [-N_B, N_A] and in all 48 orientations; a LEAF-root B of
// depth 8 is stamped at an odd offset into the solid cube of depth 12 and 16 (sparse voxeliser, sparse fill) and its counts compared
// with the boxes'; the refusals are tried; everything is freed.  Exit status 1 when something differs.
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

static uint32_t lcg(uint32_t &s, uint32_t m) { s = s * 1664525u + 1013904223u; return (s >> 8) % m; }

// boxes of a few materials over an empty background, and noise in one octant: EMPTY and LEAF nodes of every size beside bricks
static std::vector<uint16_t> test_grid(uint32_t depth, uint32_t seed)
{
    const uint32_t n = 1u << depth;
    std::vector<uint16_t> g((size_t)n * n * n, 0);
    uint32_t s = seed;
    static const uint16_t mats[4] = { 1, 5, 300, 0xFFFF };
    for (int k = 0; k < 5; ++k) {
        uint32_t lo[3], hi[3];
        for (int a = 0; a < 3; ++a) { lo[a] = lcg(s, n); hi[a] = lo[a] + 1 + lcg(s, n / 2 + 1); if (hi[a] > n) hi[a] = n; }
        const uint16_t m = mats[lcg(s, 4)];
        for (uint32_t z = lo[2]; z < hi[2]; ++z)
            for (uint32_t y = lo[1]; y < hi[1]; ++y)
                for (uint32_t x = lo[0]; x < hi[0]; ++x) g[((size_t)z * n + y) * n + x] = m;
    }
    const uint32_t h = n / 2, oct = lcg(s, 8);
    for (uint32_t z = 0; z < h; ++z)
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < h; ++x)
                if (lcg(s, 3) == 0) g[((size_t)(z + (oct >> 2) * h) * n + y + ((oct >> 1) & 1) * h) * n + x + (oct & 1) * h] = mats[lcg(s, 4)];
    return g;
}

static bool same_pools(const svo_chunk_desc &x, const svo_chunk_desc &y)
{
    return x.trees == y.trees && x.twigs == y.twigs && x.depth == y.depth && std::memcmp(x.tree, y.tree, x.trees * sizeof(uint32_t)) == 0 &&
           (x.twigs == 0 || std::memcmp(x.twig, y.twig, x.twigs * 64 * sizeof(uint16_t)) == 0);
}

// the header's rule, cell by cell: G[p] = f(G_A[p], b), b = 0 outside B's cube, else G_B[q] with q[pi(i)] = flip_i ? N_B - 1 - d_i : d_i
static uint64_t dense_stamp(const std::vector<uint16_t> &ga, int na, const std::vector<uint16_t> &gb, int nb, const svo_placement &pl, int op, std::vector<uint16_t> &g)
{
    static const int perms[6][3] = { { 0, 1, 2 }, { 0, 2, 1 }, { 1, 0, 2 }, { 1, 2, 0 }, { 2, 0, 1 }, { 2, 1, 0 } };
    const int *pi = perms[pl.orient >> 3];
    uint64_t changed = 0;
    g.resize(ga.size());
    for (int z = 0; z < na; ++z)
        for (int y = 0; y < na; ++y)
            for (int x = 0; x < na; ++x) {
                const int d[3] = { x - pl.offset[0], y - pl.offset[1], z - pl.offset[2] };
                uint16_t b = 0;
                if (d[0] >= 0 && d[0] < nb && d[1] >= 0 && d[1] < nb && d[2] >= 0 && d[2] < nb) {
                    int q[3];
                    for (int i = 0; i < 3; ++i) q[pi[i]] = (pl.orient >> i) & 1 ? nb - 1 - d[i] : d[i];
                    b = gb[((size_t)q[2] * nb + q[1]) * nb + q[0]];
                }
                const size_t at = ((size_t)z * na + y) * na + x;
                g[at] = cell_rule(op, ga[at], b);
                changed += g[at] != ga[at];
            }
    return changed;
}

// every op at one placement of B (depth db) in A (depth da)
static bool same_as_dense(uint32_t da, uint32_t db, const svo_placement &pl)
{
    const float pa[3] = { 1.0f, 2.0f, 3.0f }, pb[3] = { -4.0f, 0.0f, 9.0f };
    const std::vector<uint16_t> ga = test_grid(da, 11u * da), gb = test_grid(db, 7u * db + 1u);
    svo_chunk_desc a = {}, b = {};
    bool ok = svo_chunk_from_grid(ga.data(), da, pa, 64.0f, &a) == SVO_OK && svo_chunk_from_grid(gb.data(), db, pb, 32.0f, &b) == SVO_OK;
    std::vector<uint16_t> g;
    for (int op = 0; ok && op < 5; ++op) {
        const uint64_t dense_changed = dense_stamp(ga, 1 << da, gb, 1 << db, pl, op, g);
        svo_chunk_desc want = {}, got = {};
        uint64_t changed = 0;
        ok = svo_chunk_from_grid(g.data(), da, pa, 64.0f, &want) == SVO_OK && svo_chunk_stamp(&a, &b, &pl, op, &got, &changed) == SVO_OK && same_pools(got, want) &&
             changed == dense_changed && got.size == 64.0f && got.position[2] == 3.0f;
        free_chunk(want); free_chunk(got);
    }
    free_chunk(a); free_chunk(b);
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
    bool solid(uint32_t depth, float cell, uint16_t material, svo_chunk_desc *out) const
    {
        svo_mesh m = {};
        m.vertices = v.data(); m.indices = ix.data(); m.nvertices = 8; m.ntriangles = 12; m.cell = cell; m.material = material;
        const float pos[3] = { 0, 0, 0 };
        svo_chunk_desc shell = {};
        uint64_t filled = 0;
        const bool ok = svo_chunk_from_mesh(&m, 1, depth, pos, 128.0f, &shell) == SVO_OK && svo_chunk_fill_enclosed(&shell, material, out, &filled) == SVO_OK && filled == 254ull * 254 * 254;
        free_chunk(shell);
        return ok;
    }
};

// a LEAF-root B of depth 8 (256 cells of material 5) at the odd offset c + (129, 65, 33) into the solid cube [c - 1, c + 257)^3
static bool deep_case(uint32_t depth, int32_t c, float cell)
{
    const float lo[3] = { c * cell, c * cell, c * cell };
    svo_chunk_desc a = {}, b = {}, got = {};
    const uint32_t leaf[1] = { (1u << 30) | 5u };
    b.size = 1.0f; b.depth = 8; b.tree = leaf; b.trees = 1;
    bool ok = Box(lo, 256.0f * cell).solid(depth, cell, 3, &a);
    const svo_placement pl = { { c + 129, c + 65, c + 33 }, 0 };
    uint64_t changed = 0;
    ok = ok && svo_chunk_stamp(&a, &b, &pl, SVO_COMBINE_MAX, &got, &changed) == SVO_OK && changed == 256ull * 256 * 256 && got.depth == depth;
    free_chunk(got);
    ok = ok && svo_chunk_stamp(&a, &b, &pl, SVO_COMBINE_SUBTRACT, &got, &changed) == SVO_OK && changed == 128ull * 192 * 224;      // the two boxes' overlap
    free_chunk(got);
    const svo_placement mirrored = { { c + 129, c + 65, c + 33 }, 46 };
    ok = ok && svo_chunk_stamp(&a, &b, &mirrored, SVO_COMBINE_INTERSECT, &got, &changed) == SVO_OK && changed == 258ull * 258 * 258 - 128ull * 192 * 224;
    free_chunk(got); free_chunk(a);
    return ok;
}

int main()
{
    int bad = 0;
    uint32_t s = 2024u;
    for (uint32_t da = 2; da <= 5; ++da)
        for (uint32_t db = 2; db <= da; ++db) {
            const int na = 1 << da, nb = 1 << db;
            bool ok = true;
            for (uint32_t orient = 0; ok && orient < 48; ++orient) {               // all 48 orientations, each at a drawn offset in [-N_B, N_A]
                const svo_placement pl = { { (int32_t)lcg(s, na + nb + 1) - nb, (int32_t)lcg(s, na + nb + 1) - nb, (int32_t)lcg(s, na + nb + 1) - nb }, orient };
                ok = same_as_dense(da, db, pl);
                if (!ok) std::printf("  at offset (%d, %d, %d), orient %u\n", pl.offset[0], pl.offset[1], pl.offset[2], orient);
            }
            for (int corner = 0; ok && corner < 8; ++corner) {                      // the ends of the range, and the aligned placements
                const svo_placement far = { { corner & 1 ? na : -nb, corner & 2 ? na : -nb, corner & 4 ? na : -nb }, (uint32_t)corner * 5u };
                const svo_placement aligned = { { corner & 1 ? na - nb : 0, corner & 2 ? na - nb : 0, corner & 4 ? na - nb : 0 }, (uint32_t)corner * 6u + 1u };
                ok = same_as_dense(da, db, far) && same_as_dense(da, db, aligned);
            }
            char name[64];
            std::snprintf(name, sizeof name, "depth %u into %u", db, da);
            bad += report(name, ok);
        }
    bad += report("depth 8 LEAF into the depth-12 cube", deep_case(12, 2880, 1.0f));
    bad += report("depth 8 LEAF into the depth-16 cube", deep_case(16, 47104, 0.25f));
    {   // the refusals
        const uint32_t leaf[1] = { (1u << 30) | 3u }, back[9] = { 2u << 30, 0, 0, 0, 0, 0, 0, 0, 0 }, twig_node[1] = { 3u << 30 };
        const uint16_t brick[64] = { 0 };
        svo_chunk_desc a = {}, b = {}, out = {};
        a.size = 1.0f; a.depth = 4; a.tree = leaf; a.trees = 1;
        b = a;
        const svo_placement pl = { { 1, -2, 3 }, 7 }, turned = { { 0, 0, 0 }, 48 }, far = { { 0, 65537, 0 }, 0 }, edge = { { 65536, -65536, 0 }, 47 };
        bool ok = svo_chunk_stamp(nullptr, &b, &pl, 0, &out, nullptr) == SVO_ERR_INVALID_ARG && svo_chunk_stamp(&a, nullptr, &pl, 0, &out, nullptr) == SVO_ERR_INVALID_ARG &&
                  svo_chunk_stamp(&a, &b, &pl, 0, nullptr, nullptr) == SVO_ERR_INVALID_ARG && svo_chunk_stamp(&a, &b, &pl, 0, &a, nullptr) == SVO_ERR_INVALID_ARG &&
                  svo_chunk_stamp(&a, &b, &pl, 0, &b, nullptr) == SVO_ERR_INVALID_ARG && svo_chunk_stamp(&a, &b, &pl, 5, &out, nullptr) == SVO_ERR_INVALID_ARG &&
                  svo_chunk_stamp(&a, &b, nullptr, 0, &out, nullptr) == SVO_ERR_INVALID_ARG && svo_chunk_stamp(&a, &b, &turned, 0, &out, nullptr) == SVO_ERR_INVALID_ARG &&
                  svo_chunk_stamp(&a, &b, &far, 0, &out, nullptr) == SVO_ERR_INVALID_ARG && !out.tree && !out.twig;
        ok = ok && svo_chunk_stamp(&a, &a, &edge, SVO_COMBINE_MAX, &out, nullptr) == SVO_OK && out.trees == 1 && out.tree[0] == leaf[0];
        free_chunk(out);
        b.depth = 5;                                                    // B deeper than A
        ok = ok && svo_chunk_stamp(&a, &b, &pl, 0, &out, nullptr) == SVO_ERR_UNSUPPORTED;
        a.depth = 17; b.depth = 4;
        ok = ok && svo_chunk_stamp(&a, &b, &pl, 0, &out, nullptr) == SVO_ERR_UNSUPPORTED;
        a.depth = 4; b.depth = 1;
        ok = ok && svo_chunk_stamp(&a, &b, &pl, 0, &out, nullptr) == SVO_ERR_UNSUPPORTED;
        b.depth = 3; b.tree = back; b.trees = 9;                        // a BRANCH that points at itself
        ok = ok && svo_chunk_stamp(&a, &b, &pl, 0, &out, nullptr) == SVO_ERR_INVALID_ARG;
        b.tree = twig_node; b.trees = 1; b.twig = brick; b.twigs = 1;   // a brick above level depth-2
        ok = ok && svo_chunk_stamp(&a, &b, &pl, 0, &out, nullptr) == SVO_ERR_UNSUPPORTED && !out.tree && !out.twig;
        b.depth = 2;                                                    // ... and at it: a LEAF cleared outside an empty brick
        ok = ok && svo_chunk_stamp(&a, &b, &pl, SVO_COMBINE_INTERSECT, &out, nullptr) == SVO_OK && out.trees == 1 && out.twigs == 0 && out.tree[0] == 0;
        free_chunk(out);
        bad += report("refusals", ok);
    }
    return bad ? 1 : 0;
}
