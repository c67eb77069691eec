// extract_check.cpp — csrc/extract.cpp (svo_chunk_extract) on its own, for the host sanitizers: compiled together with it, csrc/grid.cpp,
// csrc/sparse_mesh.cpp, csrc/mesh.cpp and csrc/sparse_fill.cpp by tests/test_extract_host_sanitize.py (g++ -fsanitize=address,undefined),
// no HIP and no libsvo_amd.so.  For built-in grids with D_A <= 5 and D_C <= D_A the pools and the count are compared, index for index,
// with a dense loop - the header's rule, cell by cell - at offsets in [-N_C, N_A] and in all 48 orientations; windows of depth 8, 10
// and 2 are taken out of the solid cube of depth 12 and 16 (sparse voxeliser, sparse fill) and their counts compared with the boxes';
// the refusals are tried; everything is freed.  Exit status 1 when something differs.
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

// the header's rule, cell by cell: for every d in [0, N_C)^3, G_C[q] = G_A[offset + d] (0 outside A), q[pi(i)] = flip_i ? N_C - 1 - d_i : d_i
static uint64_t dense_extract(const std::vector<uint16_t> &ga, int na, int nc, const svo_placement &pl, std::vector<uint16_t> &g)
{
    static const int perms[6][3] = { { 0, 1, 2 }, { 0, 2, 1 }, { 1, 0, 2 }, { 1, 2, 0 }, { 2, 0, 1 }, { 2, 1, 0 } };
    const int *pi = perms[pl.orient >> 3];
    uint64_t occupied = 0;
    g.assign((size_t)nc * nc * nc, 0);
    for (int z = 0; z < nc; ++z)
        for (int y = 0; y < nc; ++y)
            for (int x = 0; x < nc; ++x) {
                const int d[3] = { x, y, z }, p[3] = { pl.offset[0] + x, pl.offset[1] + y, pl.offset[2] + z };
                uint16_t v = 0;
                if (p[0] >= 0 && p[0] < na && p[1] >= 0 && p[1] < na && p[2] >= 0 && p[2] < na) v = ga[((size_t)p[2] * na + p[1]) * na + p[0]];
                int q[3];
                for (int i = 0; i < 3; ++i) q[pi[i]] = (pl.orient >> i) & 1 ? nc - 1 - d[i] : d[i];
                g[((size_t)q[2] * nc + q[1]) * nc + q[0]] = v;
                occupied += v != 0;
            }
    return occupied;
}

// one placement of a window of depth dc in A (depth da)
static bool same_as_dense(uint32_t da, uint32_t dc, const svo_placement &pl)
{
    const float pa[3] = { 1.0f, 2.0f, 3.0f }, pc[3] = { -4.0f, 0.0f, 9.0f };
    const std::vector<uint16_t> ga = test_grid(da, 11u * da);
    svo_chunk_desc a = {}, want = {}, got = {};
    std::vector<uint16_t> g;
    const uint64_t dense_occupied = dense_extract(ga, 1 << da, 1 << dc, pl, g);
    uint64_t occupied = 0;
    const bool ok = svo_chunk_from_grid(ga.data(), da, pa, 64.0f, &a) == SVO_OK && svo_chunk_from_grid(g.data(), dc, pc, 32.0f, &want) == SVO_OK &&
                    svo_chunk_extract(&a, &pl, dc, pc, 32.0f, &got, &occupied) == SVO_OK && same_pools(got, want) && occupied == dense_occupied && got.size == 32.0f &&
                    got.position[2] == 9.0f;
    free_chunk(want); free_chunk(got); free_chunk(a);
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

// windows of the solid cube [c - 1, c + 257)^3 of material 3: depth 8 at the odd offset c + (129, 65, 33), depth 10 around the whole
// cube, depth 2 on a face of the cube and wholly inside it
static bool deep_case(uint32_t depth, int32_t c, float cell)
{
    const float lo[3] = { c * cell, c * cell, c * cell }, pos[3] = { 0, 0, 0 };
    svo_chunk_desc a = {}, got = {};
    bool ok = Box(lo, 256.0f * cell).solid(depth, cell, 3, &a);
    uint64_t occupied = 0;
    const svo_placement odd = { { c + 129, c + 65, c + 33 }, 0 }, mirrored = { { c + 129, c + 65, c + 33 }, 46 }, whole = { { c - 383, c - 255, c - 127 }, 13 },
                        face = { { c + 255, c + 8, c + 8 }, 0 }, inside = { { c + 101, c + 77, c + 33 }, 29 };
    ok = ok && svo_chunk_extract(&a, &odd, 8, pos, 1.0f, &got, &occupied) == SVO_OK && occupied == 128ull * 192 * 224 && got.depth == 8;
    free_chunk(got);
    ok = ok && svo_chunk_extract(&a, &mirrored, 8, pos, 1.0f, &got, &occupied) == SVO_OK && occupied == 128ull * 192 * 224;
    if (ok) {                                                       // ... and stamped back: nothing to put, all of it to carve
        svo_chunk_desc back = {};
        uint64_t changed = 1;
        ok = svo_chunk_stamp(&a, &got, &mirrored, SVO_COMBINE_OVER, &back, &changed) == SVO_OK && changed == 0;
        free_chunk(back);
        ok = ok && svo_chunk_stamp(&a, &got, &mirrored, SVO_COMBINE_SUBTRACT, &back, &changed) == SVO_OK && changed == occupied;
        free_chunk(back);
    }
    free_chunk(got);
    ok = ok && svo_chunk_extract(&a, &whole, 10, pos, 1.0f, &got, &occupied) == SVO_OK && occupied == 258ull * 258 * 258;
    free_chunk(got);
    ok = ok && svo_chunk_extract(&a, &face, 2, pos, 1.0f, &got, &occupied) == SVO_OK && occupied == 2ull * 4 * 4 && got.trees == 1 && got.twigs == 1 && got.twig[0] == 3 &&
         got.twig[2] == 0;
    free_chunk(got);
    ok = ok && svo_chunk_extract(&a, &inside, 2, pos, 1.0f, &got, &occupied) == SVO_OK && occupied == 64 && got.trees == 1 && got.twigs == 0 && got.tree[0] == ((1u << 30) | 3u);
    free_chunk(got); free_chunk(a);
    return ok;
}

int main()
{
    int bad = 0;
    uint32_t s = 2025u;
    for (uint32_t da = 2; da <= 5; ++da)
        for (uint32_t dc = 2; dc <= da; ++dc) {
            const int na = 1 << da, nc = 1 << dc;
            bool ok = true;
            for (uint32_t orient = 0; ok && orient < 48; ++orient) {               // all 48 orientations, each at a drawn offset in [-N_C, N_A]
                const svo_placement pl = { { (int32_t)lcg(s, na + nc + 1) - nc, (int32_t)lcg(s, na + nc + 1) - nc, (int32_t)lcg(s, na + nc + 1) - nc }, orient };
                ok = same_as_dense(da, dc, pl);
                if (!ok) std::printf("  at offset (%d, %d, %d), orient %u\n", pl.offset[0], pl.offset[1], pl.offset[2], orient);
            }
            for (int corner = 0; ok && corner < 8; ++corner) {                      // the ends of the range, and the aligned windows
                const svo_placement far = { { corner & 1 ? na : -nc, corner & 2 ? na : -nc, corner & 4 ? na : -nc }, (uint32_t)corner * 5u };
                const svo_placement aligned = { { corner & 1 ? na - nc : 0, corner & 2 ? na - nc : 0, corner & 4 ? na - nc : 0 }, (uint32_t)corner * 6u + 1u };
                ok = same_as_dense(da, dc, far) && same_as_dense(da, dc, aligned);
            }
            char name[64];
            std::snprintf(name, sizeof name, "depth %u out of %u", dc, da);
            bad += report(name, ok);
        }
    bad += report("windows of the depth-12 cube", deep_case(12, 2880, 1.0f));
    bad += report("windows of the depth-16 cube", deep_case(16, 47104, 0.25f));
    {   // the refusals
        const uint32_t leaf[1] = { (1u << 30) | 3u }, back[9] = { 2u << 30, 0, 0, 0, 0, 0, 0, 0, 0 }, twig_node[1] = { 3u << 30 };
        const uint16_t brick[64] = { 0 };
        const float pos[3] = { 0, 0, 0 };
        svo_chunk_desc a = {}, out = {};
        a.size = 1.0f; a.depth = 4; a.tree = leaf; a.trees = 1;
        const svo_placement pl = { { 1, -2, 3 }, 7 }, turned = { { 0, 0, 0 }, 48 }, far = { { 0, 65537, 0 }, 0 }, edge = { { 65536, -65536, 0 }, 47 };
        bool ok = svo_chunk_extract(nullptr, &pl, 3, pos, 1.0f, &out, nullptr) == SVO_ERR_INVALID_ARG && svo_chunk_extract(&a, &pl, 3, pos, 1.0f, nullptr, nullptr) == SVO_ERR_INVALID_ARG &&
                  svo_chunk_extract(&a, &pl, 3, pos, 1.0f, &a, nullptr) == SVO_ERR_INVALID_ARG && svo_chunk_extract(&a, nullptr, 3, pos, 1.0f, &out, nullptr) == SVO_ERR_INVALID_ARG &&
                  svo_chunk_extract(&a, &turned, 3, pos, 1.0f, &out, nullptr) == SVO_ERR_INVALID_ARG && svo_chunk_extract(&a, &far, 3, pos, 1.0f, &out, nullptr) == SVO_ERR_INVALID_ARG &&
                  svo_chunk_extract(&a, &pl, 3, nullptr, 1.0f, &out, nullptr) == SVO_ERR_INVALID_ARG && svo_chunk_extract(&a, &pl, 3, pos, 0.0f, &out, nullptr) == SVO_ERR_INVALID_ARG &&
                  !out.tree && !out.twig;
        ok = ok && svo_chunk_extract(&a, &edge, 4, pos, 1.0f, &out, nullptr) == SVO_OK && out.trees == 1 && out.tree[0] == 0;      // wholly outside
        free_chunk(out);
        ok = ok && svo_chunk_extract(&a, &pl, 5, pos, 1.0f, &out, nullptr) == SVO_ERR_UNSUPPORTED;      // C deeper than A
        ok = ok && svo_chunk_extract(&a, &pl, 1, pos, 1.0f, &out, nullptr) == SVO_ERR_UNSUPPORTED;
        a.depth = 17;
        ok = ok && svo_chunk_extract(&a, &pl, 4, pos, 1.0f, &out, nullptr) == SVO_ERR_UNSUPPORTED;
        a.depth = 3; a.tree = back; a.trees = 9;                        // a BRANCH that points at itself
        ok = ok && svo_chunk_extract(&a, &pl, 3, pos, 1.0f, &out, nullptr) == SVO_ERR_INVALID_ARG;
        a.tree = twig_node; a.trees = 1; a.twig = brick; a.twigs = 1;   // a brick above level depth-2
        ok = ok && svo_chunk_extract(&a, &pl, 2, pos, 1.0f, &out, nullptr) == SVO_ERR_UNSUPPORTED && !out.tree && !out.twig;
        a.depth = 2;                                                    // ... and at it: an empty brick read partly outside
        ok = ok && svo_chunk_extract(&a, &pl, 2, pos, 1.0f, &out, nullptr) == SVO_OK && out.trees == 1 && out.twigs == 0 && out.tree[0] == 0;
        free_chunk(out);
        bad += report("refusals", ok);
    }
    return bad ? 1 : 0;
}
