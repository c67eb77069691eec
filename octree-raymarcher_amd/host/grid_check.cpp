// grid_check.cpp — csrc/grid.cpp (svo_chunk_from_grid) on its own, for the host sanitizers: compiled together with it by
// tests/test_grid_host_sanitize.py (g++ -fsanitize=address,undefined), no HIP and no libsvo_amd.so.  Builds the pools of a few grids,
// checks their counts against a plain count of the grid's mixed blocks, frees everything.  Exit status 1 when a count is off.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/svo.h"

namespace svo { void set_error(const std::string &) {} }        // (world.cpp's, which this program does not link)

static bool mixed(const std::vector<uint16_t> &g, uint32_t N, uint32_t x, uint32_t y, uint32_t z, uint32_t e)
{
    const uint16_t v = g[((size_t)z * N + y) * N + x];
    for (uint32_t k = z; k < z + e; ++k)
        for (uint32_t j = y; j < y + e; ++j)
            for (uint32_t i = x; i < x + e; ++i) if (g[((size_t)k * N + j) * N + i] != v) return true;
    return false;
}

static int check(const char *name, const std::vector<uint16_t> &g, uint32_t depth)
{
    const uint32_t N = 1u << depth;
    const float pos[3] = { 0.0f, 0.0f, 0.0f };
    svo_chunk_desc c;
    if (svo_chunk_from_grid(g.data(), depth, pos, 128.0f, &c) != SVO_OK) { std::printf("%s: build failed\n", name); return 1; }
    uint64_t branches = 0, twigs = 0;
    for (uint32_t L = 0; L + 2 <= depth; ++L) {
        const uint32_t e = N >> L;
        for (uint32_t z = 0; z < N; z += e)
            for (uint32_t y = 0; y < N; y += e)
                for (uint32_t x = 0; x < N; x += e) if (mixed(g, N, x, y, z, e)) ++(L + 2 == depth ? twigs : branches);
    }
    uint64_t words = 0;                                             // BRANCH words in the pool
    for (uint64_t i = 0; i < c.trees; ++i) words += (c.tree[i] >> 30) == SVO_BRANCH ? 1 : 0;
    const bool ok = c.trees == 1 + 8 * branches && c.twigs == twigs && words == branches && c.depth == depth;
    std::printf("%s: %llu node words, %llu bricks: %s\n", name, (unsigned long long)c.trees, (unsigned long long)c.twigs, ok ? "ok" : "WRONG");
    std::free(const_cast<uint32_t *>(c.tree));                      // what svo_chunk_free does (world.cpp)
    std::free(const_cast<uint16_t *>(c.twig));
    return ok ? 0 : 1;
}

int main()
{
    int bad = 0;
    uint32_t seed = 12345u;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 16; };
    bad += check("depth 2, all zero", std::vector<uint16_t>(64, 0), 2);
    bad += check("depth 2, all 7", std::vector<uint16_t>(64, 7), 2);
    std::vector<uint16_t> g(64);
    for (size_t i = 0; i < g.size(); ++i) g[i] = (uint16_t)(i + 1);
    bad += check("depth 2, every material distinct", g, 2);
    g.assign(512, 0);
    for (uint32_t z = 0; z < 8; ++z)
        for (uint32_t y = 0; y < 8; ++y)
            for (uint32_t x = 0; x < 8; ++x) {
                const uint32_t o = (x >> 2) | (y >> 2) << 1 | (z >> 2) << 2;
                g[(z * 8 + y) * 8 + x] = o == 0 ? 0xFFFF : o == 1 ? 0 : o == 2 ? 9 : (uint16_t)(rnd() % 3);
            }
    bad += check("depth 3, octants", g, 3);
    g.assign(32 * 32 * 32, 0);
    for (int b = 0; b < 10; ++b) {
        const uint32_t x0 = rnd() % 28, y0 = rnd() % 28, z0 = rnd() % 28, ex = 1 + rnd() % 10, ey = 1 + rnd() % 10, ez = 1 + rnd() % 10;
        const uint16_t m = (uint16_t)(1 + rnd() % 0xFFFF);
        for (uint32_t z = z0; z < z0 + ez && z < 32; ++z)
            for (uint32_t y = y0; y < y0 + ey && y < 32; ++y)
                for (uint32_t x = x0; x < x0 + ex && x < 32; ++x) g[(z * 32 + y) * 32 + x] = m;
    }
    bad += check("depth 5, boxes", g, 5);
    svo_chunk_desc none;
    bad += svo_chunk_from_grid(g.data(), 11, nullptr, 128.0f, &none) == SVO_ERR_INVALID_ARG ? 0 : 1;
    return bad ? 1 : 0;
}
