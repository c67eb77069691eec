// mesh_check.cpp — csrc/mesh.cpp (svo_grid_add_mesh, svo_grid_fill_enclosed) on its own, for the host sanitizers: compiled together
// with it by tests/test_mesh_host_sanitize.py (g++ -fsanitize=address,undefined), no HIP and no libsvo_amd.so.  Voxelises a few meshes
// into heap grids of exactly N^3 cells - boxes on and off the lattice, one that hangs out of the grid on all six sides, triangles
// with indices out of range and vertices that are not finite - fills them, and checks the counts that are known in closed form.
// Exit status 1 when a count is off.
#include <cmath>
#include <cstdio>
#include <limits>
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
    svo_mesh desc(uint16_t material) const
    {
        svo_mesh m = {};
        m.vertices = v.data(); m.indices = ix.data(); m.materials = nullptr;
        m.nvertices = (uint32_t)(v.size() / 3); m.ntriangles = (uint32_t)(ix.size() / 3);
        m.cell = 1.0f; m.material = material;
        return m;
    }
};

static uint64_t count(const std::vector<uint16_t> &g, uint16_t value)
{
    uint64_t n = 0;
    for (uint16_t c : g) n += c == value ? 1 : 0;
    return n;
}

static int report(const char *name, bool ok) { std::printf("%s: %s\n", name, ok ? "ok" : "WRONG"); return ok ? 0 : 1; }

int main()
{
    int bad = 0;
    {   // the lattice cube: 6^3 - 2^3 shell cells, then its 2^3 interior
        Mesh m; m.box(4.0f, 8.0f);
        std::vector<uint16_t> g(16 * 16 * 16, 0);
        const svo_mesh d = m.desc(5);
        uint64_t filled = 99;
        const bool ok = svo_grid_add_mesh(&d, 4, g.data()) == SVO_OK && count(g, 5) == 208 && svo_grid_fill_enclosed(g.data(), 4, 7, &filled) == SVO_OK &&
                        filled == 8 && count(g, 7) == 8 && count(g, 0) == 4096 - 216;
        bad += report("depth 4, lattice cube and its fill", ok);
    }
    {   // off the lattice: cells 4 .. 7, whose shell is 4^3 - 2^3
        Mesh m; m.box(4.25f, 7.75f);
        std::vector<uint16_t> g(16 * 16 * 16, 0);
        const svo_mesh d = m.desc(0xFFFF);
        bad += report("depth 4, box off the lattice", svo_grid_add_mesh(&d, 4, g.data()) == SVO_OK && count(g, 0xFFFF) == 56);
    }
    {   // a box around the whole grid and beyond it on all six sides: its faces miss the grid, every clamp is exercised, nothing is marked;
        // one that cuts through the grid's cells marks the six faces' cells and encloses nothing the fill may touch
        Mesh m; m.box(-3.5f, 11.5f);
        std::vector<uint16_t> g(8 * 8 * 8, 0);
        svo_mesh d = m.desc(3);
        bool ok = svo_grid_add_mesh(&d, 3, g.data()) == SVO_OK && count(g, 0) == 512;
        Mesh c; c.box(0.5f, 7.5f);
        d = c.desc(3);
        uint64_t filled = 0;
        ok = ok && svo_grid_add_mesh(&d, 3, g.data()) == SVO_OK && count(g, 3) == 512 - 216 && svo_grid_fill_enclosed(g.data(), 3, 1, &filled) == SVO_OK && filled == 216;
        bad += report("depth 3, boxes around the grid", ok);
    }
    {   // triangles that are dropped: indices out of range (never read), vertices that are not finite, no area; and huge but finite ones
        Mesh m;
        const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity(), big = 3.0e38f;
        m.v = { 1, 1, 1, 2, 3, 1, 3, 1, 2, nan, 1, 1, 1, inf, 1, -big, -big, -big, big, big, big, big, -big, big };
        m.ix = { 0, 1, 8, 0xFFFFFFFFu, 1, 2, 0, 1, 3, 0, 4, 2, 0, 0, 1, 5, 6, 7 };
        std::vector<uint16_t> g(4 * 4 * 4, 0);
        const svo_mesh d = m.desc(9);
        bad += report("depth 2, dropped triangles", svo_grid_add_mesh(&d, 2, g.data()) == SVO_OK && count(g, 0) == 64);
        m.ix = { 0, 1, 2 };
        const svo_mesh live = m.desc(9);
        bad += report("depth 2, one triangle", svo_grid_add_mesh(&live, 2, g.data()) == SVO_OK && count(g, 9) > 0 && count(g, 9) + count(g, 0) == 64);
    }
    {   // per-triangle materials: the maximum wins, material 0 writes nothing; a depth-5 grid with a full and an empty fill
        Mesh m; m.box(10.3f, 20.6f); m.box(10.3f, 20.6f); m.box(10.3f, 20.6f);
        std::vector<uint16_t> mats(36);
        for (size_t t = 0; t < 36; ++t) mats[t] = t < 12 ? 2 : t < 24 ? 40000 : 0;
        std::vector<uint16_t> g(32 * 32 * 32, 0);
        svo_mesh d = m.desc(1);
        d.materials = mats.data();
        uint64_t filled = 0;
        bool ok = svo_grid_add_mesh(&d, 5, g.data()) == SVO_OK && count(g, 40000) == 11 * 11 * 11 - 9 * 9 * 9 && count(g, 2) == 0;
        ok = ok && svo_grid_fill_enclosed(g.data(), 5, 6, &filled) == SVO_OK && filled == 729 && svo_grid_fill_enclosed(g.data(), 5, 6, nullptr) == SVO_OK;
        bad += report("depth 5, materials and fill", ok);
    }
    {   // the refusals
        Mesh m; m.box(1.0f, 2.0f);
        std::vector<uint16_t> g(64, 0);
        svo_mesh d = m.desc(1);
        bool ok = svo_grid_add_mesh(nullptr, 2, g.data()) == SVO_ERR_INVALID_ARG && svo_grid_add_mesh(&d, 2, nullptr) == SVO_ERR_INVALID_ARG &&
                  svo_grid_add_mesh(&d, 11, g.data()) == SVO_ERR_INVALID_ARG && svo_grid_fill_enclosed(g.data(), 2, 0, nullptr) == SVO_ERR_INVALID_ARG;
        d.cell = 0.0f;
        ok = ok && svo_grid_add_mesh(&d, 2, g.data()) == SVO_ERR_INVALID_ARG;
        d.cell = 1.0f; d.vertices = nullptr;
        ok = ok && svo_grid_add_mesh(&d, 2, g.data()) == SVO_ERR_INVALID_ARG && count(g, 0) == 64;
        bad += report("refusals", ok);
    }
    return bad ? 1 : 0;
}
