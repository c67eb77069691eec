// ASan/UBSan driver for the product's host-side generator (terrain.cpp): World::init incl. water, the sparse
// extension and the bilinear pyramid path, World::shift's entering plane at negative chunk coordinates, plus the chunk
// validator.  Built by tests/test_sanitizers.py with g++.
#include <cstdio>
#include <string>
#include "../csrc/terrain.h"
#include "../csrc/world.h"

int main()
{
    using namespace svo;
    size_t nodes = 0;
    for (int variant = 0; variant < 3; ++variant) {
        TerrainParams tp;
        tp.depth = variant == 2 ? 9 : 7;
        tp.pyramid_resolution = variant == 1 ? 32 : 0;           // bilinear path beyond the pyramid base
        tp.threads = 3;
        if (variant == 2) { tp.coarse_depth = 6; tp.water = 0; tp.refine_min[0] = 60; tp.refine_max[0] = 70; tp.refine_min[1] = tp.refine_min[2] = -1e9f; tp.refine_max[1] = tp.refine_max[2] = 1e9f; }
        const int ccm[3] = { -1, -1, 0 };
        const TerrainWindow grid = TerrainWindow::whole(2, 2, 2, 128, ccm);
        // the whole grid, and the plane that enters it when it slides by -1 along x (chunk x = -2)
        for (const TerrainWindow &win : { grid, grid.entering(0, -1) }) {
            std::vector<ChunkPools> chunks;
            if (generate_window(win, tp, chunks) != 0) { std::printf("generator failed\n"); return 1; }
            for (int k = 0; k < win.size(); ++k) {
                const ChunkPools &c = chunks[(size_t)k];
                const TerrainWindow::Chunk at = win.chunk(k);
                std::string why;
                if (validate_chunk(c, why) != 0) { std::printf("invalid chunk: %s\n", why.c_str()); return 1; }
                if (!chunk_is_exact(c, 128)) { std::printf("inexact chunk\n"); return 1; }
                if (at.index < 0 || at.index >= 8 || c.position[0] != (float)at.x * 128.0f) { std::printf("chunk %d misplaced\n", k); return 1; }
                nodes += c.tree.size();
            }
        }
    }
    std::printf("nodes %zu\n", nodes);
    return nodes > 1000 ? 0 : 1;
}
