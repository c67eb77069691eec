// example_grid.cpp — your own voxels (svo_world.hpp): an empty 1x1x1 world, a dense grid installed as its chunk on the device
// (svo::World::chunk_from_grid), read back (chunk_to_grid) and compared; the host builder (svo_chunk_from_grid) must give the same pools.
// Usage: example_grid [grid depth]; exit status 2 without a HIP device, 1 when anything differs.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "svo_world.hpp"

int main(int argc, char **argv)
{
    const uint32_t depth = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 5;
    try {
        if (depth < SVO_GRID_MIN_DEPTH || depth > 8) throw svo::Error(SVO_ERR_INVALID_ARG, "example_grid: depth in [2, 8]");
        const uint32_t N = 1u << depth;
        // a ball of material 5 with a core of material 300, in a grid that is empty elsewhere
        std::vector<uint16_t> grid((size_t)N * N * N, 0);
        const float c = 0.5f * (float)N, r = 0.4f * (float)N;
        for (uint32_t z = 0; z < N; ++z)
            for (uint32_t y = 0; y < N; ++y)
                for (uint32_t x = 0; x < N; ++x) {
                    const float dx = (float)x + 0.5f - c, dy = (float)y + 0.5f - c, dz = (float)z + 0.5f - c;
                    const float q = dx * dx + dy * dy + dz * dz;
                    grid[((size_t)z * N + y) * N + x] = q < 0.25f * r * r ? 300 : q < r * r ? 5 : 0;
                }
        // the world: one EMPTY chunk of one word (any depth >= 2), uploaded
        const uint32_t empty_root = 0;
        svo_chunk_desc e;
        std::memset(&e, 0, sizeof e);
        e.size = 128.0f; e.depth = 2; e.tree = &empty_root; e.trees = 1;
        svo::World world;
        world.init(std::vector<svo_chunk_desc>(1, e), 1, 1, 1, 128);
        world.load_gpu(0);
        const size_t bytes = grid.size() * sizeof(uint16_t);
        uint16_t *gd = static_cast<uint16_t *>(svo_device_alloc(bytes)), *back = static_cast<uint16_t *>(svo_device_alloc(bytes));
        if (!gd || !back) throw svo::Error(SVO_ERR_OUT_OF_MEMORY, "example_grid");
        svo::check(svo_memcpy_h2d(gd, grid.data(), bytes), "example_grid");
        world.chunk_from_grid(0, gd, depth);
        world.chunk_to_grid(0, depth, back);
        svo::check(svo_stream_synchronize(nullptr), "example_grid");
        std::vector<uint16_t> got(grid.size());
        svo::check(svo_memcpy_d2h(got.data(), back, bytes), "example_grid");
        svo_device_free(gd); svo_device_free(back);
        size_t bad = 0;
        for (size_t i = 0; i < grid.size(); ++i) bad += got[i] != grid[i] ? 1 : 0;
        // the host twin: the same pools, index for index
        const float origin[3] = { 0.0f, 0.0f, 0.0f };
        svo_chunk_desc host;
        svo::check(svo_chunk_from_grid(grid.data(), depth, origin, 128.0f, &host), "svo_chunk_from_grid");
        const svo_chunk_desc dev = world.chunk(0);
        const bool same = dev.depth == host.depth && dev.trees == host.trees && dev.twigs == host.twigs &&
            std::memcmp(dev.tree, host.tree, host.trees * sizeof(uint32_t)) == 0 &&
            (host.twigs == 0 || std::memcmp(dev.twig, host.twig, host.twigs * SVO_TWIG_WORDS * sizeof(uint16_t)) == 0);
        std::printf("grid of depth %u: %llu node words, %llu bricks, %zu cells differ after the round trip, host pools %s\n", depth,
                    (unsigned long long)dev.trees, (unsigned long long)dev.twigs, bad, same ? "equal" : "DIFFER");
        svo_chunk_free(&host);
        return bad == 0 && same && dev.twigs > 0 ? 0 : 1;
    } catch (const svo::Error &e) {
        std::fprintf(stderr, "example_grid: %s\n", e.what());
        return e.code == SVO_ERR_NO_DEVICE ? 2 : 1;
    }
}
