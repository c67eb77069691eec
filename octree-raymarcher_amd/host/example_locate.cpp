// example_locate.cpp — svo::World::locate (svo_world.hpp) once: which voxel lies under a handful of points of a generated world.
// Usage: example_locate [tree depth]; exit status 2 without a HIP device, 1 when a record contradicts the chunk it names.
#include <cstdio>
#include <cstdlib>

#include "svo_world.hpp"

int main(int argc, char **argv)
{
    const uint32_t depth = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 6;
    try {
        svo::World world;
        world.init(2, 1, 2, 128, depth);
        world.load_gpu(0);
        // a column of points through the terrain, one in the water, one outside the world
        std::vector<float> pts;
        for (int y = 0; y < 128; y += 4) { pts.push_back(70.25f); pts.push_back((float)y + 0.5f); pts.push_back(150.75f); }
        pts.push_back(10.0f); pts.push_back(3.0f); pts.push_back(10.0f);
        pts.push_back(-5.0f); pts.push_back(3.0f); pts.push_back(10.0f);
        const int64_t n = (int64_t)pts.size() / 3;
        float *pd = static_cast<float *>(svo_device_alloc(pts.size() * sizeof(float)));
        svo_voxel *vd = static_cast<svo_voxel *>(svo_device_alloc((size_t)n * sizeof(svo_voxel)));
        if (!pd || !vd) throw svo::Error(SVO_ERR_OUT_OF_MEMORY, "example_locate");
        svo::check(svo_memcpy_h2d(pd, pts.data(), pts.size() * sizeof(float)), "example_locate");
        world.locate(pd, n, vd);
        svo::check(svo_stream_synchronize(nullptr), "example_locate");
        std::vector<svo_voxel> v((size_t)n);
        svo::check(svo_memcpy_d2h(v.data(), vd, v.size() * sizeof(svo_voxel)), "example_locate");
        svo_device_free(pd); svo_device_free(vd);
        int solid = 0, inside = 0, bad = 0;
        for (int64_t k = 0; k < n; ++k) {
            const svo_voxel &r = v[(size_t)k];
            if (!(r.flags & SVO_LOCATE_INSIDE)) continue;
            ++inside;
            solid += (r.flags & SVO_LOCATE_SOLID) ? 1 : 0;
            // the record against the chunk it names: the node is no BRANCH, the box holds the point
            const svo_chunk_desc c = world.chunk((int)r.chunk);
            const float *p = &pts[(size_t)k * 3];
            if (r.node >= c.trees || (c.tree[r.node] >> 30) == SVO_BRANCH) ++bad;
            for (int a = 0; a < 3; ++a) if (!(p[a] >= r.bmin[a] && r.bmin[a] + r.size >= p[a])) ++bad;
        }
        std::printf("located %lld points: %d inside, %d solid, %d bad\n", (long long)n, inside, solid, bad);
        const bool ok = bad == 0 && inside == (int)n - 1 && solid > 0 && solid < inside && !(v.back().flags & SVO_LOCATE_INSIDE);
        return ok ? 0 : 1;
    } catch (const svo::Error &e) {
        std::fprintf(stderr, "example_locate: %s\n", e.what());
        return e.code == SVO_ERR_NO_DEVICE ? 2 : 1;
    }
}
