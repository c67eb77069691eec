// example_shadowmap.cpp — a fixed sun (svo_world.hpp): the directional light rendered once into a shadow map, then a frame traced
// without shadow rays and shadowed by one lookup per hit; beside it the same frame with the shadow ray, for comparison.
// Usage: example_shadowmap [tree depth] [map size]; exit status 2 without a HIP device, 1 when the records are not what the header promises.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "svo_world.hpp"

int main(int argc, char **argv)
{
    const uint32_t depth = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 6;
    const int size = argc > 2 ? std::atoi(argv[2]) : 256;
    try {
        svo::World world;
        world.init(2, 1, 2, 128, depth);
        world.load_gpu(0);
        const float sun[3] = { 1.0f, -1.0f, 0.0f };             // directionalLight.direction, src/Main.cpp:116
        svo::ShadowMap map;
        world.shadowmap_fit(sun, size, size, map);
        world.shadowmap_render(map);                            // once; again after an edit
        const svo::Camera cam({ 128.0f, 150.0f, -40.0f }, { 0.0f, -0.5f, 0.866f }, { 0.0f, 1.0f, 0.0f }, 60.0f, 160, 120);
        svo::GBuffer plain, mapped, rayed;
        world.draw(cam, plain, false);
        world.draw(cam, mapped, false);                         // per frame: no shadow rays ...
        world.shadowmap_apply(cam, mapped, map, 2.0f * map.texel());     // ... one lookup per hit
        world.draw(cam, rayed, true, sun);
        svo::check(svo_stream_synchronize(nullptr), "example_shadowmap");
        const std::vector<svo_hit> p = plain.download(), m = mapped.download(), r = rayed.download();
        const std::vector<float> z = map.download();
        size_t covered = 0;
        for (float t : z) covered += std::isfinite(t) ? 1 : 0;
        int hits = 0, shadowed = 0, agree = 0, bad = 0;
        for (size_t k = 0; k < m.size(); ++k) {
            const bool hit = (p[k].flags & SVO_HIT_FLAG) && !(p[k].flags & SVO_ERR_FLAG);
            // only SVO_SHADOW_TRACED and SVO_SHADOWED of a hit's record may differ from the plain frame's, and the first is set
            const uint16_t mask = hit ? (uint16_t)~(SVO_SHADOW_TRACED | SVO_SHADOWED) : (uint16_t)0xFFFF;
            if ((p[k].flags & mask) != (m[k].flags & mask) || p[k].t != m[k].t || p[k].node != m[k].node || p[k].material != m[k].material) ++bad;
            if (!hit) continue;
            ++hits;
            if (!(m[k].flags & SVO_SHADOW_TRACED)) ++bad;
            shadowed += (m[k].flags & SVO_SHADOWED) ? 1 : 0;
            agree += ((m[k].flags ^ r[k].flags) & SVO_SHADOWED) ? 0 : 1;
        }
        std::printf("map %dx%d, %.2f units a texel, %zu texels hit; %d hits, %d shadowed by the map, %d as the shadow ray has them, %d bad\n",
                    map.width, map.height, map.texel(), covered, hits, shadowed, agree, bad);
        const bool ok = bad == 0 && hits > 1000 && shadowed > 0 && shadowed < hits && covered > 0 && covered < z.size();
        return ok ? 0 : 1;
    } catch (const svo::Error &e) {
        std::fprintf(stderr, "example_shadowmap: %s\n", e.what());
        return e.code == SVO_ERR_NO_DEVICE ? 2 : 1;
    }
}
