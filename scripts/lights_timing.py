"""Light lists on the benchmark's C3 world: ms per frame of svo_trace(shadow=1) followed by svo_trace_lights with the
default cap (one slot per pixel), with max_rays = the previous frame's pair count (count_dev[0]) and with max_rays = nlights * pixels
(the padded list: the difference is what compaction buys), and by ceil(nlights / 2) calls of svo_trace_local_shadows (today's only way
to the same occlusion bits), over bench.py's 32-camera path at 1920x1080 - host clock around work that ends in a synchronise, warm-up
first, best of --reps passes, the variants alternated within each pass - plus pairs per pixel, the scratch each variant holds, and
svo_shade_lights beside svo_shade.  Lights: seeded x and z over the world, 6 units above the terrain found by a downward svo_trace_rays;
reach 32 and 64; 2, 8 and 32 lights.  Prints one JSON line per configuration.

    python scripts/lights_timing.py [--reps 3] [--out FILE] [--nlights 2,8,32] [--reach 32,64] [--frames-only N]

--frames-only N: no timing, N frames of svo_trace + svo_trace_lights (max_rays = the previous frame's count) + svo_shade + svo_shade_lights
of the first configuration, for a run under rocprofv3 --kernel-trace --stats (the kernel times of cull, emit and resolve).
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--nlights", default="2,8,32")
    ap.add_argument("--reach", default="32,64")
    ap.add_argument("--frames-only", type=int, default=0)
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench  # noqa: E402  (its camera path)
    svo = importlib.import_module("octree-raymarcher_amd")

    def sync():
        svo.lib.svo_stream_synchronize(None)

    gw, gh, gd, depth, iw, ih = 4, 1, 4, 12, 1920, 1080
    W = svo.World.generate(gw, gh, gd, 128, depth, build_device=0)
    cams = bench.camera_path(svo, "c3_1080p_depth12_4x1x4_shadow", gw, gd, iw, ih)
    n = iw * ih
    rect = (0, 0, iw, ih)
    g, rgba, vis, cnt = svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 16), svo.DeviceBuffer(n * 4), svo.DeviceBuffer(8)
    sp = svo.shade_defaults()
    prm = svo.trace_params(shadow=True)
    # 32 seeded places over the world; every configuration takes the first nlights of them
    rng = np.random.default_rng(2026)
    xz = rng.uniform(8.0, gw * 128.0 - 8.0, (32, 2)).astype(np.float32)
    o = np.stack([xz[:, 0], np.full(32, 500.0, np.float32), xz[:, 1]], axis=1)
    down = W.chunkmarch(o, np.tile(np.array([0.0, -1.0, 0.0], np.float32), (32, 1)))
    assert np.all(down["flags"] & svo.HIT_FLAG)
    places = [(float(o[j, 0]), float(500.0 - down["t"][j] + 6.0), float(o[j, 2])) for j in range(32)]
    lines = []
    for reach in [float(x) for x in a.reach.split(",")]:
        for nl in [int(x) for x in a.nlights.split(",")]:
            lights = [svo.Light(places[j], reach, (0.02, 0.02, 0.02), (0.9, 0.7, 0.4), (1.0, 0.9, 0.7), (1.0, 0.09, 0.032)) for j in range(nl)]
            pairs = []
            for c in cams:                                              # the pair count of every camera of the path
                W.trace(c, prm, rect, g.ptr)
                W.trace_lights(c, prm, rect, g.ptr, lights, vis.ptr, count_ptr=cnt.ptr)
                sync()
                pairs.append(int(cnt.to_numpy(np.uint32, 2)[0]))
            if a.frames_only:
                for k in range(a.frames_only):
                    c = cams[k % len(cams)]
                    W.trace(c, prm, rect, g.ptr)
                    W.trace_lights(c, prm, rect, g.ptr, lights, vis.ptr, max_rays=max(pairs[(k - 1) % len(cams)], 1), count_ptr=cnt.ptr)
                    svo.shade(c, sp, rect, g.ptr, rgba.ptr)
                    svo.shade_lights(c, sp, rect, g.ptr, lights, rgba.ptr, visible_ptr=vis.ptr)
                sync()
                print(json.dumps({"frames_only": a.frames_only, "nlights": nl, "reach": reach}))
                return

            def pass_ms(what):
                sync()
                t0 = time.perf_counter()
                for k, c in enumerate(cams):
                    W.trace(c, prm, rect, g.ptr)
                    if what == "default_cap":
                        W.trace_lights(c, prm, rect, g.ptr, lights, vis.ptr)
                    elif what == "previous_count":
                        W.trace_lights(c, prm, rect, g.ptr, lights, vis.ptr, max_rays=max(pairs[k - 1], 1), count_ptr=cnt.ptr)
                    elif what == "padded":
                        W.trace_lights(c, prm, rect, g.ptr, lights, vis.ptr, max_rays=nl * n)
                    elif what == "local_shadows":
                        for j in range(0, nl, 2):
                            W.trace_local_shadows(c, prm, rect, g.ptr, point=places[j], spot=places[j + 1] if j + 1 < nl else None)
                sync()
                return (time.perf_counter() - t0) * 1e3 / len(cams)

            def shade_ms(with_lights):
                sync()
                t0 = time.perf_counter()
                for c in cams:
                    svo.shade(c, sp, rect, g.ptr, rgba.ptr)
                    if with_lights:
                        svo.shade_lights(c, sp, rect, g.ptr, lights, rgba.ptr, visible_ptr=vis.ptr)
                sync()
                return (time.perf_counter() - t0) * 1e3 / len(cams)

            variants = ["trace_alone", "default_cap", "previous_count", "padded", "local_shadows"]
            for v in variants:                                          # warm-up (scratch allocated, occupancy queried)
                pass_ms(v)
            shade_ms(False), shade_ms(True)
            times = {v: [] for v in variants + ["shade", "shade_and_lights"]}
            for _ in range(a.reps):
                for v in variants:
                    times[v].append(pass_ms(v))
                times["shade"].append(shade_ms(False))
                times["shade_and_lights"].append(shade_ms(True))
            nblocks = (n + 255) // 256
            scratch = lambda cap: 56 * cap + 8 * nl * nblocks + 8
            res = {"world": [gw, gh, gd, depth], "image": [iw, ih], "cameras": len(cams), "reps": a.reps, "nlights": nl, "reach": reach,
                   "pairs_per_pixel_mean": round(float(np.mean(pairs)) / n, 4), "pairs_per_pixel_min_max": [round(min(pairs) / n, 4), round(max(pairs) / n, 4)],
                   "frames_over_the_default_cap": int(sum(p > n for p in pairs)),
                   "frames_over_the_previous_count": int(sum(pairs[k] > max(pairs[k - 1], 1) for k in range(len(pairs)))),
                   "scratch_bytes": {"default_cap": scratch(n), "previous_count_max": scratch(max(max(pairs), 1)), "padded": scratch(nl * n),
                                     "local_shadows": 2 * n * 56 if nl > 1 else n * 56}}
            for k, v in times.items():
                res[k + "_ms"] = round(min(v), 4)
                res[k + "_ms_passes"] = [round(x, 4) for x in v]
            line = json.dumps(res)
            print(line, flush=True)
            lines.append(line)
    for b in (g, rgba, vis, cnt):
        b.free()
    W.destroy()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
