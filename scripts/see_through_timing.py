"""See-through materials on the benchmark's C3 world: the cost of building the see-through view, and ms per frame of
svo_trace against svo_trace_translucent (material 6, the generator's water) over bench.py's 32-camera path at 1920x1080, with and
without shadow rays, plus the fraction of pixels that are continued.  Prints one JSON line.

    python scripts/see_through_timing.py [--reps 3] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (its camera path)

svo = importlib.import_module("octree-raymarcher_amd")
WATER = 6


def sync():
    svo.lib.svo_stream_synchronize(None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gw, gh, gd, depth, iw, ih = 4, 1, 4, 12, 1920, 1080
    W = svo.World.generate(gw, gh, gd, 128, depth, build_device=0)
    info = W.info
    cams = bench.camera_path(svo, "c3_1080p_depth12_4x1x4_shadow", gw, gd, iw, ih)
    n = iw * ih
    surf, behind = svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 32)
    rect = (0, 0, iw, ih)

    # view build: a tiny see-through launch with the view cached, and one that has to rebuild it (the material alternates)
    def tiny(m):
        sync()
        t0 = time.perf_counter()
        W.trace(cams[0], svo.trace_params(kernel=svo.KERNEL_STACK, see_through=m), (0, 0, 8, 8), surf.ptr)
        sync()
        return time.perf_counter() - t0
    tiny(WATER)
    cached = [tiny(WATER) for _ in range(5)]
    rebuilt = [tiny(4 if k % 2 == 0 else WATER) for k in range(6)]
    build_ms = (np.median(rebuilt) - np.median(cached)) * 1e3
    view_bytes = info.wide_pool_bytes * 64 // 73 + info.mask_pool_bytes * 8 // 10     # wide entries + masks (pool capacities: an upper bound)

    def frames(translucent, shadow):
        prm = svo.trace_params(shadow=shadow, see_through=WATER if translucent else 0)
        best = None
        for _ in range(a.reps):
            sync()
            t0 = time.perf_counter()
            for c in cams:
                if translucent:
                    W.trace_translucent(c, prm, rect, surf.ptr, behind.ptr)
                else:
                    W.trace(c, prm, rect, surf.ptr)
            sync()
            dt = (time.perf_counter() - t0) * 1e3 / len(cams)
            best = dt if best is None else min(best, dt)
        return best

    res = {"world": [gw, gh, gd, depth], "image": [iw, ih], "cameras": len(cams), "view_build_ms": round(build_ms, 3),
           "view_bytes_upper_bound": int(view_bytes), "wide_pool_bytes": int(info.wide_pool_bytes), "mask_pool_bytes": int(info.mask_pool_bytes)}
    for shadow in (False, True):
        key = "shadow" if shadow else "primary"
        frames(True, shadow)                                            # warm-up (view built, scratch allocated)
        res[f"trace_ms_{key}"] = round(frames(False, shadow), 3)
        res[f"translucent_ms_{key}"] = round(frames(True, shadow), 3)
    fr = []
    for c in cams:
        W.trace_translucent(c, svo.trace_params(see_through=WATER), rect, surf.ptr, behind.ptr)
        sync()
        fl = surf.to_numpy(svo.HIT_DTYPE, n)["flags"]
        fr.append(float(np.count_nonzero(fl & svo.SEE_THROUGH)) / n)
    res["continued_fraction_mean"] = round(float(np.mean(fr)), 4)
    res["continued_fraction_min_max"] = [round(min(fr), 4), round(max(fr), 4)]
    surf.free()
    behind.free()
    W.destroy()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
