"""svo_world_locate on the benchmark's C3 world: points per second of both kernels, by device events around a batch
of launches, median of the windows after warm-up, for (a) 2^21 uniform points of the world box and (b) the hit points of one 1920x1080 frame; next to each
figure the bytes per point a perfect cache would need (12 B in, 32 B out, one 128-byte line per dependent load of the walk).

    python scripts/locate_timing.py [--runs 20] [--out profiles/locate_timing.txt]
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (its camera path)

svo = importlib.import_module("octree-raymarcher_amd")
# the compiler's resource usage of the two kernels (make -C octree-raymarcher_amd asm): VGPRs, spills, waves per SIMD
RESOURCES = {"literal": "26 VGPRs, 0 spills, 0 B LDS, 8 waves/SIMD", "stack": "37 VGPRs, 0 spills, 0 B LDS, 8 waves/SIMD"}
F = np.float32


def frame_hit_points(W, cam):
    n = cam.width * cam.height
    out = svo.DeviceBuffer(n * 32)
    W.trace(cam, svo.trace_params(), (0, 0, cam.width, cam.height), out.ptr)
    svo.lib.svo_stream_synchronize(None)
    g = out.to_numpy(svo.HIT_DTYPE, n)
    out.free()
    px, py = np.meshgrid(np.arange(cam.width, dtype=F), np.arange(cam.height, dtype=F))
    u = (((px + F(0.5)) / F(cam.width)) * F(2) - F(1)) * F(cam.tan_half_x)
    v = (F(1) - ((py + F(0.5)) / F(cam.height)) * F(2)) * F(cam.tan_half_y)
    d = (np.array(cam.forward, F) + np.array(cam.right, F) * u[..., None]) + np.array(cam.up, F) * v[..., None]
    d = (d / np.sqrt((d * d).sum(axis=2, dtype=F))[..., None]).reshape(-1, 3)
    hit = (g["flags"] & 1) != 0
    return (np.array(cam.eye, F)[None] + d[hit] * g["t"][hit][:, None]).astype(F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gw, gh, gd, iw, ih = 4, 1, 4, 1920, 1080
    W = svo.World.generate(gw, gh, gd, 128, a.depth, build_device=0)
    cam = bench.camera_path(svo, "c3_1080p_depth12_4x1x4_shadow", gw, gd, iw, ih)[0]
    rng = np.random.default_rng(2026)
    sets = {"uniform 2^21": (rng.random((1 << 21, 3)) * np.array([gw, gh, gd]) * 128.0).astype(F), "frame hit points": frame_hit_points(W, cam)}
    lines = [f"svo_world_locate, world {gw}x{gh}x{gd} chunks of depth {a.depth} ({W.info.total_trees} node words, {W.info.wide_nodes} wide nodes), "
             f"{torch.cuda.get_device_name(0)}; device events around {a.batch} launches back to back, ms per launch, median of {a.runs} such windows (the two kernels alternating) after 5 warm-up launches each"]
    for name, pts in sets.items():
        n = pts.shape[0]
        pd, out = svo.DeviceBuffer.from_numpy(pts), svo.DeviceBuffer(n * 32)
        recs, times = {}, {"literal": [], "stack": []}
        kernels = (("literal", svo.KERNEL_LITERAL), ("stack", svo.KERNEL_STACK))
        for kname, kernel in kernels:                       # warm-up of both; the records of each
            prm = svo.trace_params(kernel=kernel)
            for _ in range(5):
                W.locate(pd.ptr, n, prm, out.ptr)
            torch.cuda.synchronize()
            recs[kname] = out.to_numpy(svo.VOXEL_DTYPE, n)
        for _ in range(a.runs):                             # the two kernels alternate; a timed window is a.batch launches
            for kname, kernel in kernels:
                prm = svo.trace_params(kernel=kernel)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.batch):
                    W.locate(pd.ptr, n, prm, out.ptr)
                e1.record()
                e1.synchronize()
                times[kname].append(e0.elapsed_time(e1) / a.batch)
        for kname, kernel in kernels:
            ms = times[kname]
            r = recs[kname]
            inside = (r["flags"] & 1) != 0
            cellular = inside & (r["cell"] != svo.CELL_NONE)
            level = np.where(cellular, a.depth - 2, np.log2(128.0 / np.where(inside, r["size"], 128.0))).astype(np.float64)
            # dependent loads, one line each: the chunk table entry, then node words 0..level (literal) or one wide entry per two
            # levels and the wbase word (stack), then the brick cell
            if kname == "literal":
                loads = 1.0 + (level + 1.0) + cellular
            else:
                pad = (a.depth - 2) % 2
                loads = 1.0 + np.maximum(1.0, np.ceil((level + pad) / 2.0)) + (level > 0) + cellular
            loads = np.where(inside, loads, 0.0)
            med = float(np.median(ms))
            lines.append(f"{name:18s} {kname:8s} n = {n:8d}  median {med:8.4f} ms  (min {min(ms):.4f}, max {max(ms):.4f})  {n / med / 1e6:8.2f} G points/s  "
                         f"{RESOURCES[kname]}  perfect-cache bytes/point = 12 + 32 + 128 x {loads.mean():.2f} loads = {44 + 128 * loads.mean():.0f} "
                         f"(inside {inside.mean():.3f}, in a brick {cellular.mean():.3f}, mean node level {level[inside].mean():.2f})")
        same = np.array_equal(recs["literal"].view(np.uint8), recs["stack"].view(np.uint8))
        lines.append(f"{name:18s} literal and stack records byte-identical: {same}")
        pd.free()
        out.free()
    W.destroy()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
