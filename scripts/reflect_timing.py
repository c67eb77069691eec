"""svo_trace_reflections on the benchmark's C3 world: one 1920x1080 frame, by device events around a batch of launches,
median and min-max of the windows after warm-up, for svo_trace (the primary + shadow frame the reflections hang on), svo_hit_voxels,
svo_trace_reflections of the water (material 6) and of every material (0), and svo_shade_reflections.  All variants alternate inside
every round.  For the record, not a gate.

    python scripts/reflect_timing.py [--runs 20] [--out profiles/reflect_timing.txt]
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
WATER = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gw, gh, gd, iw, ih = 4, 1, 4, 1920, 1080
    n = iw * ih
    rect = (0, 0, iw, ih)
    W = svo.World.generate(gw, gh, gd, 128, a.depth, build_device=0)
    cam = bench.camera_path(svo, "c3_1080p_depth12_4x1x4_shadow", gw, gd, iw, ih)[0]
    prm = svo.trace_params(shadow=True)
    gb, vox, refl, rgba = svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 16)
    P = svo.shade_defaults()
    W.trace(cam, prm, rect, gb.ptr)
    W.hit_voxels(gb.ptr, n, vox.ptr)
    svo.shade(cam, P, rect, gb.ptr, rgba.ptr)
    torch.cuda.synchronize()
    g, v = gb.to_numpy(svo.HIT_DTYPE, n), vox.to_numpy(svo.VOXEL_DTYPE, n)
    usable = ((g["flags"] & svo.HIT_FLAG) != 0) & ((g["flags"] & svo.ERR_FLAG) == 0) & ((v["flags"] & svo.LOCATE_INSIDE) != 0)
    mirrors = {WATER: int((usable & (g["material"] == WATER)).sum()), 0: int(usable.sum())}
    mirror = svo.Mirror(WATER, 0.02, True, (0.5, 0.6, 0.7))

    variants = {
        "svo_trace, primary + shadow": lambda: W.trace(cam, prm, rect, gb.ptr),
        "svo_hit_voxels": lambda: W.hit_voxels(gb.ptr, n, vox.ptr),
        "svo_trace_reflections, material 6": lambda: W.trace_reflections(cam, prm, rect, gb.ptr, vox.ptr, refl.ptr, material=WATER),
        "svo_trace_reflections, material 0": lambda: W.trace_reflections(cam, prm, rect, gb.ptr, vox.ptr, refl.ptr, material=0),
    }
    times, rays, hits = {k: [] for k in variants}, {}, {}
    for name, call in variants.items():                         # warm-up; what each variant marches
        for _ in range(5):
            call()
        rays[name] = W.last_ray_count()
        if "reflections" in name:
            r = refl.to_numpy(svo.HIT_DTYPE, n)
            hits[name] = int(((r["flags"] & svo.HIT_FLAG) != 0).sum())
    for _ in range(a.runs):
        for name, call in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.batch):
                call()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.batch)
    lines = [f"svo_trace_reflections, world {gw}x{gh}x{gd} chunks of depth {a.depth} ({W.info.total_trees} node words, {W.info.wide_nodes} wide nodes), one {iw}x{ih} frame "
             f"({mirrors[0]} hits with a box of {n} pixels, {mirrors[WATER]} of them water), {torch.cuda.get_device_name(0)}; SVO_KERNEL_AUTO, shadow = 1; device events around "
             f"{a.batch} calls back to back, ms per call, median of {a.runs} such windows (all variants alternating inside every round) after 5 warm-up calls each"]
    for name in variants:
        ms = times[name]
        extra = f"  {hits[name]} reflected hits" if name in hits else ""
        if name == "svo_hit_voxels":
            lines.append(f"{name:36s} median {float(np.median(ms)):8.4f} ms  (min {min(ms):.4f}, max {max(ms):.4f})")
        else:
            lines.append(f"{name:36s} median {float(np.median(ms)):8.4f} ms  (min {min(ms):.4f}, max {max(ms):.4f})  {rays[name]} rays marched{extra}")
    base = float(np.median(times["svo_trace, primary + shadow"]))
    for m in (WATER, 0):
        lines.append(f"svo_trace_reflections, material {m}, against svo_trace: {float(np.median(times[f'svo_trace_reflections, material {m}'])) / base:.3f} of its time")
    # svo_shade_reflections over the records of the water's rays (the last warm-up state of refl is material 0's: trace the water's again)
    W.trace_reflections(cam, prm, rect, gb.ptr, vox.ptr, refl.ptr, material=WATER)
    ms = []
    for r in range(a.runs + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.batch):
            svo.shade_reflections(cam, P, mirror, rect, gb.ptr, vox.ptr, refl.ptr, rgba.ptr)
        e1.record()
        e1.synchronize()
        if r:
            ms.append(e0.elapsed_time(e1) / a.batch)
    lines.append(f"{'svo_shade_reflections, material 6':36s} median {float(np.median(ms)):8.4f} ms  (min {min(ms):.4f}, max {max(ms):.4f})  f0 0.02 with the Fresnel term, no sky")
    for b in (gb, vox, refl, rgba):
        b.free()
    W.destroy()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
