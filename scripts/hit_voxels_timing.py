"""svo_hit_voxels, svo_hit_uv and svo_shade_textured on one 1920x1080 frame of the benchmark's C3 world: device events
around a batch of launches, median of the windows after warm-up, with svo_trace and svo_shade of the same frame beside them for scale;
and the parent index's build, timed as the first svo_hit_voxels call after a change to the pools minus a warm call.

    python scripts/hit_voxels_timing.py [--runs 10] [--out profiles/hit_voxels_timing.txt]
    python scripts/hit_voxels_timing.py --scale-only      # svo_trace and svo_shade alone (runs on a build without the new entry points)
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
F = np.float32


def timed(fn, runs, batch):
    """ms per call: device events around `batch` calls back to back, one window per run, after 3 warm-up calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / batch)
    return ms


def line(what, ms, note=""):
    return f"{what:34s} median {float(np.median(ms)):8.4f} ms  (min {min(ms):.4f}, max {max(ms):.4f})  {note}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--scale-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gw, gh, gd, iw, ih = 4, 1, 4, 1920, 1080
    n = iw * ih
    rect = (0, 0, iw, ih)
    W = svo.World.generate(gw, gh, gd, 128, a.depth, build_device=0)
    cam = bench.camera_path(svo, "c3_1080p_depth12_4x1x4_shadow", gw, gd, iw, ih)[0]
    prm = svo.trace_params(shadow=True)
    P = svo.shade_defaults()
    gbuffer, rgba = svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 16)
    lines = [f"hit voxels and texturing, one {iw}x{ih} frame (primary + shadow) of the world {gw}x{gh}x{gd} chunks of depth {a.depth} "
             f"({W.info.total_trees} node words), {torch.cuda.get_device_name(0)}; device events around {a.batch} launches back to back, "
             f"ms per launch, median of {a.runs} such windows after 3 warm-up launches"]
    lines.append(line("svo_trace (shadow)", timed(lambda: W.trace(cam, prm, rect, gbuffer.ptr), a.runs, 4)))
    lines.append(line("svo_shade", timed(lambda: svo.shade(cam, P, rect, gbuffer.ptr, rgba.ptr), a.runs, a.batch)))
    if not a.scale_only:
        voxels, uv = svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 8)
        rng = np.random.default_rng(3)
        image = svo.DeviceBuffer.from_numpy(rng.integers(0, 256, (2048, 2048, 3), np.uint8))
        atlas = svo.Atlas(image.ptr, None, 2048, 2048)
        builds = []
        for k in range(4):                                  # the first call on the fresh world, then after three small edits
            if k:
                W.edit_box(0, svo.EDIT_BUILD, (10.0 + k, 120.0, 10.0), (11.0 + k, 121.0, 11.0), 3)
            torch.cuda.synchronize()
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            W.hit_voxels(gbuffer.ptr, n, voxels.ptr)
            e1.record()
            W.hit_voxels(gbuffer.ptr, n, voxels.ptr)
            e2.record()
            e2.synchronize()
            builds.append(e0.elapsed_time(e1) - e1.elapsed_time(e2))
        W.trace(cam, prm, rect, gbuffer.ptr)                # (the edits changed chunk 0: the records of the world as it is now)
        W.hit_voxels(gbuffer.ptr, n, voxels.ptr)
        torch.cuda.synchronize()
        v = voxels.to_numpy(svo.VOXEL_DTYPE, n)
        boxed = (v["flags"] & 1) != 0
        cellular = boxed & (v["cell"] != svo.CELL_NONE)
        level = np.where(cellular, np.log2(128.0 / np.where(boxed, v["size"], 128.0)) - 2, np.log2(128.0 / np.where(boxed, v["size"], 128.0)))
        index_bytes = (W.info.tree_pool_bytes // 4 // 8 + 1) * 5
        lines.append(line("parent index build (first call - warm)", builds, f"{index_bytes / 1e6:.1f} MB of index; {a.depth - 2} sweeps"))
        lines.append(line("svo_hit_voxels, warm", timed(lambda: W.hit_voxels(gbuffer.ptr, n, voxels.ptr), a.runs, a.batch),
                          f"{boxed.mean():.3f} of the records get a box, {cellular.mean():.3f} in a brick, mean node level {level[boxed].mean():.2f}: "
                          f"dependent loads per boxed record = 3 + level = {3 + level[boxed].mean():.2f}"))
        lines.append(line("svo_hit_uv", timed(lambda: svo.hit_uv(cam, 0.0, rect, gbuffer.ptr, voxels.ptr, uv.ptr), a.runs, a.batch)))
        lines.append(line("svo_shade_textured (2048^2 atlas)", timed(lambda: svo.shade_textured(cam, P, atlas, rect, gbuffer.ptr, voxels.ptr, rgba.ptr), a.runs, a.batch)))
    W.destroy()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
