"""svo_shade_sky (both filters, 2048 x 2048 faces) and svo_frame_rgba8 on one 1920x1080 frame of the benchmark's C3 world:
device events around a batch of launches, median of the windows after warm-up, with svo_shade of the same frame from the same run
beside them - the yardstick: it moves the same class of HBM traffic (32 B read + 16 B written per pixel).

    python scripts/sky_timing.py [--runs 10] [--out profiles/sky_timing.txt]
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
    return f"{what:38s} median {float(np.median(ms)):8.4f} ms  (min {min(ms):.4f}, max {max(ms):.4f})  {note}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--face", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gw, gh, gd, iw, ih = 4, 1, 4, 1920, 1080
    n = iw * ih
    rect = (0, 0, iw, ih)
    W = svo.World.generate(gw, gh, gd, 128, a.depth, build_device=0)
    cam = bench.camera_path(svo, "c3_1080p_depth12_4x1x4_shadow", gw, gd, iw, ih)[0]
    P = svo.shade_defaults()
    gbuffer, packed, rgba, rgba8 = svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 8), svo.DeviceBuffer(n * 16), svo.DeviceBuffer(n * 4)
    W.trace(cam, svo.trace_params(shadow=True), rect, gbuffer.ptr)
    svo.gbuffer_pack(gbuffer.ptr, packed.ptr, n)
    torch.cuda.synchronize()
    miss = float(((gbuffer.to_numpy(svo.HIT_DTYPE, n)["flags"] & 1) == 0).mean())
    rng = np.random.default_rng(3)
    step = a.face * a.face * 3
    faces = svo.DeviceBuffer.from_numpy(rng.integers(0, 256, 6 * step, np.uint8))
    sky = {f: svo.Sky([faces.ptr + k * step for k in range(6)], a.face, f) for f in (svo.SKY_LINEAR, svo.SKY_NEAREST)}
    lines = [f"sky and RGBA8, one {iw}x{ih} frame of the world {gw}x{gh}x{gd} chunks of depth {a.depth} ({W.info.total_trees} node words), "
             f"{miss:.3f} of its pixels sky, {a.face}x{a.face} RGB8 faces of random bytes ({6 * step / 1e6:.1f} MB), {torch.cuda.get_device_name(0)}; "
             f"device events around {a.batch} launches back to back, ms per launch, median of {a.runs} such windows after 3 warm-up launches"]
    lines.append(line("svo_shade (the yardstick)", timed(lambda: svo.shade(cam, P, rect, gbuffer.ptr, rgba.ptr), a.runs, a.batch),
                      "32 B read + 16 B written per pixel"))
    lines.append(line("svo_shade_sky, SVO_SKY_LINEAR", timed(lambda: svo.shade_sky(cam, sky[svo.SKY_LINEAR], rect, rgba.ptr, gbuffer_ptr=gbuffer.ptr), a.runs, a.batch),
                      "32 B read per pixel; per sky pixel 4 texels gathered, 12 B written"))
    lines.append(line("svo_shade_sky, SVO_SKY_NEAREST", timed(lambda: svo.shade_sky(cam, sky[svo.SKY_NEAREST], rect, rgba.ptr, gbuffer_ptr=gbuffer.ptr), a.runs, a.batch),
                      "per sky pixel 1 texel"))
    lines.append(line("svo_shade_sky, linear, packed records", timed(lambda: svo.shade_sky(cam, sky[svo.SKY_LINEAR], rect, rgba.ptr, packed_ptr=packed.ptr), a.runs, a.batch),
                      "8 B read per pixel"))
    lines.append(line("svo_frame_rgba8", timed(lambda: svo.frame_rgba8(rgba.ptr, n, rgba8.ptr), a.runs, a.batch), "16 B read + 4 B written per pixel"))
    W.destroy()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
