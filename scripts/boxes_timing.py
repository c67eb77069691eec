"""svo_shade_boxes with 0, 4 and 64 boxes (the reference's four - the cursor and three light markers - and SVO_MAX_BOXES) and
svo_cursor_place on one 1920x1080 frame of the benchmark's C3 world: device events around a batch of launches, median of
the windows after warm-up, with svo_shade of the same frame from the same run beside them - the yardstick: same image, same pixel count.

    python scripts/boxes_timing.py [--runs 10] [--out profiles/boxes_timing.txt]
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


def line(what, ms, yardstick=None, note=""):
    ratio = "" if yardstick is None else f"  {float(np.median(ms)) / yardstick:5.2f} x svo_shade"
    return f"{what:38s} median {float(np.median(ms)):8.4f} ms  (min {min(ms):.4f}, max {max(ms):.4f}){ratio}  {note}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gw, gh, gd, iw, ih = 4, 1, 4, 1920, 1080
    n = iw * ih
    rect = (0, 0, iw, ih)
    W = svo.World.generate(gw, gh, gd, 128, a.depth, build_device=0)
    cam = bench.camera_path(svo, "c3_1080p_depth12_4x1x4_shadow", gw, gd, iw, ih)[0]
    P = svo.shade_defaults()
    gbuffer, rgba = svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 16)
    W.trace(cam, svo.trace_params(shadow=True), rect, gbuffer.ptr)
    svo.shade(cam, P, rect, gbuffer.ptr, rgba.ptr)
    torch.cuda.synchronize()
    g = gbuffer.to_numpy(svo.HIT_DTYPE, n)
    hit = (g["flags"] & 1) != 0
    # the boxes sit on the surface the frame shows: cubes of edge 16 (the reference's cursor) centred on the hits of random pixels, the
    # first one the cursor, every other one solid and opaque
    rng = np.random.default_rng(3)
    eye = np.array(cam.eye, np.float64)
    fwd, right, up = (np.array(v, np.float64) for v in (cam.forward, cam.right, cam.up))
    boxes = np.zeros(svo.MAX_BOXES, svo.BOX_DTYPE)
    picks = rng.choice(np.nonzero(hit)[0], svo.MAX_BOXES, replace=False)
    for i, k in enumerate(picks):
        px, py = k % iw, k // iw
        d = fwd + right * (((px + 0.5) / iw * 2 - 1) * cam.tan_half_x) + up * ((1 - (py + 0.5) / ih * 2) * cam.tan_half_y)
        d /= np.linalg.norm(d)
        boxes[i]["bmin"] = eye + d * float(g["t"][k]) - 8.0
        boxes[i]["size"] = 16.0
        boxes[i]["color"] = (0.8, 0.8, 0.8) if i == 0 else rng.random(3)
        boxes[i]["alpha"] = 0.2 if i == 0 else 1.0
        boxes[i]["style"] = svo.BOX_CURSOR if i == 0 else svo.BOX_SOLID
    boxes_dev = svo.DeviceBuffer.from_numpy(boxes)
    centre = (ih // 2) * iw + iw // 2
    lines = [f"edit cursor and marker cubes, one {iw}x{ih} frame of the world {gw}x{gh}x{gd} chunks of depth {a.depth} ({W.info.total_trees} node words), "
             f"{float(hit.mean()):.3f} of its pixels hits, cubes of edge 16 centred on the hits of random pixels, {torch.cuda.get_device_name(0)}; "
             f"device events around {a.batch} launches back to back, ms per launch, median of {a.runs} such windows after 3 warm-up launches"]
    shade_ms = timed(lambda: svo.shade(cam, P, rect, gbuffer.ptr, rgba.ptr), a.runs, a.batch)
    y = float(np.median(shade_ms))
    lines.append(line("svo_shade (the yardstick)", shade_ms, None, "32 B read + 16 B written per pixel"))
    lines.append(line("svo_shade_boxes, 0 boxes", timed(lambda: svo.shade_boxes(cam, boxes_dev.ptr, 0, rect, rgba.ptr), a.runs, a.batch), y, "no launch"))
    for count in (4, svo.MAX_BOXES):
        svo.shade(cam, P, rect, gbuffer.ptr, rgba.ptr)
        before = rgba.to_numpy(np.float32, n * 4)
        svo.shade_boxes(cam, boxes_dev.ptr, count, rect, rgba.ptr)
        torch.cuda.synchronize()
        covered = float((rgba.to_numpy(np.float32, n * 4) != before).reshape(n, 4).any(axis=1).mean())

        def pair():
            svo.shade(cam, P, rect, gbuffer.ptr, rgba.ptr)
            svo.shade_boxes(cam, boxes_dev.ptr, count, rect, rgba.ptr)

        # over a fresh image every time (the frame loop's case): the pair, less the yardstick
        pair_ms = timed(pair, a.runs, a.batch)
        lines.append(line(f"svo_shade + svo_shade_boxes, {count} boxes", pair_ms, None,
                          f"boxes alone = pair - svo_shade = {float(np.median(pair_ms)) - y:.4f} ms = {(float(np.median(pair_ms)) - y) / y:.2f} x svo_shade; "
                          f"{covered:.3f} of the pixels written"))
        # over the image it has already drawn on: every fragment fails the depth test (f == D), nothing is stored
        lines.append(line(f"svo_shade_boxes, {count} boxes, drawn again", timed(lambda: svo.shade_boxes(cam, boxes_dev.ptr, count, rect, rgba.ptr), a.runs, a.batch), y,
                          "16 B read per pixel, no store"))
    lines.append(line("svo_cursor_place", timed(lambda: svo.cursor_place(cam.eye, cam.forward, gbuffer.ptr + 32 * centre, 16.0, boxes_dev.ptr), a.runs, a.batch),
                      y, "one thread"))
    W.destroy()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
