"""svo_hit_ao on the benchmark's C3 world: one 1920x1080 frame, by device events around a batch of launches, median and
min-max of the windows after warm-up, for (i) svo_hit_ao on both walks, (ii) the baseline it replaces - ONE svo_world_locate launch over the same 8 x hits neighbour points, generated beforehand;
the generation and the fold are not timed, which favours the baseline - and svo_shade_ao against its 36 bytes per pixel.  All variants
alternate inside every round.  (profiles/ao_timing_mappings.txt is this script's output from when k_hit_ao still had its second mapping,
one lane per pixel, chosen per call through the hooks variant: the measurement after which that mapping was deleted.)

    python scripts/ao_timing.py [--runs 20] [--out profiles/ao_timing.txt]
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402  (its camera path)
import ao_model  # noqa: E402  (the neighbour points of the baseline, the fold)

svo = importlib.import_module("octree-raymarcher_amd")
# the compiler's resource usage (-Rpass-analysis=kernel-resource-usage on csrc/device.hip and csrc/shade.hip): VGPRs, spills, waves per SIMD
RESOURCES = {("octet", "literal"): "24 VGPRs", ("octet", "stack"): "33 VGPRs", ("locate", "literal"): "26 VGPRs", ("locate", "stack"): "37 VGPRs"}
F = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gw, gh, gd, iw, ih = 4, 1, 4, 1920, 1080
    n = iw * ih
    rect = (0, 0, iw, ih)
    W = svo.World.generate(gw, gh, gd, 128, a.depth, build_device=0)
    cam = bench.camera_path(svo, "c3_1080p_depth12_4x1x4_shadow", gw, gd, iw, ih)[0]
    gb, vox, ao = svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 4)
    W.trace(cam, svo.trace_params(), rect, gb.ptr)
    W.hit_voxels(gb.ptr, n, vox.ptr)
    torch.cuda.synchronize()
    g, v = gb.to_numpy(svo.HIT_DTYPE, n), vox.to_numpy(svo.VOXEL_DTYPE, n)
    on, N, fu, fv = ao_model.neighbour_points([{"depth": a.depth}] * (gw * gh * gd), 128, cam, None, g, v, ao_model.resolved_eps())
    pts = np.ascontiguousarray(N.reshape(-1, 3))
    pd, recs = svo.DeviceBuffer.from_numpy(pts), svo.DeviceBuffer(pts.shape[0] * 32)
    lines = [f"svo_hit_ao, world {gw}x{gh}x{gd} chunks of depth {a.depth} ({W.info.total_trees} node words, {W.info.wide_nodes} wide nodes), one {iw}x{ih} frame "
             f"({int(on.sum())} hits of {n} pixels, {pts.shape[0]} neighbour points), {torch.cuda.get_device_name(0)}; device events around {a.batch} launches "
             f"back to back, ms per launch, median of {a.runs} such windows (all variants alternating inside every round) after 5 warm-up launches each; "
             f"every kernel: 0 spills, 0 B LDS, 8 waves/SIMD"]

    def hit_ao(_, kernel):
        W.hit_ao(cam, svo.trace_params(kernel=kernel), rect, gb.ptr, vox.ptr, ao.ptr)

    def locate(_, kernel):
        W.locate(pd.ptr, pts.shape[0], svo.trace_params(kernel=kernel), recs.ptr)

    kernels = {"literal": svo.KERNEL_LITERAL, "stack": svo.KERNEL_STACK}
    variants = [(m, k, hit_ao) for m in ("octet",) for k in kernels] + [("locate", k, locate) for k in kernels]
    floats, times = {}, {(m, k): [] for m, k, _ in variants}
    for m, k, call in variants:                                 # warm-up; what each variant writes
        for _ in range(5):
            call(m, kernels[k])
        torch.cuda.synchronize()
        if m == "locate":
            want = np.ones(n, F)
            want[on] = ao_model.fold(((recs.to_numpy(svo.VOXEL_DTYPE, pts.shape[0])["flags"] & 2) != 0).reshape(-1, 8), fu, fv)
            floats[(m, k)] = want
        else:
            floats[(m, k)] = ao.to_numpy(F, n)
    for _ in range(a.runs):
        for m, k, call in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.batch):
                call(m, kernels[k])
            e1.record()
            e1.synchronize()
            times[(m, k)].append(e0.elapsed_time(e1) / a.batch)
    what = {"octet": "svo_hit_ao, eight lanes per pixel", "locate": "svo_world_locate, 8 x hits points"}
    for m, k, _ in variants:
        ms = times[(m, k)]
        med = float(np.median(ms))
        lines.append(f"{what[m]:36s} {k:8s} median {med:8.4f} ms  (min {min(ms):.4f}, max {max(ms):.4f})  {pts.shape[0] / med / 1e6:7.2f} G neighbour points/s  {RESOURCES[(m, k)]}")
    first = floats[("octet", "literal")]
    same = all(np.array_equal(first.view(np.uint32), f.view(np.uint32)) for f in floats.values())
    lines.append(f"both svo_hit_ao walks and the fold of both baselines' records write the same floats: {same} (ao < 1 on {int((first < 1).sum())} pixels)")
    for k in kernels:
        lines.append(f"svo_hit_ao against the baseline, {k}: {np.median(times[('octet', k)]) / np.median(times[('locate', k)]):.3f} of its time")
    # svo_shade_ao: 4 B of ao and 16 B of pixel read, 12 B written back where ao < 1 (the store is skipped where the factor is 1)
    rgba = svo.DeviceBuffer(n * 16)
    svo.shade(cam, svo.shade_defaults(), rect, gb.ptr, rgba.ptr)
    ms = []
    for r in range(a.runs + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.batch):
            svo.shade_ao(ao.ptr, 0.5, n, rgba.ptr)
        e1.record()
        e1.synchronize()
        if r:
            ms.append(e0.elapsed_time(e1) / a.batch)
    med = float(np.median(ms))
    dark = float((first < 1).mean())
    lines.append(f"svo_shade_ao, strength 0.5                     median {med:8.4f} ms  (min {min(ms):.4f}, max {max(ms):.4f})  {n * 36 / med / 1e6:7.1f} GB/s at 36 B per pixel "
                 f"(4 + 16 read, 16 written; {n * (20 + 12 * dark) / med / 1e6:.1f} GB/s counting the 12 B it writes on the {dark:.3f} of the pixels with ao < 1)")
    for b in (gb, vox, ao, pd, recs, rgba):
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
