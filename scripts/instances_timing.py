"""Voxel model instances on the benchmark's C3 world: ms per frame of svo_trace(shadow=1), svo_trace_instances and
svo_trace_instance_shadows over bench.py's 32-camera path at 1920x1080, with 32 placements of a depth-6 model (a 64^3 shell), timed
with HIP events recorded between the calls - one host synchronisation per pass over the path, warm-up pass first, best of --reps passes
(every pass is in the JSON), the variants alternated within each pass.  The variants: max_rays = 0 (one slot per pixel) and max_rays =
the previous frame's count_dev[0], for each stage.  Placements: 32 seeded places (x, z uniform over the world), the model's centre
`scale` * 40 units above the terrain found by a downward svo_trace_rays, seeded rotations; one configuration per --scales entry, and
the share of the screen the instances own is reported with it.  Prints one JSON line per configuration.

    python scripts/instances_timing.py [--reps 3] [--out FILE] [--scales 0.25,1.0] [--frames-only N] [--far-eye]

--frames-only N: no timing, N frames of svo_trace + both stages (max_rays = the previous frame's counts) of the first configuration,
for a run under rocprofv3 --kernel-trace --stats (the kernel times of cull, scan, emit, march and resolve).

--far-eye: no frames; 50 000 rays from ONE eye D model units from the model's centre towards seeded points of its box, through
svo_trace_rays and svo_trace_segments (tmax = +inf) on both kernels, host clock around a synchronised call, best of 4 - and the same
rays started 60 units in front of the centre.  What the march costs when `t` is so large that `t + eps` no longer advances it.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np


def model_grid(n=64):
    """The shell of tests/instances_model.py at twice the resolution: a hollow ball with a hole and a slot, two materials."""
    z, y, x = np.meshgrid(*(np.arange(n) + 0.5,) * 3, indexing="ij")
    c, s = n / 2, n / 32
    r = np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2)
    g = np.where((r >= 9.5 * s) & (r <= 14.5 * s), 3, 0).astype(np.uint16)
    g[(g != 0) & (np.abs(y - c) < 3 * s)] = 5
    g[(x > c) & ((y - c) ** 2 + (z - c) ** 2 < 25 * s * s)] = 0
    g[(y > c) & (np.abs(x - 14 * s) < 2.5 * s) & (np.abs(z - c) < 7 * s)] = 0
    return g


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt((a * a).sum())
    co, si = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + si * K + (1 - co) * (K @ K)


def far_eye(svo, Mw):
    import time
    rng = np.random.default_rng(1)
    n = 50000
    for dist, near in ((1250.0, False), (3300.0, False), (3300.0, True)):
        v = np.array([0.3, 0.5, -0.81])
        o = np.tile((32.0 + dist * v / np.linalg.norm(v)).astype(np.float32), (n, 1))
        d = rng.uniform(0.0, 64.0, (n, 3)) - o
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        if near:
            o = (o + d * np.float32(dist - 60.0)).astype(np.float32)
        od, dd, td, out = (svo.DeviceBuffer.from_numpy(a) for a in (o, d, np.full(n, np.inf, np.float32), np.zeros(n * 8, np.uint32)))
        for kernel in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
            prm = svo.trace_params(kernel=kernel)
            for bounded in (False, True):
                best = float("inf")
                for _ in range(4):
                    svo.lib.svo_stream_synchronize(None)
                    t0 = time.perf_counter()
                    if bounded:
                        Mw.trace_segments(od.ptr, dd.ptr, td.ptr, n, prm, out.ptr)
                    else:
                        Mw.trace_rays(od.ptr, dd.ptr, n, prm, out.ptr)
                    svo.lib.svo_stream_synchronize(None)
                    best = min(best, time.perf_counter() - t0)
                r = out.to_numpy(svo.HIT_DTYPE, n)
                print(json.dumps({"far_eye": dist, "started_60_in_front": near, "kernel": kernel, "bounded": bounded, "rays": n, "ms": round(best * 1e3, 3),
                                  "hits": int((r["flags"] & 1).sum()), "runaways": int(np.count_nonzero(r["flags"] & 0x8000))}), flush=True)
        for b in (od, dd, td, out):
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scales", default="0.25,1.0")
    ap.add_argument("--frames-only", type=int, default=0)
    ap.add_argument("--far-eye", action="store_true")
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench  # noqa: E402  (its camera path)
    svo = importlib.import_module("octree-raymarcher_amd")
    hip = C.CDLL("libamdhip64.so.7")                        # the runtime the library is already linked against
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]

    def sync():
        assert svo.lib.svo_stream_synchronize(None) == 0

    def event():
        e = C.c_void_p()
        assert hip.hipEventCreate(C.byref(e)) == 0
        return e

    def elapsed(e0, e1):
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return float(ms.value)

    gw, gh, gd, depth, iw, ih = 4, 1, 4, 12, 1920, 1080
    Mw = svo.World.create([svo.chunk_from_grid(model_grid(64), (0.0, 0.0, 0.0), 64.0)], 1, 1, 1, 64)
    Mw.upload(0)
    if a.far_eye:
        far_eye(svo, Mw)
        Mw.destroy()
        return
    W = svo.World.generate(gw, gh, gd, 128, depth, build_device=0)
    cams = bench.camera_path(svo, "c3_1080p_depth12_4x1x4_shadow", gw, gd, iw, ih)
    n = iw * ih
    rect = (0, 0, iw, ih)
    g, merged, owner = svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 4)
    cnt1, cnt2 = svo.DeviceBuffer(8), svo.DeviceBuffer(8)
    prm = svo.trace_params(shadow=True)
    bias = 1.0 / 256.0
    rng = np.random.default_rng(2026)
    xz = rng.uniform(40.0, gw * 128.0 - 40.0, (32, 2)).astype(np.float32)
    o = np.stack([xz[:, 0], np.full(32, 500.0, np.float32), xz[:, 1]], axis=1)
    down = W.chunkmarch(o, np.tile(np.array([0.0, -1.0, 0.0], np.float32), (32, 1)))
    assert np.all(down["flags"] & svo.HIT_FLAG)
    ground = 500.0 - down["t"]
    rots = [rotation(rng.normal(size=3), float(rng.uniform(0.0, 360.0))) for _ in range(32)]
    ev = [[event() for _ in range(4)] for _ in cams]
    lines = []
    for scale in [float(x) for x in a.scales.split(",")]:
        inst = []
        for j in range(32):
            centre = np.array([o[j, 0], ground[j] + 40.0 * scale, o[j, 2]], np.float64)
            inst.append(svo.Instance(rots[j], centre - scale * (rots[j] @ np.array([32.0, 32.0, 32.0])), scale))
        pairs1, pairs2, owned = [], [], []
        for c in cams:                                                  # the pair counts and the coverage of every camera of the path
            W.trace(c, prm, rect, g.ptr)
            W.trace_instances(Mw, c, prm, rect, g.ptr, inst, merged.ptr, owner.ptr, max_rays=32 * n, count_ptr=cnt1.ptr)
            W.trace_instance_shadows(Mw, c, prm, rect, inst, merged.ptr, owner.ptr, max_rays=32 * n, bias=bias, count_ptr=cnt2.ptr)
            sync()
            pairs1.append(int(cnt1.to_numpy(np.uint32, 2)[0]))
            pairs2.append(int(cnt2.to_numpy(np.uint32, 2)[0]))
            owned.append(int(np.count_nonzero(owner.to_numpy(np.uint32, n))))
        if a.frames_only:
            for k in range(a.frames_only):
                c, p = cams[k % len(cams)], (k - 1) % len(cams)
                W.trace(c, prm, rect, g.ptr)
                W.trace_instances(Mw, c, prm, rect, g.ptr, inst, merged.ptr, owner.ptr, max_rays=max(pairs1[p], 1), count_ptr=cnt1.ptr)
                W.trace_instance_shadows(Mw, c, prm, rect, inst, merged.ptr, owner.ptr, max_rays=max(pairs2[p], 1), bias=bias, count_ptr=cnt2.ptr)
            sync()
            print(json.dumps({"frames_only": a.frames_only, "scale": scale}))
            return

        def pass_ms(previous):
            """(svo_trace, stage 1, stage 2) ms per frame of one pass over the path, from the events between the calls"""
            sync()
            for k, c in enumerate(cams):
                m1, m2 = (max(pairs1[k - 1], 1), max(pairs2[k - 1], 1)) if previous else (0, 0)
                hip.hipEventRecord(ev[k][0], None)
                W.trace(c, prm, rect, g.ptr)
                hip.hipEventRecord(ev[k][1], None)
                W.trace_instances(Mw, c, prm, rect, g.ptr, inst, merged.ptr, owner.ptr, max_rays=m1, count_ptr=cnt1.ptr)
                hip.hipEventRecord(ev[k][2], None)
                W.trace_instance_shadows(Mw, c, prm, rect, inst, merged.ptr, owner.ptr, max_rays=m2, bias=bias, count_ptr=cnt2.ptr)
                hip.hipEventRecord(ev[k][3], None)
            sync()
            return tuple(sum(elapsed(e[i], e[i + 1]) for e in ev) / len(cams) for i in range(3))

        variants = {"default_cap": False, "previous_count": True}
        for v in variants.values():                                     # warm-up (scratch allocated, occupancy queried)
            pass_ms(v)
        times = {v: [] for v in variants}
        for _ in range(a.reps):
            for name, v in variants.items():
                times[name].append(pass_ms(v))
        res = {"world": [gw, gh, gd, depth], "image": [iw, ih], "cameras": len(cams), "reps": a.reps, "instances": 32, "model_depth": 6, "scale": scale,
               "screen_share_owned_mean": round(float(np.mean(owned)) / n, 4), "screen_share_owned_min_max": [round(min(owned) / n, 4), round(max(owned) / n, 4)],
               "pairs_per_pixel_stage1_mean": round(float(np.mean(pairs1)) / n, 4), "pairs_per_pixel_stage2_mean": round(float(np.mean(pairs2)) / n, 4),
               "frames_over_the_default_cap": [int(sum(p > n for p in pairs1)), int(sum(p > n for p in pairs2))],
               "frames_over_the_previous_count": [int(sum(p[k] > max(p[k - 1], 1) for k in range(len(p)))) for p in (pairs1, pairs2)]}
        for name, passes in times.items():
            best = min(passes, key=sum)
            res[name + "_ms"] = dict(zip(("trace", "instances", "instance_shadows"), (round(x, 4) for x in best)))
            res[name + "_ms_passes"] = [[round(x, 4) for x in p] for p in passes]
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
    for b in (g, merged, owner, cnt1, cnt2):
        b.free()
    Mw.destroy()
    W.destroy()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
