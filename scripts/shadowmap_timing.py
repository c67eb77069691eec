"""The shadow map on the benchmark's C3 world: what a frame costs with the shadow ray and with the map, and what the
map costs to render.  bench.py's 32-camera path at 1920x1080, the directional light at normalize(1, -1, 0), HIP events on the null
stream around each pass over the path, best of --reps passes.  Steps (--step, default all; one JSON line each):

    ray      svo_trace with shadow = 1: existing code, the baseline
    map      svo_trace with shadow = 0 alone, and followed by svo_shadowmap_apply against a 2048^2 map (svo_shadowmap_fit, bias two texels)
    render   svo_shadowmap_render alone at 1024^2, 2048^2 and 4096^2, per kernel the launch picks by itself

    python scripts/shadowmap_timing.py [--step ray|map|render ...] [--reps 3] [--out FILE]

Each step builds the world anew, so that a caller can run every step in a process of its own under its own time limit; --out appends.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUN = (1.0, -1.0, 0.0)


class Events:
    """HIP events on the null stream: ms of device time between start() and stop()."""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so.7")               # the runtime the library is already linked against
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def start(self):
        assert self.hip.hipEventRecord(self.a, None) == 0

    def stop(self):
        assert self.hip.hipEventRecord(self.b, None) == 0 and self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return float(ms.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", nargs="*", default=["ray", "map", "render"], choices=["ray", "map", "render"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bench  # noqa: E402  (its camera path)
    svo = importlib.import_module("octree-raymarcher_amd")
    if svo.device_count() < 1:
        sys.exit("shadowmap_timing: no HIP device (nothing is timed without one)")
    ev = Events()
    gw, gh, gd, depth, iw, ih = 4, 1, 4, 12, 1920, 1080
    n, rect = iw * ih, (0, 0, iw, ih)

    def emit(res):
        res.update(world=[gw, gh, gd, depth], image=[iw, ih], reps=a.reps)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def best(fn, per):
        """ms per `per` of fn(): one warm-up pass, then the best of --reps passes (all listed)."""
        fn()
        svo.lib.svo_stream_synchronize(None)
        passes = []
        for _ in range(a.reps):
            ev.start()
            fn()
            passes.append(ev.stop() / per)
        return round(min(passes), 4), [round(x, 4) for x in passes]

    for step in a.step:
        W = svo.World.generate(gw, gh, gd, 128, depth, build_device=0)
        cams = bench.camera_path(svo, "c3_1080p_depth12_4x1x4_shadow", gw, gd, iw, ih)
        g = svo.DeviceBuffer(n * 32)
        res = {"step": step, "cameras": len(cams)}
        if step == "ray":
            prm = svo.trace_params(shadow=True, light_dir=SUN)
            res["trace_shadow_ray_ms"], res["trace_shadow_ray_ms_passes"] = best(lambda: [W.trace(c, prm, rect, g.ptr) for c in cams], len(cams))
        elif step == "map":
            prm = svo.trace_params(shadow=False)
            m = W.shadowmap_fit(SUN, 2048, 2048)
            zbuf = svo.DeviceBuffer(m.width * m.height * 4)
            m.depth_dev = zbuf.ptr
            bias = 2.0 * 2.0 * max(m.half_width / m.width, m.half_height / m.height)
            W.shadowmap_render(m, prm)

            def frames():
                for c in cams:
                    W.trace(c, prm, rect, g.ptr)
                    svo.shadowmap_apply(c, m, 0.0, bias, rect, g.ptr)

            res["trace_no_shadow_ms"], res["trace_no_shadow_ms_passes"] = best(lambda: [W.trace(c, prm, rect, g.ptr) for c in cams], len(cams))
            res["trace_plus_apply_ms"], res["trace_plus_apply_ms_passes"] = best(frames, len(cams))
            res["apply_alone_ms"], res["apply_alone_ms_passes"] = best(lambda: [svo.shadowmap_apply(c, m, 0.0, bias, rect, g.ptr) for c in cams], len(cams))
            # what the lookup says against the shadow ray, on the path's last camera (a diagnostic: DESIGN.md 6p explains the gap)
            fl = g.to_numpy(svo.HIT_DTYPE, n)["flags"]
            W.trace(cams[-1], svo.trace_params(shadow=True, light_dir=SUN), rect, g.ptr)
            svo.lib.svo_stream_synchronize(None)
            fr = g.to_numpy(svo.HIT_DTYPE, n)["flags"]
            sel = ((fl & svo.HIT_FLAG) != 0) & ((fl & svo.ERR_FLAG) == 0)
            res.update(map=[m.width, m.height], texel=round(2.0 * m.half_width / m.width, 4), bias=round(bias, 4), hits_last_camera=int(sel.sum()),
                       shadowed_by_map=round(float(((fl & svo.SHADOWED) != 0)[sel].mean()), 4), shadowed_by_ray=round(float(((fr & svo.SHADOWED) != 0)[sel].mean()), 4),
                       agreement=round(float(((fl & svo.SHADOWED) == (fr & svo.SHADOWED))[sel].mean()), 4))
            zbuf.free()
        else:
            prm = svo.trace_params(shadow=False)
            for size in (1024, 2048, 4096):
                m = W.shadowmap_fit(SUN, size, size)
                zbuf = svo.DeviceBuffer(size * size * 4)
                m.depth_dev = zbuf.ptr
                res[f"render_{size}_ms"], res[f"render_{size}_ms_passes"] = best(lambda: W.shadowmap_render(m, prm), 1)
                z = zbuf.to_numpy(np.float32, size * size)
                res[f"render_{size}_texels_hit"] = round(float(np.isfinite(z).mean()), 4)
                res[f"render_{size}_scratch_bytes"] = size * size * 56
                zbuf.free()
        g.free()
        W.destroy()
        emit(res)


if __name__ == "__main__":
    main()
