"""svo_world_chunk_from_grid and svo_world_chunk_to_grid on heightfield grids of depth 7, 8 and 9, each beside a
device-to-device hipMemcpyAsync of the same grid bytes on the same stream - the yardstick: the copy moves 2 x the grid's bytes, the
summary pass 1 x plus 1/64.  svo_world_chunk_from_grid is synchronous (it drains the device and is complete on return): host clock
around the call.  Its base summary kernel alone: the device events the library takes around it under SVO_BUILD_TIMING, read from
stderr.  svo_world_chunk_to_grid and the copy: device events around a batch.  Medians of --runs runs after warm-up.

    python scripts/grid_timing.py [--runs 10] [--depths 7 8 9] [--out profiles/grid_timing.txt]
"""
import argparse
import ctypes as C
import importlib
import os
import re
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import grid_model as G  # noqa: E402  (the heightfield with caves of the tests, at any depth)

svo = importlib.import_module("octree-raymarcher_amd")


def hip_runtime():
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
        try:
            return C.CDLL(name)
        except OSError:
            pass
    raise RuntimeError("libamdhip64 not found")


def event_ms(fn, runs, batch):
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


def captured_stderr(fn):
    """What the C library writes to stderr while fn runs."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode(errors="replace")


def line(what, ms, note=""):
    return f"{what:44s} median {float(np.median(ms)):9.4f} ms  (min {min(ms):.4f}, max {max(ms):.4f})  {note}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--depths", type=int, nargs="+", default=[7, 8, 9])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    empty = dict(position=(0.0, 0.0, 0.0), size=128.0, depth=2, tree=np.zeros(1, np.uint32), twig=np.zeros(0, np.uint16))
    lines = [f"chunks from dense grids and back, {torch.cuda.get_device_name(0)}; heightfield with caves (tests/grid_model.py); "
             f"medians of {a.runs} runs after 3 warm-up calls; GB/s = grid bytes / time"]
    for depth in a.depths:
        grid = G.heightfield(depth)
        nbytes = grid.nbytes
        src = torch.from_numpy(grid.view(np.int16)).cuda()
        dst = torch.empty_like(src)
        W = svo.World.create([empty], 1, 1, 1, 128).upload(0)
        build = lambda: W.chunk_from_grid(0, src.data_ptr(), depth)
        os.environ.pop("SVO_BUILD_TIMING", None)
        for _ in range(3):
            build()
        whole = []
        for _ in range(a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            build()
            whole.append((time.perf_counter() - t0) * 1e3)
        os.environ["SVO_BUILD_TIMING"] = "1"
        text = captured_stderr(lambda: [build() for _ in range(a.runs)])
        os.environ.pop("SVO_BUILD_TIMING", None)
        base = [float(m) for m in re.findall(r"\[svo grid\] summary base, depth \d+: ([0-9.]+) ms", text)]
        info = W.info
        to_grid = event_ms(lambda: W.chunk_to_grid(0, depth, dst.data_ptr()), a.runs, 10)
        torch.cuda.synchronize()
        assert torch.equal(src, dst), "the grid read back differs"
        copy = event_ms(lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, None), a.runs, 10)     # 3 = hipMemcpyDeviceToDevice
        gbs = lambda ms: f"{nbytes / 1e6 / float(np.median(ms)):8.1f} GB/s"
        lines.append(f"depth {depth}: {nbytes / 1e6:.1f} MB of grid -> {info.total_trees} node words, {info.total_twigs} bricks")
        lines.append(line("svo_world_chunk_from_grid (whole call, host)", whole))
        lines.append(line("  k_grid_summary alone", base, gbs(base)))
        lines.append(line("svo_world_chunk_to_grid", to_grid, gbs(to_grid)))
        lines.append(line("hipMemcpyAsync device-to-device, same bytes", copy, gbs(copy) + " (of grid bytes; it moves twice that)"))
        W.destroy()
        del src, dst
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
