"""svo_device_grid_add_mesh and svo_device_grid_fill_enclosed beside their host twins on
  sphere7   a UV sphere of 20 000 triangles at depth 7
  sphere9   one of 300 312 triangles at depth 9
  span9     one triangle across the whole grid at depth 9
  fill9     the fill of sphere9's shell
The device calls are complete when they return: HIP events around the call, the grid restored outside the events, warm-up first, best
of --runs.  The host twins: one thread, host clock, one run each (--no-host leaves them out).  Every device grid is compared with the
host twin's, cell for cell.

    python scripts/mesh_timing.py [--runs 3] [--out profiles/mesh.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/mesh_timing.py --once CASE
        one device call of CASE and nothing else (no warm-up, no host twin): the kernel split, and k_fill_sweep's calls = the sweeps
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import mesh_model as M  # noqa: E402  (the UV sphere of the tests, at any resolution)

svo = importlib.import_module("octree-raymarcher_amd")


def inputs(case):
    """depth, vertices, indices of a case"""
    if case == "sphere7":
        return 7, *M.uv_sphere((64.3, 63.8, 64.1), 50.2, nu=100, nv=101)
    if case in ("sphere9", "fill9"):
        return 9, *M.uv_sphere((256.3, 255.8, 256.1), 200.7, nu=388, nv=388)
    if case == "span9":
        return 9, np.array([[-5.0, -3.0, -4.0], [520.0, 515.0, 100.0], [40.0, 518.0, 517.0]], np.float32), np.array([[0, 1, 2]], np.uint32)
    raise ValueError(case)


class Case:
    def __init__(self, case):
        self.case = case
        self.depth, self.v, self.ix = inputs(case)
        n = 1 << self.depth
        self.start = np.zeros((n, n, n), np.uint16)         # what the timed call begins with
        if case == "fill9":
            svo.grid_add_mesh(self.start, self.v, self.ix, material=3)
        self.dv = torch.from_numpy(self.v).cuda()
        self.di = torch.from_numpy(self.ix.view(np.int32)).cuda()
        self.d0 = torch.from_numpy(self.start.view(np.int16)).cuda()
        self.grid = torch.empty_like(self.d0)
        self.filled = None

    def restore(self):
        self.grid.copy_(self.d0)

    def device(self):
        if self.case == "fill9":
            self.filled = svo.device_grid_fill_enclosed(self.grid.data_ptr(), self.depth, 2)
        else:
            svo.device_grid_add_mesh(self.grid.data_ptr(), self.depth, self.dv.data_ptr(), self.v.shape[0], self.di.data_ptr(), self.ix.shape[0], material=3)

    def host(self):
        g = self.start.copy()
        t0 = time.perf_counter()
        filled = None
        if self.case == "fill9":
            filled = svo.grid_fill_enclosed(g, 2)
        else:
            svo.grid_add_mesh(g, self.v, self.ix, material=3)
        return (time.perf_counter() - t0) * 1e3, g, filled

    def device_ms(self, runs):
        ms = []
        for k in range(runs + 1):                           # the first one is the warm-up
            self.restore()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.device()
            e1.record()
            e1.synchronize()
            if k:
                ms.append(e0.elapsed_time(e1))
        return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cases", nargs="+", default=["sphere7", "sphere9", "span9", "fill9"])
    ap.add_argument("--once", default=None, help="one device call of this case, for a profiler")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.once:
        c = Case(a.once)
        c.restore()
        torch.cuda.synchronize()
        c.device()
        print(f"{a.once}: one call" + (f", {c.filled} cells filled" if c.filled is not None else ""))
        return
    lines = [f"meshes into grids, {torch.cuda.get_device_name(0)}; device: HIP events around the call, best of {a.runs} after a warm-up call; "
             "host twin: one thread, one run"]
    for name in a.cases:
        c = Case(name)
        ms = c.device_ms(a.runs)
        got = c.grid.cpu().numpy().view(np.uint16)
        what = f"{name}: depth {c.depth}, {c.ix.shape[0]} triangles" if name != "fill9" else f"{name}: depth {c.depth}, {c.filled} cells filled"
        text = f"{what:48s} device best {min(ms):9.3f} ms (runs {', '.join(f'{m:.3f}' for m in ms)})"
        if not a.no_host:
            host_ms, want, filled = c.host()
            assert np.array_equal(got, want), f"{name}: the device grid differs from the host twin's"
            if name == "fill9":
                assert filled == c.filled
            text += f"   host twin {host_ms:10.1f} ms   x{host_ms / min(ms):.0f}   grids equal, {int((want != 0).sum())} cells set"
        lines.append(text)
        del c
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
