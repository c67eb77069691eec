#!/usr/bin/env python3
"""clearance_estimate.py — CPU estimate of what "retire a shadow ray at the first clear cell" would save.

No GPU.  Generates the 4x1x4 world with the CPU oracle, replays three cameras of bench.py's path at 192x108, and for every
lit shadow ray re-marches it with tests/clearance_model.py to find the step at which it first locates a cell whose way to
the light is clear.  A step is one tree step or one brick cell of the oracle's counters; the model's counts are checked
against the oracle's for every re-marched ray.  Prints one table; --out writes it to a file as well.

    python scripts/clearance_estimate.py --depth 10 12 --out profiles/light_clearance_estimate.txt
"""
from __future__ import annotations

import argparse
import math
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clearance_model as CM  # noqa: E402
import oracle_binding as ob  # noqa: E402

P = CM.P
LIGHT = (1.0, -1.0, 0.0)
CAMERAS = [  # (name, eye, forward): bench.py camera_path() at theta = 0 (plus its off-lattice offsets), at theta = 1.449, and its grazing view
    ("survey-like", (256.31, 150.07, -39.87), (0.0, -0.5, 0.866)),
    ("orbit-like", (330.0, 155.0, -19.0), (0.866 * math.sin(0.22 * math.sin(1.449)), -0.5 + 0.08 * (math.cos(2.898) - 1.0),
                                           0.866 * math.cos(0.22 * math.sin(1.449)))),
    ("grazing", (250.3, 90.0, 5.0), (0.06, -0.04, 1.0)),
]


def make_camera(eye, forward, width, height, vfov_deg=60.0, up_hint=(0.0, 1.0, 0.0)):
    """The package's make_camera(), restated so that this script needs no GPU extension."""
    f = np.asarray(forward, np.float64)
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up_hint, np.float64))
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    ty = math.tan(math.radians(vfov_deg) * 0.5)
    cam = ob.OCamera()
    cam.eye[:] = [float(np.float32(x)) for x in eye]
    cam.forward[:] = [float(np.float32(x)) for x in f]
    cam.right[:] = [float(np.float32(x)) for x in r]
    cam.up[:] = [float(np.float32(x)) for x in u]
    cam.tan_half_x, cam.tan_half_y, cam.width, cam.height = ty * width / height, ty, width, height
    return cam


def cam_dict(cam):
    return dict(eye=tuple(cam.eye), forward=tuple(cam.forward), right=tuple(cam.right), up=tuple(cam.up),
                tan_half_x=cam.tan_half_x, tan_half_y=cam.tan_half_y, width=cam.width, height=cam.height)


_MODEL = None


def _march(origin):
    r = _MODEL.march_lit(origin)
    return (r["hit"], r["tree_steps"], r["brick_cells"], r["chunk_descs"], r["first_clear"] or 0, r["first_clear_chunk_descs"] or 0)


def replay(model, world, cam, jobs):
    """-> dict of the figures of one camera."""
    global _MODEL
    w, h = cam.width, cam.height
    prm0, prm1 = ob.make_params(shadow=False), ob.make_params(shadow=True, light_dir=LIGHT)
    _, c0 = world.trace_image(cam, params=prm0, counters=True, threads=jobs)
    rec, c1 = world.trace_image(cam, params=prm1, counters=True, threads=jobs)
    c0, c1 = c0.astype(np.int64), c1.astype(np.int64)
    prim = (c0[..., 3] + c0[..., 1]).reshape(-1)
    shad = ((c1[..., 3] + c1[..., 1]) - (c0[..., 3] + c0[..., 1])).reshape(-1)
    shad_chunks = (c1[..., 2] - c0[..., 2]).reshape(-1)
    flags = rec["flags"].reshape(-1)
    hit = (flags & P.HIT_FLAG) != 0
    lit = hit & ((flags & P.SHADOWED) == 0)
    dark = hit & ((flags & P.SHADOWED) != 0)
    cd = cam_dict(cam)
    idx = np.nonzero(lit)[0]
    origins = []
    for k in idx:
        alpha, beta = P.camera_ray(cd, int(k % w), int(k // w))
        origins.append(P.vadd(alpha, P.vmuls(beta, np.float32(rec["t"].reshape(-1)[k]) - model.eps)))
    _MODEL = model
    if jobs > 1:
        with mp.get_context("fork").Pool(jobs) as pool:
            res = pool.map(_march, origins, chunksize=64)
    else:
        res = [_march(o) for o in origins]
    res = np.array(res, np.int64).reshape(-1, 6)
    steps = res[:, 1] + res[:, 2]
    mismatch = int(np.count_nonzero((steps != shad[idx]) | (res[:, 3] != shad_chunks[idx]) | (res[:, 0] != 0)))
    found = res[:, 4] > 0
    removed = np.where(found, steps - res[:, 4], 0)
    removed_chunks = np.where(found, res[:, 3] - res[:, 5], 0)
    total = int(prim.sum() + shad[hit].sum())
    return dict(pixels=w * h, hits=int(hit.sum()), lit=int(lit.sum()), dark=int(dark.sum()), prim_steps=int(prim.sum()),
                lit_steps=int(shad[lit].sum()), dark_steps=int(shad[dark].sum()), total=total, mismatch=mismatch,
                found=int(found.sum()), first_mean=float(res[found, 4].mean()) if found.any() else float("nan"),
                first_median=float(np.median(res[found, 4])) if found.any() else float("nan"),
                first_p90=float(np.percentile(res[found, 4], 90)) if found.any() else float("nan"),
                removed=int(removed.sum()), lit_chunks=int(res[:, 3].sum()), removed_chunks=int(removed_chunks.sum()))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--depth", type=int, nargs="+", default=[10], help="tree depths to replay, one table each (12 takes minutes)")
    ap.add_argument("--width", type=int, default=192)
    ap.add_argument("--height", type=int, default=108)
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    text = "".join(table(depth, args) for depth in args.depth)
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


def table(depth, args):
    t0 = time.time()
    dims = (4, 1, 4)
    world = ob.OracleWorld.generate(*dims, chunksize=128, depth=depth)
    model = CM.model_of(world, dims, 128, LIGHT)
    lines = [f"# light clearance estimate: 4x1x4 world, depth {depth}, {args.width}x{args.height}, light normalize{LIGHT}",
             f"# u = {model.u:.3e}, D1 = {model.d1:.3e}, D2 = {model.d2:.3e}, S_MIN = 1/{int(1 / CM.S_MIN)}; "
             "a step = one tree step or one brick cell of the oracle's counters",
             "# removed = steps a lit ray takes AFTER the step that first locates a clear cell; share = removed / all steps of the frame",
             "camera       hits   lit  dark | steps prim  lit-shadow dark-shadow | lit rays w/ clear  first clear step mean/med/p90 | "
             "removed  share of all | chunk steps lit / removed | model!=oracle"]
    tot_removed = tot_all = 0
    for name, eye, fwd in CAMERAS:
        r = replay(model, world, make_camera(eye, fwd, args.width, args.height), args.jobs)
        tot_removed += r["removed"]
        tot_all += r["total"]
        lines.append(f"{name:<12}{r['hits']:>5} {r['lit']:>5} {r['dark']:>5} | {r['prim_steps']:>10} {r['lit_steps']:>11} {r['dark_steps']:>11} | "
                     f"{r['found']:>6} of {r['lit']:<6}   {r['first_mean']:>6.1f} / {r['first_median']:.0f} / {r['first_p90']:.0f}"
                     f"{'':>10} | {r['removed']:>7}  {r['removed'] / r['total']:.4f}       | {r['lit_chunks']:>6} / {r['removed_chunks']:<6}"
                     f"      | {r['mismatch']}")
    lines.append(f"all three: removed {tot_removed} of {tot_all} steps = {tot_removed / tot_all:.4f}   "
                 f"(go if >= 0.05)   [{time.time() - t0:.0f} s]")
    world.close()
    return "\n".join(lines) + "\n\n"


if __name__ == "__main__":
    sys.exit(main())
