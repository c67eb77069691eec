#!/usr/bin/env python3
"""brick_clearance_estimate.py — CPU estimate of what "settle a lit shadow ray at the primary hit from its brick's flag" would
save.

No GPU.  The world, the cameras and the replay are those of scripts/clearance_estimate.py.  For every lit shadow ray the model
of tests/brick_clearance_model.py repeats the hit block's test - the origin is located in an empty cell of the brick the primary
ray hit, and that brick carries the flag - and the re-march of tests/clearance_model.py counts the steps the ray takes TODAY:
up to the step that first locates a clear EMPTY node (§6t), or all of them.  A step is one tree step or one brick cell of the
oracle's counters; the model's counts are checked against the oracle's for every re-marched ray.

    python scripts/brick_clearance_estimate.py --depth 10 12 --out profiles/brick_clearance_estimate.txt
"""
from __future__ import annotations

import argparse
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import brick_clearance_model as BM  # noqa: E402
import clearance_estimate as CE  # noqa: E402
import oracle_binding as ob  # noqa: E402

P = BM.P
LIGHT, CAMERAS, make_camera = CE.LIGHT, CE.CAMERAS, CE.make_camera
GO_SHARE = 0.04

_MODEL = None


def _one(job):
    origin, chunk, node = job
    r = _MODEL.march_lit(origin)
    in_brick, in_empty, settled = _MODEL.settles(origin, chunk, node)
    word = _MODEL.bmat_word(chunk, node) if settled else 0
    return (r["hit"], r["tree_steps"], r["brick_cells"], r["chunk_descs"], r["first_clear"] or 0, r["first_clear_chunk_descs"] or 0,
            in_brick, in_empty, settled, word == 0xFFFF)


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
    rec = rec.reshape(-1)
    flags = rec["flags"]
    hit = (flags & P.HIT_FLAG) != 0
    lit = hit & ((flags & P.SHADOWED) == 0)
    cd = CE.cam_dict(cam)
    idx = np.nonzero(lit)[0]
    work = []
    for k in idx:
        alpha, beta = P.camera_ray(cd, int(k % w), int(k // w))
        origin = P.vadd(alpha, P.vmuls(beta, np.float32(rec["t"][k]) - model.eps))
        work.append((origin, int(rec["chunk"][k]), int(rec["node"][k]) if rec["cell"][k] != P.CELL_NONE else -1))
    _MODEL = model
    if jobs > 1:
        with mp.get_context("fork").Pool(jobs) as pool:
            res = pool.map(_one, work, chunksize=32)
    else:
        res = [_one(j) for j in work]
    res = np.array(res, np.int64).reshape(-1, 10)
    steps = res[:, 1] + res[:, 2]
    mismatch = int(np.count_nonzero((steps != shad[idx]) | (res[:, 3] != shad_chunks[idx]) | (res[:, 0] != 0)))
    found = res[:, 4] > 0
    today = np.where(found, res[:, 4], steps)                   # light clearance retires the ray at its first clear node
    today_chunks = np.where(found, res[:, 5], res[:, 3])
    settled = res[:, 8] != 0
    unflaggable = settled & (res[:, 9] != 0)
    total_ref = int(prim.sum() + shad[hit].sum())
    total_today = total_ref - int((steps - today).sum())
    return dict(hits=int(hit.sum()), lit=int(lit.sum()), in_brick=int(res[:, 6].sum()), in_empty=int(res[:, 7].sum()),
                settled=int(settled.sum()), settled_steps=int(today[settled].sum()), settled_chunks=int(today_chunks[settled].sum()),
                unflaggable=int(unflaggable.sum()), unflaggable_steps=int(today[unflaggable].sum()),
                shadow_rays=int(hit.sum()), total_today=total_today, total_ref=total_ref, mismatch=mismatch)


def table(depth, args):
    t0 = time.time()
    dims = (4, 1, 4)
    world = ob.OracleWorld.generate(*dims, chunksize=128, depth=depth)
    model = BM.model_of(world, dims, 128, LIGHT)
    lines = [f"# brick clearance estimate: 4x1x4 world, depth {depth}, {args.width}x{args.height}, light normalize{LIGHT}",
             f"# u = {model.u:.3e}, D1 = {model.d1:.3e}, D2 = {model.d2:.3e}, brick premises hold: {model.brick_enabled}; "
             "a step = one tree step or one brick cell of the oracle's counters",
             "# settled = lit rays whose origin lies in an empty cell of the hit brick and that brick has every empty cell clear; their steps "
             "are those they take today (up to the first clear EMPTY node of 6t); share = those steps / all steps of the frame today",
             "camera       hits   lit | origin in hit brick | settled  of shadow rays | steps today  chunk steps | all steps today "
             "(reference) | share  | settled in bricks bmat cannot flag (steps) | model!=oracle"]
    tot = dict(settled=0, settled_steps=0, total_today=0, unflaggable=0, lit=0, shadow_rays=0, unflaggable_steps=0)
    for name, eye, fwd in CAMERAS:
        r = replay(model, world, make_camera(eye, fwd, args.width, args.height), args.jobs)
        for k in tot:
            tot[k] += r[k]
        lines.append(f"{name:<12}{r['hits']:>5} {r['lit']:>5} | {r['in_brick']:>19} | {r['settled']:>7}  {r['settled'] / max(r['shadow_rays'], 1):>15.3f} | "
                     f"{r['settled_steps']:>11} {r['settled_chunks']:>12} | {r['total_today']:>15} ({r['total_ref']:>9}) | "
                     f"{r['settled_steps'] / r['total_today']:.4f} | {r['unflaggable']:>6} ({r['unflaggable_steps']}){'':>28} | {r['mismatch']}")
    share = (tot["settled_steps"] - tot["unflaggable_steps"]) / tot["total_today"]
    lines.append(f"all three: {tot['settled']} of {tot['lit']} lit rays settled ({tot['settled'] / max(tot['shadow_rays'], 1):.3f} of all shadow rays), "
                 f"{tot['settled_steps']} of {tot['total_today']} steps = {tot['settled_steps'] / tot['total_today']:.4f}; "
                 f"{tot['unflaggable']} of them ({tot['unflaggable'] / max(tot['settled'], 1):.3f}) in bricks a 16-bit bmat cannot flag, "
                 f"share without those {share:.4f}   (go if >= {GO_SHARE})   [{time.time() - t0:.0f} s]")
    world.close()
    return "\n".join(lines) + "\n\n"


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


if __name__ == "__main__":
    sys.exit(main())
