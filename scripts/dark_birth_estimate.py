#!/usr/bin/env python3
"""dark_birth_estimate.py — CPU estimate of what "settle a shadow ray that starts in an occupied cell of the hit brick" would
save.

No GPU.  The world, the cameras and the replay are those of scripts/brick_clearance_estimate.py.  For every DARK shadow ray the
reference's arithmetic (BrickClearanceModel.locate) names the brick and the cell its origin lies in; a ray whose origin lies in
an occupied cell of the brick its primary ray hit is what the hit block settles, and tests/dark_birth_model.py repeats the hit
block's own test on it.  A dark ray takes all of its steps today (§6t and §6u end lit rays only); "all steps today" is the
frame's total after §6t and §6u, as profiles/brick_clearance_estimate.txt has it: its "all steps today" minus its settled steps.
A step is one tree step or one brick cell of the oracle's counters; the re-march's counts are checked against the oracle's for
every dark ray.

For the record only, the rays a one-cell look-ahead would settle: origin in an EMPTY cell of the hit brick, hit inside that
brick's first twigmarch (one tree step).

    python scripts/dark_birth_estimate.py --depth 10 12 --out profiles/dark_birth_estimate.txt

By default "all steps today" is read from the text of profiles/brick_clearance_estimate.txt - the table whose header names this depth
and frame size, its '|' columns as scripts/brick_clearance_estimate.py writes them - and its reference total is checked against this
run's oracle.  Without such a table the lit-ray replay is repeated (minutes, and memory per worker, at depth 12); a table in another
layout is an error, not a fall-back: --totals-from '' forces the replay.
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
import brick_clearance_estimate as BE  # noqa: E402
import brick_clearance_model as BM  # noqa: E402
import clearance_estimate as CE  # noqa: E402
import dark_birth_model as DM  # noqa: E402
import oracle_binding as ob  # noqa: E402

P = BM.P
LIGHT, CAMERAS, make_camera = CE.LIGHT, CE.CAMERAS, CE.make_camera
TABLE = {10: (25022, 17903, 35806), 12: (24865, 17769, 35538)}          # the issue's figures at 192x108: dark, in an occupied cell, their steps

_MODEL = None


def _one(job):
    origin, chunk, node = job
    geo = _MODEL.geo
    r = geo.march_lit(origin)
    at = geo.locate(origin)
    in_brick = at is not None and at["kind"] == BM.TWIG and at["cell"] is not None and (at["chunk"], at["node"]) == (chunk, node)
    occupied = False
    if in_brick:
        ch = geo.chunks[chunk]
        occupied = ch.twig[ch.tree[node] & 0x3FFFFFFF][at["cell"]] != 0
    hit_block = _MODEL.dark([origin], chunk, node, at["bmin"], at["size"])[0] if in_brick else False
    return (r["hit"], r["tree_steps"], r["brick_cells"], r["chunk_descs"], in_brick, occupied, hit_block)


def recorded_totals(path, depth, width, height):
    """{camera: (all steps today after 6t and 6u, reference steps)} from the table that scripts/brick_clearance_estimate.py wrote for this
    depth and frame size (its "all steps today" minus its settled steps), or None.  That replay decides a flag per brick and costs far
    more than everything this script does; it is repeated only where no record of it exists."""
    if not path or not os.path.exists(path):
        return None
    out, on = {}, False
    for line in open(path):
        if line.startswith("# brick clearance estimate"):
            on = f"depth {depth}, {width}x{height}," in line
        elif on and "|" in line and not line.startswith(("#", "camera")):
            f = [c.strip() for c in line.split("|")]
            steps = int(f[3].split()[0])
            today, ref = f[4].replace("(", " ").replace(")", " ").split()
            out[f[0].split()[0]] = (int(today) - steps, int(ref))
    return out or None


def replay(model, world, cam, jobs, totals=None):
    """-> dict of the figures of one camera; totals: (all steps today, reference steps) where a record of them exists."""
    global _MODEL
    w, h = cam.width, cam.height
    prm0, prm1 = ob.make_params(shadow=False), ob.make_params(shadow=True, light_dir=LIGHT)
    _, c0 = world.trace_image(cam, params=prm0, counters=True, threads=jobs)
    rec, c1 = world.trace_image(cam, params=prm1, counters=True, threads=jobs)
    c0, c1 = c0.astype(np.int64), c1.astype(np.int64)
    shad = ((c1[..., 3] + c1[..., 1]) - (c0[..., 3] + c0[..., 1])).reshape(-1)
    shad_chunks = (c1[..., 2] - c0[..., 2]).reshape(-1)
    rec = rec.reshape(-1)
    flags = rec["flags"]
    hit = (flags & P.HIT_FLAG) != 0
    dark = hit & ((flags & P.SHADOWED) != 0)
    cd = CE.cam_dict(cam)
    idx = np.nonzero(dark)[0]
    work = []
    for k in idx:
        alpha, beta = P.camera_ray(cd, int(k % w), int(k // w))
        origin = P.vadd(alpha, P.vmuls(beta, np.float32(rec["t"][k]) - model.eps))
        work.append((origin, int(rec["chunk"][k]), int(rec["node"][k]) if rec["cell"][k] != P.CELL_NONE else -1))
    model.geo.is_clear = lambda *a: False               # (a dark ray meets no clear node, §6t; the re-march need not ask)
    _MODEL = model
    if jobs > 1:
        with mp.get_context("fork").Pool(jobs) as pool:
            res = pool.map(_one, work, chunksize=32)
    else:
        res = [_one(j) for j in work]
    del model.geo.is_clear
    res = np.array(res, np.int64).reshape(-1, 7)
    steps = res[:, 1] + res[:, 2]
    mismatch = int(np.count_nonzero((steps != shad[idx]) | (res[:, 3] != shad_chunks[idx]) | (res[:, 0] != 1)))
    in_brick, occupied = res[:, 4] != 0, res[:, 5] != 0
    ahead = in_brick & ~occupied & (res[:, 1] == 1)      # hit inside the hit brick's first twigmarch, from an empty cell
    if totals is None:
        lit = BE.replay(model.geo, world, cam, jobs)     # the frame's total after 6t and 6u
        totals, lit_mismatch = (lit["total_today"] - lit["settled_steps"], lit["total_ref"]), lit["mismatch"]
    else:
        lit_mismatch = 0
        c0s = int((c0[..., 3] + c0[..., 1]).reshape(-1).sum() + shad[hit].sum())
        assert c0s == totals[1], ("the recorded table is not of this world and camera", c0s, totals)
    return dict(hits=int(hit.sum()), dark=int(dark.sum()), in_brick=int(in_brick.sum()), settled=int(occupied.sum()),
                settled_steps=int(steps[occupied].sum()), settled_chunks=int(res[occupied, 3].sum()),
                hit_block_differs=int(np.count_nonzero(res[:, 6] != res[:, 5])),
                ahead=int(ahead.sum()), ahead_steps=int(steps[ahead].sum()), ahead_second=int(np.count_nonzero(ahead & (res[:, 2] == 2))),
                total_today=totals[0], total_ref=totals[1], mismatch=mismatch + lit_mismatch)


def table(depth, args):
    t0 = time.time()
    dims = (4, 1, 4)
    world = ob.OracleWorld.generate(*dims, chunksize=128, depth=depth)
    model = DM.model_of(world, dims, 128, LIGHT)
    lines = [f"# dark birth estimate: 4x1x4 world, depth {depth}, {args.width}x{args.height}, light normalize{LIGHT}",
             f"# premises hold: {model.enabled}; a step = one tree step or one brick cell of the oracle's counters",
             "# settled = dark rays whose origin the reference's arithmetic locates in an occupied cell of the brick the primary ray hit; their "
             "steps are all they take (dark rays are not shortened by 6t / 6u); all steps today = the frame's total after 6t and 6u",
             "# look-ahead (not done) = dark rays from an EMPTY cell of the hit brick that hit inside that brick's first twigmarch",
             "camera       hits  dark | origin in hit brick | settled  of shadow rays | their steps  chunk steps | all steps today (reference) | share  | "
             "look-ahead rays (steps, at the 2nd cell) | hit block != locate | model!=oracle"]
    keys = ("hits", "dark", "settled", "settled_steps", "total_today", "ahead", "ahead_steps", "ahead_second", "hit_block_differs", "mismatch")
    tot = dict.fromkeys(keys, 0)
    recorded = recorded_totals(args.totals_from, depth, args.width, args.height)
    lines.insert(2, "# all steps today: " + (f"from {os.path.relpath(args.totals_from, ROOT)} (its all steps today minus its settled steps; the reference "
                                               "total is checked against this run's)" if recorded else "from the lit-ray replay of scripts/brick_clearance_estimate.py"))
    for name, eye, fwd in CAMERAS:
        r = replay(model, world, make_camera(eye, fwd, args.width, args.height), args.jobs, recorded.get(name) if recorded else None)
        for k in tot:
            tot[k] += r[k]
        lines.append(f"{name:<12}{r['hits']:>5} {r['dark']:>5} | {r['in_brick']:>19} | {r['settled']:>7}  {r['settled'] / max(r['hits'], 1):>15.3f} | "
                     f"{r['settled_steps']:>11} {r['settled_chunks']:>12} | {r['total_today']:>15} ({r['total_ref']:>9}) | "
                     f"{r['settled_steps'] / r['total_today']:.4f} | {r['ahead']:>6} ({r['ahead_steps']}, {r['ahead_second']}){'':>19} | "
                     f"{r['hit_block_differs']:>19} | {r['mismatch']}")
    lines.append(f"all three: {tot['settled']} of {tot['dark']} dark rays settled ({tot['settled'] / max(tot['dark'], 1):.3f} of the dark, "
                 f"{tot['settled'] / max(tot['hits'], 1):.3f} of all shadow rays), {tot['settled_steps']} of {tot['total_today']} steps = "
                 f"{tot['settled_steps'] / tot['total_today']:.4f}; look-ahead: {tot['ahead']} rays, {tot['ahead_steps']} steps = "
                 f"{tot['ahead_steps'] / tot['total_today']:.4f} ({tot['ahead_second']} at the second cell); hit block != locate: "
                 f"{tot['hit_block_differs']}; model != oracle: {tot['mismatch']}   [{time.time() - t0:.0f} s]")
    if (args.width, args.height) == (192, 108) and depth in TABLE:
        want = TABLE[depth]
        got = (tot["dark"], tot["settled"], tot["settled_steps"])
        verdict = "reproduced" if got == want else ("LESS THAN HALF: the premise is wrong" if 2 * got[1] < want[1] else "differs")
        lines.append(f"expected (dark, settled, their steps) = {want}: {verdict}")
    world.close()
    return "\n".join(lines) + "\n\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--depth", type=int, nargs="+", default=[10], help="tree depths to replay, one table each (12 takes minutes)")
    ap.add_argument("--width", type=int, default=192)
    ap.add_argument("--height", type=int, default=108)
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=None)
    ap.add_argument("--totals-from", default=os.path.join(ROOT, "profiles", "brick_clearance_estimate.txt"),
                    help="the brick clearance estimate's table to take 'all steps today' from where it has this depth and frame size ('' = replay)")
    args = ap.parse_args(argv)
    text = "".join(table(depth, args) for depth in args.depth)
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
