#!/usr/bin/env python3
"""The worlds and ray lists of tests/test_gpu_descent_request.py, and the march of them through ONE build of the library in its own
process (the binding loads one library per process, like tests/variant_check.py).  Test infrastructure.

    python tests/descent_request_cases.py <path to libsvo_*.so> <reference.npz>

marches every list with the stack kernel, shadow ray on, under both semantics, and compares the records with the oracle's, which
the test computed once and stored in <reference.npz>.  A timing build (-DSVO_STACK_TIMING) also reports what its step counters say
about BRANCH entries: the lists must reach them wherever the tree has a second wide level.  exit 0 = every check passed.
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHUNK = 128
RAYS = 2000                 # per list; two lists per world
# single chunks of levels 1 - 5 (depth - 2: odd and even, top pad 1 and 0, one to three wide levels - a BRANCH entry needs two), and a
# 2x1x2 world whose chunks differ in depth, so that a lane carries its descent column from a deep chunk into a shallow one
WORLDS = [("depth3", (1, 1, 1), (3,)), ("depth4", (1, 1, 1), (4,)), ("depth5", (1, 1, 1), (5,)), ("depth6", (1, 1, 1), (6,)),
          ("depth7", (1, 1, 1), (7,)), ("mixed", (2, 1, 2), (8, 5, 5, 8))]
SEMANTICS = (0, 1)          # the CPU march, its GLSL twin


def chunks_of(svo, dims, depths):
    """The chunks of a world of `dims` whose chunk i has depth depths[i] (the generator is deterministic: every process gets the same)."""
    w, h, d = dims
    gen = {depth: svo.World.generate(w, h, d, CHUNK, depth) for depth in sorted(set(depths))}
    chunks = [gen[depth].chunk(i) for i, depth in enumerate(depths)]
    for g in gen.values():
        g.destroy()
    return chunks


def wide_boundary_rays(rng, n, lo, hi, pitch, voxel):
    """Axis-parallel rays whose origins sit on the lattice of the deepest wide nodes (pitch = 16 voxels: 4 entries of a brick's edge
    each) or one voxel to either side of it, on every axis: consecutive tree steps then cross wide-node boundaries, where the descent
    cache is cut back and the next BRANCH entry pushed again.  Half of them start in front of the world and run through all of it."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    cells = np.floor((hi - lo) / pitch).astype(np.int64)
    o = lo + rng.integers(0, cells + 1, (n, 3)) * pitch + rng.choice([-voxel, 0.0, voxel], (n, 3))
    axis, sign = rng.integers(0, 3, n), rng.choice([-1.0, 1.0], n)
    d = np.zeros((n, 3))
    d[np.arange(n), axis] = sign
    far = np.nonzero(rng.random(n) < 0.5)[0]
    o[far, axis[far]] = np.where(sign[far] > 0, lo[axis[far]] - 3.7, hi[axis[far]] + 3.7)
    return o.astype(np.float32), d.astype(np.float32)


def ray_lists(name, dims, depths):
    sys.path.insert(0, HERE)
    from helpers import random_rays
    rng = np.random.default_rng(7000 + sum(ord(c) for c in name))
    lo, hi = (0.0, 0.0, 0.0), (dims[0] * CHUNK, dims[1] * CHUNK, dims[2] * CHUNK)
    voxel = CHUNK / 2.0 ** max(depths)
    return {"random": random_rays(rng, RAYS, lo, hi), "boundary": wide_boundary_rays(rng, RAYS, lo, hi, min(16.0 * voxel, CHUNK), voxel)}


def march_all(svo, ref, timing=False):
    """Every world, list and semantics through the loaded library's stack kernel against `ref[f"{world}/{list}/{semantics}"]`."""
    from helpers import assert_gbuffer_equal
    report = []
    for name, dims, depths in WORLDS:
        chunks = chunks_of(svo, dims, depths)
        W = svo.World.create(chunks, *dims, CHUNK)
        W.upload(0)
        for lname, (o, d) in ray_lists(name, dims, depths).items():
            for sem in SEMANTICS:
                got = W.chunkmarch(o, d, shadow=True, kernel=svo.KERNEL_STACK, semantics=sem)
                assert_gbuffer_equal(got, ref[f"{name}/{lname}/{sem}"], f"{name}/{lname}/semantics {sem}")
            if timing:
                report.append((name, lname, max(depths)) + branch_counters(svo, W, o, d))
        W.destroy()
    return report


def branch_counters(svo, W, o, d):
    """(-DSVO_STACK_TIMING) lanes that sat a BRANCH entry out and lanes that took it inside the step, summed over the launch's waves
    (kernel_stack.hip.h, the counter block at the kernel's end: six uint4 per wave, the asm step's own in the last)."""
    n = o.shape[0]
    od, dd, out = svo.DeviceBuffer.from_numpy(o), svo.DeviceBuffer.from_numpy(d), svo.DeviceBuffer(n * 32)
    nwaves_max = 256 * 32
    ctr = svo.DeviceBuffer.from_numpy(np.zeros(nwaves_max * 6 * 4, np.uint32))
    W.trace_rays(od.ptr, dd.ptr, n, svo.trace_params(shadow=True, kernel=svo.KERNEL_STACK, counters_dev=ctr.ptr), out.ptr)
    svo.lib.svo_stream_synchronize(None)
    c = ctr.to_numpy(np.uint32, nwaves_max * 6 * 4).reshape(nwaves_max, 6, 4).astype(np.int64)
    for b in (od, dd, out, ctr):
        b.free()
    return int(c[:, 5, 2].sum()), int(c[:, 5, 3].sum())


if __name__ == "__main__":
    lib_path, ref_path = os.path.abspath(sys.argv[1]), sys.argv[2]
    os.environ["SVO_AMD_LIB"] = lib_path
    for p in (HERE, ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    svo = importlib.import_module("octree-raymarcher_amd")
    assert os.path.samefile(svo.LIB_PATH, lib_path)
    if svo.device_count() < 1:
        print("no HIP device"); sys.exit(3)
    timing = "timing" in os.path.basename(lib_path)
    report = march_all(svo, np.load(ref_path, allow_pickle=False), timing)
    for name, lname, depth, sat_out, chased in report:
        print(f"{name}/{lname}: {sat_out} lanes sat a BRANCH out, {chased} took it inside the step")
        # a BRANCH entry points at a wide node of the next wide level: none in a tree of one wide level (depth <= 4), and no ray that
        # reaches the terrain of a deeper tree gets there without one
        if depth >= 5:
            assert sat_out + chased > 0, (name, lname)
    print("descent lists: every record equal to the oracle's")
