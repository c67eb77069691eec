#!/usr/bin/env python3
"""The worlds and ray lists of tests/test_gpu_chunk_step.py, and the march of them through ONE build of the library in its own process
(the binding loads one library per process, like tests/blocks_cases.py).  Test infrastructure.

    python tests/chunk_step_cases.py <path to libsvo_*.so> <reference.npz>

marches every case with the stack kernel and compares every field with the oracle's records, which the test computed once and stored
in <reference.npz>.  exit 0 = every check passed.

What is marched is the chunk step of k_trace_stack (chunk_step_asm.hip.h; the C++ twin of chunk_step_cxx.hip.h in the `cxxstep` build),
on worlds of depth 3 - 5 and lists of 4,096 rays, beyond the grids of tests/blocks_cases.py:

  caps      cap_chunk 1, 2, 3 on the 3x1x2 world: rays end on the cap in each chunk of their path
  outside   origins outside the world that miss its box, run along a face of it, or are aimed at a corner or an edge
  faces     origins exactly on chunk faces and on negative exact multiples of the chunk edge (World::index sends those one chunk down and the
            containment test ends the ray); directions with a zero component from such an origin (0 * inf in the escape distance)
  shift     the 3x1x2 world after svo_world_shift: the grid's first chunk is no longer chunk 0
  mixed     chunks of depth 3, 5, 4, 5 side by side: the descent cache is cleared across chunks of different `levels`
  table     the 9x1x8 world, whose 72 chunks lie outside the chunk table in LDS: shadow rays on and off, the shader twin, far ends under both
            semantics
  glsl      SVO_SEMANTICS_GLSL on the 2x2x2neg world: a point that is not contained steps on out of the box found for it
  segments  svo_trace_segments with far ends just before, on and just behind the chunk faces the rays cross
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import blocks_cases as blocks       # noqa: E402
import segments_model as seg        # noqa: E402

CHUNK = blocks.CHUNK
RAYS = blocks.RAYS
F = np.float32
GRIDS = {name: (dims, depth, ccm) for name, dims, depth, ccm in blocks.GRID_WORLDS}
CAPS = (1, 2, 3)
MIXED_DEPTHS = (3, 5, 4, 5)         # chunks 0..3 of a 2x1x2 world, World::index order ((y * d + z) * w + x)
SHIFT = (1, 0, 0)


def unit(d):
    d = np.asarray(d, np.float64)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def outside_rays(rng, n, lo, hi):
    """A quarter each: origins beyond a face whose ray runs parallel to that face (even rays: it misses the box) or away from it (odd rays:
    the box lies behind the origin - src/Traverse.cpp:115-125 has no tnear > 0 test, the march starts at a negative t); rays that run IN a
    face plane of the box (the closed box test holds with equality); rays aimed at a corner; rays aimed at a point of an edge.  float32
    rounding puts the last two just inside or just outside."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    q = n // 4
    o = np.empty((n, 3)); d = np.empty((n, 3))
    # start beyond a face, never turn back towards it
    o[:q] = lo + rng.random((q, 3)) * ext
    ax = rng.integers(0, 3, q); side = rng.integers(0, 2, q)
    o[np.arange(q), ax] = np.where(side == 1, hi[ax] + 1.0 + 50.0 * rng.random(q), lo[ax] - 1.0 - 50.0 * rng.random(q))
    d[:q] = rng.normal(size=(q, 3))
    d[np.arange(q), ax] = np.abs(d[np.arange(q), ax]) * np.where(side == 1, 1.0, -1.0) * (np.arange(q) % 2)
    # grazing: the origin's coordinate on axis a is a face's, the direction has no component on that axis; from outside and from inside
    s = slice(q, 2 * q)
    o[s] = lo - 0.25 * ext + rng.random((q, 3)) * 1.5 * ext
    ax = rng.integers(0, 3, q); side = rng.integers(0, 2, q)
    o[np.arange(q, 2 * q), ax] = np.where(side == 1, hi[ax], lo[ax])
    d[s] = rng.normal(size=(q, 3))
    d[np.arange(q, 2 * q), ax] = 0.0
    # corners and edges: from outside, aimed at the feature
    corner = np.where(rng.integers(0, 2, (2 * q, 3)) == 1, hi, lo)
    target = corner.copy()
    e = rng.integers(0, 3, q)
    target[q:, :][np.arange(q), e] = (lo + rng.random((q, 3)) * ext)[np.arange(q), e]         # a point on the edge through that corner
    away = np.where(corner == hi, 1.0, -1.0) * (5.0 + 80.0 * rng.random((2 * q, 3)))
    o[2 * q:2 * q + 2 * q] = corner + away
    d[2 * q:2 * q + 2 * q] = target - o[2 * q:2 * q + 2 * q]
    rest = n - 4 * q
    if rest:
        o[4 * q:] = o[:rest]; d[4 * q:] = d[:rest]
    nz = np.linalg.norm(d, axis=1) > 0
    d[~nz] = (1.0, 0.0, 0.0)
    return o.astype(F), unit(d).astype(F)


def face_rays(rng, n, lo, hi):
    """Origins INSIDE the world with one to three coordinates on exact multiples of the chunk edge (the planes through 0 and the negative
    multiples among them); a third of the directions have a zero component on such an axis (0 * inf = NaN in the escape distance), a
    third point down the pinned axis, the rest are generic.  No component on a pinned axis is smaller than 0.05 unless it is 0: a ray that
    leaves a chunk face by less than an ulp per step creeps for 10^8 steps of the reference (tests/test_gpu_parity.py marches those, with small
    caps) and past the kernels' bound on a single ray (STEP_GUARD), which is not the chunk step's business."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    o = lo + rng.random((n, 3)) * (hi - lo)
    d = rng.normal(size=(n, 3))
    for j in range(n):
        axes = rng.permutation(3)[: rng.integers(1, 4)]
        for a in axes:
            o[j, a] = np.clip(np.round(o[j, a] / CHUNK) * CHUNK, lo[a], hi[a])
        for a in axes:
            d[j, a] = np.copysign(max(abs(d[j, a]), 0.05), d[j, a])
        if j % 3 == 0:
            d[j, axes[0]] = 0.0
        elif j % 3 == 1:
            d[j, axes[0]] = -abs(d[j, axes[0]])
    return o.astype(F), unit(d).astype(F)


def mixed_chunks(svo):
    """2x1x2 chunks of depth 3, 5, 4, 5 from grids: rolling ground of several materials, a different height field per chunk."""
    out = []
    for i, depth in enumerate(MIXED_DEPTHS):
        n = 1 << depth
        z, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        h = (0.35 + 0.2 * np.sin((x / n) * 5.0 + i) * np.cos((z / n) * 4.0 - i)) * n
        y = np.arange(n)[None, :, None]
        g = np.where(y < h[:, None, :], 1 + ((x[:, None, :] // 2 + z[:, None, :] // 2 + y) % 5), 0).astype(np.uint16)     # [z, y, x]
        pos = (float(CHUNK * (i % 2)), 0.0, float(CHUNK * (i // 2)))
        out.append(svo.chunk_from_grid(g, position=pos, size=float(CHUNK)))
    return out


def mixed_lists():
    from helpers import random_rays
    rng = np.random.default_rng(4101)
    lo, hi = (0.0, 0.0, 0.0), (2.0 * CHUNK, 1.0 * CHUNK, 2.0 * CHUNK)
    o, d = random_rays(rng, RAYS, lo, hi, inside_frac=0.7)
    # half of them run low over the ground, across the seams between the chunks
    k = RAYS // 2
    o[:k, 1] = 70.0 + 40.0 * rng.random(k)
    d[:k, 1] = -0.15 * np.abs(d[:k, 1])
    d[:k] = unit(d[:k])
    return {"random": (o.astype(F), d.astype(F)), "faces": face_rays(rng, RAYS, lo, hi)}


def mixed_camera(svo):
    return svo.make_camera((20.3, 110.0, -30.0), (0.45, -0.45, 0.77), (0.0, 1.0, 0.0), 70.0, 45, 27)


def segment_rays(rng, n, lo, hi):
    """Rays from inside the world, above the ground, that cross chunk faces, and for each the parameter t at which it crosses the first
    one: far ends are put one float before, on and one float behind that t (and a few at twice and half of it)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    o = lo + rng.random((n, 3)) * (hi - lo)
    o[:, 1] = lo[1] + 60.0 + 50.0 * rng.random(n)
    d = rng.normal(size=(n, 3))
    d[:, 1] = -0.3 * np.abs(d[:, 1])
    d = unit(d)
    o32, d32 = o.astype(F), d.astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        nxt = np.where(d32 > 0, np.floor(o32 / CHUNK) + 1, np.ceil(o32 / CHUNK) - 1) * CHUNK
        t = (nxt.astype(F) - o32) / d32
    t[:, 1] = np.inf                                            # (one chunk high: no face to cross on y)
    t = np.where(np.isfinite(t) & (t > 0), t, np.inf).min(axis=1).astype(F)
    t = np.where(np.isfinite(t), t, F(50.0)).astype(F)
    kind = np.arange(n) % 5
    tmax = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [np.nextafter(t, F(0)), t, np.nextafter(t, F(np.inf)), F(2.0) * t], F(0.5) * t).astype(F)
    return o32, d32, tmax


def case_lists():
    """name -> (world key, origins, dirs); every list RAYS long, from a seed of its own."""
    out = {}
    from helpers import random_rays
    lo, hi = blocks.box_of(*[GRIDS["3x1x2"][k] for k in (0, 2)])
    rng = np.random.default_rng(4001)
    out["caps/random"] = ("3x1x2",) + random_rays(rng, RAYS, lo, hi, inside_frac=0.6)
    o, d = random_rays(rng, RAYS, lo, hi, inside_frac=1.0)      # long, flat rays over the ground: several chunks on their path
    o[:, 1] = 45.0 + 45.0 * rng.random(RAYS)
    d[:, 1] = -0.08 * np.abs(d[:, 1])
    out["caps/flat"] = ("3x1x2", o.astype(F), unit(d).astype(F))
    out["outside"] = ("3x1x2",) + outside_rays(np.random.default_rng(4002), RAYS, lo, hi)
    for name in ("3x1x2neg", "2x2x2neg"):
        lo, hi = blocks.box_of(*[GRIDS[name][k] for k in (0, 2)])
        out[f"faces/{name}"] = (name,) + face_rays(np.random.default_rng(4003 + len(name)), RAYS, lo, hi)
        out[f"lattice/{name}"] = (name,) + blocks.lattice_plane_rays(np.random.default_rng(4013 + len(name)), RAYS, lo, hi)
    lo, hi = blocks.box_of(*[GRIDS["9x1x8"][k] for k in (0, 2)])
    out["table"] = ("9x1x8",) + face_rays(np.random.default_rng(4004), RAYS, lo, hi)
    return out


def shifted_box():
    dims, _, ccm = GRIDS["3x1x2"]
    return blocks.box_of(dims, tuple(c + s for c, s in zip(ccm, SHIFT)))


def shifted_lists():
    from helpers import random_rays
    lo, hi = shifted_box()
    rng = np.random.default_rng(4005)
    return {"random": random_rays(rng, RAYS, lo, hi), "faces": face_rays(rng, RAYS, lo, hi)}


def segment_list():
    lo, hi = blocks.box_of(*[GRIDS["3x1x2neg"][k] for k in (0, 2)])
    return segment_rays(np.random.default_rng(4006), RAYS, lo, hi)


def generate(svo, name):
    dims, depth, ccm = GRIDS[name]
    return svo.World.generate(*dims, CHUNK, depth, chunkcoordmin=ccm)


def oracle_of(ob, W, dims, ccm):
    return ob.OracleWorld.from_chunks([W.chunk(i) for i in range(dims[0] * dims[1] * dims[2])], *dims, CHUNK, ccm)


# ---- the oracle's records of everything above (computed once by the test; host code only)
def reference(svo, ob):
    ref = {}
    lists = case_lists()
    worlds = {}
    for name in GRIDS:
        W = generate(svo, name)
        worlds[name] = (W, oracle_of(ob, W, GRIDS[name][0], GRIDS[name][2]))
    for key, (wname, o, d) in lists.items():
        O = worlds[wname][1]
        if key.startswith("caps/"):
            ref[key + "/free"] = O.trace_rays(o, d, params=ob.make_params(shadow=True), threads=8)
            for cap in CAPS:
                ref[f"{key}/{cap}"] = O.trace_rays(o, d, params=ob.make_params(shadow=True, caps=(cap, 0, 0)), threads=8)
        else:
            for sh in (False, True):
                ref[f"{key}/{int(sh)}"] = O.trace_rays(o, d, params=ob.make_params(shadow=sh), threads=8)
    # the shader twin on the negative grid (a point that is not contained steps on) and the CPU march of the same list beside it
    _, o, d = lists["faces/2x2x2neg"]
    ref["glsl/faces"] = worlds["2x2x2neg"][1].trace_rays(o, d, params=ob.make_params(shadow=True, semantics=1), threads=8)
    _, o, d = lists["lattice/2x2x2neg"]
    ref["glsl/lattice"] = worlds["2x2x2neg"][1].trace_rays(o, d, params=ob.make_params(shadow=True, semantics=1), threads=8)
    ref["glsl/image"] = worlds["2x2x2neg"][1].trace_image(blocks.grid_camera(svo, GRIDS["2x2x2neg"][0], GRIDS["2x2x2neg"][2]),
                                                          params=ob.make_params(shadow=True, semantics=1), threads=8)
    # the table outside LDS under the shader twin and, under both semantics, with a far end per ray (the unbounded hit of the ray before: kept
    # and dropped hits, exact ties); one camera through the 3x1x2 and the 9x1x8 world as well
    _, o, d = lists["table"]
    ref["table/glsl"] = worlds["9x1x8"][1].trace_rays(o, d, params=ob.make_params(shadow=True, semantics=1), threads=8)
    for name in ("3x1x2", "9x1x8"):
        ref[f"image/{name}"] = worlds[name][1].trace_image(blocks.grid_camera(svo, GRIDS[name][0], GRIDS[name][2]), params=ob.make_params(shadow=True), threads=8)
    # which origins of the faces lists the chunk found for them does not contain (World::index_float one chunk down)
    for name in ("3x1x2neg", "2x2x2neg"):
        _, o, _ = lists[f"faces/{name}"]
        ref[f"faces/{name}/uncontained"] = uncontained(ob, worlds[name][1], o)
    # segments: the unbounded records and the far ends
    o, d, tmax = segment_list()
    for sem in (0, 1):
        ref[f"segments/{sem}"] = worlds["3x1x2neg"][1].trace_rays(o, d, params=ob.make_params(shadow=True, semantics=sem), threads=8)
    # the world after a shift
    W = worlds["3x1x2"][0]
    W.shift(SHIFT)
    ccm = tuple(int(v) for v in W.info.chunkcoordmin)
    O = oracle_of(ob, W, GRIDS["3x1x2"][0], ccm)
    for lname, (o, d) in shifted_lists().items():
        ref[f"shift/{lname}"] = O.trace_rays(o, d, params=ob.make_params(shadow=True), threads=8)
    ref["shift/image"] = O.trace_image(blocks.grid_camera(svo, GRIDS["3x1x2"][0], ccm), params=ob.make_params(shadow=True), threads=8)
    ref["shift/ccm"] = np.array(ccm, np.int64)
    for W, _ in worlds.values():
        W.destroy()
    # chunks of mixed depth
    O = ob.OracleWorld.from_chunks(mixed_chunks(svo), 2, 1, 2, CHUNK)
    for lname, (o, d) in mixed_lists().items():
        ref[f"mixed/{lname}"] = O.trace_rays(o, d, params=ob.make_params(shadow=True), threads=8)
    ref["mixed/image"] = O.trace_image(mixed_camera(svo), params=ob.make_params(shadow=True), threads=8)
    return ref


def uncontained(ob, O, origins):
    """Per origin (inside the world box): does the chunk World::index_float finds for it NOT contain it (src/Traverse.cpp:154)?"""
    import ctypes as C
    out = np.zeros(len(origins), bool)
    for j, p in enumerate(np.asarray(origins, F)):
        q = (C.c_int * 3)()
        ob.lib.orc_world_index_float(C.byref(O.w), ob.vec3(p), q)
        r = O.w.chunk[ob.lib.orc_world_index3(C.byref(O.w), q[0], q[1], q[2])]
        lo = (r.position.x, r.position.y, r.position.z)
        out[j] = not ob.lib.orc_isInsideCube(ob.vec3(p), ob.vec3(lo), ob.vec3([c + r.size for c in lo]))
    return out


# ---- the marches
def march_all(svo, ref):
    from helpers import assert_gbuffer_equal
    lists = case_lists()
    worlds = {}
    for name in GRIDS:
        worlds[name] = generate(svo, name)
        worlds[name].upload(0)
    K = svo.KERNEL_STACK
    for key, (wname, o, d) in lists.items():
        W = worlds[wname]
        if key.startswith("caps/"):
            for cap in CAPS:
                assert_gbuffer_equal(W.chunkmarch(o, d, shadow=True, kernel=K, caps=(cap, 0, 0)), ref[f"{key}/{cap}"], f"{key}, cap_chunk {cap}")
        else:
            for sh in (False, True):
                assert_gbuffer_equal(W.chunkmarch(o, d, shadow=sh, kernel=K), ref[f"{key}/{int(sh)}"], f"{key}, shadow {sh}")
    W = worlds["2x2x2neg"]
    for lname in ("faces", "lattice"):
        _, o, d = lists[f"{lname}/2x2x2neg"]
        assert_gbuffer_equal(W.chunkmarch(o, d, shadow=True, kernel=K, semantics=svo.SEMANTICS_GLSL), ref[f"glsl/{lname}"], f"glsl/{lname}")
    got = W.draw(blocks.grid_camera(svo, GRIDS["2x2x2neg"][0], GRIDS["2x2x2neg"][2]), shadow=True, kernel=K, semantics=svo.SEMANTICS_GLSL)
    assert_gbuffer_equal(got, ref["glsl/image"], "glsl/image")
    _, o, d = lists["table"]
    W = worlds["9x1x8"]
    assert_gbuffer_equal(W.chunkmarch(o, d, shadow=True, kernel=K, semantics=svo.SEMANTICS_GLSL), ref["table/glsl"], "table/glsl")
    for sem, key in ((0, "table/1"), (1, "table/glsl")):
        tmax = seg.near_ties(ref[key])
        got = W.chunkmarch(o, d, shadow=True, kernel=K, semantics=sem, tmax=tmax)
        assert_gbuffer_equal(got, seg.expected(ref[key], tmax), f"table, segments, semantics {sem}")
    for name in ("3x1x2", "9x1x8"):
        got = worlds[name].draw(blocks.grid_camera(svo, GRIDS[name][0], GRIDS[name][2]), shadow=True, kernel=K)
        assert_gbuffer_equal(got, ref[f"image/{name}"], f"image/{name}")
    o, d, tmax = segment_list()
    for sem in (0, 1):
        got = worlds["3x1x2neg"].chunkmarch(o, d, shadow=True, kernel=K, semantics=sem, tmax=tmax)
        assert_gbuffer_equal(got, seg.expected(ref[f"segments/{sem}"], tmax), f"segments, semantics {sem}")
    W = worlds["3x1x2"]
    W.shift(SHIFT)
    ccm = tuple(int(v) for v in W.info.chunkcoordmin)
    assert ccm == tuple(int(v) for v in ref["shift/ccm"])
    for lname, (o, d) in shifted_lists().items():
        assert_gbuffer_equal(W.chunkmarch(o, d, shadow=True, kernel=K), ref[f"shift/{lname}"], f"shift/{lname}")
    assert_gbuffer_equal(W.draw(blocks.grid_camera(svo, GRIDS["3x1x2"][0], ccm), shadow=True, kernel=K), ref["shift/image"], "shift/image")
    for W in worlds.values():
        W.destroy()
    W = svo.World.create(mixed_chunks(svo), 2, 1, 2, CHUNK)
    W.upload(0)
    for lname, (o, d) in mixed_lists().items():
        assert_gbuffer_equal(W.chunkmarch(o, d, shadow=True, kernel=K), ref[f"mixed/{lname}"], f"mixed/{lname}")
    assert_gbuffer_equal(W.draw(mixed_camera(svo), shadow=True, kernel=K), ref["mixed/image"], "mixed/image")
    W.destroy()


if __name__ == "__main__":
    lib_path, ref_path = os.path.abspath(sys.argv[1]), sys.argv[2]
    os.environ["SVO_AMD_LIB"] = lib_path
    svo = importlib.import_module("octree-raymarcher_amd")
    assert os.path.samefile(svo.LIB_PATH, lib_path)
    if svo.device_count() < 1:
        print("no HIP device"); sys.exit(3)
    march_all(svo, np.load(ref_path, allow_pickle=False))
    print("chunk step: every record of every case equal to the oracle's")
