"""The "clear way to the light" predicate (tests/clearance_model.py) against the CPU oracle.  No GPU.

Soundness by brute force: for every cell the model marks clear, shadow rays from its interior, its faces, edges and
corners (the first and the last float of the cell on every axis, chunk seams among them) must all be lit on the oracle.
Every planted fault of the model must be caught, and the estimate script's re-march must count the oracle's steps."""
from __future__ import annotations

import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import clearance_model as CM
import clearance_positions as CP
import oracle_binding as ob

f32 = np.float32
DIMS, CHUNK, DEPTH = (2, 1, 2), 128, 5            # voxels of 4 units, bricks of 16
LIGHTS = {"default": (1.0, -1.0, 0.0), "oblique": (0.5, -1.0, 0.3), "down": (0.0, -1.0, 0.0), "up": (0.0, 1.0, 0.0)}


def _build(world, ci, lo, hi, material=5):
    dt, dw = ob.Delta(), ob.Delta()
    ob.lib.orc_build(C.byref(world.w.chunk[ci]), ob.vec3(lo), ob.vec3(hi), material, C.byref(dt), C.byref(dw))


def _terrain(dims=DIMS, chunkcoordmin=(0, 0, 0)):
    return ob.OracleWorld.generate(*dims, chunksize=CHUNK, depth=DEPTH, chunkcoordmin=chunkcoordmin)


def _flat(dims=DIMS, chunkcoordmin=(0, 0, 0), boxes=CP.STRUCTURES):
    """Flat ground under open sky, towers (the default light comes from -x: they shade the chunk beside them), an arch over the
    seam x = 128 and a roof one voxel thick - CP.STRUCTURES, moved with the world; each box goes to the chunk that World::index
    names for it, which is chunk `position` only where chunkcoordmin is a multiple of the grid."""
    w = ob.OracleWorld.generate(*dims, chunksize=CHUNK, depth=DEPTH, chunkcoordmin=chunkcoordmin, amplitude=0.0, yshift=16.0, water=False)
    for lo, hi in CP.translated(boxes, dims, chunkcoordmin, CHUNK):
        _build(w, CP.oracle_chunk_at(ob, w, CP.centre(lo, hi)), lo, hi)
    return w


SCENES = {"terrain": _terrain, "flat": _flat}


def _cell_samples(lo, size):
    """Per axis: the first two and the last float32 of [lo, lo + size) and the middle -> 64 origins located in the cell."""
    axes = []
    for a in range(3):
        l, h = f32(lo[a]), f32(lo[a] + size)
        axes.append([l, np.nextafter(l, f32(np.inf)), f32(lo[a] + size * 0.5), np.nextafter(h, f32(-np.inf))])
    return np.array([(x, y, z) for x in axes[0] for y in axes[1] for z in axes[2]], f32)


def _violations(world, model, eps=0.0):
    """(clear cells, rays from clear cells that the oracle finds occupied); eps: the march's, 0 = its own 1/8192."""
    origins = []
    for ci in range(len(model.chunks)):
        for off, lo, size in model.empty_nodes(ci):
            if model.is_clear(ci, off, lo, size):
                origins.append(_cell_samples(lo, size))
    if not origins:
        return 0, 0
    o = np.concatenate(origins)
    d = np.tile(np.array(model.sdir, f32), (len(o), 1))
    rec = world.trace_rays(o, d, params=ob.make_params(shadow=False, eps=eps), threads=4)
    return len(origins), int(np.count_nonzero(rec["flags"] & 1))


@pytest.fixture(scope="module")
def worlds():
    made = {k: f() for k, f in SCENES.items()}
    yield made
    for w in made.values():
        w.close()


@pytest.mark.parametrize("light", sorted(LIGHTS))
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_clear_cells_are_lit(worlds, scene, light):
    world = worlds[scene]
    model = CM.model_of(world, DIMS, CHUNK, LIGHTS[light])
    assert model.enabled
    cells, bad = _violations(world, model)
    print(f"{scene}/{light}: {cells} clear cells, {bad} shadowed samples")
    assert bad == 0
    if light != "up":
        assert cells > 0, "no clear cell: the comparison would pass vacuously"


def test_premises_switch_the_rule_off(worlds):
    world = worlds["flat"]
    assert not CM.model_of(world, DIMS, CHUNK, (1.0, -1.0, 1e-4)).enabled          # a component below S_MIN: grazing a chunk face
    m = CM.ClearanceModel([world.chunk(i) for i in range(4)], DIMS, CHUNK, LIGHTS["default"], eps=1.0 / 4096 * 1.5)
    assert not m.enabled                                                            # eps not a power of two
    assert not any(m.is_clear(0, off, lo, size) for off, lo, size in m.empty_nodes(0)[:50])


@pytest.mark.parametrize("fault,scene,light", [("brick_empty", "flat", "default"), ("no_neighbour", "flat", "default"),
                                               ("brick_empty", "terrain", "oblique")])
def test_planted_fault_is_caught_by_the_oracle(worlds, fault, scene, light):
    world = worlds[scene]
    model = CM.model_of(world, DIMS, CHUNK, LIGHTS[light], faults=(fault,))
    cells, bad = _violations(world, model)
    print(f"{fault} on {scene}/{light}: {cells} clear cells, {bad} shadowed samples")
    assert bad > 0


@pytest.mark.parametrize("fault", ["no_delta", "wrong_way"])
def test_planted_dilation_fault_is_caught(worlds, fault):
    """A box that misses the exact prism, or the octant, by less than a sample's rounding (half of D1, half of D2) must still count:
    what the dilation is for.  Without it, or with its sign turned, the box is let through.

    This checks the region tests, not the oracle: NO oracle ray could be constructed that a model without the dilation gets wrong.
    Node boxes lie on the dyadic voxel lattice, so a box is either at least a voxel away from a cell's exact prism or touches it,
    and a touching box meets the closed test at d = 0 as well; a counterexample needs a box strictly outside the exact prism and
    within a few float spacings of it, which only an oblique direction and a search over ~1e5 boxes per hit would produce.  The
    brute-force scenes above pass with `no_delta` and with `wrong_way` planted (0 shadowed samples on all eight scene / light pairs).  The dilation
    rests on the proof in DESIGN 6t alone; the faults the oracle does catch are in test_planted_fault_is_caught_by_the_oracle."""
    world = worlds["flat"]
    good = CM.model_of(world, DIMS, CHUNK, LIGHTS["down"])
    bad = CM.model_of(world, DIMS, CHUNK, LIGHTS["down"], faults=(fault,))
    clo, chi = (32.0, 16.0, 32.0), (36.0, 20.0, 36.0)                              # light straight down: the prism is the column over C
    for which in ("d1", "d2"):
        d = getattr(good, which)
        near = ((36.0 + 0.5 * d, 40.0, 32.0), (40.0, 44.0, 36.0))                   # beside the column, half a dilation away
        assert good._prism(*near, clo, chi, d)
        assert not bad._prism(*near, clo, chi, getattr(bad, which))
    below = ((32.0, 8.0, 32.0), (36.0, 16.0 - 0.5 * good.d2, 36.0))                 # behind C by half a dilation: R2 must keep it
    assert good._octant_grown(*below, clo, chi, good.d2)
    assert not bad._octant_grown(*below, clo, chi, bad.d2)


def test_estimate_script_counts_the_oracles_steps():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "clearance_estimate.py")
    spec = importlib.util.spec_from_file_location("clearance_estimate", path)
    est = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(est)
    world = ob.OracleWorld.generate(4, 1, 4, chunksize=128, depth=6)
    model = CM.model_of(world, (4, 1, 4), 128, est.LIGHT)
    for name, eye, fwd in est.CAMERAS:
        r = est.replay(model, world, est.make_camera(eye, fwd, 48, 27), jobs=1)
        assert r["lit"] > 0 and r["mismatch"] == 0, (name, r)
        assert 0 < r["found"] <= r["lit"] and 0 < r["removed"] < r["lit_steps"], (name, r)
    world.close()
