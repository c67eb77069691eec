"""The per-brick clear flag (tests/brick_clearance_model.py) against the CPU oracle.  No GPU.

Soundness by brute force: from every EMPTY cell of every brick the model flags, shadow rays from the cell's interior, faces,
edges and corners (the first two floats, the middle and the last float of the cell on every axis, chunk seams among them) must
all be lit on the oracle.  Every planted fault of the model must be caught, and the estimate script's re-march must count the
oracle's steps."""
from __future__ import annotations

import importlib.util
import os

import numpy as np
import pytest

import brick_clearance_model as BM
import oracle_binding as ob
import test_light_clearance_cpu as T

f32 = np.float32
DIMS, CHUNK, LIGHTS, SCENES = T.DIMS, T.CHUNK, T.LIGHTS, T.SCENES


def _violations(world, model, eps=0.0):
    """(flagged bricks, empty cells sampled, rays from them that the oracle finds occupied); eps: the march's, 0 = its own 1/8192."""
    origins, bricks = [], 0
    for ci in range(len(model.chunks)):
        for off, lo, size in model.twig_nodes(ci):
            if not model.brick_flag(ci, off, lo, size):
                continue
            bricks += 1
            for k in model.clear_cells(ci, off, lo, size)[0]:
                clo, _ = BM._cell_box(lo, size * 0.25, k)
                origins.append(T._cell_samples(clo, size * 0.25))
    if not origins:
        return bricks, 0, 0
    o = np.concatenate(origins)
    d = np.tile(np.array(model.sdir, f32), (len(o), 1))
    rec = world.trace_rays(o, d, params=ob.make_params(shadow=False, eps=eps), threads=4)
    return bricks, len(origins), int(np.count_nonzero(rec["flags"] & 1))


@pytest.fixture(scope="module")
def worlds():
    made = {k: f() for k, f in SCENES.items()}
    yield made
    for w in made.values():
        w.close()


@pytest.mark.parametrize("light", sorted(LIGHTS))
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_cells_of_flagged_bricks_are_lit(worlds, scene, light):
    world = worlds[scene]
    model = BM.model_of(world, DIMS, CHUNK, LIGHTS[light])
    assert model.brick_enabled
    bricks, cells, bad = _violations(world, model)
    print(f"{scene}/{light}: {bricks} flagged bricks, {cells} empty cells, {bad} shadowed samples")
    assert bad == 0
    if light != "up":
        assert cells > 0, "no flagged brick with an empty cell: the comparison would pass vacuously"


def test_origins_are_located_in_their_cell(worlds):
    """(c) of the proof: an origin taken from a cell is located in that brick and cell by the arithmetic the hit block repeats."""
    world = worlds["flat"]
    model = BM.model_of(world, DIMS, CHUNK, LIGHTS["default"])
    seen = 0
    for ci in range(len(model.chunks)):
        for off, lo, size in model.twig_nodes(ci)[:40]:
            for k in model.clear_cells(ci, off, lo, size)[0][:4]:
                clo, _ = BM._cell_box(lo, size * 0.25, k)
                for o in T._cell_samples(clo, size * 0.25)[::7]:
                    at = model.locate(o)
                    assert (at["chunk"], at["node"], at["cell"]) == (ci, off, k)
                    seen += 1
    assert seen > 0


def test_premises_switch_the_rule_off(worlds):
    world = worlds["flat"]
    chunks = [world.chunk(i) for i in range(4)]
    assert not BM.model_of(world, DIMS, CHUNK, (1.0, -1.0, 1e-4)).brick_enabled     # 6t's premise on the direction
    m = BM.BrickClearanceModel(chunks, DIMS, CHUNK, LIGHTS["default"], chunkcoordmin=(-1, 0, 0))
    assert m.enabled and not m.brick_enabled                                         # a negative coordinate: p - bmin may round
    assert m.flagged_bricks() == 0
    m = BM.BrickClearanceModel(chunks, DIMS, CHUNK, LIGHTS["default"], chunkcoordmin=(1 << 19, 0, 0), eps=16.0)
    assert m.enabled and not m.brick_enabled                                         # u = 8 out there: the voxels of 4 are off the float lattice
    assert m.flagged_bricks() == 0


@pytest.mark.parametrize("fault,scene,light", [("own_cells", "flat", "down"), ("own_cells", "terrain", "default"),
                                               ("bricks_empty", "terrain", "oblique"), ("bricks_empty", "flat", "default"),
                                               ("no_neighbour", "flat", "default")])
def test_planted_fault_is_caught_by_the_oracle(worlds, fault, scene, light):
    world = worlds[scene]
    model = BM.model_of(world, DIMS, CHUNK, LIGHTS[light], faults=(fault,))
    bricks, cells, bad = _violations(world, model)
    print(f"{fault} on {scene}/{light}: {bricks} flagged bricks, {cells} empty cells, {bad} shadowed samples")
    assert bad > 0


def test_a_flag_asks_more_than_6t_of_the_cells_it_covers(worlds):
    """A brick's cells see matter that 6t never lets near a clear node: the flagged bricks are a proper subset of all bricks, and
    on the flat scene the bricks of the ground under open sky are among them."""
    world = worlds["flat"]
    model = BM.model_of(world, DIMS, CHUNK, LIGHTS["down"])
    total = sum(len(model.twig_nodes(ci)) for ci in range(4))
    flagged = model.flagged_bricks()
    print(f"flat/down: {flagged} of {total} bricks flagged")
    assert 0 < flagged < total


def test_estimate_script_counts_the_oracles_steps():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "brick_clearance_estimate.py")
    spec = importlib.util.spec_from_file_location("brick_clearance_estimate", path)
    est = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(est)
    world = ob.OracleWorld.generate(4, 1, 4, chunksize=128, depth=6)
    model = BM.model_of(world, (4, 1, 4), 128, est.LIGHT)
    for name, eye, fwd in est.CAMERAS:
        r = est.replay(model, world, est.make_camera(eye, fwd, 48, 27), jobs=1)
        assert r["lit"] > 0 and r["mismatch"] == 0, (name, r)
        assert 0 < r["settled"] <= r["in_empty"] <= r["in_brick"] <= r["lit"], (name, r)
        assert 0 < r["settled_steps"] < r["total_today"] <= r["total_ref"], (name, r)
    world.close()
