"""The "dark at birth" rule (tests/dark_birth_model.py) against the CPU oracle.  No GPU.

Soundness by brute force: from every OCCUPIED cell of every brick, shadow rays from the cell's interior, faces, edges and corners
(the first two floats, the middle and the last float of the cell on every axis, chunk seams among them) must all be shadowed on
the oracle after exactly one chunk step, one tree step and one brick cell.  Origins the hit block's test has to refuse are
refused, every planted fault of the model is caught, the premise on the world's position is seen from both sides, and the
estimate script's counts are the oracle's."""
from __future__ import annotations

import importlib.util
import os

import numpy as np
import pytest

import clearance_positions as CP
import dark_birth_model as DM
import oracle_binding as ob
import test_light_clearance_cpu as T

f32 = np.float32
DIMS, CHUNK, LIGHTS, SCENES = T.DIMS, T.CHUNK, T.LIGHTS, T.SCENES
POSITIONS = {"neg": False, "deep": True, "limit": True}          # is the rule on there?  (§6v: no world corner below 0)


def _cell_lo(lo, leaf, k):
    return (lo[0] + leaf * (k & 3), lo[1] + leaf * ((k >> 2) & 3), lo[2] + leaf * (k >> 4))


def _far_face_samples(lo, size):
    """Origins on the brick's far face on at least one axis (cell 4 there) and one float below Blo on at least one axis."""
    axes = []
    for a in range(3):
        l, h = f32(lo[a]), f32(lo[a] + size)
        axes.append([np.nextafter(l, f32(-np.inf)), l, f32(lo[a] + size * 0.5), np.nextafter(h, f32(-np.inf)), h])
    pts = np.array([(x, y, z) for x in axes[0] for y in axes[1] for z in axes[2]], f32)
    lo32, hi32 = np.array(lo, f32), np.array([lo[a] + size for a in range(3)], f32)
    return pts[((pts < lo32) | (pts >= hi32)).any(axis=1)]


def _march(world, model, origins, eps=0.0):
    """-> bool [N]: the oracle finds the ray from the origin shadowed in one chunk step, one tree step and one brick cell."""
    d = np.tile(np.array(model.sdir, f32), (len(origins), 1))
    rec, cnt = world.trace_rays(origins, d, params=ob.make_params(shadow=False, eps=eps), counters=True, threads=4)
    return ((rec["flags"] & 1) != 0) & (cnt[:, 1] == 1) & (cnt[:, 2] == 1) & (cnt[:, 3] == 1)


def _brute(world, model, eps=0.0, every_cell=False, far_face=False):
    """(origins the model settles, those of them the oracle does not find shadowed at its first cell, origins the model refuses).
    Origins: 64 per occupied cell (every_cell: per cell) of every brick; far_face: and the brick's far face and the floats below Blo."""
    origins, settled = [], []
    for ci in range(len(model.chunks)):
        for off, lo, size in model.twig_nodes(ci):
            leaf = size * 0.25
            words = model.chunks[ci].twig[model.chunks[ci].tree[off] & 0x3FFFFFFF]
            o = [T._cell_samples(_cell_lo(lo, leaf, k), leaf) for k in range(64) if every_cell or words[k] != 0]
            if far_face:
                o.append(_far_face_samples(lo, size))
            if not o:
                continue
            o = np.concatenate(o)
            origins.append(o)
            settled.append(model.dark(o, ci, off, lo, size))
    o, s = np.concatenate(origins), np.concatenate(settled)
    agree = _march(world, model, o[s], eps) if s.any() else np.zeros(0, bool)
    return int(s.sum()), int((~agree).sum()), int((~s).sum())


@pytest.fixture(scope="module")
def worlds():
    made = {k: f() for k, f in SCENES.items()}
    yield made
    for w in made.values():
        w.close()


@pytest.fixture(scope="module")
def placed():
    made = {}

    def get(name, scene):
        if (name, scene) not in made:
            pos = CP.POSITIONS[name]
            made[(name, scene)] = (T._flat if scene == "flat" else T._terrain)(pos["dims"], pos["ccm"])
        return made[(name, scene)]
    yield get
    for w in made.values():
        w.close()


@pytest.mark.parametrize("light", sorted(LIGHTS))
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_origins_in_occupied_cells_are_shadowed_at_once(worlds, scene, light):
    world = worlds[scene]
    model = DM.model_of(world, DIMS, CHUNK, LIGHTS[light])
    assert model.enabled
    settled, bad, refused = _brute(world, model)
    print(f"{scene}/{light}: {settled} origins in occupied cells, {bad} not shadowed in one tree step and one brick cell, {refused} refused")
    assert settled > 10000 and bad == 0 and refused == 0


def test_far_face_and_below_the_box_are_not_settled(worlds):
    """A coordinate on the brick's far face is cell 4 and one float below Blo is a negative difference: refused, whatever the
    cell that a clamped or wrapped index would name holds."""
    world = worlds["flat"]
    model = DM.model_of(world, DIMS, CHUNK, LIGHTS["default"])
    seen = 0
    for ci in range(len(model.chunks)):
        for off, lo, size in model.twig_nodes(ci)[:60]:
            o = _far_face_samples(lo, size)
            assert len(o) == 125 - 27 and not model.dark(o, ci, off, lo, size).any()
            seen += len(o)
    assert seen > 0
    settled, bad, refused = _brute(world, model, far_face=True)                 # ... and nothing settled is wrong with them in the set
    assert bad == 0 and refused > 0


@pytest.mark.parametrize("fault,scene,light", [("clamp", "flat", "default"), ("clamp", "terrain", "oblique"),
                                               ("transposed", "flat", "default"), ("transposed", "terrain", "down"),
                                               ("other_brick", "flat", "default"), ("other_brick", "terrain", "default")])
def test_planted_fault_is_caught_by_the_oracle(worlds, fault, scene, light):
    world = worlds[scene]
    model = DM.model_of(world, DIMS, CHUNK, LIGHTS[light], faults=(fault,))
    settled, bad, _ = _brute(world, model, every_cell=True, far_face=True)
    print(f"{fault} on {scene}/{light}: {settled} origins settled, {bad} of them not shadowed at their first cell on the oracle")
    assert bad > 0


@pytest.mark.parametrize("light", sorted(LIGHTS))
@pytest.mark.parametrize("name,scene", [(n, s) for n in sorted(POSITIONS) for s in sorted(SCENES)])
def test_positions(placed, name, scene, light):
    """Off the origin (`limit`, `deep`: every sample rounded by the full u; toroidal index) the rule holds as it stands.  At `neg` it
    is off, and has to be: the reference's World::index sends the first two floats above x = -128 or z = -128 to the chunk below,
    whose box does not hold them, and the march ends lit."""
    pos = CP.POSITIONS[name]
    world = placed(name, scene)
    model = DM.model_of(world, pos["dims"], CHUNK, LIGHTS[light], pos["ccm"])
    assert model.enabled == POSITIONS[name]
    settled, bad, refused = _brute(world, model, eps=pos["eps"])
    print(f"{name}/{scene}/{light}: {settled} settled, {bad} wrong, {refused} refused")
    assert bad == 0
    if model.enabled:
        assert settled > 10000 and refused == 0
    else:
        assert settled == 0
        forced = DM.model_of(world, pos["dims"], CHUNK, LIGHTS[light], pos["ccm"], faults=("no_premises",))
        settled, bad, _ = _brute(world, forced, eps=pos["eps"])
        print(f"{name}/{scene}/{light} with the premise ignored: {settled} settled, {bad} wrong")
        assert settled > 10000 and bad > 0


@pytest.mark.parametrize("name,fault", [("deep", "clamp"), ("deep", "transposed"), ("limit", "other_brick")])
def test_planted_fault_is_caught_off_the_origin(placed, name, fault):
    pos = CP.POSITIONS[name]
    world = placed(name, "flat")
    model = DM.model_of(world, pos["dims"], CHUNK, LIGHTS["default"], pos["ccm"], faults=(fault,))
    settled, bad, _ = _brute(world, model, eps=pos["eps"], every_cell=True, far_face=True)
    print(f"{fault} at {name}: {settled} settled, {bad} wrong")
    assert bad > 0


def test_premises():
    w = T._flat()
    chunks = [w.chunk(i) for i in range(4)]
    assert DM.DarkBirthModel(chunks, DIMS, CHUNK, (1.0, -1.0, 1e-4)).enabled                      # 6t's premise on the direction: not needed
    assert DM.DarkBirthModel(chunks, DIMS, CHUNK, LIGHTS["default"], eps=1.5 / 4096).enabled       # nor a power-of-two eps
    assert DM.DarkBirthModel(chunks, DIMS, CHUNK, LIGHTS["default"], eps=2.0 ** -20).enabled       # nor eps >= 2u
    assert not DM.DarkBirthModel(chunks, DIMS, CHUNK, LIGHTS["default"], chunkcoordmin=(0, 0, -1)).enabled
    w.close()


def test_estimate_script_counts_the_oracles_steps():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "dark_birth_estimate.py")
    spec = importlib.util.spec_from_file_location("dark_birth_estimate", path)
    est = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(est)
    world = ob.OracleWorld.generate(4, 1, 4, chunksize=128, depth=6)
    model = DM.model_of(world, (4, 1, 4), 128, est.LIGHT)
    for name, eye, fwd in est.CAMERAS:
        r = est.replay(model, world, est.make_camera(eye, fwd, 48, 27), jobs=1)
        assert r["dark"] > 0 and r["mismatch"] == 0, (name, r)
        assert 0 < r["settled"] <= r["in_brick"] <= r["dark"], (name, r)
        assert r["settled_steps"] == 2 * r["settled"] and r["hit_block_differs"] == 0, (name, r)
        assert 0 < r["settled_steps"] < r["total_today"] <= r["total_ref"], (name, r)
    world.close()
