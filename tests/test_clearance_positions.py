"""Light clearance and brick clearance on the device away from the one world the other clearance tests use: worlds
off the origin up to and beyond the limit eps = 2u of the premises (the 4x1x4 headline world sits exactly on it), a chunkcoordmin
that is no multiple of the grid (the toroidal index every svo_world_shift leaves), negative coordinates, a second chunk layer whose
chunks are one EMPTY node each, every eps around the premise - tests/clearance_positions.py has the table - and every call that
changes the pools, each of which has to drop the bits.  Worlds of four chunks of 128 at depth 6, images of 64x48, two cameras.

The reference is the CPU oracle for the records and the float64 models (tests/clearance_model.py, tests/brick_clearance_model.py)
for the counts; both sides of a count evaluate the same float64 expressions, so no tolerance anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

import clearance_positions as CP
from helpers import assert_gbuffer_equal
import test_brick_clearance as TB
import test_light_clearance as T

pytestmark = pytest.mark.gpu

ROOT, CHUNK, W_IMG, H_IMG, LIGHTS, POSITIONS = T.ROOT, T.CHUNK, T.W_IMG, T.H_IMG, T.LIGHTS, CP.POSITIONS
NONE = ((0.0, 0.0, 0.0), 0)


def views(svo, pos):
    return T.cameras(svo, pos["ccm"], CP.SLAB_CAMERAS if pos["slab"] else CP.CAMERAS)


def counts_of_the_models(ob, O, light, dims, ccm, eps=0.0):
    """(clear nodes, flagged bricks the device can store) over the oracle world's pools."""
    model = TB.brick_model(ob, O, light, dims, ccm, eps)            # (a BrickClearanceModel is a ClearanceModel)
    clear = sum(1 for ci in range(len(model.chunks)) for e in model.empty_nodes(ci) if model.is_clear(ci, *e))
    return clear, model.flagged_bricks(stored_only=True), model


def records_equal(svo, ob, O, W, cams, light, what, **prm):
    """One frame and two frames per launch against the oracle, and the ray count of the first frame."""
    want = T.want_of(ob, O, cams, light, **prm)
    assert_gbuffer_equal(T.march(svo, W, cams, light, **prm), want, f"{what}: two frames per launch")
    assert_gbuffer_equal(T.march(svo, W, cams[:1], light, **prm), want[:W_IMG * H_IMG], f"{what}: one frame")
    O.trace_image(cams[0], params=ob.make_params(shadow=True, light_dir=light, **prm))
    assert W.last_ray_count() == O.last_rays, f"{what}: a retired or settled shadow ray is counted as the oracle counts it"
    return want


# ---------------------------------------------------------------------------------------------- 1. records and counts at every position
# (the light from below reaches nothing but the slab: every other scene leaves `up` vacuous)
@pytest.mark.parametrize("name,light", [(n, l) for n in sorted(POSITIONS) for l in ("default", "oblique", "down", "up") if l != "up" or POSITIONS[n]["slab"]])
def test_records_and_counts_at_every_position(svo, oracle, name, light):
    pos = POSITIONS[name]
    dims, ccm, eps = pos["dims"], pos["ccm"], pos["eps"]
    O, W = T.scene(svo, oracle, "slab" if pos["slab"] else "structures", dims, ccm)
    cams = views(svo, pos)
    W.prepare_light(LIGHTS[light])
    sdir, clear = W.prepared_light()
    assert np.array_equal(np.array(sdir, np.float32), np.array(T.ob_sdir(LIGHTS[light]), np.float32))
    bricks = W.prepared_bricks()
    want_clear, want_bricks, model = counts_of_the_models(oracle, O, LIGHTS[light], dims, ccm, pos["sweep_eps"])
    print(f"{name}/{light}: device {clear} clear nodes, {bricks} flagged bricks; model {want_clear}, {want_bricks} (u = 2^{int(np.log2(model.u))})")
    assert model.enabled and model.brick_enabled == (min(ccm) >= 0)
    assert (clear, bricks) == (want_clear, want_bricks)
    assert clear > 0, "the sweep runs wherever the direction allows it, whatever eps a later launch brings"
    if min(ccm) < 0:
        assert bricks == 0, "a negative coordinate: every flag is written 0"
    else:
        assert bricks > 0
    whole = [ci for ci in range(4) if model.chunks[ci].tree[0] >> 30 == 0]
    if dims == (2, 2, 1):                                           # a chunk that is one EMPTY node fills 64 slots and counts once
        assert len(whole) == 2                                      # the upper layer over the ground, the lower layer under the slab
        once = sum(1 for ci in whole if model.is_clear(ci, 0, model.chunks[ci].lo, float(CHUNK)))
        inner = sum(1 for ci in range(4) if ci not in whole for e in model.empty_nodes(ci) if model.is_clear(ci, *e))
        assert clear == inner + once
        if light == "up" or not pos["slab"]:                        # (any other light comes through the slab to the layer under it)
            assert once > 0, "no whole-chunk EMPTY node is clear: the level-0 branch of the sweep's count is not reached"
    assert ((eps or CP.EPS) >= 2.0 * model.u) == pos["bits"]          # (what use_light_clearance has to find for the launches below)
    records_equal(svo, oracle, O, W, cams, LIGHTS[light], f"{name}/{light}", eps=eps)
    if name == "beyond":                                            # the same bits with an eps that lets them be used
        records_equal(svo, oracle, O, W, cams, LIGHTS[light], f"{name}/{light}, eps = 1/4096", eps=1.0 / 4096)
    assert W.prepared_light() == (sdir, clear) and W.prepared_bricks() == bricks
    W.destroy()


# ---------------------------------------------------------------------------------------------- 2. the bits are in use where they should be
def _lanes(script, variant, position):
    lib = os.path.join(ROOT, "octree-raymarcher_amd", "build", f"libsvo_{variant}.so")
    assert os.path.exists(lib), f"{lib} missing: __graft_entry__.build() makes it"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", script), lib, "lanes", position], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [int(v) for v in r.stdout.split("LANE_STEPS")[1].replace("RAYS", " ").split()]


@pytest.mark.parametrize("variant,position", [("timing", "limit"), ("timing", "deep"), ("timing64", "deep")])
def test_shadow_lanes_do_retire(svo, oracle, variant, position):
    """tests/test_light_clearance.py::test_shadow_lanes_do_retire, its rule and its reason, where eps = 2u: bit-equal records cannot
    see a retire that never fires, and at `limit` that is the headline workload's gain."""
    removed, total = T.removed_by_the_model(svo, oracle, position)
    assert removed > 0.05 * total, (removed, total)
    on, off = _lanes("test_light_clearance.py", variant, position)[:2]
    print(f"{variant} at {position}: {off} lane-steps with the bits off, {on} with them on ({off - on} fewer); the model removes {removed} of {total} oracle steps")
    assert off - on >= removed // 2, (on, off, removed)


@pytest.mark.parametrize("variant,position", [("timing", "limit"), ("timing", "deep"), ("timing64", "deep")])
def test_settled_rays_take_no_steps(svo, oracle, variant, position):
    """tests/test_brick_clearance.py::test_settled_rays_take_no_steps, its rule and its reason, where eps = 2u."""
    rays, steps, total = TB.settled_by_the_model(svo, oracle, position)
    assert rays > 100 and steps > 0.05 * total, (rays, steps, total)
    on, off, rays_on, rays_off, rays_oracle = _lanes("test_brick_clearance.py", variant, position)[:5]
    print(f"{variant} at {position}: {off} lane-steps with the flags off, {on} with them on ({off - on} fewer); the model settles {rays} rays "
          f"that take {steps} of {total} oracle steps; {rays_on} rays counted")
    assert off - on >= steps // 2, (on, off, steps)
    assert rays_on == rays_off == rays_oracle


def test_beyond_the_limit_no_lane_retires(svo, oracle):
    """At `beyond` the march's own eps is below 2u: the bits are there (the sweep ran) and must not be used.  The margin is what a
    kernel that used them would save: the model's clear nodes decided with eps = 1/4096, the rays marched with 1/8192.  Equal lane
    counts are not asked for: whether the sum is independent of the schedule has not been measured."""
    removed, total = T.removed_by_the_model(svo, oracle, "beyond", sweep_eps=1.0 / 4096)
    assert removed > 0.05 * total, (removed, total)
    on, off = _lanes("test_light_clearance.py", "timing", "beyond")[:2]       # (the script compares both launches' records with the oracle)
    print(f"timing at beyond: {off} lane-steps with the bits off, {on} with them on; using the bits would remove {removed} of {total} oracle steps")
    assert off - on < removed // 2, (on, off, removed)


# ---------------------------------------------------------------------------------------------- 3. every path that changes the pools drops the bits
BOX = ((88.0, 48.0, 48.0), (120.0, 80.0, 80.0))         # in chunk A = [0, 128)^3 of the world's frame; under the default light its shadow falls on B = A + 128 x


def _moved(p, ccm):
    return tuple(a + b for a, b in zip(p, CP.offset(ccm)))


def _grid_with(W, chunk, fill):
    g = W.chunk_grid(chunk, 6)                           # [z, y, x], cells of 2
    fill(g)
    return g


def _box_cells(g):
    (x0, y0, z0), (x1, y1, z1) = [[int(v) // 2 for v in c] for c in BOX]
    g[z0:z1, y0:y1, x0:x1] = 5


def _checkerboard(g):
    z, y, x = np.indices(g.shape)
    g[(y >= 16) & ((x // 4 + y // 4 + z // 4) % 2 == 0)] = 5     # whole bricks, every other one: 3657 node words where the slot holds 2048 and
                                                                  # the four slots' tail a quarter of them all (1.1 s of brick model; single cells: 12 s)


def _mutate(svo, ob, O, W, what, A, ccm):
    """Applies mutation `what`; -> adds matter to chunk A (and the oracle world O then holds the same, where the oracle can build it)."""
    lo, hi = _moved(BOX[0], ccm), _moved(BOX[1], ccm)
    if what == "edit_ball":
        assert W.edit_ball(A, svo.EDIT_BUILD, _moved((100.0, 64.0, 64.0), ccm), 24.0, 5) == svo.SVO_OK
    elif what == "edit_ball_all":
        rc, chunks = W.edit_ball_all(svo.EDIT_BUILD, _moved((128.0, 64.0, 64.0), ccm), 24.0, 5)
        assert rc == svo.SVO_OK and len(chunks) == 2 and A in chunks, "the ball lies across the x seam"
    elif what == "edit_cube":
        rc, chunks = W.edit_cube(svo.EDIT_BUILD, lo, hi[0] - lo[0], 5)
        assert rc == svo.SVO_OK and chunks == [A]
    elif what in ("update", "update_realloc"):
        import ctypes as C
        dt, dw = ob.Delta(), ob.Delta()
        ob.lib.orc_build(C.byref(O.w.chunk[A]), ob.vec3(lo), ob.vec3(hi), 5, C.byref(dt), C.byref(dw))
        assert W.update(A, O.chunk(A), realloc=what == "update_realloc") == svo.SVO_OK
    elif what == "chunk_from_grid":
        assert W.set_chunk_grid(A, _grid_with(W, A, _box_cells)) == svo.SVO_OK
    elif what == "outgrow":
        assert W.set_chunk_grid(A, _grid_with(W, A, _checkerboard)) == svo.SVO_OK
    elif what == "compact":
        assert W.compact(A) == svo.SVO_OK
    elif what == "coarsen":
        assert W.coarsen(A) == svo.SVO_OK
        assert W.chunk(A)["depth"] == 5
    else:
        raise AssertionError(what)
    return what not in ("compact", "coarsen")


def _read_back(ob, W, dims, ccm):
    n = dims[0] * dims[1] * dims[2]
    return ob.OracleWorld.from_chunks([W.chunk(i) for i in range(n)], *dims, CHUNK, ccm)


def _shadowed_in(want, chunk):
    return int((((want["flags"] & 5) == 5) & (want["chunk"] == chunk)).sum())


def _dropped_then_restored(svo, ob, W, ref, dims, ccm, cams, light, what):
    """Steps 3 to 8: the bits are gone, records equal the reference, no launch prepares on its own, the call restores the bits and
    the counts are those of the models on the new pools."""
    assert W.prepared_light() == NONE and W.prepared_bricks() == 0, f"{what} drops the bits"
    want = records_equal(svo, ob, ref, W, cams, light, f"after {what}, bits dropped")
    assert W.prepared_light() == NONE and W.prepared_bricks() == 0, "no launch prepares a changed world on its own"
    W.prepare_light(light)
    clear, bricks = W.prepared_light()[1], W.prepared_bricks()
    want_clear, want_bricks, _ = counts_of_the_models(ob, ref, light, dims, ccm)
    print(f"after {what}: device {clear} clear nodes, {bricks} flagged bricks; model {want_clear}, {want_bricks}")
    assert (clear, bricks) == (want_clear, want_bricks) and clear > 0 and bricks > 0
    records_equal(svo, ob, ref, W, cams, light, f"after {what}, prepared again")
    return want


@pytest.mark.parametrize("what", ["edit_ball", "edit_ball_all", "edit_cube", "update", "update_realloc", "chunk_from_grid", "compact", "coarsen", "outgrow"])
def test_every_change_of_the_pools_drops_the_bits(svo, oracle, what, monkeypatch, capfd):
    """The `structures` world at `limit`, default light.  A stale bit in a chunk the change did not touch is harmful exactly when the
    change puts matter into chunk A that shades chunk B: so it does, the oracle's shadowed count over B's hits rises by more than
    50 (the margin of test_first_launch_prepares_an_edit_drops_and_the_call_restores), and a stale bit would leave such a record lit."""
    pos = POSITIONS["limit"]
    dims, ccm, light = pos["dims"], pos["ccm"], LIGHTS["default"]
    O, W = T.scene(svo, oracle, "structures", dims, ccm)
    cams = views(svo, pos)
    A, B = W.index(*W.index_float(_moved((64.0, 64.0, 64.0), ccm))), W.index(*W.index_float(_moved((192.0, 64.0, 64.0), ccm)))
    assert A != B and A == CP.oracle_chunk_at(oracle, O, _moved((64.0, 64.0, 64.0), ccm))
    before = T.want_of(oracle, O, cams, light)
    W.prepare_light(light)
    assert W.prepared_light()[1] > 0 and W.prepared_bricks() > 0
    assert_gbuffer_equal(T.march(svo, W, cams, light), before, "prepared, before the change")
    if what == "outgrow":
        monkeypatch.setenv("SVO_BUILD_TIMING", "1")
        capfd.readouterr()
    adds = _mutate(svo, oracle, O, W, what, A, ccm)
    if what == "outgrow":
        err = capfd.readouterr().err
        monkeypatch.delenv("SVO_BUILD_TIMING")
        assert "no room at the tails, packing the world again" in err, err[-2000:]
    ref = _read_back(oracle, W, dims, ccm)
    after = _dropped_then_restored(svo, oracle, W, ref, dims, ccm, cams, light, what)
    if adds:
        rise = _shadowed_in(after, B) - _shadowed_in(before, B)
        print(f"{what}: {rise} more shadowed records in chunk {B}")
        assert rise > 50, "the new matter's shadow in the chunk beside it"
    if what in ("update", "update_realloc"):             # here the oracle built the same box itself: a second, independent reference
        assert_gbuffer_equal(after, T.want_of(oracle, O, cams, light), "the pools read back against the oracle's own edit")
    W.destroy()


def test_a_shift_drops_the_bits(svo, oracle):
    """svo_world_shift by (+1, 0, 0) on the lake world at `limit`: the reference is an oracle world generated at the new chunkcoordmin,
    which owes the device nothing; the index is toroidal afterwards."""
    pos = POSITIONS["limit"]
    dims, ccm, light = pos["dims"], pos["ccm"], LIGHTS["default"]
    O, W = T.scene(svo, oracle, "lake", dims, ccm)
    W.prepare_light(light)
    assert W.prepared_light()[1] > 0 and W.prepared_bricks() > 0
    assert_gbuffer_equal(T.march(svo, W, T.cameras(svo, ccm), light), T.want_of(oracle, O, T.cameras(svo, ccm), light), "prepared, before the shift")
    assert W.shift((1, 0, 0)) == svo.SVO_OK
    ccm = (ccm[0] + 1, ccm[1], ccm[2])
    assert tuple(W.info.chunkcoordmin) == ccm and W.index(*W.index_float(_moved((1.0, 1.0, 1.0), ccm))) == 1
    ref = oracle.OracleWorld.generate(*dims, chunksize=CHUNK, depth=6, chunkcoordmin=ccm)
    _dropped_then_restored(svo, oracle, W, ref, dims, ccm, T.cameras(svo, ccm), light, "shift")
    W.destroy()


def test_an_upload_makes_the_world_fresh_again(svo, oracle):
    """The one case in which a launch may prepare on its own: the world was uploaded after its last change.  Both ways to a world:
    created from host arrays, and generated on the device (its pools come to the host when svo_world_chunk reads them back)."""
    pos = POSITIONS["limit"]
    dims, ccm, light = pos["dims"], pos["ccm"], LIGHTS["default"]
    O, R = T.scene(svo, oracle, "structures", dims, ccm)
    cams = views(svo, pos)
    n = dims[0] * dims[1] * dims[2]
    W = svo.World.create([O.chunk(i) for i in range(n)], *dims, CHUNK, chunkcoordmin=ccm)
    W.upload(0)
    A = W.index(*W.index_float(_moved((64.0, 64.0, 64.0), ccm)))
    for what, world in (("created from host arrays", W), ("generated on the device", R)):
        world.prepare_light(light)
        assert world.prepared_light()[1] > 0 and world.prepared_bricks() > 0
        assert world.edit_ball(A, svo.EDIT_BUILD, _moved((100.0, 64.0, 64.0), ccm), 24.0, 5) == svo.SVO_OK
        assert world.prepared_light() == NONE and world.prepared_bricks() == 0
        ref = _read_back(oracle, world, dims, ccm)
        want = T.want_of(oracle, ref, cams, light)
        world.upload(0)
        assert world.prepared_light() == NONE and world.prepared_bricks() == 0, "an upload prepares nothing"
        assert_gbuffer_equal(T.march(svo, world, cams, light), want, f"{what}: the first launch after the upload")
        clear, bricks = world.prepared_light()[1], world.prepared_bricks()
        want_clear, want_bricks, _ = counts_of_the_models(oracle, ref, light, dims, ccm)
        print(f"{what}, edited, uploaded again: the launch prepared {clear} clear nodes, {bricks} flagged bricks; model {want_clear}, {want_bricks}")
        assert (clear, bricks) == (want_clear, want_bricks) and clear > 0 and bricks > 0, "a fresh world: its first shadowed launch prepares its light"
        records_equal(svo, oracle, ref, world, cams, light, f"{what}: prepared by the launch")
        world.destroy()


# ---------------------------------------------------------------------------------------------- 4. the 64-bit addressing variant
@pytest.mark.parametrize("script", ["test_light_clearance.py", "test_brick_clearance.py"])
def test_wide64_at_deep_and_on_the_slab(script):
    lib = os.path.join(ROOT, "octree-raymarcher_amd", "build", "libsvo_wide64.so")
    assert os.path.exists(lib), f"{lib} missing: __graft_entry__.build() makes it"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", script), lib, "scenes", "deep", "stacked_slab"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
