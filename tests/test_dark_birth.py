"""Dark at birth on the device (the hit block of kernel_stack.hip.h, device.hip use_dark_birth): a shadow ray whose origin
the hit block locates in an occupied cell of the brick its primary ray hit is settled "shadowed" at that hit - one record, no step -
and every record still equals the oracle's bit for bit: whatever the light, with the clearance bits prepared and after an edit has
dropped them (where only this rule is on), in both normal modes, under every switch and on every path that has to ignore the rule.
Worlds of 2x1x2 chunks at depth 6-7 (the scenes of tests/test_brick_clearance.py), images of 64x48.

`python tests/test_dark_birth.py <library> scenes|lanes|flags|edited` runs against a variant build (tests/variant_check.py's mechanism)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_gbuffer_equal, random_rays
import test_brick_clearance as TB
import test_light_clearance as T

pytestmark = pytest.mark.gpu

ROOT, DIMS, CHUNK, W_IMG, H_IMG, LIGHTS = T.ROOT, T.DIMS, T.CHUNK, T.W_IMG, T.H_IMG, T.LIGHTS
NONE = ((0.0, 0.0, 0.0), 0)
BALL = ((100.0, 64.0, 64.0), 24.0)                  # in chunk 0: under the default light its shadow falls across the seam x = 128


def read_back(ob, W):
    return ob.OracleWorld.from_chunks([W.chunk(i) for i in range(4)], *DIMS, CHUNK)


def equal_in_both_modes(svo, ob, O, W, light, what, cams=None, **prm):
    """One and two frames per launch, cube and face normals, against the oracle; svo_trace_last_ray_count against the oracle's."""
    cams = cams or T.cameras(svo)
    for mode in (svo.NORMAL_CUBE, svo.NORMAL_FACE):
        want = T.want_of(ob, O, cams, light, normal_mode=mode, **{k: v for k, v in prm.items() if k == "eps"})
        assert_gbuffer_equal(T.march(svo, W, cams, light, normal_mode=mode, **prm), want, f"{what}, normal mode {mode}: two frames per launch")
        assert_gbuffer_equal(T.march(svo, W, cams[:1], light, normal_mode=mode, **prm), want[:W_IMG * H_IMG], f"{what}, normal mode {mode}: one frame")
        O.trace_image(cams[0], params=ob.make_params(shadow=True, light_dir=light, normal_mode=mode, **{k: v for k, v in prm.items() if k == "eps"}))
        assert W.last_ray_count() == O.last_rays, "a settled shadow ray must still be counted"
    return want


def prepared_then_dropped(svo, ob, O, W, light, what, cams=None):
    """The clearance bits prepared for `light`; then a ball edit drops them and nothing prepares them again: only this rule is on."""
    W.prepare_light(light)
    want = equal_in_both_modes(svo, ob, O, W, light, f"{what}, prepared", cams)
    assert W.edit_ball(0, svo.EDIT_BUILD, *BALL, 5) == svo.SVO_OK
    assert W.prepared_light() == NONE and W.prepared_bricks() == 0
    ref = read_back(ob, W)
    after = equal_in_both_modes(svo, ob, ref, W, light, f"{what}, bits dropped by edit_ball", cams)
    assert W.prepared_light() == NONE and W.prepared_bricks() == 0, "no launch prepares an edited world on its own"
    return want, after


@pytest.mark.parametrize("light", sorted(LIGHTS))
@pytest.mark.parametrize("name", ["open", "structures", "lake", "mixed"])
def test_records_equal_the_oracle(svo, oracle, name, light):
    O, W = TB.scene(svo, oracle, name)
    want, after = prepared_then_dropped(svo, oracle, O, W, LIGHTS[light], f"{name}/{light}")
    if light != "up":
        assert ((want["flags"] & 4) != 0).sum() > 20 and ((after["flags"] & 4) != 0).sum() > 20, "shadowed records are in the picture"
    W.destroy()


def test_every_switch(svo, oracle):
    O, W = TB.scene(svo, oracle, "structures")
    light, cams = LIGHTS["default"], T.cameras(svo)
    W.prepare_light(light)
    want = T.want_of(oracle, O, cams, light)
    for what, prm in (("SVO_SHADOW_NO_DARK_BIRTH", dict(dark_birth=False)), ("SVO_SHADOW_NO_CLEARANCE", dict(light_clearance=False)),
                      ("SVO_SHADOW_NO_BRICK_CLEARANCE", dict(brick_clearance=False)),
                      ("both 6u switches", dict(light_clearance=False, brick_clearance=False)),
                      ("all three", dict(light_clearance=False, brick_clearance=False, dark_birth=False)),
                      ("no ray settled at its hit", dict(brick_clearance=False, dark_birth=True)),
                      ("the rule off, the flags on", dict(brick_clearance=True, dark_birth=False))):
        assert_gbuffer_equal(T.march(svo, W, cams, light, **prm), want, what)
    assert svo.trace_params(shadow=True, dark_birth=False).shadow == 1 | svo.SHADOW_NO_DARK_BIRTH == 9
    assert svo.trace_params(shadow=False, dark_birth=False).shadow == 0
    W.destroy()


def test_bricks_of_several_materials_and_of_material_0x9000(svo, oracle):
    """Bricks that bmat stores as 0xFFFF - several materials, or one of 0x8000 and above: the rule reads the mask, not the word."""
    light = LIGHTS["default"]
    O, W = T.pair(svo, oracle, **T.FLAT)
    T.build_both(svo, oracle, O, W, [(0, (32.0, 16.0, 32.0), (64.0, 20.0, 64.0)), (1, (160.0, 16.0, 32.0), (192.0, 20.0, 64.0))], material=0x9000)
    T.build_both(svo, oracle, O, W, [(0, (34.0, 20.0, 34.0), (62.0, 22.0, 62.0)), (2, (40.0, 16.0, 160.0), (90.0, 18.0, 200.0))], material=7)
    T.build_both(svo, oracle, O, W, [(2, (42.0, 18.0, 160.0), (88.0, 20.0, 200.0))], material=9)
    want = equal_in_both_modes(svo, oracle, O, W, light, "special bricks, nothing prepared")
    assert {0x9000, 7, 9} <= set(np.unique(want["material"]).tolist())
    W.prepare_light(light)
    equal_in_both_modes(svo, oracle, O, W, light, "special bricks, prepared")
    W.destroy()


def test_a_leaf_node_hit_is_not_settled(svo, oracle):
    """A hit on a LEAF node (cell = SVO_CELL_NONE) carries the tree's frame, not a brick's: it is marched.  The towers of the
    structures are LEAF nodes; shadowed and lit records of such hits are in the picture and equal the oracle's."""
    O, W = TB.scene(svo, oracle, "structures")
    for light in ("default", "oblique"):
        want = T.want_of(oracle, O, T.cameras(svo), LIGHTS[light])
        leaf = want["cell"] == 0xFF                                  # SVO_CELL_NONE
        assert (leaf & ((want["flags"] & 7) == 7)).sum() > 10, "shadowed LEAF hits"
        if light == "default":
            assert (leaf & ((want["flags"] & 7) == 3)).sum() > 10, "lit LEAF hits"
        assert_gbuffer_equal(T.march(svo, W, T.cameras(svo), LIGHTS[light]), want, f"LEAF hits/{light}")
    W.destroy()


def test_paths_that_ignore_the_rule(svo, oracle):
    """GLSL semantics, tile costs, the see-through view, ray lists and segments: the records they gave before, with the switch on and off."""
    O, W = TB.scene(svo, oracle, "lake")
    light, one = LIGHTS["default"], T.cameras(svo)[:1]
    want = T.want_of(oracle, O, one, light)
    ntiles = ((W_IMG + 7) // 8) * ((H_IMG + 7) // 8)
    literal_see = W.draw(one[0], shadow=True, kernel=svo.KERNEL_LITERAL, light_dir=light, see_through=6).reshape(-1)
    costs = []
    for on in (True, False):
        assert_gbuffer_equal(T.march(svo, W, one, light, semantics=svo.SEMANTICS_GLSL, dark_birth=on), T.want_of(oracle, O, one, light, semantics=1), f"GLSL semantics, rule {on}")
        cost = svo.DeviceBuffer(ntiles * 2 * 4)
        assert_gbuffer_equal(T.march(svo, W, one, light, tile_cost_dev=cost.ptr, dark_birth=on), want, f"tile costs recorded, rule {on}")
        costs.append(cost.to_numpy(np.uint32, ntiles * 2).copy())
        cost.free()
        assert_gbuffer_equal(T.march(svo, W, one, light, see_through=6, dark_birth=on), literal_see, f"the see-through view against the literal kernel, rule {on}")
    assert np.array_equal(costs[0], costs[1]), "a settled ray would change the recorded costs"
    assert costs[0].reshape(-1, 2)[:, 1].max() >= 2, "shadow rays' step counts"
    o, d = random_rays(np.random.default_rng(11), 6000, (0, 0, 0), (256, 128, 256))
    prm = oracle.make_params(shadow=True, light_dir=light)
    assert_gbuffer_equal(W.chunkmarch(o, d, shadow=True, kernel=svo.KERNEL_STACK, light_dir=light), O.trace_rays(o, d, params=prm, threads=8), "a ray list")
    far = W.chunkmarch(o, d, shadow=True, kernel=svo.KERNEL_STACK, light_dir=light, tmax=1e30)
    assert_gbuffer_equal(far, O.trace_rays(o, d, params=prm, threads=8), "segments with a far end beyond everything")
    assert_gbuffer_equal(W.draw(one[0], shadow=True, kernel=svo.KERNEL_LITERAL, light_dir=light), want.reshape(H_IMG, W_IMG), "the literal kernel")
    W.destroy()


@pytest.mark.parametrize("eps", [1.0 / 4096 * 1.5, 1.0 / 32768], ids=["no_power_of_two", "below_2u"])
def test_an_eps_that_switches_the_clearance_bits_off(svo, oracle, eps):
    """The bits are prepared and never used with such an eps (tests/clearance_positions.py `below_eps`).  The rule has no premise on eps:
    with 1.5 / 4096 it is on alone; below 2u the launch leaves it off by default (DESIGN 6v "Host"), and the records are the oracle's."""
    O, W = TB.scene(svo, oracle, "structures")
    W.prepare_light(LIGHTS["default"])
    equal_in_both_modes(svo, oracle, O, W, LIGHTS["default"], f"eps = {eps}", eps=eps)
    W.destroy()


@pytest.mark.parametrize("variant", ["cxxstep", "wide64"])
def test_variant_builds(variant):
    lib = os.path.join(ROOT, "octree-raymarcher_amd", "build", f"libsvo_{variant}.so")
    assert os.path.exists(lib), f"{lib} missing: __graft_entry__.build() makes it"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), lib, "scenes"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def count_lane_steps(svo, W, cam, light, want, a, b):
    """Lane-steps of the frame under shadow words `a` and `b`: the asm step's own count of marching lanes summed over its wave-steps
    (StepStats.lanes, sixth uint4 of a wave's counters), records against `want` every time, svo_trace_last_ray_count.
    The sum depends on the schedule a little: a wave that finds no tile left counts as draining and skips bricks that are bound to miss
    (kernel_stack.hip.h SVO_SURE_MISS_WHEN), and a process's first launch runs on another schedule than its later ones.  So: one launch
    that is not counted, three per setting in turn, and the pair that is worst for the claim - the most steps under `a`, the fewest under `b`."""
    waves = 256 * 32
    steps, rays = {"a": [], "b": []}, {}
    for name, shadow in (("warm-up", a),) + (("a", a), ("b", b)) * 3:
        ctr = svo.DeviceBuffer.from_numpy(np.zeros(waves * 6 * 4, np.uint32))
        buf = svo.DeviceBuffer(W_IMG * H_IMG * 32)
        prm = svo.trace_params(shadow=True, kernel=svo.KERNEL_STACK, light_dir=light, counters_dev=ctr.ptr)
        prm.shadow = shadow
        W.trace(cam, prm, (0, 0, W_IMG, H_IMG), buf.ptr)
        svo.lib.svo_stream_synchronize(None)
        assert_gbuffer_equal(buf.to_numpy(svo.HIT_DTYPE, W_IMG * H_IMG), want, f"timing build, shadow = {shadow} ({name})")
        if name != "warm-up":
            steps[name].append(int(ctr.to_numpy(np.uint32, waves * 6 * 4).reshape(waves, 6, 4)[:, 5, 1].astype(np.int64).sum()))
            rays[name] = W.last_ray_count()
        ctr.free(); buf.free()
    print(f"lane-steps under shadow = {a}: {steps['a']}, under shadow = {b}: {steps['b']}")
    return max(steps["a"]), min(steps["b"]), rays["a"], rays["b"]


def lane_steps(svo, ob, what):
    """(script mode, a timing build) the open scene's first camera, default light.
    lanes:  the rule on against SVO_SHADOW_NO_DARK_BIRTH, bits and flags on both times;
    flags:  the flags alone - SVO_SHADOW_NO_DARK_BIRTH (flags on, rule off) against SVO_SHADOW_NO_BRICK_CLEARANCE (neither settles a ray);
    edited: after edit_ball has dropped bits and flags and nothing has prepared them again, the rule on (it is all that is on) against
            SVO_SHADOW_NO_DARK_BIRTH; the model's count for the edited world, read back from the device, goes out with the figures."""
    O, W = T.scene(svo, ob, "open")
    light, cam = LIGHTS["default"], T.cameras(svo)[0]
    W.prepare_light(light)
    a, b = {"lanes": (1, 1 | svo.SHADOW_NO_DARK_BIRTH), "flags": (1 | svo.SHADOW_NO_DARK_BIRTH, 1 | svo.SHADOW_NO_BRICK_CLEARANCE),
            "edited": (1, 1 | svo.SHADOW_NO_DARK_BIRTH)}[what]
    model = ""
    if what == "edited":
        assert W.prepared_bricks() > 0
        assert W.edit_ball(0, svo.EDIT_BUILD, *BALL, 5) == svo.SVO_OK
        assert W.prepared_light() == NONE and W.prepared_bricks() == 0
        O = read_back(ob, W)
        model = " MODEL %d %d %d" % model_counts(ob, O, cam, light)
    want = T.want_of(ob, O, [cam], light)
    on, off, rays_on, rays_off = count_lane_steps(svo, W, cam, light, want, a, b)
    if what == "edited":
        assert W.prepared_light() == NONE and W.prepared_bricks() == 0
    W.destroy()
    O.trace_image(cam, params=ob.make_params(shadow=True, light_dir=light))
    print(f"LANE_STEPS {on} {off} RAYS {rays_on} {rays_off} {O.last_rays}{model}")


def model_counts(ob, O, cam, light):
    """(rays, oracle steps, all steps) of the frame that the rule settles on oracle world O: shadowed rays of brick-cell hits whose
    origin tests/dark_birth_model.py locates in an occupied cell of the hit brick; their steps are the oracle's own counts."""
    import dark_birth_model
    model = dark_birth_model.model_of(O, DIMS, CHUNK, light)
    P = dark_birth_model.P
    _, c0 = O.trace_image(cam, params=ob.make_params(shadow=False), counters=True, threads=8)
    rec, c1 = O.trace_image(cam, params=ob.make_params(shadow=True, light_dir=light), counters=True, threads=8)
    rec = rec.reshape(-1)
    shadow_steps = ((c1[..., 3] + c1[..., 1]).astype(np.int64) - (c0[..., 3] + c0[..., 1])).reshape(-1)
    cd = dict(eye=tuple(cam.eye), forward=tuple(cam.forward), right=tuple(cam.right), up=tuple(cam.up),
              tan_half_x=cam.tan_half_x, tan_half_y=cam.tan_half_y, width=cam.width, height=cam.height)
    rays = steps = 0
    for k in np.nonzero(((rec["flags"] & 7) == 7) & (rec["cell"] != P.CELL_NONE))[0]:      # hit in a brick cell, shadow traced, shadowed
        alpha, beta = P.camera_ray(cd, int(k % W_IMG), int(k // W_IMG))
        origin = P.vadd(alpha, P.vmuls(beta, np.float32(rec["t"][k]) - model.eps))
        if model.dark_at_hit(origin, int(rec["chunk"][k]), int(rec["node"][k])):
            assert shadow_steps[k] == 2, "one tree step and one brick cell"
            rays += 1
            steps += int(shadow_steps[k])
    return rays, steps, int(c1[..., 3].sum() + c1[..., 1].sum())


_settled = {}


def settled_by_the_model(svo, ob):
    """model_counts of the open scene's first camera under the default light."""
    if not _settled:
        O = ob.OracleWorld.generate(*DIMS, chunksize=CHUNK, depth=6, **T.FLAT)
        _settled["open"] = model_counts(ob, O, T.cameras(svo)[0], LIGHTS["default"])
        O.close()
    return _settled["open"]


def run_lanes(variant, what):
    lib = os.path.join(ROOT, "octree-raymarcher_amd", "build", f"libsvo_{variant}.so")
    assert os.path.exists(lib), f"{lib} missing: __graft_entry__.build() makes it"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), lib, what], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [int(v) for v in r.stdout.split("LANE_STEPS")[1].replace("RAYS", " ").replace("MODEL", " ").split()]


@pytest.mark.parametrize("variant", ["timing", "timing64"])
def test_settled_rays_take_no_steps(svo, oracle, variant):
    """No comparison above notices a rule that never settles a ray.  The timing builds count the asm step's marching lanes per
    wave-step: with the rule on, the open scene must take fewer lane-steps than with SVO_SHADOW_NO_DARK_BIRTH (bits and flags on both
    times), on both addressing variants, and count the same rays.  The bound comes from the model, not from the kernel: the two oracle
    steps of a settled ray are lane-steps the kernel takes with the rule off and not with it on; half of the model's figure is
    asked for, as tests/test_brick_clearance.py does and for its reason."""
    rays, steps, total = settled_by_the_model(svo, oracle)
    assert rays > 100 and steps == 2 * rays, (rays, steps, total)
    on, off, rays_on, rays_off, rays_oracle = run_lanes(variant, "lanes")[:5]
    print(f"{variant}: {off} lane-steps with the rule off, {on} with it on ({off - on} fewer); the model settles {rays} rays "
          f"that take {steps} of {total} oracle steps; {rays_on} rays counted")
    assert on < off and off - on >= steps // 2, (on, off, steps)
    assert rays_on == rays_off == rays_oracle, "svo_trace_last_ray_count counts a settled shadow ray as the oracle does"


@pytest.mark.parametrize("variant", ["timing", "timing64"])
def test_the_flags_alone_settle_rays(svo, oracle, variant):
    """tests/test_brick_clearance.py::test_settled_rays_take_no_steps compares a default launch with one under
    SVO_SHADOW_NO_BRICK_CLEARANCE.  Since that bit switches this rule off as well, the rule's own saving is part of that difference, and
    flags that settled nothing would no longer be noticed there.  Here the rule is off on both sides: SVO_SHADOW_NO_DARK_BIRTH (flags
    on) against SVO_SHADOW_NO_BRICK_CLEARANCE (neither), the node bits on both times.  The bound is that test's, from its model: half of
    the oracle steps that the rays settled by the flags take today."""
    rays, steps, total = TB.settled_by_the_model(svo, oracle)
    assert rays > 100 and steps > 0.05 * total, (rays, steps, total)
    on, off, rays_on, rays_off, rays_oracle = run_lanes(variant, "flags")[:5]
    print(f"{variant}: {off} lane-steps with neither rule, {on} with the flags alone ({off - on} fewer); the model settles {rays} rays "
          f"that take {steps} of {total} oracle steps; {rays_on} rays counted")
    assert off - on >= steps // 2, (on, off, steps)
    assert rays_on == rays_off == rays_oracle


def test_rays_settle_after_an_edit():
    """After edit_ball the bits and the flags are gone and this rule is all that is on: it must still settle rays.  The model's count is
    taken on the edited world as the device holds it; half of its steps is asked for, as above."""
    on, off, rays_on, rays_off, rays_oracle, rays, steps, total = run_lanes("timing", "edited")[:8]
    print(f"after edit_ball: {off} lane-steps with the rule off, {on} with it on ({off - on} fewer); the model settles {rays} rays "
          f"that take {steps} of {total} oracle steps; {rays_on} rays counted")
    assert rays > 100 and steps == 2 * rays, (rays, steps, total)
    assert on < off and off - on >= steps // 2, (on, off, steps)
    assert rays_on == rays_off == rays_oracle


if __name__ == "__main__":
    import variant_check
    svo_, ob_ = variant_check.load(os.path.abspath(sys.argv[1]))
    if svo_.device_count() < 1:
        print("no HIP device"); sys.exit(3)
    if sys.argv[2] in ("lanes", "flags", "edited"):
        lane_steps(svo_, ob_, sys.argv[2])
        sys.exit(0)
    for name_ in ("structures", "lake", "mixed"):
        for light_ in ("default", "oblique"):
            O_, W_ = TB.scene(svo_, ob_, name_)
            prepared_then_dropped(svo_, ob_, O_, W_, LIGHTS[light_], f"{name_}/{light_}")
            W_.destroy()
    print("dark birth: structures, lake and mixed depths under two lights, prepared and after an edit, equal the oracle")
