"""svo_trace_instances and svo_trace_instance_shadows on the GPU.

Both stages are specified in separately rounded float, so what they leave is compared whole with tests/instances_model.py: the
transform, the box rule, the pairs and their ranks rebuilt in numpy float32, the model rays marched by the unchanged CPU oracle.  The
scene is that of tests/test_lights.py with the eight placements of instances_model.scene_instances() of a 32^3 shell; the floors
asserted on the model's own statistics keep the comparison from passing vacuously.  A record is equal when its t, its integer fields and
its normal are bit for bit the model's; a NaN normal component equals a NaN one (the payload is not the ABI's)."""
import numpy as np
import pytest

import instances_model as IM
import local_shadows_model as M
import shade_model as sm
from helpers import assert_gbuffer_equal

pytestmark = pytest.mark.gpu

KERNELS = {"stack": 2, "literal": 1}
W_, H_ = 128, 96
N_ = W_ * H_
FULL = (0, 0, W_, H_)
ROOMY = 8 * N_                                              # a slot for every pair there could be
PAD = 64
SENTINEL = np.uint32(0xDEADBEEF)
NOT_UPLOADED, INVALID = -5, -1


@pytest.fixture(scope="module")
def scene(svo, oracle):
    if svo.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    W = svo.World.generate(2, 1, 2, 128, 8)
    chunks = [W.chunk(i) for i in range(4)]
    W.upload(0)
    chunk = svo.chunk_from_grid(IM.model_grid(), (0.0, 0.0, 0.0), float(IM.MODEL_SIZE))
    assert chunk["depth"] == IM.MODEL_DEPTH
    Mw = svo.World.create([chunk], 1, 1, 1, IM.MODEL_SIZE)
    Mw.upload(0)
    S = dict(W=W, Mw=Mw, ow=oracle.OracleWorld.from_chunks(chunks, 2, 1, 2, 128), om=oracle.OracleWorld.from_chunks([chunk], 1, 1, 1, IM.MODEL_SIZE),
             box=IM.world_box((0, 0, 0), (1, 1, 1), IM.MODEL_SIZE), cam=svo.default_camera(2, 2, 128, W_, H_), inst=IM.scene_instances())
    yield S
    Mw.destroy()
    W.destroy()


@pytest.fixture(scope="module")
def frames(scene, oracle):
    """The oracle's svo_trace records of the whole image (shadow on) per semantics, computed once and never written."""
    out = {s: scene["ow"].trace_image(scene["cam"], params=oracle.make_params(shadow=True, semantics=s), threads=8).reshape(-1) for s in (0, 1)}
    for f in out.values():
        f.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def wanted(scene, frames, oracle):
    """The model's stage 1 of the whole image with a slot for every pair, per semantics; never written."""
    return {s: IM.trace(oracle, scene["om"], scene["box"], scene["cam"], FULL, frames[s], scene["inst"], semantics=s, max_rays=ROOMY) for s in (0, 1)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_records(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, what
    for f in ("flags", "material", "chunk", "node", "cell"):
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at {bad[:8]} (of {bad.size}): got {got[f][bad[:8]]} want {want[f][bad[:8]]}"
    bad = np.nonzero(_bits(got["t"]) != _bits(want["t"]))[0]
    assert bad.size == 0, f"{what}: t differs at {bad[:8]} (of {bad.size}): got {got['t'][bad[:8]]} want {want['t'][bad[:8]]}"
    same = (np.isnan(got["normal"]) & np.isnan(want["normal"])) | (_bits(got["normal"]) == _bits(want["normal"]))
    bad = np.nonzero(~same.all(axis=1))[0]
    assert bad.size == 0, f"{what}: normal differs at {bad[:8]} (of {bad.size}): got {got['normal'][bad[:4]]} want {want['normal'][bad[:4]]}"


def assert_words(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[:6]}: got {got[bad[:6]]} want {want[bad[:6]]}"


class Frame:
    """The device buffers of one frame: the G-buffer, merged (behind it a sentinel record's worth of words), owner, the counts."""

    def __init__(self, svo, rect, in_place=False):
        self.svo, self.rect, self.n = svo, rect, rect[2] * rect[3]
        n = self.n
        self.g = svo.DeviceBuffer.from_numpy(np.full(n * 8 + PAD, SENTINEL, np.uint32))
        self.merged = self.g if in_place else svo.DeviceBuffer.from_numpy(np.full(n * 8 + PAD, SENTINEL, np.uint32))
        self.owner = svo.DeviceBuffer.from_numpy(np.full(n + PAD, SENTINEL, np.uint32))
        self.count = svo.DeviceBuffer.from_numpy(np.full(2 + PAD, SENTINEL, np.uint32))
        self.in_place = in_place

    def records(self, buf):
        words = buf.to_numpy(np.uint32, self.n * 8 + PAD)
        assert np.all(words[self.n * 8:] == SENTINEL), "wrote past w*h records"
        return words[:self.n * 8].view(self.svo.HIT_DTYPE).copy()

    def owners(self):
        words = self.owner.to_numpy(np.uint32, self.n + PAD)
        assert np.all(words[self.n:] == SENTINEL), "wrote past w*h owner words"
        return words[:self.n]

    def counts(self):
        words = self.count.to_numpy(np.uint32, 2 + PAD)
        assert np.all(words[2:] == SENTINEL), "wrote past the two counts"
        return int(words[0]), int(words[1])

    def free(self):
        for b in {self.g, self.merged, self.owner, self.count}:
            b.free()


def stage1(svo, S, prm, rect=FULL, max_rays=ROOMY, in_place=False, inst=None, keep=False):
    """svo_trace, then svo_trace_instances: dict(before, merged, owner, counts, rays) (and the Frame, not freed, if `keep`)."""
    inst = S["inst"] if inst is None else inst
    fr = Frame(svo, rect, in_place)
    S["W"].trace(S["cam"], prm, rect, fr.g.ptr)
    svo.lib.svo_stream_synchronize(None)
    before = fr.records(fr.g)
    S["W"].trace_instances(S["Mw"], S["cam"], prm, rect, fr.g.ptr, IM.instance_structs(svo, inst), fr.merged.ptr, fr.owner.ptr, max_rays=max_rays,
                           count_ptr=fr.count.ptr)
    rays = S["Mw"].last_ray_count()
    svo.lib.svo_stream_synchronize(None)
    out = dict(before=before, merged=fr.records(fr.merged), owner=fr.owners(), counts=fr.counts(), rays=rays)
    if not in_place:
        assert np.array_equal(fr.records(fr.g).view(np.uint8), before.view(np.uint8)), "svo_trace_instances wrote to the G-buffer"
    if keep:
        out["frame"] = fr
    else:
        fr.free()
    return out


def check_floors(m):
    """The issue's floors, on the model's own statistics of the list with a slot for every pair."""
    s = m["stats"]
    for j in IM.VISIBLE:
        assert s[j]["owned"] >= 200, (j, s[j])
    assert sum(x["lost_to_scene"] for x in s) >= 100 and m["contested"] >= 50
    assert s[IM.OFF_SCREEN]["pairs"] == 0 and s[IM.HIDDEN]["pairs"] > 0 and s[IM.HIDDEN]["owned"] == 0
    assert all(x["runaways"] == 0 and x["dropped"] == 0 for x in s)
    assert s[IM.AROUND_EYE]["pairs"] >= N_ // 2             # every ray starts inside its box: tn = 0


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("semantics", [0, 1])
def test_stage1_equals_the_model(svo, scene, frames, wanted, kernel, semantics):
    want = wanted[semantics]
    print(f"kernel {kernel} semantics {semantics}: pairs {want['counts']} contested {want['contested']} {want['stats']}")
    check_floors(want)
    got = stage1(svo, scene, svo.trace_params(shadow=True, kernel=KERNELS[kernel], semantics=semantics))
    assert_gbuffer_equal(got["before"], frames[semantics], "svo_trace")
    assert got["counts"] == want["counts"] and want["counts"][0] == want["counts"][1]
    assert_words(got["owner"], want["owner"], f"owner, kernel {kernel} semantics {semantics}")
    assert_records(got["merged"], want["merged"], f"merged, kernel {kernel} semantics {semantics}")
    assert got["rays"] == ROOMY
    if semantics == 0:
        assert want["counts"][0] == 17329 and [s["owned"] for s in want["stats"]] == [475, 402, 469, 459, 0, 408, 543, 0]


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_capped(svo, oracle, scene, frames, wanted, kernel):
    """max_rays = half the pairs: the later instances' pairs have no slot and count as no hit; the default cap, one slot per pixel,
    drops too; the model world's last launch was of cap rays."""
    prm = svo.trace_params(shadow=True, kernel=KERNELS[kernel])
    total = wanted[0]["counts"][0]
    for max_rays in (total // 2, 0, total, total - 1, 1):
        want = IM.trace(oracle, scene["om"], scene["box"], scene["cam"], FULL, frames[0], scene["inst"], max_rays=max_rays)
        cap = max_rays or N_
        assert want["counts"] == (total, min(total, cap)) and sum(s["dropped"] for s in want["stats"]) == max(total - cap, 0)
        got = stage1(svo, scene, prm, max_rays=max_rays)
        assert got["counts"] == want["counts"] and got["rays"] == cap
        assert_words(got["owner"], want["owner"], f"owner, max_rays {max_rays}")
        assert_records(got["merged"], want["merged"], f"merged, max_rays {max_rays}")
        if max_rays == total // 2:
            assert np.count_nonzero(want["owner"] != wanted[0]["owner"]) >= 500          # the drop is seen


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_in_place_and_rectangle(svo, oracle, scene, frames, wanted, kernel):
    prm = svo.trace_params(shadow=True, kernel=KERNELS[kernel])
    got = stage1(svo, scene, prm, in_place=True)
    assert_words(got["owner"], wanted[0]["owner"], "in place: owner")
    assert_records(got["merged"], wanted[0]["merged"], "in place: merged")
    # off the origin, 100 pixels wide: rows do not end with a wave, the image not with a block
    rect = (20, 10, 100, 70)
    frame = scene["ow"].trace_image(scene["cam"], rect=rect, params=oracle.make_params(shadow=True), threads=8).reshape(-1)
    for max_rays in (ROOMY, 0):
        want = IM.trace(oracle, scene["om"], scene["box"], scene["cam"], rect, frame, scene["inst"], max_rays=max_rays)
        assert (want["owner"] != 0).sum() >= 1500 and want["counts"][0] > 7000
        got = stage1(svo, scene, prm, rect=rect, max_rays=max_rays, in_place=max_rays == 0)
        assert_gbuffer_equal(got["before"], frame, "svo_trace, rectangle")
        assert got["counts"] == want["counts"] and got["rays"] == want["cap"]
        assert_words(got["owner"], want["owner"], f"rectangle, max_rays {max_rays}: owner")
        assert_records(got["merged"], want["merged"], f"rectangle, max_rays {max_rays}: merged")
    crop = wanted[0]["owner"].reshape(H_, W_)[10:80, 20:120].reshape(-1)
    assert_words(IM.trace(oracle, scene["om"], scene["box"], scene["cam"], rect, frame, scene["inst"], max_rays=ROOMY)["owner"], crop, "rectangle = crop of the whole image")


def test_one_pixel_and_one_instance(svo, oracle, scene, frames):
    prm = svo.trace_params(shadow=True)
    for rect, inst in (((40, 30, 1, 1), scene["inst"]), ((0, 40, 128, 3), scene["inst"][1:2]), (FULL, scene["inst"][7:8])):
        frame = scene["ow"].trace_image(scene["cam"], rect=rect, params=oracle.make_params(shadow=True), threads=8).reshape(-1)
        want = IM.trace(oracle, scene["om"], scene["box"], scene["cam"], rect, frame, inst)
        got = stage1(svo, scene, prm, rect=rect, max_rays=0, inst=inst)
        assert got["counts"] == want["counts"] and got["rays"] == rect[2] * rect[3]
        assert_words(got["owner"], want["owner"], f"{rect}: owner")
        assert_records(got["merged"], want["merged"], f"{rect}: merged")
    assert got["counts"] == (0, 0) and not got["owner"].any()                            # the instance behind the camera


def shadow_floors(m1, s2):
    owned, c = m1["owner"] != 0, s2["considered"]
    lit = c & owned & ~s2["by_model"] & ~s2["by_scene"]
    assert (c & ~owned & s2["by_model"]).sum() >= 100, "scene pixels newly shadowed by an instance"
    assert (c & owned & s2["by_scene"]).sum() >= 100, "owned pixels shadowed by the terrain"
    assert (c & owned & s2["by_model"]).sum() >= 50, "owned pixels shadowed by an instance"
    assert lit.sum() >= 200 and s2["runaways"] == 0


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("semantics", [0, 1])
def test_stage2_equals_the_model(svo, oracle, scene, frames, wanted, kernel, semantics):
    """The shadow stage on stage 1's buffers, with bias = 0 (the march's eps) and with 1/256, and once with half the slots."""
    m1 = wanted[semantics]
    prm = svo.trace_params(shadow=True, kernel=KERNELS[kernel], semantics=semantics)
    structs = IM.instance_structs(svo, scene["inst"])
    for bias, cut in ((0.0, False), (IM.BIAS, False), (IM.BIAS, True)):
        full = IM.shadows(oracle, scene["ow"], scene["om"], scene["box"], scene["cam"], FULL, m1["merged"], m1["owner"], scene["inst"], semantics=semantics,
                          max_rays=ROOMY, bias=bias)
        shadow_floors(m1, full)
        max_rays = full["counts"][0] // 2 if cut else ROOMY
        want = IM.shadows(oracle, scene["ow"], scene["om"], scene["box"], scene["cam"], FULL, m1["merged"], m1["owner"], scene["inst"], semantics=semantics,
                          max_rays=max_rays, bias=bias) if cut else full
        if cut:
            assert np.count_nonzero(want["merged"]["flags"] != full["merged"]["flags"]) >= 100
        got = stage1(svo, scene, prm, keep=True)
        fr = got["frame"]
        assert_gbuffer_equal(got["before"], frames[semantics], "svo_trace, shadow = 1")
        assert_records(got["merged"], m1["merged"], "stage 1")
        fr.count.free()
        fr.count = svo.DeviceBuffer.from_numpy(np.full(2 + PAD, SENTINEL, np.uint32))
        scene["W"].trace_instance_shadows(scene["Mw"], scene["cam"], prm, FULL, structs, fr.merged.ptr, fr.owner.ptr, max_rays=max_rays, bias=bias,
                                          count_ptr=fr.count.ptr)
        model_rays, scene_rays = scene["Mw"].last_ray_count(), scene["W"].last_ray_count()
        svo.lib.svo_stream_synchronize(None)
        after, owner, counts = fr.records(fr.merged), fr.owners(), fr.counts()
        fr.free()
        what = f"stage 2, kernel {kernel} semantics {semantics} bias {bias} max_rays {max_rays}"
        assert counts == want["counts"] and model_rays == max_rays and scene_rays == N_, what
        assert_words(owner, m1["owner"], what + ": owner")
        assert_records(after, want["merged"], what)
        changed = after.view(np.uint8).reshape(N_, 32) != got["merged"].view(np.uint8).reshape(N_, 32)
        assert not changed[:, :18].any() and not changed[:, 20:].any(), what + ": a byte outside the flag word changed"
        assert not (changed[:, 18:20].any(axis=1) & ~want["considered"]).any(), what + ": a pixel that is not considered was written"
        assert np.all((after["flags"][want["considered"]] & IM.TRACED) != 0), what


def test_shading_the_merged_frame(svo, scene, wanted):
    """svo_shade takes no world: it runs on merged_dev as it stands, and gives the owned pixels the float64 model's colours within
    shade_model's own tolerance."""
    prm = svo.trace_params(shadow=True)
    got = stage1(svo, scene, prm, keep=True)
    fr = got["frame"]
    scene["W"].trace_instance_shadows(scene["Mw"], scene["cam"], prm, FULL, IM.instance_structs(svo, scene["inst"]), fr.merged.ptr, fr.owner.ptr, max_rays=ROOMY,
                                      bias=IM.BIAS)
    P = svo.shade_defaults()
    rgba = svo.DeviceBuffer(N_ * 16)
    svo.shade(scene["cam"], P, FULL, fr.merged.ptr, rgba.ptr)
    assert svo.lib.svo_stream_synchronize(None) == 0
    records, image = fr.records(fr.merged), rgba.to_numpy(np.float32, N_ * 4).reshape(N_, 4)
    rgba.free()
    fr.free()
    owned = wanted[0]["owner"] != 0
    want, cond = sm.shade(scene["cam"], P, FULL, records)
    assert np.array_equal(np.isnan(image[owned]), np.isnan(want[owned]))
    r = sm.within(image, want, cond, sm.K_GPU)[owned]
    assert owned.sum() >= 2000 and np.nanmax(r) <= 1.0, float(np.nanmax(r))
    lit = owned & ((records["flags"] & IM.SHADOWED) == 0)
    assert lit.sum() >= 200 and image[lit][:, :3].max() > 0.05


def test_refusals_on_the_device(svo, scene):
    cam, prm = scene["cam"], svo.trace_params()
    structs = IM.instance_structs(svo, scene["inst"])
    chunk = svo.chunk_from_grid(IM.model_grid(), (0.0, 0.0, 0.0), float(IM.MODEL_SIZE))
    host = svo.World.create([chunk], 1, 1, 1, IM.MODEL_SIZE)                                # never uploaded
    fake = 256
    for s, m in ((scene["W"], host), (host, scene["Mw"])):
        with pytest.raises(svo.SvoError) as e:
            s.trace_instances(m, cam, prm, FULL, fake, structs, fake, fake)
        assert e.value.code == NOT_UPLOADED
        with pytest.raises(svo.SvoError) as e:
            s.trace_instance_shadows(m, cam, prm, FULL, structs, fake, fake)
        assert e.value.code == NOT_UPLOADED
    with pytest.raises(svo.SvoError) as e:                                                  # the arguments still come first
        scene["W"].trace_instances(host, cam, prm, FULL, fake, structs * 5, fake, fake)
    assert e.value.code == INVALID
    for empty in ((0, 0, 0, 96), (5, 5, 0, 0)):                                             # an empty rectangle is SVO_OK and touches nothing
        scene["W"].trace_instances(scene["Mw"], cam, prm, empty, fake, structs, fake, fake)
        scene["W"].trace_instance_shadows(scene["Mw"], cam, prm, empty, structs, fake, fake)
    host.destroy()


def test_worlds_on_two_devices_are_refused(svo, scene):
    if svo.device_count() < 2:
        pytest.skip("one device: a second world cannot be resident elsewhere")
    chunk = svo.chunk_from_grid(IM.model_grid(), (0.0, 0.0, 0.0), float(IM.MODEL_SIZE))
    other = svo.World.create([chunk], 1, 1, 1, IM.MODEL_SIZE)
    other.upload(1)
    fake = 256
    with pytest.raises(svo.SvoError) as e:
        scene["W"].trace_instances(other, scene["cam"], svo.trace_params(), FULL, fake, IM.instance_structs(svo, scene["inst"]), fake, fake)
    assert e.value.code == INVALID
    other.destroy()
