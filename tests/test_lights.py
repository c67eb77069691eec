"""svo_trace_lights and svo_shade_lights on the GPU.

svo_trace_lights is specified in separately rounded float, so its words are compared whole with tests/lights_model.py: the pairs
rebuilt in numpy float32, marched by the unchanged CPU oracle, ranked, capped and dropped as include/svo.h says.  The scene is that of
tests/test_local_shadows.py with ten lights (lights_model.LIGHTS); the floors asserted on the model's own statistics keep the
comparison from passing vacuously.  svo_shade_lights runs on the synthetic G-buffer of tests/shade_model.py against the float64 model,
with that file's tolerance at K_GPU = 8 (never fitted to the kernel).  Largest |got - want| / tolerance measured on an MI355X: 0.067
(nine lights, no words); K needed: 0, the fixed terms 1e-6 + 2e-5 |want| cover the kernel's error.

Run as a script - python tests/test_lights.py <libsvo_*.so> - it puts one variant build of the library through the first case
(one library per process, as tests/variant_check.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lights_model as LM
import local_shadows_model as M
import shade_model as sm
from helpers import assert_gbuffer_equal

pytestmark = pytest.mark.gpu

KERNELS = {"stack": 2, "literal": 1}
WATER = 6
W_, H_ = 128, 96
N_ = W_ * H_
PAD = 64
SENTINEL = np.uint32(0xDEADBEEF)
LIT = (0, 1, 2, 3, 4, 7)                                    # the lights of the scene that are neither wholly occluded nor empty


@pytest.fixture(scope="module")
def scene(svo, oracle):
    if svo.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    W = svo.World.generate(2, 1, 2, 128, 8)
    chunks = [W.chunk(i) for i in range(4)]
    W.upload(0)
    ow = oracle.OracleWorld.from_chunks(chunks, 2, 1, 2, 128)
    yield W, ow, svo.default_camera(2, 2, 128, W_, H_)
    W.destroy()


@pytest.fixture(scope="module")
def frames(scene, oracle):
    """The oracle's svo_trace records of the whole image (shadow on) per semantics, computed once and never written."""
    _, ow, cam = scene
    out = {s: ow.trace_image(cam, params=oracle.make_params(shadow=True, semantics=s), threads=8) for s in (0, 1)}
    for f in out.values():
        f.setflags(write=False)
    return out


def run_gpu(svo, W, cam, rect, prm, lights, max_rays=0, records=None, translucent=False, stream=0, sync=True):
    """svo_trace (or svo_trace_translucent, or an upload of `records`), then svo_trace_lights: dict(before, after, words, counts, rays)."""
    n = rect[2] * rect[3]
    g = svo.DeviceBuffer.from_numpy(records) if records is not None else svo.DeviceBuffer(max(n, 1) * 32)
    if records is None and translucent:
        b = svo.DeviceBuffer(max(n, 1) * 32)
        W.trace_translucent(cam, prm, rect, g.ptr, b.ptr, stream=stream)
    elif records is None:
        W.trace(cam, prm, rect, g.ptr, stream=stream)
    svo.lib.svo_stream_synchronize(stream or None)
    before = g.to_numpy(svo.HIT_DTYPE, n)
    if records is None and translucent:
        b.free()
    vis = svo.DeviceBuffer.from_numpy(np.full(n + PAD, SENTINEL, np.uint32))
    cnt = svo.DeviceBuffer.from_numpy(np.full(2 + PAD, SENTINEL, np.uint32))
    W.trace_lights(cam, prm, rect, g.ptr, LM.light_structs(svo, lights), vis.ptr, max_rays=max_rays, count_ptr=cnt.ptr, stream=stream)
    rays = W.last_ray_count(stream)
    svo.lib.svo_stream_synchronize(stream or None)
    words, counts, after = vis.to_numpy(np.uint32, n + PAD), cnt.to_numpy(np.uint32, 2 + PAD), g.to_numpy(svo.HIT_DTYPE, n)
    for buf in (g, vis, cnt):
        buf.free()
    assert np.all(words[n:] == SENTINEL), "svo_trace_lights wrote past w*h words"
    assert np.all(counts[2:] == SENTINEL), "svo_trace_lights wrote past the two counts"
    assert np.array_equal(before.view(np.uint8), after.view(np.uint8)), "svo_trace_lights wrote to the G-buffer"
    return dict(before=before, words=words[:n], counts=(int(counts[0]), int(counts[1])), rays=rays)


def assert_words(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[:6]}: got {[hex(x) for x in got[bad[:6]]]} want {[hex(x) for x in want[bad[:6]]]}"


def check_floors(stats):
    """The issue's floors, on the model's own statistics of the unbounded list."""
    for j in LIT:
        assert stats[j]["occluded"] >= 100 and stats[j]["visible"] >= 500, (j, stats[j])
    for j, s in enumerate(stats):
        if j < 8:                                           # (light 8 reaches two back-facing hits and nothing else, light 9 about a hundred)
            assert s["backfacing"] >= 200, (j, s)
        assert s["runaways"] == 0 and s["nearest"] > 1e-3, (j, s)
    assert stats[8]["pairs"] == 0 and all(stats[j]["visible"] == 0 and stats[j]["pairs"] > 0 for j in (5, 6, 9))


def words_case(svo, oracle, W, ow, cam, frame, kernel, semantics):
    rect = (0, 0, cam.width, cam.height)
    n = cam.width * cam.height
    want = LM.trace(oracle, ow, cam, rect, frame, LM.LIGHTS, semantics=semantics, max_rays=10 * n)
    print(f"kernel {kernel} semantics {semantics}: usable {want['usable']} pairs {want['counts']} {want['stats']}")
    check_floors(want["stats"])
    got = run_gpu(svo, W, cam, rect, svo.trace_params(shadow=True, kernel=kernel, semantics=semantics), LM.LIGHTS, max_rays=10 * n)
    assert_gbuffer_equal(got["before"], frame, "svo_trace")
    assert_words(got["words"], want["words"], f"kernel {kernel} semantics {semantics}")
    assert got["counts"] == want["counts"] and want["counts"][0] == want["counts"][1]
    assert got["rays"] == 10 * n
    return want


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("semantics", [0, 1])
def test_words_equal_the_model(svo, oracle, scene, frames, kernel, semantics):
    W, ow, cam = scene
    want = words_case(svo, oracle, W, ow, cam, frames[semantics], KERNELS[kernel], semantics)
    if semantics == 0:
        assert want["usable"] == 7087 and want["counts"][0] == 19123
        assert [s["pairs"] for s in want["stats"]] == [1177, 1614, 5976, 684, 2843, 33, 287, 6371, 0, 138]


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_overflow(svo, oracle, scene, frames, kernel):
    """Pairs without a slot are not marched and count as lit: the default cap (one slot per pixel), one slot, exactly enough slots."""
    W, ow, cam = scene
    rect = (0, 0, W_, H_)
    prm = svo.trace_params(shadow=True, kernel=KERNELS[kernel])
    want = LM.trace(oracle, ow, cam, rect, frames[0], LM.LIGHTS)
    assert want["counts"] == (19123, 12288) and want["stats"][4]["dropped"] == 6 and all(want["stats"][j]["dropped"] == want["stats"][j]["pairs"] for j in (5, 6, 7, 9))
    got = run_gpu(svo, W, cam, rect, prm, LM.LIGHTS)
    assert_words(got["words"], want["words"], "default cap")
    assert got["counts"] == (19123, 12288) and got["rays"] == N_
    full = LM.trace(oracle, ow, cam, rect, frames[0], LM.LIGHTS, max_rays=19123)
    assert np.count_nonzero(full["words"] != want["words"]) >= 1000         # the dropped pairs of lights 5, 6, 7 and 9 are lit, and were occluded
    for max_rays in (1, 19123, 19122):
        want = LM.trace(oracle, ow, cam, rect, frames[0], LM.LIGHTS, max_rays=max_rays)
        got = run_gpu(svo, W, cam, rect, prm, LM.LIGHTS, max_rays=max_rays)
        assert_words(got["words"], want["words"], f"max_rays {max_rays}")
        assert got["counts"] == (19123, min(19123, max_rays)) == want["counts"] and got["rays"] == max_rays


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_against_local_shadows(svo, oracle, scene, kernel):
    """No oracle march: one light whose reach holds everything sees what svo_trace_local_shadows' point light sees, on the facing hits."""
    W, ow, cam = scene
    rect = (0, 0, W_, H_)
    prm = svo.trace_params(shadow=True, kernel=KERNELS[kernel])
    got = run_gpu(svo, W, cam, rect, prm, [(M.POINT, 1e4)], max_rays=N_)
    g = svo.DeviceBuffer(N_ * 32)
    W.trace(cam, prm, rect, g.ptr)
    W.trace_local_shadows(cam, prm, rect, g.ptr, point=M.POINT)
    svo.lib.svo_stream_synchronize(None)
    rec = g.to_numpy(svo.HIT_DTYPE, N_)
    g.free()
    o, d = M.camera_rays(oracle, cam, rect)
    sel = M.usable(rec)
    pair, back, _ = LM.MODEL.pairs(M.sample_points(o, d, rec, M.resolved_eps(0)), rec["normal"].astype(np.float32), sel, [(M.POINT, 1e4)])
    assert np.array_equal(pair[0] | back[0], sel) and back[0].sum() >= 500 and pair[0].sum() >= 2000
    want = pair[0] & ((rec["flags"] & M.SHADOWED_POINT) == 0)
    assert 500 <= want.sum() <= pair[0].sum() - 500
    assert_words(got["words"], want.astype(np.uint32), "bit 0 against svo_trace_local_shadows")


def many_lights():
    """32 lights: the ten of the scene and 22 copies of the six lit ones, shifted by seeded offsets."""
    rng = np.random.default_rng(32)
    lights = list(LM.LIGHTS)
    while len(lights) < 32:
        (x, y, z), reach = LM.LIGHTS[LIT[len(lights) % len(LIT)]]
        dx, dy, dz = rng.uniform(-12.0, 12.0, 3)
        lights.append(((float(np.float32(x + dx)), float(np.float32(y + abs(dy))), float(np.float32(z + dz))), reach))
    return lights


def test_bit_31(svo, oracle, scene, frames):
    W, ow, cam = scene
    rect = (0, 0, W_, H_)
    lights = many_lights()
    want = LM.trace(oracle, ow, cam, rect, frames[0], lights, max_rays=32 * N_)
    got = run_gpu(svo, W, cam, rect, svo.trace_params(shadow=True), lights, max_rays=32 * N_)
    assert_words(got["words"], want["words"], "32 lights")
    assert got["counts"] == want["counts"] and got["rays"] == 32 * N_
    assert np.count_nonzero(got["words"] & np.uint32(1 << 31)) >= 100
    assert all(s["runaways"] == 0 for s in want["stats"])
    # and with the default cap: the later lights have no slots
    want = LM.trace(oracle, ow, cam, rect, frames[0], lights)
    got = run_gpu(svo, W, cam, rect, svo.trace_params(shadow=True), lights)
    assert want["counts"][0] > 3 * N_ and want["stats"][31]["dropped"] == want["stats"][31]["pairs"] >= 100
    assert_words(got["words"], want["words"], "32 lights, default cap")


def test_permutation(svo, scene):
    """Without overflow a light's bit does not depend on its place in the list."""
    W, _, cam = scene
    rect = (0, 0, W_, H_)
    prm = svo.trace_params(shadow=True)
    a = run_gpu(svo, W, cam, rect, prm, LM.LIGHTS, max_rays=10 * N_)["words"]
    b = run_gpu(svo, W, cam, rect, prm, LM.LIGHTS[::-1], max_rays=10 * N_)["words"]
    back = np.zeros(N_, np.uint32)
    for j in range(10):
        back |= ((b >> np.uint32(9 - j)) & np.uint32(1)) << np.uint32(j)
    assert np.count_nonzero(a) >= 3000
    assert_words(back, a, "reversed list")


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_rectangle_is_a_crop(svo, oracle, scene, frames, kernel):
    W, ow, cam = scene
    rect = (24, 16, 72, 56)
    prm = svo.trace_params(shadow=True, kernel=KERNELS[kernel])
    frame = ow.trace_image(cam, rect=rect, params=oracle.make_params(shadow=True), threads=8)
    want = LM.trace(oracle, ow, cam, rect, frame, LM.LIGHTS, max_rays=10 * 72 * 56)
    assert sum(s["visible"] for s in want["stats"]) >= 1000 and sum(s["occluded"] for s in want["stats"]) >= 1000
    got = run_gpu(svo, W, cam, rect, prm, LM.LIGHTS, max_rays=10 * 72 * 56)
    assert_words(got["words"], want["words"], "rectangle")
    whole = run_gpu(svo, W, cam, (0, 0, W_, H_), prm, LM.LIGHTS, max_rays=10 * N_)["words"]
    assert_words(got["words"], whole.reshape(H_, W_)[16:72, 24:96].reshape(-1), "rectangle = crop of the whole image")


@pytest.mark.parametrize("width,rect", [(W_, (64, 70, 1, 1)), (W_, (62, 68, 3, 5)), (130, (0, 70, 130, 1)), (300, (0, 52, 300, 1)), (W_, (0, 40, 128, 5))],
                         ids=["1x1", "3x5", "130x1", "300x1", "128x5"])
def test_shapes(svo, oracle, scene, width, rect):
    """One pixel, a few, and strips that end 2 lanes into a wave's third (130) and 44 threads into a second block (300): the wave and
    block edges of the rank, with every cap from none to all."""
    W, ow, _ = scene
    cam = svo.default_camera(2, 2, 128, width, H_)
    n = rect[2] * rect[3]
    frame = ow.trace_image(cam, rect=rect, params=oracle.make_params(shadow=True), threads=8)
    assert M.usable(frame).sum() >= 1
    prm = svo.trace_params(shadow=True)
    total = LM.trace(oracle, ow, cam, rect, frame, LM.LIGHTS, max_rays=10 * n)["counts"][0]
    assert total >= 2
    for max_rays in (10 * n, 0, total // 2 + 1):
        want = LM.trace(oracle, ow, cam, rect, frame, LM.LIGHTS, max_rays=max_rays)
        got = run_gpu(svo, W, cam, rect, prm, LM.LIGHTS, max_rays=max_rays)
        assert_words(got["words"], want["words"], f"{rect} max_rays {max_rays}")
        assert got["counts"] == want["counts"] and got["rays"] == want["cap"]


def test_one_light(svo, oracle, scene, frames):
    W, ow, cam = scene
    rect = (0, 0, W_, H_)
    for j in (2, 8):                                        # a light with many pairs, and the one with none
        want = LM.trace(oracle, ow, cam, rect, frames[0], LM.LIGHTS[j:j + 1])
        got = run_gpu(svo, W, cam, rect, svo.trace_params(shadow=True), LM.LIGHTS[j:j + 1])
        assert_words(got["words"], want["words"], f"light {j} alone")
        assert got["counts"] == want["counts"] and got["rays"] == N_ and np.all(got["words"] <= 1)
    assert got["counts"] == (0, 0)


def test_nan_normals(svo, oracle, scene, frames):
    """A NaN normal (the SVO_NORMAL_CUBE hit whose integer vector is zero) faces every light."""
    W, ow, cam = scene
    rect = (0, 0, W_, H_)
    frame = np.array(frames[0], copy=True).reshape(-1)
    rng = np.random.default_rng(200)
    pick = rng.choice(np.nonzero(M.usable(frame))[0], 200, replace=False)
    frame["normal"][pick] = np.float32(np.nan)
    frame["normal"][pick[:50], 1] = 1.0                     # NaN in some components only
    want = LM.trace(oracle, ow, cam, rect, frame, LM.LIGHTS, max_rays=10 * N_)
    plain = LM.trace(oracle, ow, cam, rect, frames[0], LM.LIGHTS, max_rays=10 * N_)
    o, d = M.camera_rays(oracle, cam, rect)
    P = M.sample_points(o, d, frame, M.resolved_eps(0))
    for j, (position, reach) in enumerate(LM.LIGHTS):       # those pixels are pairs of every light in reach
        _, q = LM.light_vectors(P, position)
        assert np.array_equal(want["pair"][j][pick], q[pick] <= np.float32(reach) * np.float32(reach)), j
    assert want["pair"][:, pick].sum() >= plain["pair"][:, pick].sum() + 100
    got = run_gpu(svo, W, cam, rect, svo.trace_params(shadow=True), LM.LIGHTS, max_rays=10 * N_, records=frame)
    assert_words(got["words"], want["words"], "NaN normals")
    assert got["counts"] == want["counts"]


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_see_through_water(svo, oracle, scene, frames, kernel):
    """Light 5 sits in the lake: the water is what hides it, see_through is what shows it."""
    W, ow, cam = scene
    rect = (0, 0, W_, H_)
    ow6 = oracle.OracleWorld.from_chunks([svo.see_through_chunk(W.chunk(i), WATER) for i in range(4)], 2, 1, 2, 128)
    frame = ow6.trace_image(cam, params=oracle.make_params(shadow=True), threads=8)
    want = LM.trace(oracle, ow6, cam, rect, frame, LM.LIGHTS, max_rays=10 * N_)
    plain = LM.trace(oracle, ow, cam, rect, frames[0], LM.LIGHTS, max_rays=10 * N_)
    assert plain["stats"][5]["visible"] == 0 and want["stats"][5]["visible"] >= 20
    got = run_gpu(svo, W, cam, rect, svo.trace_params(shadow=True, kernel=KERNELS[kernel], see_through=WATER), LM.LIGHTS, max_rays=10 * N_)
    assert_gbuffer_equal(got["before"], frame, "svo_trace, see_through")
    assert_words(got["words"], want["words"], f"see_through {kernel}")
    assert np.count_nonzero(got["words"] & 32) >= 20


def test_translucent_surface_records(svo, oracle, scene):
    W, _, cam = scene
    rect = (0, 0, W_, H_)
    prm = svo.trace_params(shadow=True, see_through=WATER)
    got = run_gpu(svo, W, cam, rect, prm, LM.LIGHTS, max_rays=10 * N_, translucent=True)
    assert np.count_nonzero(got["before"]["flags"] & svo.SEE_THROUGH) > 500
    ow6 = oracle.OracleWorld.from_chunks([svo.see_through_chunk(W.chunk(i), WATER) for i in range(4)], 2, 1, 2, 128)
    want = LM.trace(oracle, ow6, cam, rect, got["before"], LM.LIGHTS, max_rays=10 * N_)      # marched with the caller's params: through the water
    assert_words(got["words"], want["words"], "translucent surface")
    assert got["counts"] == want["counts"]


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_frame_without_shadow_rays(svo, oracle, scene, frames, kernel):
    W, ow, cam = scene
    rect = (0, 0, W_, H_)
    frame = ow.trace_image(cam, params=oracle.make_params(shadow=False), threads=8)
    assert np.count_nonzero(frame["flags"] & M.SHADOWED) == 0 and np.count_nonzero(frames[0]["flags"] & M.SHADOWED) > 1000
    want = LM.trace(oracle, ow, cam, rect, frame, LM.LIGHTS, max_rays=10 * N_)
    got = run_gpu(svo, W, cam, rect, svo.trace_params(shadow=False, kernel=KERNELS[kernel]), LM.LIGHTS, max_rays=10 * N_)
    assert_gbuffer_equal(got["before"], frame, "svo_trace, shadow = 0")
    assert_words(got["words"], want["words"], f"shadow = 0, {kernel}")
    assert_words(got["words"], LM.trace(oracle, ow, cam, rect, frames[0], LM.LIGHTS, max_rays=10 * N_)["words"], "the words do not depend on the frame's shadow flags")


def test_two_streams_share_the_scratch(svo, oracle, scene):
    """Four frames (svo_trace, then svo_trace_lights behind it) on two streams, nothing in between: the lists, their records and the
    ranks live in one scratch of the world.  Job A has ten lights and ten slots per pixel, job B three lights and the default cap,
    so the two lay the scratch out differently, and they look through different cameras (tests/test_local_shadows.py's, 64 x 48)."""
    W, ow, _ = scene
    hip = C.CDLL("libamdhip64.so.7")                        # the runtime the library is already linked against
    w, h = 64, 48
    rect, n = (0, 0, w, h), w * h
    jobs_of = {"A": (svo.default_camera(2, 2, 128, w, h), LM.LIGHTS, 10 * n),
               "B": (svo.make_camera((20.0, 50.0, 64.0), (0.7, -0.7, 0.0), (0.0, 1.0, 0.0), 60.0, w, h), LM.LIGHTS[:3], 0)}
    prm = svo.trace_params(shadow=True)

    def issue(which, stream=0):
        cam, lights, max_rays = jobs_of[which]
        g, vis = svo.DeviceBuffer(n * 32), svo.DeviceBuffer.from_numpy(np.full(n, SENTINEL, np.uint32))
        W.trace(cam, prm, rect, g.ptr, stream=stream)
        W.trace_lights(cam, prm, rect, g.ptr, LM.light_structs(svo, lights), vis.ptr, max_rays=max_rays, stream=stream)
        return g, vis

    def fetch(bufs):
        out = bufs[1].to_numpy(np.uint32, n)
        for b in bufs:
            b.free()
        return out

    single = {}
    for which, (cam, lights, max_rays) in jobs_of.items():
        bufs = issue(which)
        svo.lib.svo_stream_synchronize(None)
        single[which] = fetch(bufs)
        frame = ow.trace_image(cam, params=oracle.make_params(shadow=True), threads=8)
        want = LM.trace(oracle, ow, cam, rect, frame, lights, max_rays=max_rays)
        assert want["counts"][0] >= 500, which
        assert_words(single[which], want["words"], f"single stream, job {which}")
    streams = []
    for _ in range(2):
        s = C.c_void_p()
        assert hip.hipStreamCreateWithFlags(C.byref(s), 1) == 0            # hipStreamNonBlocking
        streams.append(s.value)
    jobs = [(which, issue(which, stream=streams[k % 2])) for k, which in enumerate(("B", "A", "A", "B"))]
    for s in streams:
        svo.lib.svo_stream_synchronize(s)
    for which, bufs in jobs:
        assert_words(fetch(bufs), single[which], f"two streams, job {which}")
    for s in streams:
        hip.hipStreamDestroy(C.c_void_p(s))


def test_across_a_world_change(svo, oracle):
    W = svo.World.generate(2, 1, 2, 128, 8)
    W.upload(0)
    cam = svo.default_camera(2, 2, 128, W_, H_)
    rect = (0, 0, W_, H_)

    def check(what):
        ow = oracle.OracleWorld.from_chunks([W.chunk(i) for i in range(4)], 2, 1, 2, 128)
        frame = ow.trace_image(cam, params=oracle.make_params(shadow=True), threads=8)
        want = LM.trace(oracle, ow, cam, rect, frame, LM.LIGHTS, max_rays=10 * N_)
        for kernel in (2, 1):
            got = run_gpu(svo, W, cam, rect, svo.trace_params(shadow=True, kernel=kernel), LM.LIGHTS, max_rays=10 * N_)
            assert_words(got["words"], want["words"], f"{what} kernel {kernel}")
        return frame.reshape(-1), want["words"]

    f0, w0 = check("fresh")
    # a wall across chunk 0, between the terrain west of it and light 2
    W.edit_box(0, svo.EDIT_BUILD, (90.0, 0.0, 0.0), (94.0, 127.0, 127.0), 5)
    f1, w1 = check("after edit_box")
    same = M.usable(f0) & (f0["t"].view(np.uint32) == f1["t"].view(np.uint32)) & (f0["node"] == f1["node"])
    newly = same & ((w0 & 4) != 0) & ((w1 & 4) == 0)
    assert newly.sum() >= 200, newly.sum()                  # terrain the camera still sees, now in the wall's shadow
    W.destroy()


def test_variants(svo, oracle):
    """The first case through every library of `make variants` (SVO_AMD_LIB; one library per process, one after the other)."""
    from test_variants import VARIANTS, lib_of
    for name in sorted({n for n, _ in VARIANTS}):
        assert os.path.exists(lib_of(name)), f"{lib_of(name)} missing: __graft_entry__.build() makes it"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), lib_of(name)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, name + "\n" + r.stdout[-3000:] + r.stderr[-3000:]


# ---- svo_shade_lights on the synthetic G-buffer ------------------------------------------------------------------------------
FSENT = np.float32(-12345.678)


@pytest.fixture(scope="module")
def shading(svo):
    """(cam, params, rect, records, lights, base image, masks): shade_model's general buffer under the custom material table; eight
    lights beside sample points of every depth, with reaches from 6 to 200, and a ninth whose reach is its distance from one pixel."""
    cam, P, rect, g = sm.general_case(svo, dict())
    assert tuple(float(m.shininess) for m in P.materials) == sm.CUSTOM_SHININESS and rect == sm.RECT
    n = rect[2] * rect[3]
    rng = np.random.default_rng(77)
    p = sm.terms(cam, P, rect, g)["p"]
    hit = np.nonzero(((g["flags"] & sm.HIT) != 0) & ~np.isnan(g["normal"]).any(axis=1))[0]
    order = hit[np.argsort(g["t"][hit])]
    lights = []
    for i, reach in enumerate((6.0, 12.0, 25.0, 40.0, 60.0, 90.0, 120.0, 200.0)):
        k = order[(2 * i + 1) * order.size // 16]
        pos = [float(np.float32(c)) for c in p[k] + rng.normal(size=3) * 0.25 * reach]
        lights.append(svo.Light(pos, reach, ambient=rng.uniform(0.0, 0.2, 3), diffuse=rng.uniform(0.2, 1.0, 3), specular=rng.uniform(0.2, 1.0, 3),
                                attenuation=(1.0, float(rng.uniform(0.0, 0.1)), float(rng.uniform(0.0, 0.02)))))
    kb = int(order[order.size // 3])
    pos = np.array([np.float32(c) for c in p[kb] + np.array([6.0, 8.0, 0.0])], np.float64)
    lights.append(svo.Light([float(c) for c in pos], float(np.float32(np.sqrt(((pos - p[kb]) ** 2).sum()))), ambient=(0.3, 0.3, 0.3), diffuse=(1.0, 1.0, 1.0),
                            specular=(1.0, 1.0, 1.0), attenuation=(1.0, 0.0, 0.0)))
    base = rng.uniform(0.0, 1.0, (n, 4)).astype(np.float32)
    masks = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return cam, P, rect, g, lights, base, masks, kb


def _shade_lights(svo, cam, P, rect, g, lights, base, masks):
    n = rect[2] * rect[3]
    src = svo.DeviceBuffer.from_numpy(g)
    out = svo.DeviceBuffer.from_numpy(np.concatenate([base.reshape(-1), np.full(PAD * 4, FSENT, np.float32)]))
    vis = svo.DeviceBuffer.from_numpy(masks) if masks is not None else None
    svo.shade_lights(cam, P, rect, src.ptr, lights, out.ptr, visible_ptr=vis.ptr if vis else None)
    assert svo.lib.svo_stream_synchronize(None) == 0
    got = out.to_numpy(np.float32, (n + PAD) * 4)
    for b in (src, out) + ((vis,) if vis else ()):
        b.free()
    assert np.all(got[n * 4:] == FSENT), "wrote past w*h pixels"
    return got[:n * 4].reshape(n, 4)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_shade(got, base, add, cond, g, what, capsys):
    hit = (np.asarray(g).reshape(-1)["flags"] & sm.HIT) != 0
    want = base.astype(np.float64)
    want[:, :3] += add
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN elsewhere than the model's"
    assert np.array_equal(_bits(got[:, 3]), _bits(base[:, 3])), f"{what}: a depth float was written"
    assert np.array_equal(_bits(got[~hit]), _bits(base[~hit])), f"{what}: a miss was written"
    r = sm.within(got, want, cond, sm.K_GPU)
    worst = float(np.nanmax(r))
    with capsys.disabled():
        print(f"\n  {what:52s} |got - want| / tolerance(K={sm.K_GPU}) <= {worst:.3f}   K needed {sm.needed_K(got, want, cond):.3f}", end="")
    k = np.unravel_index(np.nanargmax(r), r.shape)
    assert worst <= 1.0, f"{what}: record {k[0]} component {k[1]} got {got[k]} want {want[k]} cond {cond[k[0]]}"


def test_shade_lights_matches_model(svo, shading, capsys):
    cam, P, rect, g, lights, base, masks, kb = shading
    hit = (g["flags"] & sm.HIT) != 0
    add, cond, ratio = LM.shade_lights(cam, P, rect, g, lights, masks)
    with np.errstate(invalid="ignore"):
        assert np.nanmin(ratio) < 0.05 and np.nanmax(ratio) > 1.5
        assert all(20 <= np.count_nonzero(ratio[j] < 1.0) for j in range(9)) and all(200 <= np.count_nonzero(ratio[j] > 1.0) for j in range(7))
        for lo, hi in ((0.0, 0.25), (0.25, 0.5), (0.5, 0.75), (0.75, 1.0), (1.0, 1.5)):
            assert np.count_nonzero((ratio > lo) & (ratio <= hi)) >= 100
    assert abs(ratio[8][kb] - 1.0) < 1e-6
    assert np.isnan(add).any() and (cond > 0).mean() > 0.3
    got = _shade_lights(svo, cam, P, rect, g, lights, base, masks)
    _check_shade(got, base, add, cond, g, "svo_shade_lights, random masks", capsys)
    assert np.count_nonzero((_bits(got[:, :3]) != _bits(base[:, :3])).any(axis=1)) >= 1000
    # beyond every reach the pixel keeps its bits, whatever its word says (the five small lights: the largest reaches every pixel)
    add, cond, ratio = LM.shade_lights(cam, P, rect, g, lights[:5], masks)
    with np.errstate(invalid="ignore"):
        outside = hit & np.all(ratio > 1.0 + 1e-5, axis=0)
    assert outside.sum() >= 500 and (hit & ~outside).sum() >= 500
    got = _shade_lights(svo, cam, P, rect, g, lights[:5], base, masks)
    _check_shade(got, base, add, cond, g, "svo_shade_lights, five lights", capsys)
    assert np.array_equal(_bits(got[outside]), _bits(base[outside]))


def test_shade_lights_null_words_mean_unshadowed(svo, shading, capsys):
    cam, P, rect, g, lights, base, masks, _ = shading
    ones = _shade_lights(svo, cam, P, rect, g, lights, base, np.full(masks.shape, 0xFFFFFFFF, np.uint32))
    null = _shade_lights(svo, cam, P, rect, g, lights, base, None)
    assert np.array_equal(_bits(null), _bits(ones))
    add, cond, _ = LM.shade_lights(cam, P, rect, g, lights, None)
    _check_shade(null, base, add, cond, g, "svo_shade_lights, no words", capsys)


def test_shade_lights_zero_words_leave_the_ambient_terms(svo, shading, capsys):
    cam, P, rect, g, lights, base, masks, _ = shading
    got = _shade_lights(svo, cam, P, rect, g, lights, base, np.zeros(masks.shape, np.uint32))
    add, cond, _ = LM.shade_lights(cam, P, rect, g, lights, np.zeros(masks.shape, np.uint32))
    assert np.all(cond == 0.0)
    _check_shade(got, base, add, cond, g, "svo_shade_lights, words of zero", capsys)
    dark = [svo.Light(tuple(L.position), L.reach, ambient=tuple(L.ambient), attenuation=(L.constant, L.linear, L.quadratic)) for L in lights]
    only_ambient, _, _ = LM.shade_lights(cam, P, rect, g, dark, None)
    finite = ~np.isnan(add).any(axis=1)
    assert np.allclose(add[finite], only_ambient[finite], rtol=1e-12, atol=0.0) and np.any(add[finite] > 1e-3)


def test_shade_lights_one_light_and_thin_rectangles(svo, shading, capsys):
    cam, P, rect, g, lights, base, masks, _ = shading
    add, cond, _ = LM.shade_lights(cam, P, rect, g, lights[5:6], masks)
    assert np.count_nonzero(np.nan_to_num(add)) >= 300
    _check_shade(_shade_lights(svo, cam, P, rect, g, lights[5:6], base, masks), base, add, cond, g, "svo_shade_lights, one light", capsys)
    for rect in ((57, 31, 1, 1), (130, 0, 1, 97), (0, 96, 131, 1)):
        n = rect[2] * rect[3]
        gg = g[7:7 + n].copy()
        gg["flags"][0] |= sm.HIT
        gg["normal"][0] = sm.cube_normals()[4]
        add, cond, _ = LM.shade_lights(cam, P, rect, gg, lights, masks[:n])
        assert n == 1 or np.count_nonzero(np.nan_to_num(add)) >= 10
        got = _shade_lights(svo, cam, P, rect, gg, lights, base[:n], masks[:n])
        _check_shade(got, base[:n], add, cond, gg, f"svo_shade_lights {rect}", capsys)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from variant_check import load
    svo_, ob_ = load(os.path.abspath(sys.argv[1]))
    if svo_.device_count() < 1:
        print("no HIP device")
        sys.exit(3)
    W0 = svo_.World.generate(2, 1, 2, 128, 8)
    chunks0 = [W0.chunk(i) for i in range(4)]
    W0.upload(0)
    ow0 = ob_.OracleWorld.from_chunks(chunks0, 2, 1, 2, 128)
    cam0 = svo_.default_camera(2, 2, 128, W_, H_)
    for semantics_ in (0, 1):
        frame0 = ow0.trace_image(cam0, params=ob_.make_params(shadow=True, semantics=semantics_), threads=8)
        for kernel_ in (2, 1):
            words_case(svo_, ob_, W0, ow0, cam0, frame0, kernel_, semantics_)
    W0.destroy()
    print("light lists: words equal to the model's")
