"""svo_trace_local_shadows on the GPU: one shadow flag per local light (SVO_SHADOWED_POINT / SVO_SHADOWED_SPOT), checked record for
record against the unchanged CPU oracle (tests/local_shadows_model.py rebuilds the occlusion rays in numpy float32, marches them with
ow.trace_rays and applies the `t < dist` rule), and svo_shade's use of the flags against sums of oracle.shade_image runs.

Run as a script - python tests/test_local_shadows.py <libsvo_*.so> - it puts one variant build of the library through the flags case
(one library per process, as tests/variant_check.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import local_shadows_model as M
from helpers import assert_gbuffer_equal
from test_shading import ATOL, RTOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"stack": 2, "literal": 1}
WATER = 6
W_, H_ = 128, 96
BITS = M.SHADOWED_POINT | M.SHADOWED_SPOT
ROCK = (100.3, 40.0, 100.3)                                    # 20 units under the terrain's surface
UNDER_WATER = (64.5, 3.0, 64.5)                                 # in the lake: below the water level (6), above the lake bed


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


def run_gpu(svo, W, cam, rect, prm, point, spot, translucent=False):
    """svo_trace (or svo_trace_translucent), then svo_trace_local_shadows: (records before, records after, rays of the second call[, behind before, behind after])."""
    n = rect[2] * rect[3]
    g, b = svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 32)
    if translucent:
        W.trace_translucent(cam, prm, rect, g.ptr, b.ptr)
    else:
        W.trace(cam, prm, rect, g.ptr)
    svo.lib.svo_stream_synchronize(None)
    before, behind0 = g.to_numpy(svo.HIT_DTYPE, n), b.to_numpy(svo.HIT_DTYPE, n)
    W.trace_local_shadows(cam, prm, rect, g.ptr, point=point, spot=spot)
    rays = W.last_ray_count()
    after, behind1 = g.to_numpy(svo.HIT_DTYPE, n), b.to_numpy(svo.HIT_DTYPE, n)
    g.free()
    b.free()
    return (before, after, rays, behind0, behind1) if translucent else (before, after, rays)


def check_untouched(before, after):
    """Records without a usable hit are byte-identical; of the others only the flag bits 5-7 may differ."""
    sel = M.usable(before)
    assert np.array_equal(before[~sel].view(np.uint8), after[~sel].view(np.uint8))
    a, b = after.copy(), before.copy()
    a["flags"] &= np.uint16(0xFFFF ^ (BITS | M.LOCAL_SHADOWS))
    b["flags"] &= np.uint16(0xFFFF ^ (BITS | M.LOCAL_SHADOWS))
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert np.all((after["flags"][sel] & M.LOCAL_SHADOWS) != 0)


def flags_case(svo, oracle, W, ow, cam, kernel, semantics, shadow):
    rect = (0, 0, cam.width, cam.height)
    frame = ow.trace_image(cam, params=oracle.make_params(shadow=shadow, semantics=semantics), threads=8)
    stats = {}
    want = M.expected(oracle, ow, cam, rect, frame, M.POINT, M.SPOT, semantics, stats)
    print(f"kernel {kernel} semantics {semantics} shadow {shadow}: {stats}")
    for light, s in stats.items():              # the inputs keep the comparison from passing vacuously (the oracle's own result)
        assert s["occluded"] >= 0.10 and s["lit"] >= 0.10, (light, s)
        assert s["behind"] >= 500, (light, s)
        assert s["differs"] >= 0.30, (light, s)
        assert s["runaways"] == 0 and s["nearest"] > 1e-3, (light, s)
    before, after, rays = run_gpu(svo, W, cam, rect, svo.trace_params(shadow=shadow, kernel=kernel, semantics=semantics), M.POINT, M.SPOT)
    assert_gbuffer_equal(before, frame, "svo_trace")
    assert_gbuffer_equal(after, want, f"local shadows kernel {kernel} semantics {semantics} shadow {shadow}")
    check_untouched(before, after)
    assert rays == 2 * cam.width * cam.height


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("semantics", [0, 1])
def test_flags(svo, oracle, scene, kernel, shadow, semantics):
    W, ow, cam = scene
    flags_case(svo, oracle, W, ow, cam, KERNELS[kernel], semantics, shadow)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_one_light_only(svo, oracle, scene, kernel):
    W, ow, cam = scene
    rect = (0, 0, W_, H_)
    prm = svo.trace_params(shadow=True, kernel=KERNELS[kernel])
    frame = ow.trace_image(cam, params=oracle.make_params(shadow=True), threads=8)
    for point, spot, copied in ((M.POINT, None, M.SHADOWED_SPOT), (None, M.SPOT, M.SHADOWED_POINT)):
        before, after, rays = run_gpu(svo, W, cam, rect, prm, point, spot)
        assert_gbuffer_equal(after, M.expected(oracle, ow, cam, rect, frame, point, spot, 0), f"one light {kernel}")
        assert np.array_equal((after["flags"] & copied) != 0, (after["flags"] & M.SHADOWED) != 0)
        assert np.count_nonzero(after["flags"] & copied) > 1000
        assert rays == W_ * H_
        check_untouched(before, after)
    buf = svo.DeviceBuffer(W_ * H_ * 32)
    with pytest.raises(svo.SvoError) as e:
        W.trace_local_shadows(cam, prm, rect, buf.ptr)
    assert e.value.code == -1
    buf.free()


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_rectangle(svo, oracle, scene, kernel):
    W, ow, cam = scene
    rect = (24, 16, 72, 56)
    frame = ow.trace_image(cam, rect=rect, params=oracle.make_params(shadow=True), threads=8)
    stats = {}
    want = M.expected(oracle, ow, cam, rect, frame, M.POINT, M.SPOT, 0, stats)
    assert all(s["occluded"] > 0.05 and s["lit"] > 0.05 for s in stats.values()), stats
    before, after, rays = run_gpu(svo, W, cam, rect, svo.trace_params(shadow=True, kernel=KERNELS[kernel]), M.POINT, M.SPOT)
    assert_gbuffer_equal(after, want, f"rectangle {kernel}")
    assert rays == 2 * 72 * 56
    # the same pixels of the whole image's call
    _, whole, _ = run_gpu(svo, W, cam, (0, 0, W_, H_), svo.trace_params(shadow=True, kernel=KERNELS[kernel]), M.POINT, M.SPOT)
    assert_gbuffer_equal(after, whole.reshape(H_, W_)[16:72, 24:96], "rectangle = crop of the whole image")


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_awkward_lights(svo, oracle, scene, kernel):
    W, ow, cam = scene
    rect = (0, 0, W_, H_)
    prm = svo.trace_params(shadow=True, kernel=KERNELS[kernel])
    frame = ow.trace_image(cam, params=oracle.make_params(shadow=True), threads=8)
    # a light exactly on one pixel's sample point: q == 0, no ray, not occluded
    o, d = M.camera_rays(oracle, cam, rect)
    P = M.sample_points(o, d, frame, M.resolved_eps(0))
    k = int(np.nonzero(M.usable(frame.reshape(-1)))[0][2000])
    on_p = tuple(float(c) for c in P[k])
    _, after, _ = run_gpu(svo, W, cam, rect, prm, on_p, None)
    assert (after["flags"][k] & M.LOCAL_SHADOWS) and not (after["flags"][k] & M.SHADOWED_POINT)
    assert_gbuffer_equal(after, M.expected(oracle, ow, cam, rect, frame, on_p, None, 0), "light on a sample point")
    # outside the world box
    for outside in ((-300.0, 400.0, -200.0), (128.0, 300.0, 128.0)):
        stats = {}
        want = M.expected(oracle, ow, cam, rect, frame, None, outside, 0, stats)
        assert 0.1 < stats["spot"]["occluded"] < 0.9
        _, after, _ = run_gpu(svo, W, cam, rect, prm, None, outside)
        assert_gbuffer_equal(after, want, f"light outside the world {outside}")
    # inside solid rock: nearly every hit pixel is occluded
    stats = {}
    want = M.expected(oracle, ow, cam, rect, frame, ROCK, M.SPOT, 0, stats)
    assert stats["point"]["occluded"] >= 0.95, stats
    _, after, _ = run_gpu(svo, W, cam, rect, prm, ROCK, M.SPOT)
    assert_gbuffer_equal(after, want, "light inside rock")


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_see_through_water(svo, oracle, scene, kernel):
    W, ow, cam = scene
    rect = (0, 0, W_, H_)
    ow6 = oracle.OracleWorld.from_chunks([svo.see_through_chunk(W.chunk(i), WATER) for i in range(4)], 2, 1, 2, 128)
    frame = ow6.trace_image(cam, params=oracle.make_params(shadow=True), threads=8)
    stats, plain = {}, {}
    want = M.expected(oracle, ow6, cam, rect, frame, UNDER_WATER, M.SPOT, 0, stats)
    M.expected(oracle, ow, cam, rect, ow.trace_image(cam, params=oracle.make_params(shadow=True), threads=8), UNDER_WATER, None, 0, plain)
    assert stats["point"]["lit"] > 0.05 and plain["point"]["lit"] == 0.0        # the water is what hides this light: see_through is what shows it
    _, after, _ = run_gpu(svo, W, cam, rect, svo.trace_params(shadow=True, kernel=KERNELS[kernel], see_through=WATER), UNDER_WATER, M.SPOT)
    assert_gbuffer_equal(after, want, f"see_through {kernel}")


def test_packed_path_and_shading(svo, oracle, scene):
    W, ow, cam = scene
    rect = (0, 0, W_, H_)
    n = W_ * H_
    sp = svo.shade_defaults()
    prm = svo.trace_params(shadow=True)
    g, pk, g2, rgba, rgba_pk, rgba0 = (svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 8), svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 16),
                                       svo.DeviceBuffer(n * 16), svo.DeviceBuffer(n * 16))
    W.trace(cam, prm, rect, g.ptr)
    svo.shade(cam, sp, rect, g.ptr, rgba0.ptr)                  # before the call: no record carries SVO_LOCAL_SHADOWS
    svo.lib.svo_stream_synchronize(None)
    plain = g.to_numpy(svo.HIT_DTYPE, n)
    W.trace_local_shadows(cam, prm, rect, g.ptr, point=M.POINT, spot=M.SPOT)
    svo.gbuffer_pack(g.ptr, pk.ptr, n)
    svo.gbuffer_unpack(pk.ptr, g2.ptr, n)
    svo.shade(cam, sp, rect, g.ptr, rgba.ptr)
    svo.shade_packed(cam, sp, rect, pk.ptr, rgba_pk.ptr)
    svo.lib.svo_stream_synchronize(None)
    rec, rec2 = g.to_numpy(svo.HIT_DTYPE, n), g2.to_numpy(svo.HIT_DTYPE, n)
    got, got_pk, got0 = (b.to_numpy(np.float32, n * 4).reshape(n, 4) for b in (rgba, rgba_pk, rgba0))
    for b in (g, pk, g2, rgba, rgba_pk, rgba0):
        b.free()
    sel = M.usable(rec)
    # the packed record carries the three bits
    assert np.array_equal(rec2["flags"], rec["flags"] & (0xFF | M.ERR)) and np.array_equal(rec2["t"].view(np.uint32), rec["t"].view(np.uint32))
    assert np.count_nonzero(rec2["flags"] & M.SHADOWED_POINT) > 1000 and np.count_nonzero(rec2["flags"][sel] & M.SHADOWED_POINT == 0) > 500
    close = lambda a, b, atol: (np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= atol + RTOL * np.abs(b))
    assert np.all(close(got_pk, got, ATOL))
    # without SVO_LOCAL_SHADOWS: the oracle's shading of the record as it is (one shadow term for all three lights)
    want0 = oracle.shade_image(cam, sp, rect, plain).reshape(n, 4)
    assert np.all(close(got0, want0, ATOL))
    # with it: the sum of three oracle runs, run i with light i's colours alone and SVO_SHADOWED replaced by light i's bit
    total = np.zeros((n, 3), np.float64)
    depth = None
    for keep, bit in (("point", M.SHADOWED_POINT), ("directional", M.SHADOWED), ("spot", M.SHADOWED_SPOT)):
        one = svo.shade_defaults()
        for name in ("point", "directional", "spot"):
            if name != keep:
                for f in ("ambient", "diffuse", "specular"):
                    getattr(getattr(one, name), f)[:] = [0.0, 0.0, 0.0]
        r = rec.copy()
        r["flags"] = (r["flags"] & np.uint16(0xFFFF ^ M.SHADOWED)) | np.where(rec["flags"] & bit, M.SHADOWED, 0).astype(np.uint16)
        img = oracle.shade_image(cam, one, rect, r).reshape(n, 4)
        total += img[:, :3]
        depth = img[:, 3]
    want = total.astype(np.float32)
    assert np.all(close(got[:, :3], want, 3 * ATOL))
    assert np.all(close(got[:, 3], depth, ATOL))
    # the flags move the picture (both lights attenuate to little over most of this view: only that some pixels change visibly)
    assert np.any(sel & (np.abs(got[:, :3] - got0[:, :3]).max(axis=1) > 1e-3))


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_translucent_surface(svo, oracle, scene, kernel):
    W, ow, cam = scene
    rect = (0, 0, W_, H_)
    prm = svo.trace_params(shadow=True, kernel=KERNELS[kernel], see_through=WATER)
    surface, after, rays, behind0, behind1 = run_gpu(svo, W, cam, rect, prm, M.POINT, M.SPOT, translucent=True)
    assert rays == 2 * W_ * H_
    assert np.count_nonzero(surface["flags"] & svo.SEE_THROUGH) > 500
    assert np.array_equal(after["flags"] & svo.SEE_THROUGH, surface["flags"] & svo.SEE_THROUGH)
    assert np.array_equal(behind0.view(np.uint8), behind1.view(np.uint8))
    check_untouched(surface, after)
    # the occlusion rays are marched with the caller's params: through the water
    ow6 = oracle.OracleWorld.from_chunks([svo.see_through_chunk(W.chunk(i), WATER) for i in range(4)], 2, 1, 2, 128)
    assert_gbuffer_equal(after, M.expected(oracle, ow6, cam, rect, surface, M.POINT, M.SPOT, 0), f"translucent surface {kernel}")


def test_two_streams_share_the_scratch(svo, oracle, scene):
    """Four frames (svo_trace, then svo_trace_local_shadows behind it) on two streams, nothing in between: the ray lists and their
    records live in one scratch of the world.  Job A asks for both lights, job B for the point light alone, so the two lay the scratch
    out differently (twice as many rays), and they look through different cameras (the two of test_see_through.py's two-stream test,
    64 x 48: 1775 and 3072 usable hits by the oracle)."""
    W, ow, _ = scene
    hip = C.CDLL("libamdhip64.so.7")                        # the runtime the library is already linked against
    w, h = 64, 48
    rect, n = (0, 0, w, h), w * h
    jobs_of = {"A": (svo.default_camera(2, 2, 128, w, h), M.POINT, M.SPOT),
               "B": (svo.make_camera((20.0, 50.0, 64.0), (0.7, -0.7, 0.0), (0.0, 1.0, 0.0), 60.0, w, h), M.POINT, None)}
    prm = svo.trace_params(shadow=True)

    def issue(which, stream=0):
        cam, point, spot = jobs_of[which]
        g = svo.DeviceBuffer(n * 32)
        W.trace(cam, prm, rect, g.ptr, stream=stream)
        W.trace_local_shadows(cam, prm, rect, g.ptr, point=point, spot=spot, stream=stream)
        return g

    def fetch(g):
        out = g.to_numpy(svo.HIT_DTYPE, n)
        g.free()
        return out

    single = {}
    for which, (cam, point, spot) in jobs_of.items():
        g = issue(which)
        svo.lib.svo_stream_synchronize(None)
        single[which] = fetch(g)
        frame = ow.trace_image(cam, params=oracle.make_params(shadow=True), threads=8)
        assert M.usable(frame).sum() >= 32, which
        assert_gbuffer_equal(single[which], M.expected(oracle, ow, cam, rect, frame, point, spot, 0), f"single stream, job {which}")
    assert np.count_nonzero(np.any(single["A"].view(np.uint8).reshape(n, 32) != single["B"].view(np.uint8).reshape(n, 32), axis=1)) >= 32
    streams = []
    for _ in range(2):
        s = C.c_void_p()
        assert hip.hipStreamCreateWithFlags(C.byref(s), 1) == 0            # hipStreamNonBlocking
        streams.append(s.value)
    jobs = [(which, issue(which, stream=streams[k % 2])) for k, which in enumerate(("B", "A", "A", "B"))]
    for s in streams:
        svo.lib.svo_stream_synchronize(s)
    for which, g in jobs:
        assert np.array_equal(fetch(g).view(np.uint8), single[which].view(np.uint8)), f"two streams, job {which}"
    for s in streams:
        hip.hipStreamDestroy(C.c_void_p(s))


def test_across_a_world_change(svo, oracle):
    W = svo.World.generate(2, 1, 2, 128, 8)
    W.upload(0)
    cam = svo.default_camera(2, 2, 128, W_, H_)
    rect = (0, 0, W_, H_)
    light = (128.0, 120.0, 128.0)                               # above the terrain, in the middle of the world

    def check(what):
        ow = oracle.OracleWorld.from_chunks([W.chunk(i) for i in range(4)], 2, 1, 2, 128)
        frame = ow.trace_image(cam, params=oracle.make_params(shadow=True), threads=8)
        stats = {}
        want = M.expected(oracle, ow, cam, rect, frame, light, None, 0, stats)
        for kernel in (2, 1):
            _, after, _ = run_gpu(svo, W, cam, rect, svo.trace_params(shadow=True, kernel=kernel), light, None)
            assert_gbuffer_equal(after, want, f"{what} kernel {kernel}")
        return want, stats["point"]

    before, _ = check("fresh")
    # a wall across chunk 0, between the terrain west of it and the light
    W.edit_box(0, svo.EDIT_BUILD, (90.0, 0.0, 0.0), (94.0, 127.0, 127.0), 5)
    after, _ = check("after edit_box")
    same = M.usable(before) & (before["t"].view(np.uint32) == after["t"].view(np.uint32)) & (before["node"] == after["node"])
    newly = same & ((before["flags"] & M.SHADOWED_POINT) == 0) & ((after["flags"] & M.SHADOWED_POINT) != 0)
    assert newly.sum() >= 200, newly.sum()                    # terrain the camera still sees, now in the wall's shadow
    W.destroy()


def test_variants(svo, oracle):
    """The flags case through every library of `make variants` (SVO_AMD_LIB; one library per process, one after the other)."""
    from test_variants import VARIANTS, lib_of
    for name in sorted({n for n, _ in VARIANTS}):
        assert os.path.exists(lib_of(name)), f"{lib_of(name)} missing: __graft_entry__.build() makes it"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), lib_of(name)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, name + "\n" + r.stdout[-3000:] + r.stderr[-3000:]


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
    for kernel_ in (2, 1):
        for semantics_ in (0, 1):
            flags_case(svo_, ob_, W0, ow0, svo_.default_camera(2, 2, 128, W_, H_), kernel_, semantics_, True)
    W0.destroy()
    print("local shadows: flags equal to the oracle's")
