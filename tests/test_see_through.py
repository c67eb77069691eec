"""See-through materials on the GPU: svo_trace* with svo_trace_params.see_through, svo_trace_translucent and svo_shade_translucent,
each checked bit for bit against the CPU oracle on the REWRITTEN world (LEAF(m) words and cells m set to 0 in numpy), which is what
the see-through march is defined to equal."""
import ctypes as C

import numpy as np
import pytest

from helpers import adversarial_rays, assert_gbuffer_equal, random_rays

pytestmark = pytest.mark.gpu

WATER = 6
KERNELS = {"stack": 2, "literal": 1}


def _oracle_of(svo, oracle, world, material):
    info = world.info
    n = info.width * info.height * info.depth
    chunks = [svo.see_through_chunk(world.chunk(i), material) for i in range(n)]
    return oracle.OracleWorld.from_chunks(chunks, info.width, info.height, info.depth, info.chunksize, tuple(info.chunkcoordmin))


@pytest.fixture(scope="module")
def water_world(svo, oracle):
    if svo.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    W = svo.World.generate(2, 1, 2, 128, 8)
    W.upload(0)
    yield W, _oracle_of(svo, oracle, W, WATER)
    W.destroy()


def _camera_rays(svo, oracle, cam, rect=None):
    ocam = oracle.camera_from(cam)
    x0, y0, w, h = rect if rect is not None else (0, 0, cam.width, cam.height)
    o = np.zeros((h, w, 3), np.float32)
    d = np.zeros((h, w, 3), np.float32)
    vo, vd = oracle.Vec3(), oracle.Vec3()
    for y in range(h):
        for x in range(w):
            oracle.lib.orc_camera_ray(C.byref(ocam), x0 + x, y0 + y, C.byref(vo), C.byref(vd))
            o[y, x] = (vo.x, vo.y, vo.z)
            d[y, x] = (vd.x, vd.y, vd.z)
    return o.reshape(-1, 3), d.reshape(-1, 3)


def _ray_sets(svo, oracle):
    rng = np.random.default_rng(2606)
    lo, hi = (0.0, 0.0, 0.0), (256.0, 128.0, 256.0)
    cam = svo.default_camera(2, 2, 128, 48, 32)
    sets = [_camera_rays(svo, oracle, cam), random_rays(rng, 1500, lo, hi), adversarial_rays(rng, 1600, lo, hi)]
    # origins inside the water (below y = 6), in every direction, and axis-parallel ones on the water's lattice
    o = np.column_stack([rng.random(1200) * 256.0, 0.25 + rng.random(1200) * 5.5, rng.random(1200) * 256.0])
    d = rng.normal(size=(1200, 3))
    d[:300] = 0.0
    d[np.arange(300), rng.integers(0, 3, 300)] = rng.choice([-1.0, 1.0], 300)
    o[:150] = np.round(o[:150] * 2.0) / 2.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sets.append((o.astype(np.float32), d.astype(np.float32)))
    return np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets])


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("semantics", [0, 1])
def test_trace_rays_see_through_water(svo, oracle, water_world, kernel, shadow, semantics):
    W, ow = water_world
    o, d = _ray_sets(svo, oracle)
    got = W.chunkmarch(o, d, shadow=shadow, kernel=KERNELS[kernel], semantics=semantics, see_through=WATER)
    want = ow.trace_rays(o, d, params=oracle.make_params(shadow=shadow, semantics=semantics), threads=8)
    assert_gbuffer_equal(got, want, f"see-through rays {kernel} shadow={shadow} semantics={semantics}")
    assert not np.any((got["flags"] & 1).astype(bool) & (got["material"] == WATER))
    # the plain march of the same rays does hit the water: the field is what changed the records
    plain = W.chunkmarch(o, d, kernel=KERNELS[kernel], semantics=semantics)
    assert np.count_nonzero((plain["flags"] & 1).astype(bool) & (plain["material"] == WATER)) > 100


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_trace_and_frames_see_through(svo, oracle, water_world, kernel):
    W, ow = water_world
    cam = svo.default_camera(2, 2, 128, 96, 64)
    got = W.draw(cam, shadow=True, kernel=KERNELS[kernel], see_through=WATER)
    want = ow.trace_image(cam, params=oracle.make_params(shadow=True), threads=8)
    assert_gbuffer_equal(got, want, f"svo_trace see_through {kernel}")
    cam2 = svo.make_camera((130.3, 60.0, 20.0), (0.1, -0.7, 0.7), (0.0, 1.0, 0.0), 60.0, 96, 64)
    out = svo.DeviceBuffer(2 * 96 * 64 * 32)
    W.trace_frames([cam, cam2], svo.trace_params(shadow=True, kernel=KERNELS[kernel], see_through=WATER), (0, 0, 96, 64), out.ptr)
    svo.lib.svo_stream_synchronize(None)
    g = out.to_numpy(svo.HIT_DTYPE, 2 * 96 * 64)
    out.free()
    assert_gbuffer_equal(g[: 96 * 64], want, "svo_trace_frames frame 0")
    assert_gbuffer_equal(g[96 * 64:], ow.trace_image(cam2, params=oracle.make_params(shadow=True), threads=8), "svo_trace_frames frame 1")


def _continuations(svo, oracle, cam, surface, rect):
    """The continuation rays of svo_trace_translucent rebuilt on the host: orc_camera_ray's direction, origin o + d * t1 in float32."""
    o, d = _camera_rays(svo, oracle, cam, rect)
    t1 = surface["t"].reshape(-1).astype(np.float32)
    p1 = (o + d * t1[:, None]).astype(np.float32)           # numpy rounds each float32 op: no contraction
    return p1, d


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("shadow", [False, True])
def test_trace_translucent(svo, oracle, water_world, kernel, shadow):
    W, ow = water_world
    cam = svo.default_camera(2, 2, 128, 128, 96)
    rect = (0, 0, 128, 96)
    surface, behind = W.draw_translucent(cam, WATER, shadow=shadow, kernel=KERNELS[kernel])
    plain = W.draw(cam, shadow=shadow, kernel=KERNELS[kernel])
    s = surface.reshape(-1)
    cont = ((plain["flags"] & 1) != 0) & ((plain["flags"] & svo.ERR_FLAG) == 0) & (plain["material"] == WATER)
    cont = cont.reshape(-1)
    assert cont.mean() >= 0.05, f"only {cont.mean():.3f} of the pixels see water"
    assert np.array_equal((s["flags"] & svo.SEE_THROUGH) != 0, cont)
    s_cleared = s.copy()
    s_cleared["flags"] &= np.uint16(0xFFFF ^ svo.SEE_THROUGH)
    assert_gbuffer_equal(s_cleared, plain, "surface = svo_trace(see_through=0)")
    p1, d = _continuations(svo, oracle, cam, surface, rect)
    want = ow.trace_rays(p1[cont], d[cont], params=oracle.make_params(shadow=shadow), threads=8)
    b = behind.reshape(-1)
    assert_gbuffer_equal(b[cont], want, f"behind records {kernel}")
    assert np.all(b[~cont].view(np.uint8).reshape(-1, 32) == 0), "pixels that are not continued are all-zero"
    assert np.count_nonzero(b[cont]["flags"] & 1) > 0.1 * cont.sum()      # a lake bed is seen (the rest leave through the world's floor)


def test_two_streams_share_the_continuation_list(svo, oracle, water_world):
    """Four svo_trace_translucent calls on two streams, nothing in between: the continuation lists live in one scratch of the world, and
    a call that did not wait for the one before it would march the other camera's rays.  Two cameras at 64 x 48; the second is not the
    cam2 of test_trace_and_frames_see_through, which sees no water at this size (the oracle says), but one over the lake: 484 and 1459
    pixels continue."""
    W, ow = water_world
    hip = C.CDLL("libamdhip64.so.7")                        # the runtime the library is already linked against
    w, h = 64, 48
    rect, n = (0, 0, w, h), w * h
    cams = {"A": svo.default_camera(2, 2, 128, w, h), "B": svo.make_camera((20.0, 50.0, 64.0), (0.7, -0.7, 0.0), (0.0, 1.0, 0.0), 60.0, w, h)}
    prm = svo.trace_params(see_through=WATER)

    def issue(which, stream=0):
        bufs = svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 32)
        W.trace_translucent(cams[which], prm, rect, bufs[0].ptr, bufs[1].ptr, stream=stream)
        return bufs

    def fetch(bufs):
        out = tuple(b.to_numpy(svo.HIT_DTYPE, n) for b in bufs)
        for b in bufs:
            b.free()
        return out

    single = {}
    for which, cam in cams.items():
        bufs = issue(which)
        svo.lib.svo_stream_synchronize(None)
        surface, behind = single[which] = fetch(bufs)
        plain = W.draw(cam).reshape(-1)
        cont = ((plain["flags"] & 1) != 0) & ((plain["flags"] & svo.ERR_FLAG) == 0) & (plain["material"] == WATER)
        assert cont.sum() >= 32, f"camera {which}: only {cont.sum()} pixels see water"
        assert np.array_equal((surface["flags"] & svo.SEE_THROUGH) != 0, cont)
        p1, d = _continuations(svo, oracle, cam, surface, rect)
        assert_gbuffer_equal(behind[cont], ow.trace_rays(p1[cont], d[cont], params=oracle.make_params(), threads=8), f"single stream, camera {which}")
        assert np.all(behind[~cont].view(np.uint8).reshape(-1, 32) == 0), "pixels that are not continued are all-zero"
    for k in (0, 1):                                            # the two jobs differ: records of one cannot pass for the other's
        assert np.count_nonzero(np.any(single["A"][k].view(np.uint8).reshape(n, 32) != single["B"][k].view(np.uint8).reshape(n, 32), axis=1)) >= 32
    streams = []
    for _ in range(2):
        s = C.c_void_p()
        assert hip.hipStreamCreateWithFlags(C.byref(s), 1) == 0            # hipStreamNonBlocking
        streams.append(s.value)
    jobs = [(which, issue(which, stream=streams[k % 2])) for k, which in enumerate(("B", "A", "A", "B"))]
    for s in streams:
        svo.lib.svo_stream_synchronize(s)
    for which, bufs in jobs:
        for name, got, want in zip(("surface", "behind"), fetch(bufs), single[which]):
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"two streams, camera {which}: {name}"
    for s in streams:
        hip.hipStreamDestroy(C.c_void_p(s))


def test_view_follows_edits(svo, oracle):
    W = svo.World.generate(2, 1, 2, 128, 8)
    W.upload(0)
    cam = svo.default_camera(2, 2, 128, 64, 48)

    def check(material, what):
        ow = _oracle_of(svo, oracle, W, material)
        want = ow.trace_image(cam, params=oracle.make_params(shadow=True), threads=8)
        for kernel in (2, 1):
            assert_gbuffer_equal(W.draw(cam, shadow=True, kernel=kernel, see_through=material), want, f"{what} kernel {kernel}")

    check(WATER, "fresh")
    W.edit_box(0, svo.EDIT_DESTROY, (20.0, -2.0, 40.0), (90.0, 4.0, 110.0))     # a pit dug under the water
    check(WATER, "after edit_box")
    W.shift((1, 0, 0))
    check(WATER, "after shift")
    W.compact(0)
    check(WATER, "after compact")
    for m in (4, WATER, 4, WATER):
        check(m, f"see_through {m}")
    W.destroy()


def test_deep_device_built_world(svo, oracle):
    W = svo.World.generate(2, 1, 2, 128, 12, build_device=0)
    cam = svo.default_camera(2, 2, 128, 1920, 1080)
    rect = (380, 880, 96, 48)                                   # a crop of the bench view over the water
    got = W.draw(cam, rect=rect, shadow=True, kernel=2, see_through=WATER)
    ow = _oracle_of(svo, oracle, W, WATER)
    want = ow.trace_image(cam, rect=rect, params=oracle.make_params(shadow=True), threads=8)
    assert_gbuffer_equal(got, want, "depth 12 see-through")
    plain = W.draw(cam, rect=rect, kernel=2)
    assert np.count_nonzero((plain["flags"] & 1).astype(bool) & (plain["material"] == WATER)) > 0
    W.destroy()


@pytest.mark.parametrize("absorption", [0.0, 0.2])
def test_shade_translucent(svo, oracle, water_world, absorption):
    W, _ = water_world
    cam = svo.default_camera(2, 2, 128, 128, 96)
    rect = (0, 0, 128, 96)
    n = 128 * 96
    sp = svo.shade_defaults()
    prm = svo.trace_params(shadow=True, see_through=WATER)
    surf, behind, rgba, plain_rgba = (svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 16), svo.DeviceBuffer(n * 16))
    W.trace_translucent(cam, prm, rect, surf.ptr, behind.ptr)
    svo.shade_translucent(cam, sp, rect, surf.ptr, behind.ptr, rgba.ptr, absorption=absorption)
    svo.shade(cam, sp, rect, surf.ptr, plain_rgba.ptr)
    svo.lib.svo_stream_synchronize(None)
    s = surf.to_numpy(svo.HIT_DTYPE, n)
    b = behind.to_numpy(svo.HIT_DTYPE, n)
    got = rgba.to_numpy(np.float32, n * 4).reshape(n, 4)
    plain = plain_rgba.to_numpy(np.float32, n * 4).reshape(n, 4)
    for buf in (surf, behind, rgba, plain_rgba):
        buf.free()
    cs = oracle.shade_image(cam, sp, rect, s).reshape(n, 4)
    bt = b.copy()
    bt["t"] = (s["t"] + b["t"]).astype(np.float32)
    cb = oracle.shade_image(cam, sp, rect, bt).reshape(n, 4)
    k = np.float32(0.5 if absorption == 0.0 else absorption)
    a = np.clip(b["t"] * k, 0.0, 1.0).astype(np.float32)[:, None]
    blend = (s["flags"] & svo.SEE_THROUGH != 0) & (b["flags"] & 1 != 0)
    want = cs.copy()
    want[blend, :3] = cb[blend, :3] * (1.0 - a[blend]) + cs[blend, :3] * a[blend]
    want[blend, 3] = cb[blend, 3]
    assert blend.mean() >= 0.02                                  # water pixels with a lake bed behind them
    both_nan = np.isnan(got) & np.isnan(want)
    assert np.all(both_nan | (np.abs(got - want) <= 1e-6 + 2e-5 * np.abs(want)))         # test_shading.py's tolerance
    flagged = (s["flags"] & svo.SEE_THROUGH) != 0
    assert np.array_equal(got[~flagged], plain[~flagged], equal_nan=True),"pixels without SVO_SEE_THROUGH are svo_shade's"
