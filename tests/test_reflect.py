"""svo_trace_reflections and svo_shade_reflections on the GPU, against tests/reflect_model.py: the records of the mirror rays bit for bit
against the CPU oracle's march of the model's rays - both kernels, both semantics, with and without shadow rays, on the lake and on every
material of the default view -, a sub-rectangle, the surface records of a translucent frame, after an edit, on two streams; the shade
stage exactly where it can be exact (f0 = 0, f0 = 1 against a background and a one-colour sky) and within the shading stage's tolerance
against the float64 model.  tests/test_reflect_cpu.py asserts what the scenes hold."""
import ctypes as C

import numpy as np
import pytest

import hit_voxels_model as H
import reflect_model as M
import shade_model as S
import sky_model
from helpers import assert_gbuffer_equal

pytestmark = pytest.mark.gpu

KERNELS = {"literal": 1, "stack": 2}
F = np.float32
RECT = (0, 0, *M.IMAGE)
N = M.IMAGE[0] * M.IMAGE[1]
MISS_RAY = ((0.0, -256.0, -512.0), (-1.0, 0.0, 0.0))       # a ray whose line misses the 2 x 1 x 2 world: what a pixel that does not reflect gets


def rows(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8).reshape(-1, 32)


class Lake:
    """The resident world, its chunks and the oracle's twin; per (view, kernel, semantics, shadow) the G-buffer World.draw traces and the
    boxes svo_hit_voxels writes for it; per frame and material the model's rays and records.  Computed once, never changed."""

    def __init__(self, svo, oracle):
        self.svo, self.oracle = svo, oracle
        self.W = svo.World.generate(*M.WORLD)
        self.W.upload(0)
        self.chunks = [self.W.chunk(i) for i in range(4)]
        self.ow = oracle.OracleWorld.from_chunks(self.chunks, 2, 1, 2, 128)
        self._frames, self._want = {}, {}

    def frame(self, view, kernel="stack", semantics=0, shadow=True):
        key = (view, kernel, semantics, shadow)
        if key not in self._frames:
            cam = M.camera(self.svo, view)
            g = self.W.draw(cam, shadow=shadow, kernel=KERNELS[kernel], semantics=semantics).reshape(-1)
            v = self.W.hit_boxes(g)
            assert np.array_equal(rows(v), rows(H.hit_voxels(self.chunks, g)))
            self._frames[key] = (cam, g, v)
        return self._frames[key]

    def want(self, view, material, kernel="stack", semantics=0, shadow=True):
        key = (view, material, kernel, semantics, shadow)
        if key not in self._want:
            cam, g, v = self.frame(view, kernel, semantics, shadow)
            self._want[key] = M.reflect_records(self.oracle, self.ow, cam, RECT, g, v, material, shadow=shadow, semantics=semantics)
        return self._want[key]


@pytest.fixture(scope="module")
def lake(svo, oracle):
    if svo.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    L = Lake(svo, oracle)
    yield L
    L.W.destroy()


def check_records(got, rays, want, what):
    on = rays["on"]
    hits = int(((want["flags"] & 1) != 0)[on].sum())
    print(f"{what}: {int(on.sum())} mirror pixels, {hits} reflected hits")
    assert on.sum() >= 1000 and hits >= 500 and on.sum() - hits >= 150
    assert_gbuffer_equal(got, want, what)
    assert not rows(got)[~on].any(), f"{what}: a pixel that is not a mirror pixel is not all zero"


def trace(svo, W, cam, g, v, material, prm, rect=RECT, stream=0):
    """One svo_trace_reflections call on device copies of the records: -> (reflect records, the copies read back, the ray count)."""
    n = g.size
    gd, vd, out = svo.DeviceBuffer.from_numpy(g), svo.DeviceBuffer.from_numpy(v), svo.DeviceBuffer.from_numpy(np.full(n * 8, 0xA5A5A5A5, np.uint32))
    try:
        W.trace_reflections(cam, prm, rect, gd.ptr, vd.ptr, out.ptr, material=material, stream=stream)
        count = W.last_ray_count(stream)                    # (synchronises the stream)
        return out.to_numpy(svo.HIT_DTYPE, n), gd.to_numpy(svo.HIT_DTYPE, n), vd.to_numpy(svo.VOXEL_DTYPE, n), count
    finally:
        for b in (gd, vd, out):
            b.free()


def records_case(svo, lake, view, material, kernel, semantics, shadow):
    cam, g, v = lake.frame(view, kernel, semantics, shadow)
    rays, want = lake.want(view, material, kernel, semantics, shadow)
    prm = svo.trace_params(shadow=shadow, kernel=KERNELS[kernel], semantics=semantics)
    got, g_after, v_after, count = trace(svo, lake.W, cam, g, v, material, prm)
    what = f"{view} material {material} {kernel} semantics {semantics} shadow {shadow}"
    check_records(got, rays, want, what)
    assert np.array_equal(rows(g_after), rows(g)) and np.array_equal(rows(v_after), rows(v)), f"{what}: the call wrote to its inputs"
    # the ray count is svo_trace_rays' for that list
    o = np.where(rays["on"][:, None], rays["O"], np.array(MISS_RAY[0], F))
    d = np.where(rays["on"][:, None], rays["R"], np.array(MISS_RAY[1], F))
    listed = lake.W.chunkmarch(o, d, shadow=shadow, kernel=KERNELS[kernel], semantics=semantics)
    assert np.array_equal(rows(listed), rows(got)), f"{what}: svo_trace_rays on the model's list"
    assert count == lake.W.last_ray_count() and count >= N, f"{what}: ray count"


@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("semantics", [0, 1])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_records_of_the_lake(svo, lake, kernel, semantics, shadow):
    records_case(svo, lake, "lakeN", M.WATER, kernel, semantics, shadow)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_records_of_every_material(svo, lake, kernel):
    """material = 0 on the default view: faces of all three axes, terrain and water."""
    records_case(svo, lake, "default", 0, kernel, 0, True)
    rays, _ = lake.want("default", 0, kernel)
    assert np.bincount(rays["axis"][rays["on"]], minlength=3).min() >= 500


def test_a_rectangle_equals_the_crop(svo, lake):
    x0, y0, w, h = rect = (24, 16, 72, 56)
    cam, g, v = lake.frame("lakeN")
    rays, want = lake.want("lakeN", M.WATER)
    crop = (slice(y0, y0 + h), slice(x0, x0 + w))
    part = lambda a: np.ascontiguousarray(a.reshape(M.IMAGE[1], M.IMAGE[0])[crop]).reshape(-1)
    got, _, _, count = trace(svo, lake.W, cam, part(g), part(v), M.WATER, svo.trace_params(shadow=True), rect=rect)
    on = part(rays["on"])
    assert on.sum() >= 1000 and (~on).sum() >= 500
    assert_gbuffer_equal(got, part(want), "rectangle")
    assert not rows(got)[~on].any() and count >= w * h
    # an empty rectangle launches nothing and needs no buffers
    lake.W.trace_reflections(cam, svo.trace_params(), (3, 3, 0, 5), None, None, None, material=M.WATER)


class Shaded:
    """svo_shade's image of a frame (`base`, read back), the GPU's reflect records for it, and svo_shade_reflections over a fresh copy."""

    def __init__(self, svo, lake, view, material=M.WATER):
        self.svo, self.material = svo, material
        self.cam, self.g, self.v = lake.frame(view)
        self.rays, _ = lake.want(view, material)
        self.P = S.explicit(svo.shade_defaults())
        assert F(self.P.eps) == M.resolved_eps(0)
        self.reflect = trace(svo, lake.W, self.cam, self.g, self.v, material, svo.trace_params(shadow=True))[0]
        self.bufs = [svo.DeviceBuffer.from_numpy(a) for a in (self.g, self.v, self.reflect)] + [svo.DeviceBuffer(N * 16)]
        svo.shade(self.cam, self.P, RECT, self.bufs[0].ptr, self.bufs[3].ptr)
        svo.lib.svo_stream_synchronize(None)
        self.base = self.bufs[3].to_numpy(F, N * 4).reshape(N, 4)
        self.hit = (self.reflect["flags"] & 1) != 0

    def shade(self, f0, fresnel, background=(0.0, 0.0, 0.0), sky=None):
        svo, (gd, vd, rd, rgba) = self.svo, self.bufs
        svo.lib.svo_memcpy_h2d(rgba.ptr, self.base.ctypes.data, self.base.nbytes)
        svo.shade_reflections(self.cam, self.P, svo.Mirror(self.material, f0, fresnel, background, sky), RECT, gd.ptr, vd.ptr, rd.ptr, rgba.ptr)
        svo.lib.svo_stream_synchronize(None)
        return rgba.to_numpy(F, N * 4).reshape(N, 4)

    def free(self):
        for b in self.bufs:
            b.free()


@pytest.fixture(scope="module")
def shaded(svo, lake):
    made = {}

    def get(view):
        if view not in made:
            made[view] = Shaded(svo, lake, view)
        return made[view]

    yield get
    for s in made.values():
        s.free()


def u32(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def test_shade_exact_cases(svo, shaded):
    s = shaded("lakeW")
    on, hit = s.rays["on"], s.hit
    away = on & ~hit
    assert on.sum() >= 3000 and away.sum() >= 150 and (~on).sum() >= 3000
    # f0 = 0 without the Fresnel term: F == 0, nothing is written
    assert np.array_equal(u32(s.shade(0.0, False, (0.3, 0.4, 0.5))), u32(s.base))
    # f0 = 1: a reflection that leaves the world is exactly the background; nothing else is touched
    bg = (0.25, 0.5, 0.8125)
    got = s.shade(1.0, False, bg)
    assert np.array_equal(u32(got[away, :3]), u32(np.broadcast_to(np.array(bg, F), (int(away.sum()), 3))))
    assert np.array_equal(u32(got[~hit]), u32(M.blend(s.base, on, M.fresnel(s.rays["c"], 1.0, False), np.array(bg, F))[~hit])), "the float32 blend"
    assert np.array_equal(u32(got[~on]), u32(s.base[~on])), "a pixel that is not a mirror pixel was written"
    assert np.array_equal(u32(got[:, 3]), u32(s.base[:, 3])), "a depth float was written"
    assert (u32(got[on & hit, :3]) != u32(s.base[on & hit, :3])).any(axis=1).mean() > 0.9
    # ... and with a sky of one colour exactly that colour, for both filters; the background is not used
    faces = sky_model.flat_faces(5, 137)
    fd = svo.DeviceBuffer.from_numpy(faces)
    for filt in (svo.SKY_LINEAR, svo.SKY_NEAREST):
        sky = svo.Sky([fd.ptr + f * 75 for f in range(6)], 5, filt)
        sk = s.shade(1.0, False, bg, sky)
        assert np.all(sk[away, :3] == F(137) / F(255))
        assert np.array_equal(u32(sk[~away]), u32(got[~away]))
    fd.free()


@pytest.mark.parametrize("f0,fresnel", [(0.02, True), (0.5, False)])
@pytest.mark.parametrize("view", ["lakeW", "lakeN"])
def test_shade_within_the_shading_tolerance(svo, shaded, view, f0, fresnel):
    """Against the float64 model evaluated from the GPU's own reflect records, over svo_shade's own output: shade_model.within with K_GPU
    and cond scaled by F - the reflected path normalises less than the pixel path, so the project's figures apply unchanged."""
    s = shaded(view)
    bg = (0.1, 0.35, 0.6)
    got = s.shade(f0, fresnel, bg)
    want, cond, Fr = M.shade_reflections(s.P, f0, fresnel, bg, s.rays, s.reflect, s.base)
    on = s.rays["on"]
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN elsewhere than the model's"
    assert np.array_equal(u32(got[~on]), u32(s.base[~on])) and np.array_equal(u32(got[:, 3]), u32(s.base[:, 3]))
    r = S.within(got, want, cond, S.K_GPU)
    worst = float(np.nanmax(r))
    moved = np.abs(got[on, :3].astype(np.float64) - s.base[on, :3]).max(axis=1)
    print(f"{view} f0 {f0} fresnel {fresnel}: F in [{Fr[on].min():.4f}, {Fr[on].max():.4f}], |got - want| / tolerance <= {worst:.3f}, "
          f"K needed {S.needed_K(got, want, cond):.3f}, {int((moved > 1e-3).sum())} of {int(on.sum())} mirror pixels moved by more than 1e-3")
    assert (s.hit & on).sum() >= 1000 and (moved > 1e-3).sum() >= 500
    if fresnel:
        assert Fr[on].min() >= F(f0) and Fr[on].max() > 4 * f0, "grazing pixels reflect more"
    k = np.unravel_index(np.nanargmax(r), r.shape)
    assert worst <= 1.0, f"pixel {k[0]} component {k[1]}: got {got[k]} want {want[k]} cond {cond[k[0]]}"


def test_translucent_frame(svo, oracle, lake):
    """The surface records of svo_trace_translucent (SVO_SEE_THROUGH on the water) through svo_hit_voxels, then the water's reflections."""
    cam = M.camera(svo, "lakeN")
    surface, _ = lake.W.draw_translucent(cam, M.WATER, shadow=True)
    g = surface.reshape(-1)
    assert ((g["flags"] & svo.SEE_THROUGH) != 0).sum() >= 5000
    v = lake.W.hit_boxes(g)
    rays, want = M.reflect_records(oracle, lake.ow, cam, RECT, g, v, M.WATER, shadow=True)
    got = trace(svo, lake.W, cam, g, v, M.WATER, svo.trace_params(shadow=True))[0]
    check_records(got, rays, want, "translucent surface")
    # see_through = 6 in the reflection launch itself: the mirror rays march past water, too
    prm = svo.trace_params(shadow=True, see_through=M.WATER)
    twin = oracle.OracleWorld.from_chunks([svo.see_through_chunk(c, M.WATER) for c in lake.chunks], 2, 1, 2, 128)
    want = np.zeros(N, H.HIT_DTYPE)
    want[rays["on"]] = twin.trace_rays(rays["O"][rays["on"]], rays["R"][rays["on"]], params=oracle.make_params(shadow=True), threads=8)
    assert_gbuffer_equal(trace(svo, lake.W, cam, g, v, M.WATER, prm)[0], want, "see_through in the reflection launch")


def test_the_call_after_an_edit_sees_the_edit(svo, oracle):
    """svo_world_edit_box builds a block of material 5 that stands in the lake in lakeN's view: the next call's records equal the model on
    the edited chunks, and the water in front of the block mirrors it.  Nothing is cached."""
    W = svo.World.generate(*M.WORLD)
    W.upload(0)
    cam = M.camera(svo, "lakeN")

    def frame(what):
        chunks = [W.chunk(i) for i in range(4)]
        ow = oracle.OracleWorld.from_chunks(chunks, 2, 1, 2, 128)
        g = W.draw(cam, shadow=True).reshape(-1)
        v = W.hit_boxes(g)
        rays, want = M.reflect_records(oracle, ow, cam, RECT, g, v, M.WATER, shadow=True)
        for kernel in sorted(KERNELS):
            got = trace(svo, W, cam, g, v, M.WATER, svo.trace_params(shadow=True, kernel=KERNELS[kernel]))[0]
            check_records(got, rays, want, f"{what} {kernel}")
        return rays, want

    _, before = frame("before the edit")
    W.edit_box(2, svo.EDIT_BUILD, (116.0, 6.5, 196.0), (126.0, 30.0, 204.0), 5)
    rays, after = frame("after the edit")
    seen = int((rays["on"] & ((after["flags"] & 1) != 0) & (after["material"] == 5)).sum())
    print(f"the block is mirrored in {seen} pixels")
    assert seen >= 50 and not ((before["flags"] & 1 != 0) & (before["material"] == 5)).any()
    W.destroy()


def test_two_streams_share_the_scratch(svo, lake):
    """Four calls on two streams with two cameras, nothing in between: the ray lists live in one scratch of the world, and a call that did
    not wait for the one before it would march the other camera's rays."""
    hip = C.CDLL("libamdhip64.so.7")                        # the runtime the library is already linked against
    prm = svo.trace_params(shadow=True)
    views = {"A": "lakeN", "B": "lakeW"}
    wants = {k: lake.want(v, M.WATER)[1] for k, v in views.items()}
    assert (rows(wants["A"]) != rows(wants["B"])).any(axis=1).sum() >= 1000
    streams = []
    for _ in range(2):
        s = C.c_void_p()
        assert hip.hipStreamCreateWithFlags(C.byref(s), 1) == 0            # hipStreamNonBlocking
        streams.append(s.value)
    jobs = []
    for k, which in enumerate(("B", "A", "A", "B")):
        cam, g, v = lake.frame(views[which])
        bufs = svo.DeviceBuffer.from_numpy(g), svo.DeviceBuffer.from_numpy(v), svo.DeviceBuffer(N * 32)
        jobs.append((which, bufs))
    svo.lib.svo_stream_synchronize(None)
    for k, (which, bufs) in enumerate(jobs):
        cam = lake.frame(views[which])[0]
        lake.W.trace_reflections(cam, prm, RECT, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, material=M.WATER, stream=streams[k % 2])
    for s in streams:
        svo.lib.svo_stream_synchronize(s)
    for which, bufs in jobs:
        got = bufs[2].to_numpy(svo.HIT_DTYPE, N)
        for b in bufs:
            b.free()
        assert_gbuffer_equal(got, wants[which], f"two streams, camera {which}")
    for s in streams:
        hip.hipStreamDestroy(C.c_void_p(s))


def test_statuses_on_a_resident_world(svo, lake):
    """What only a resident world can answer: the kernel id and an image too large, both settled before any device work; a refused
    call writes nothing."""
    cam, g, v = lake.frame("lakeN")
    gd, vd = svo.DeviceBuffer.from_numpy(g), svo.DeviceBuffer.from_numpy(v)
    sentinel = np.full(N * 8, 0x5A5A5A5A, np.uint32)
    out = svo.DeviceBuffer.from_numpy(sentinel)

    def code(prm, rect=RECT, material=M.WATER):
        with pytest.raises(svo.SvoError) as e:
            lake.W.trace_reflections(cam, prm, rect, gd.ptr, vd.ptr, out.ptr, material=material)
        return e.value.code

    assert code(svo.trace_params(kernel=9)) == -1
    assert code(svo.trace_params(semantics=7)) == -1
    assert code(svo.trace_params(), material=0x10000) == -1
    assert code(svo.trace_params(), rect=(0, 0, 1 << 16, 1 << 15)) == -6
    svo.lib.svo_stream_synchronize(None)
    assert np.array_equal(out.to_numpy(np.uint32, N * 8), sentinel), "a refused call wrote to reflect_dev"
    for b in (gd, vd, out):
        b.free()
