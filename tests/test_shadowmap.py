"""The shadow map on the GPU: svo_shadowmap_render's depth image and svo_shadowmap_apply's flags, compared bit for bit with
tests/shadowmap_model.py (the texel rays and the projection in numpy float32 with the header's expressions, the rays marched by the
unchanged CPU oracle).  tests/test_shadowmap_cpu.py checks, on the oracle alone, that the scene keeps these comparisons from passing
vacuously.

Run as a script - python tests/test_shadowmap.py <libsvo_*.so> - it puts one variant build of the library through the render and the
apply case on map A (one library per process, as tests/variant_check.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import shadowmap_model as M
from helpers import assert_gbuffer_equal
from test_shading import ATOL, RTOL

pytestmark = pytest.mark.gpu

KERNELS = {"stack": 2, "literal": 1}
MAPS = {"A": M.MAP_A, "B": M.MAP_B}
WATER = 6
W_, H_ = 128, 96
POINT, SPOT = M.LM.POINT, M.LM.SPOT


class Scene:
    """The 2x1x2 depth-8 world on the device and in the oracle, and what the oracle makes of it: computed once, shared, left unchanged."""

    def __init__(self, svo, oracle):
        self.svo, self.oracle = svo, oracle
        self.W = svo.World.generate(2, 1, 2, 128, 8)
        self.chunks = [self.W.chunk(i) for i in range(4)]
        self.W.upload(0)
        self.ow = oracle.OracleWorld.from_chunks(self.chunks, 2, 1, 2, 128)
        self.cam = svo.default_camera(2, 2, 128, W_, H_)
        self._depth, self._frame = {}, {}

    def depth(self, which, semantics=0):
        if (which, semantics) not in self._depth:
            cfg = MAPS[which]
            stats = {}
            d = M.depth_image(self.oracle, self.ow, M.make_map(self.svo, cfg["size"], cfg["half"]), semantics, stats)
            assert stats["runaways"] == 0 and 0.3 < stats["hit"] < 0.95, stats
            d.setflags(write=False)
            self._depth[which, semantics] = d
        return self._depth[which, semantics]

    def frame(self, shadow, semantics=0, rect=None):
        key = (shadow, semantics, rect)
        if key not in self._frame:
            f = self.ow.trace_image(self.cam, rect=rect, params=self.oracle.make_params(shadow=shadow, semantics=semantics), threads=8)
            f.setflags(write=False)
            self._frame[key] = f
        return self._frame[key]


@pytest.fixture(scope="module")
def scene(svo, oracle):
    if svo.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    s = Scene(svo, oracle)
    yield s
    s.W.destroy()


def render(svo, W, m_or_cfg, prm, stream=0, sync=True):
    """svo_shadowmap_render into a fresh depth image: (map, device buffer)."""
    m = m_or_cfg if isinstance(m_or_cfg, svo.ShadowMap) else M.make_map(svo, m_or_cfg["size"], m_or_cfg["half"])
    buf = svo.DeviceBuffer.from_numpy(np.full(m.width * m.height, -1.0, np.float32))
    m.depth_dev = buf.ptr
    W.shadowmap_render(m, prm, stream)
    if sync:
        svo.lib.svo_stream_synchronize(stream or None)
    return m, buf


def depth_of(m, buf):
    return buf.to_numpy(np.float32, m.width * m.height).reshape(m.height, m.width)


def assert_depth_equal(got, want, what):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{what}: {len(bad)} texels differ, first (j, i) {bad[:4].tolist()}: got {[got[tuple(b)] for b in bad[:4]]} want {[want[tuple(b)] for b in bad[:4]]}"


def render_case(svo, scene, which, kernel, semantics):
    prm = svo.trace_params(shadow=True, kernel=kernel, semantics=semantics)        # (shadow is dropped: the rays counted below are the texels')
    m, buf = render(svo, scene.W, MAPS[which], prm)
    rays = scene.W.last_ray_count()
    got = depth_of(m, buf)
    buf.free()
    want = scene.depth(which, semantics)
    assert_depth_equal(got, want, f"map {which} kernel {kernel} semantics {semantics}")
    assert rays == m.width * m.height
    miss = ~np.isfinite(want)
    assert miss.sum() > 100 and np.all(got[miss] == np.inf) and np.all(got[~miss] > 0)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("semantics", [0, 1])
def test_render_map_a(svo, scene, kernel, semantics):
    render_case(svo, scene, "A", KERNELS[kernel], semantics)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_render_map_b(svo, scene, kernel):
    render_case(svo, scene, "B", KERNELS[kernel], 0)


def check_untouched(before, after):
    """Records without a usable hit are byte-identical; of the others only the flag bits 1 and 2 may differ, and bit 1 is set."""
    sel = M.LM.usable(before)
    assert np.array_equal(before[~sel].view(np.uint8), after[~sel].view(np.uint8))
    a, b = after.copy(), before.copy()
    a["flags"] &= np.uint16(0xFFFF ^ (M.SHADOWED | M.SHADOW_TRACED))
    b["flags"] &= np.uint16(0xFFFF ^ (M.SHADOWED | M.SHADOW_TRACED))
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert np.all((after["flags"][sel] & M.SHADOW_TRACED) != 0)


def apply_case(svo, oracle, scene, which, kernel, rect=None, shadow=False, semantics=0):
    """svo_trace, then svo_shadowmap_apply against the map rendered with the same kernel: (records before, records after, expected)."""
    cfg = MAPS[which]
    x0, y0, w, h = rect or (0, 0, W_, H_)
    prm = svo.trace_params(shadow=shadow, kernel=kernel, semantics=semantics)
    m, buf = render(svo, scene.W, cfg, prm, sync=False)
    g = svo.DeviceBuffer(w * h * 32)
    scene.W.trace(scene.cam, prm, (x0, y0, w, h), g.ptr)
    svo.lib.svo_stream_synchronize(None)
    before = g.to_numpy(svo.HIT_DTYPE, w * h)
    svo.shadowmap_apply(scene.cam, m, float(M.LM.resolved_eps(semantics)) if semantics else 0.0, cfg["bias"], (x0, y0, w, h), g.ptr)
    svo.lib.svo_stream_synchronize(None)
    after = g.to_numpy(svo.HIT_DTYPE, w * h)
    g.free()
    buf.free()
    stats = {}
    want = M.expected(oracle, scene.cam, rect, scene.frame(False, semantics, rect), m, scene.depth(which, semantics), cfg["bias"], semantics, stats)
    what = f"map {which} kernel {kernel} rect {rect} shadow {shadow} semantics {semantics}"
    print(what, stats)
    assert stats["shadowed"] >= 0.05 and stats["lit"] >= 0.05, stats
    assert_gbuffer_equal(before, scene.frame(shadow, semantics, rect), "svo_trace, " + what)
    assert_gbuffer_equal(after, want, what)
    check_untouched(before, after)
    return before, after, want


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("which", sorted(MAPS))
def test_apply(svo, oracle, scene, which, kernel):
    apply_case(svo, oracle, scene, which, KERNELS[kernel])


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_apply_rectangle(svo, oracle, scene, kernel):
    _, after, _ = apply_case(svo, oracle, scene, "B", KERNELS[kernel], rect=(24, 16, 72, 56))
    _, whole, _ = apply_case(svo, oracle, scene, "B", KERNELS[kernel])
    assert_gbuffer_equal(after, whole.reshape(H_, W_)[16:72, 24:96], "rectangle = crop of the whole image")


def test_apply_glsl_semantics(svo, oracle, scene):
    apply_case(svo, oracle, scene, "A", KERNELS["stack"], semantics=1)


def test_apply_overwrites_the_shadow_rays_verdict(svo, oracle, scene):
    before, after, want = apply_case(svo, oracle, scene, "A", KERNELS["stack"], shadow=True)
    sel = M.LM.usable(before)
    changed = (before["flags"] & M.SHADOWED) != (after["flags"] & M.SHADOWED)
    assert changed[sel].sum() > 500 and np.all((before["flags"][sel] & M.SHADOW_TRACED) != 0)
    _, plain, _ = apply_case(svo, oracle, scene, "A", KERNELS["stack"], shadow=False)
    assert np.array_equal(after.view(np.uint8), plain.view(np.uint8))                  # the same records as from a shadow = 0 frame
    # a frame that has been through svo_trace_local_shadows keeps bits 5-7
    cfg = M.MAP_A
    rect, n = (0, 0, W_, H_), W_ * H_
    prm = svo.trace_params(shadow=True)
    m, buf = render(svo, scene.W, cfg, prm, sync=False)
    g = svo.DeviceBuffer(n * 32)
    scene.W.trace(scene.cam, prm, rect, g.ptr)
    scene.W.trace_local_shadows(scene.cam, prm, rect, g.ptr, point=POINT, spot=SPOT)
    svo.lib.svo_stream_synchronize(None)
    local = g.to_numpy(svo.HIT_DTYPE, n)
    svo.shadowmap_apply(scene.cam, m, 0.0, cfg["bias"], rect, g.ptr)
    svo.lib.svo_stream_synchronize(None)
    got = g.to_numpy(svo.HIT_DTYPE, n)
    g.free()
    buf.free()
    keep = np.uint16(M.LM.LOCAL_SHADOWS | M.LM.SHADOWED_POINT | M.LM.SHADOWED_SPOT)
    assert np.count_nonzero(local["flags"] & M.LM.SHADOWED_POINT) > 1000 and np.all((local["flags"][sel] & M.LM.LOCAL_SHADOWS) != 0)
    assert np.array_equal(got["flags"] & keep, local["flags"] & keep)
    check_untouched(local, got)
    stripped = got.copy()
    stripped["flags"] &= ~keep
    assert_gbuffer_equal(stripped, want, "apply behind svo_trace_local_shadows")


def test_shade_uses_the_applied_flags(svo, oracle, scene):
    cfg = M.MAP_A
    rect, n = (0, 0, W_, H_), W_ * H_
    prm = svo.trace_params(shadow=False)
    sp = svo.shade_defaults()
    m, buf = render(svo, scene.W, cfg, prm, sync=False)
    g, rgba0, rgba = svo.DeviceBuffer(n * 32), svo.DeviceBuffer(n * 16), svo.DeviceBuffer(n * 16)
    scene.W.trace(scene.cam, prm, rect, g.ptr)
    svo.shade(scene.cam, sp, rect, g.ptr, rgba0.ptr)
    svo.shadowmap_apply(scene.cam, m, 0.0, cfg["bias"], rect, g.ptr)
    svo.shade(scene.cam, sp, rect, g.ptr, rgba.ptr)
    svo.lib.svo_stream_synchronize(None)
    got0, got = (b.to_numpy(np.float32, n * 4).reshape(n, 4) for b in (rgba0, rgba))
    for b in (g, rgba0, rgba, buf):
        b.free()
    want_records = M.expected(oracle, scene.cam, None, scene.frame(False), m, scene.depth("A"), cfg["bias"])
    want = oracle.shade_image(scene.cam, sp, rect, want_records).reshape(n, 4)
    close = lambda a, b: (np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= ATOL + RTOL * np.abs(b))
    assert np.all(close(got, want))
    shadowed = (want_records["flags"] & M.SHADOWED) != 0
    assert shadowed.sum() > 1000 and np.count_nonzero(np.abs(got[shadowed, :3] - got0[shadowed, :3]).max(axis=1) > 1e-3) > 500      # the flags darken the picture


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_see_through_water(svo, oracle, scene, kernel):
    """A shadow map that water does not darken: the model's map of the world with water rewritten to 0."""
    ow6 = oracle.OracleWorld.from_chunks([svo.see_through_chunk(c, WATER) for c in scene.chunks], 2, 1, 2, 128)
    cfg = M.MAP_B
    want = M.depth_image(oracle, ow6, M.make_map(svo, cfg["size"], cfg["half"]))
    opaque = scene.depth("B")
    assert np.count_nonzero(want.view(np.uint32) != opaque.view(np.uint32)) >= 100
    m, buf = render(svo, scene.W, cfg, svo.trace_params(kernel=KERNELS[kernel], see_through=WATER))
    got = depth_of(m, buf)
    buf.free()
    assert_depth_equal(got, want, f"see_through {kernel}")
    m, buf = render(svo, scene.W, cfg, svo.trace_params(kernel=KERNELS[kernel]))          # ... and the opaque one is still what it was
    assert_depth_equal(depth_of(m, buf), opaque, f"opaque after see_through {kernel}")
    buf.free()


def test_known_answer(svo, oracle):
    """A floor slab under a floating plate (tests/test_shadowmap_cpu.py): what lies under the plate is shadowed, what lies clear of it is lit."""
    from test_shadowmap_cpu import known_scene
    K, chunk, ow, m, cam = known_scene(svo, oracle)
    K.upload(0)
    texel = 2.0 * max(m.half_width / m.width, m.half_height / m.height)
    bias = 2.0 * texel
    frame = ow.trace_image(cam, params=oracle.make_params(shadow=False), threads=8)
    sel, P = M.sample_points(oracle, cam, None, frame)
    under, clear = M.known_sets(P, sel, frame["material"], texel + bias)
    assert under.sum() >= 50 and clear.sum() >= 50
    for kernel in (2, 1):
        m2, buf = render(svo, K, m, svo.trace_params(kernel=kernel), sync=False)
        got = K.draw(cam, kernel=kernel, shadowmap=(m2, bias)).reshape(-1)
        assert_depth_equal(depth_of(m2, buf), M.depth_image(oracle, ow, m2), f"known answer, kernel {kernel}")
        buf.free()
        assert np.all((got["flags"][under] & M.SHADOWED) != 0) and not np.any(got["flags"][clear] & M.SHADOWED), kernel
        assert np.all((got["flags"][under | clear] & M.SHADOW_TRACED) != 0)
        assert_gbuffer_equal(got, M.expected(oracle, cam, None, frame, m2, M.depth_image(oracle, ow, m2), bias), f"known answer, kernel {kernel}")
    K.destroy()


def test_a_rendered_map_is_stale_after_an_edit(svo, oracle):
    W = svo.World.generate(2, 1, 2, 128, 8)
    W.upload(0)
    O = oracle.OracleWorld.generate(2, 1, 2, 128, 8)
    prm = svo.trace_params()
    m, buf = render(svo, W, M.MAP_A, prm)
    old = depth_of(m, buf)
    assert_depth_equal(old, M.depth_image(oracle, O, m), "before the edit")
    lo, hi = (60.0, 100.0, 60.0), (76.0, 116.0, 76.0)                   # a 16-unit cube above the terrain
    W.edit_box(0, svo.EDIT_BUILD, lo, hi, 5)
    dt, dw = oracle.Delta(), oracle.Delta()
    oracle.lib.orc_build(C.byref(O.w.chunk[0]), oracle.vec3(lo), oracle.vec3(hi), 5, C.byref(dt), C.byref(dw))
    assert_depth_equal(depth_of(m, buf), old, "nothing re-renders the map behind the caller's back")
    for kernel in (2, 1):
        m2, buf2 = render(svo, W, M.MAP_A, svo.trace_params(kernel=kernel))
        new = depth_of(m2, buf2)
        buf2.free()
        assert np.count_nonzero(new.view(np.uint32) != old.view(np.uint32)) >= 4
        assert_depth_equal(new, M.depth_image(oracle, O, m2), f"after the edit, kernel {kernel}")
    buf.free()
    W.destroy()


def test_two_streams_share_the_scratch(svo, scene):
    """Two renders into two maps on two streams, nothing in between: the list and the records live in one scratch of the world."""
    hip = C.CDLL("libamdhip64.so.7")                        # the runtime the library is already linked against
    prm = svo.trace_params()
    single = {}
    for which in ("A", "B"):
        m, buf = render(svo, scene.W, MAPS[which], prm)
        single[which] = depth_of(m, buf)
        buf.free()
        assert_depth_equal(single[which], scene.depth(which), f"single stream, map {which}")
    streams = []
    for _ in range(2):
        h = C.c_void_p()
        assert hip.hipStreamCreateWithFlags(C.byref(h), 1) == 0            # hipStreamNonBlocking
        streams.append(h.value)
    jobs = [(which, render(svo, scene.W, MAPS[which], prm, stream=streams[k % 2], sync=False)) for k, which in enumerate(("B", "A", "A", "B"))]
    for s in streams:
        svo.lib.svo_stream_synchronize(s)
    for which, (m, buf) in jobs:
        assert_depth_equal(depth_of(m, buf), single[which], f"two streams, map {which}")
        buf.free()
    for s in streams:
        hip.hipStreamDestroy(C.c_void_p(s))


def test_example_on_gpu(svo):
    from test_shadowmap_cpu import EXAMPLE, build_example
    build_example()
    r = subprocess.run([EXAMPLE, "6", "256"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map 256x256" in r.stdout and " 0 bad" in r.stdout


def test_variants(svo, oracle):
    """The render and the apply case through every library of `make variants` (SVO_AMD_LIB; one library per process, one after the other)."""
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
    scene_ = Scene(svo_, ob_)
    for kernel_ in (2, 1):
        for semantics_ in (0, 1):
            render_case(svo_, scene_, "A", kernel_, semantics_)
        apply_case(svo_, ob_, scene_, "A", kernel_)
    scene_.W.destroy()
    print("shadow map: depth image and flags equal to the model's")
