"""GPU parity: the HIP kernels (through the C ABI) against the CPU oracle on the same octree.

Bar (BASELINE.json north_star / SURVEY.md App. D): hit flag, chunk, node, brick cell and material
bit-exact; t within 1e-4*max(1,t) and normal within 1e-6 (helpers.py also requires t bit-equal,
which is what the kernels are built to deliver).
"""
import numpy as np
import pytest

from helpers import FUZZ_CASES, adversarial_rays, assert_gbuffer_equal, chunks_of, creeping_rays, guard_boundary_rays, random_rays

pytestmark = pytest.mark.gpu

KERNELS = ["literal", "stack"]


def _kid(svo, name):
    return {"literal": svo.KERNEL_LITERAL, "stack": svo.KERNEL_STACK}[name]


@pytest.fixture(scope="module")
def worlds(svo, oracle):
    """(name) -> (product world uploaded, oracle world over the SAME arrays, box)."""
    out = {}
    specs = {
        "c1_depth8": dict(w=1, h=1, d=1, depth=8, ccm=(0, 0, 0)),            # BASELINE configs[0] scene
        "grid_2x1x2_d6": dict(w=2, h=1, d=2, depth=6, ccm=(0, 0, 0)),
        "grid_neg_2x2x2_d5": dict(w=2, h=2, d=2, depth=5, ccm=(-1, -1, -1)),  # negative coords: index_float off-by-one path
        "depth2": dict(w=1, h=1, d=1, depth=2, ccm=(0, 0, 0)),               # root is a TWIG / LEAF / EMPTY
        "depth10": dict(w=1, h=1, d=1, depth=10, ccm=(0, 0, 0)),
    }
    for name, s in specs.items():
        W = svo.World.generate(s["w"], s["h"], s["d"], 128, s["depth"], chunkcoordmin=s["ccm"])
        n = s["w"] * s["h"] * s["d"]
        O = oracle.OracleWorld.from_chunks(chunks_of(W, n), s["w"], s["h"], s["d"], 128, s["ccm"])
        W.upload(0)
        lo = np.array(s["ccm"], dtype=np.float64) * 128
        hi = lo + np.array([s["w"], s["h"], s["d"]]) * 128
        out[name] = (W, O, lo, hi, s)
    yield out
    for W, O, *_ in out.values():
        W.destroy()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["c1_depth8", "grid_2x1x2_d6", "grid_neg_2x2x2_d5", "depth2", "depth10"])
def test_random_rays(svo, oracle, worlds, name, kernel):
    W, O, lo, hi, _ = worlds[name]
    rng = np.random.default_rng(1234)
    o, d = random_rays(rng, 20000, lo, hi)
    want = O.trace_rays(o, d, threads=8)
    got = W.chunkmarch(o, d, kernel=_kid(svo, kernel))
    assert (want["flags"] & 1).sum() > 1000
    assert_gbuffer_equal(got, want, f"{name}/{kernel}")


@pytest.mark.parametrize("kernel", KERNELS)
def test_shadow_rays(svo, oracle, worlds, kernel):
    W, O, lo, hi, _ = worlds["grid_2x1x2_d6"]
    rng = np.random.default_rng(7)
    o, d = random_rays(rng, 20000, lo, hi)
    want = O.trace_rays(o, d, params=oracle.make_params(shadow=True), threads=8)
    got = W.chunkmarch(o, d, shadow=True, kernel=_kid(svo, kernel))
    assert ((want["flags"] & svo.SHADOWED) != 0).sum() > 100
    assert_gbuffer_equal(got, want, f"shadow/{kernel}")
    assert W.last_ray_count() == O.last_rays


@pytest.mark.parametrize("kernel", KERNELS)
def test_camera_image_c1(svo, oracle, worlds, kernel):
    """BASELINE configs[0]: 256x256 primary rays, depth-8 single chunk."""
    W, O, lo, hi, s = worlds["c1_depth8"]
    cam = svo.default_camera(1, 1, 128, 256, 256)
    want = O.trace_image(cam, threads=8)
    got = W.draw(cam, kernel=_kid(svo, kernel))
    assert (want["flags"] & 1).mean() > 0.1
    assert_gbuffer_equal(got, want, f"c1/{kernel}")


@pytest.mark.parametrize("kernel", KERNELS)
def test_camera_rect_and_bands(svo, oracle, worlds, kernel):
    W, O, lo, hi, s = worlds["grid_2x1x2_d6"]
    cam = svo.default_camera(2, 2, 128, 200, 120)       # ragged: not a multiple of the 8x8 tile
    full = O.trace_image(cam, params=oracle.make_params(shadow=True), threads=8)
    got = W.draw(cam, shadow=True, kernel=_kid(svo, kernel))
    assert_gbuffer_equal(got, full, f"full/{kernel}")
    sub = W.draw(cam, rect=(37, 11, 101, 53), shadow=True, kernel=_kid(svo, kernel))
    assert_gbuffer_equal(sub, full[11:64, 37:138], f"rect/{kernel}")
    # interleaved bands (the multi-GPU partition): rank 1 of 2, 8-row bands
    nb = (120 // 8 + 1) // 2
    buf = svo.DeviceBuffer(nb * 8 * 200 * 32)
    W.trace_rows(cam, svo.trace_params(shadow=True, kernel=_kid(svo, kernel)), 1, 2, nb, 8, buf.ptr)
    svo.lib.svo_stream_synchronize(None)
    bands = buf.to_numpy(svo.HIT_DTYPE, nb * 8 * 200).reshape(nb, 8, 200)
    for k in range(nb):
        y0 = (1 + 2 * k) * 8
        rows = full[y0:y0 + 8]
        assert_gbuffer_equal(bands[k, :rows.shape[0]], rows, f"band{k}/{kernel}")
        if rows.shape[0] < 8:
            assert np.all(bands[k, rows.shape[0]:]["flags"] == 0)


@pytest.mark.parametrize("kernel", KERNELS)
def test_edge_case_rays(svo, oracle, worlds, kernel):
    """Axis-parallel rays (inf/NaN reciprocals), origins on faces/corners, outside the world, inside solid."""
    W, O, lo, hi, s = worlds["grid_2x1x2_d6"]
    o, d = [], []
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    rng = np.random.default_rng(3)
    for a in axes:
        for _ in range(300):
            p = lo + rng.random(3) * (hi - lo)
            o.append(p); d.append(a)
        # origin exactly on a world face / corner, and exactly on voxel lattice planes
        o.append(lo); d.append(a)
        o.append(hi); d.append(a)
        o.append((64.0, 32.0, 64.0)); d.append(a)
        o.append((0.0, 0.0, 0.0)); d.append(a)
        o.append((128.0, 16.0, 128.0)); d.append(a)          # on the chunk seam
        o.append((-50.0, 20.0, 60.0)); d.append(a)           # outside, may or may not enter
        o.append((300.0, 500.0, 60.0)); d.append(a)
    # deep inside solid terrain, and high in the sky looking down
    for _ in range(500):
        o.append((rng.random() * 256, 1.0, rng.random() * 256)); d.append(rng.normal(size=3))
        o.append((rng.random() * 256, 127.0, rng.random() * 256)); d.append((0.001 * rng.normal(), -1.0, 0.001 * rng.normal()))
    # zero direction and NaN direction: must terminate as misses
    o.append((10.0, 100.0, 10.0)); d.append((0.0, 0.0, 0.0))
    o.append((10.0, 100.0, 10.0)); d.append((np.nan, 1.0, 0.0))
    o = np.array(o, dtype=np.float32)
    d = np.array(d, dtype=np.float64)
    nrm = np.linalg.norm(d, axis=1, keepdims=True)
    d = np.where(nrm > 0, d / np.where(nrm > 0, nrm, 1), d).astype(np.float32)
    want = O.trace_rays(o, d, threads=8)
    got = W.chunkmarch(o, d, kernel=_kid(svo, kernel))
    assert_gbuffer_equal(got, want, f"edge/{kernel}")


@pytest.mark.parametrize("kernel", KERNELS)
def test_empty_and_tiny_launches(svo, oracle, worlds, kernel):
    W, O, lo, hi, s = worlds["c1_depth8"]
    got = W.chunkmarch(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), kernel=_kid(svo, kernel))
    assert got.shape == (0,)
    o = np.array([[64, 120, 64]], np.float32); d = np.array([[0, -1, 0]], np.float32)
    assert_gbuffer_equal(W.chunkmarch(o, d, kernel=_kid(svo, kernel)), O.trace_rays(o, d), "single")


def test_counters_match_oracle(svo, oracle, worlds):
    """The literal kernel's reference work counters (used to price algorithmic bytes) equal the oracle's."""
    W, O, lo, hi, s = worlds["grid_2x1x2_d6"]
    rng = np.random.default_rng(11)
    o, d = random_rays(rng, 5000, lo, hi)
    want, wc = O.trace_rays(o, d, params=oracle.make_params(shadow=True), counters=True, threads=8)
    got, gc = W.chunkmarch(o, d, shadow=True, kernel=svo.KERNEL_LITERAL, counters=True)
    assert_gbuffer_equal(got, want, "counters")
    assert np.array_equal(gc, wc)


def test_auto_kernel_is_stack_and_literal_agrees(svo, worlds):
    W, O, lo, hi, s = worlds["depth10"]
    assert W.info.exact_geometry == 1
    cam = svo.default_camera(1, 1, 128, 320, 200)
    a = W.draw(cam, shadow=True, kernel=svo.KERNEL_AUTO)
    b = W.draw(cam, shadow=True, kernel=svo.KERNEL_LITERAL)
    assert_gbuffer_equal(a, b, "auto-vs-literal")


def test_inexact_geometry_uses_literal(svo, oracle):
    """Chunk size 100 (not a power of two): voxel corners are not exact floats -> stack kernel refused, literal used."""
    W0 = svo.World.generate(1, 1, 1, 100, 6)
    assert W0.info.exact_geometry == 0
    O = oracle.OracleWorld.from_chunks(chunks_of(W0, 1), 1, 1, 1, 100)
    W0.upload(0)
    rng = np.random.default_rng(5)
    o, d = random_rays(rng, 5000, (0, 0, 0), (100, 100, 100))
    assert_gbuffer_equal(W0.chunkmarch(o, d), O.trace_rays(o, d, threads=8), "size100")
    with pytest.raises(svo.SvoError):
        W0.chunkmarch(o, d, kernel=svo.KERNEL_STACK)
    W0.destroy()


def test_world_update_after_edits(svo, oracle):
    """World::modify path: the oracle's restatement of Ocroot::build / destroy edits a chunk (dirty ranges = Ocdelta),
    svo_world_update re-sends the ranges (in place, and by re-packing when the pools outgrow their slot), and the
    march over the edited world matches the oracle again."""
    import ctypes as C
    O = oracle.OracleWorld.generate(2, 1, 1, 128, 6)
    W = svo.World.create([O.chunk(i) for i in range(2)], 2, 1, 1, 128)
    W.upload(0)
    rng = np.random.default_rng(99)
    o, d = random_rays(rng, 8000, (0, 0, 0), (256, 128, 128))
    assert_gbuffer_equal(W.chunkmarch(o, d, shadow=True), O.trace_rays(o, d, params=oracle.make_params(shadow=True), threads=8), "before")
    edits = [("build", (20, 60, 20), (50, 90, 50), 5), ("destroy", (0, 0, 0), (128, 40, 30), 0),
             ("build", (100, 100, 100), (101, 101, 101), 5), ("destroy", (30, 70, 30), (40, 80, 40), 0)]
    for kind, lo, hi, mat in edits:
        dt, dw = oracle.Delta(), oracle.Delta()
        root = C.byref(O.w.chunk[0])
        if kind == "build":
            oracle.lib.orc_build(root, oracle.vec3(lo), oracle.vec3(hi), mat, C.byref(dt), C.byref(dw))
        else:
            oracle.lib.orc_destroy(root, oracle.vec3(lo), oracle.vec3(hi), C.byref(dt), C.byref(dw))
        c = O.chunk(0)
        W.update(0, c, tree_range=(min(dt.left, c["tree"].size), dt.right), twig_range=(min(dw.left, c["twig"].size // 64), dw.right),
                 realloc=bool(dt.realloc_ or dw.realloc_))
        want = O.trace_rays(o, d, params=oracle.make_params(shadow=True), threads=8)
        for k in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
            assert_gbuffer_equal(W.chunkmarch(o, d, shadow=True, kernel=k), want, f"after {kind} {lo}")
    # the edits really changed the picture
    assert (want["material"] == 5).sum() > 0
    W.destroy()


def test_world_update_patches_its_host_copy_and_takes_a_bad_patch_back(svo, oracle):
    """svo_world_update without `realloc` patches the library's host copy over the dirty ranges (plus what was appended) instead of
    copying the chunk: after a sequence of such updates svo_world_chunk returns the caller's pools word for word; an update whose dirty
    range carries a malformed node is refused and leaves both copies - host and HBM - as they were; the next good update goes through."""
    import ctypes as C
    O = oracle.OracleWorld.generate(1, 1, 1, 128, 7)
    W = svo.World.create([O.chunk(0)], 1, 1, 1, 128)
    W.upload(0)
    rng = np.random.default_rng(5)
    o, d = random_rays(rng, 6000, (0, 0, 0), (128, 128, 128))
    patched = 0
    for k in range(12):
        lo = rng.uniform(5, 100, 3); hi = lo + rng.uniform(0.5, 25, 3)
        dt, dw = oracle.Delta(), oracle.Delta()
        root = C.byref(O.w.chunk[0])
        if k % 3 == 2:
            oracle.lib.orc_destroy(root, oracle.vec3(lo), oracle.vec3(hi), C.byref(dt), C.byref(dw))
        else:
            oracle.lib.orc_build(root, oracle.vec3(lo), oracle.vec3(hi), 3 + k % 4, C.byref(dt), C.byref(dw))
        c = O.chunk(0)
        realloc = bool(dt.realloc_ or dw.realloc_)
        patched += not realloc
        W.update(0, c, tree_range=(min(dt.left, c["tree"].size), dt.right), twig_range=(min(dw.left, c["twig"].size // 64), dw.right), realloc=realloc)
        mine = W.chunk(0)
        assert np.array_equal(mine["tree"], c["tree"]) and np.array_equal(mine["twig"], c["twig"]), f"host copy after update {k}"
    assert patched >= 6
    want = O.trace_rays(o, d, params=oracle.make_params(shadow=True), threads=8)
    for kern in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
        assert_gbuffer_equal(W.chunkmarch(o, d, shadow=True, kernel=kern), want, f"after patched updates/{kern}")
    # a malformed node inside the dirty range: refused, nothing changes
    good = O.chunk(0)
    bad = dict(good); bad["tree"] = good["tree"].copy()
    victim = int(np.nonzero((bad["tree"] >> 30) == 2)[0][-1])                   # the last BRANCH: send it past the pool
    bad["tree"][victim] = (2 << 30) | (bad["tree"].size + 8)
    with pytest.raises(svo.SvoError) as e:
        W.update(0, bad, tree_range=(victim, victim + 1), twig_range=(0, 0))
    assert e.value.code == -4
    mine = W.chunk(0)
    assert np.array_equal(mine["tree"], good["tree"]) and np.array_equal(mine["twig"], good["twig"]), "a refused patch is taken back"
    assert_gbuffer_equal(W.chunkmarch(o, d, shadow=True, kernel=svo.KERNEL_STACK), want, "after the refused update")
    dt, dw = oracle.Delta(), oracle.Delta()
    oracle.lib.orc_build(C.byref(O.w.chunk[0]), oracle.vec3((60, 100, 60)), oracle.vec3((64, 104, 64)), 6, C.byref(dt), C.byref(dw))
    c = O.chunk(0)
    W.update(0, c, tree_range=(min(dt.left, c["tree"].size), dt.right), twig_range=(min(dw.left, c["twig"].size // 64), dw.right), realloc=bool(dt.realloc_ or dw.realloc_))
    want = O.trace_rays(o, d, params=oracle.make_params(shadow=True), threads=8)
    assert_gbuffer_equal(W.chunkmarch(o, d, shadow=True, kernel=svo.KERNEL_STACK), want, "the next good update")
    W.destroy()


# (a wide-tree rebuild that fails - fault injection - behind svo_world_update / edit_box / shift: tests/test_variants.py, `hooks`;
# the shipped library no longer reads the injection variable)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("eps,caps,light", [
    (1.0 / 4096.0, (0, 0, 0), (1.0, -1.0, 0.0)),          # the GLSL twin's EPS
    (0.0, (2, 7, 3), (0.3, -0.8, 0.5)),                   # tiny step caps: most rays give up early, exactly like the oracle
    (1.0 / 1024.0, (3, 1000, 2), (0.0, -1.0, 0.0)),       # vertical light: axis-parallel shadow rays
])
def test_custom_eps_caps_and_light(svo, oracle, worlds, kernel, eps, caps, light):
    W, O, lo, hi, _ = worlds["grid_2x1x2_d6"]
    rng = np.random.default_rng(21)
    o, d = random_rays(rng, 12000, lo, hi)
    want = O.trace_rays(o, d, params=oracle.make_params(shadow=True, light_dir=light, eps=eps, caps=caps), threads=8)
    got = W.chunkmarch(o, d, shadow=True, kernel=_kid(svo, kernel), light_dir=light, eps=eps, caps=caps)
    assert_gbuffer_equal(got, want, f"custom/{kernel}")
    assert (want["flags"] & 1).sum() > 300


def test_packed_gbuffer_roundtrip(svo, worlds):
    """svo_gbuffer_pack / unpack: t, normal, material and flags survive the 8-byte form bit for bit (ids are dropped)."""
    W, O, lo, hi, _ = worlds["grid_2x1x2_d6"]
    cam = svo.default_camera(2, 2, 128, 333, 177)
    g = W.draw(cam, shadow=True)
    # add rays that start inside solid (NaN normals) through the list interface
    rng = np.random.default_rng(4)
    o = np.stack([rng.random(500) * 256, np.full(500, 1.0), rng.random(500) * 256], axis=1).astype(np.float32)
    d = np.tile(np.array([[0, 1, 0]], np.float32), (500, 1))
    g2 = W.chunkmarch(o, d)
    allg = np.concatenate([g.reshape(-1), g2])
    n = allg.size
    a = svo.DeviceBuffer.from_numpy(allg); p = svo.DeviceBuffer(n * 8); b = svo.DeviceBuffer(n * 32)
    svo.gbuffer_pack(a.ptr, p.ptr, n); svo.gbuffer_unpack(p.ptr, b.ptr, n)
    svo.lib.svo_stream_synchronize(None)
    back = b.to_numpy(svo.HIT_DTYPE, n)
    assert np.array_equal(back["t"].view(np.uint32), allg["t"].view(np.uint32))
    assert np.array_equal(back["material"], allg["material"]) and np.array_equal(back["flags"], allg["flags"])
    nb, na = back["normal"], allg["normal"]
    same = (nb.view(np.uint32) == na.view(np.uint32)) | (np.isnan(nb) & np.isnan(na)) | ((nb == 0) & (na == 0))   # -0 vs +0 components
    assert np.all(same)
    assert np.isnan(allg["normal"]).any() and ((allg["flags"] & 4) != 0).any()
    assert np.all(back["node"] == 0) and np.all(back["cell"] == 0)


def test_trace_argument_errors(svo, worlds):
    W, O, lo, hi, _ = worlds["c1_depth8"]
    cam = svo.default_camera(1, 1, 128, 64, 64)
    buf = svo.DeviceBuffer(64 * 64 * 32)
    for rect in [(-1, 0, 8, 8), (0, 0, -8, 8)]:
        with pytest.raises(svo.SvoError) as e:
            W.trace(cam, svo.trace_params(), rect, buf.ptr)
        assert e.value.code == -1
    with pytest.raises(svo.SvoError) as e:
        W.trace(cam, svo.trace_params(), (0, 0, 8, 8), 0)             # null output
    assert e.value.code == -1
    with pytest.raises(svo.SvoError) as e:
        W.trace_rows(cam, svo.trace_params(), 0, 0, 4, 8, buf.ptr)    # band_stride 0
    assert e.value.code == -1
    with pytest.raises(svo.SvoError) as e:
        W.trace(cam, svo.trace_params(kernel=7), (0, 0, 8, 8), buf.ptr)
    assert e.value.code == -1
    W.trace(cam, svo.trace_params(), (0, 0, 0, 0), buf.ptr)           # empty rectangle: no-op
    assert W.last_ray_count() == 0


def test_launch_ring_wraps_without_sync(svo, worlds):
    """200 unsynchronised launches over 3 streams (the work-cursor ring has 64 slots): every frame complete and equal."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so.7")                 # the runtime the library is already linked against
    W, O, lo, hi, _ = worlds["grid_2x1x2_d6"]
    cam = svo.default_camera(2, 2, 128, 160, 96)
    ref = W.draw(cam, shadow=True).reshape(-1)
    streams = []
    for _ in range(3):
        h = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(h)) == 0
        streams.append(h.value)
    bufs = [svo.DeviceBuffer(160 * 96 * 32) for _ in range(200)]
    prm = svo.trace_params(shadow=True, kernel=svo.KERNEL_STACK)
    for i, b in enumerate(bufs):
        W.trace(cam, prm, (0, 0, 160, 96), b.ptr, streams[i % 3])
    for s in streams:
        svo.lib.svo_stream_synchronize(s)
    rays = W.last_ray_count(streams[(len(bufs) - 1) % 3])
    assert rays == 160 * 96 + int((ref["flags"] & 1).sum())
    for i in (0, 1, 63, 64, 65, 127, 128, 199):
        got = bufs[i].to_numpy(svo.HIT_DTYPE, 160 * 96)
        assert got.tobytes() == ref.tobytes(), f"launch {i} differs"
    for s in streams:
        hip.hipStreamDestroy(ctypes.c_void_p(s))


@pytest.mark.parametrize("tpw", [0, 4, 64, 100000])
def test_tiles_per_wave_is_only_a_launch_shape(svo, worlds, tpw):
    """svo_trace_params.tiles_per_wave changes how many persistent waves share the tiles, never the records."""
    W, O, lo, hi, _ = worlds["grid_2x1x2_d6"]
    cam = svo.default_camera(2, 2, 128, 203, 131)
    ref = W.draw(cam, shadow=True, kernel=svo.KERNEL_LITERAL).reshape(-1)
    buf = svo.DeviceBuffer(203 * 131 * 32)
    W.trace(cam, svo.trace_params(shadow=True, kernel=svo.KERNEL_STACK, tiles_per_wave=tpw), (0, 0, 203, 131), buf.ptr)
    svo.lib.svo_stream_synchronize(None)
    assert buf.to_numpy(svo.HIT_DTYPE, 203 * 131).tobytes() == ref.tobytes()


@pytest.mark.parametrize("nfl", [2, 4, 8, 1000])
def test_launches_in_flight_is_only_a_launch_shape(svo, worlds, nfl):
    """svo_trace_params.launches_in_flight shrinks the persistent grid to 2/n of the wave slots, never the records."""
    W, O, lo, hi, _ = worlds["grid_2x1x2_d6"]
    cam = svo.default_camera(2, 2, 128, 203, 131)
    ref = W.draw(cam, shadow=True, kernel=svo.KERNEL_LITERAL).reshape(-1)
    buf = svo.DeviceBuffer(203 * 131 * 32)
    W.trace(cam, svo.trace_params(shadow=True, kernel=svo.KERNEL_STACK, tiles_per_wave=4, launches_in_flight=nfl), (0, 0, 203, 131), buf.ptr)
    svo.lib.svo_stream_synchronize(None)
    assert buf.to_numpy(svo.HIT_DTYPE, 203 * 131).tobytes() == ref.tobytes()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("nframes", [1, 3, 16])
def test_frames_in_one_launch_equal_separate_traces(svo, worlds, kernel, nframes):
    """svo_trace_frames / svo_trace_rows_frames: F cameras behind one set of cursors == F separate launches."""
    W, O, lo, hi, _ = worlds["grid_2x1x2_d6"]
    w, h = 171, 93
    cams = [svo.make_camera((100.0 + 9.0 * f, 140.0 - 5.0 * f, -30.0 + 4.0 * f), (0.05 * f, -0.5, 0.8), (0.0, 1.0, 0.0), 50.0 + 3 * f, w, h)
            for f in range(nframes)]
    prm = svo.trace_params(shadow=True, kernel=_kid(svo, kernel), tiles_per_wave=2)
    single = []
    one = svo.DeviceBuffer(w * h * 32)
    for c in cams:
        W.trace(c, prm, (0, 0, w, h), one.ptr)
        svo.lib.svo_stream_synchronize(None)
        single.append(one.to_numpy(svo.HIT_DTYPE, w * h).copy())
    allb = svo.DeviceBuffer(nframes * w * h * 32)
    W.trace_frames(cams, prm, (0, 0, w, h), allb.ptr)
    svo.lib.svo_stream_synchronize(None)
    got = allb.to_numpy(svo.HIT_DTYPE, nframes * w * h).reshape(nframes, w * h)
    rays = W.last_ray_count()
    for f in range(nframes):
        assert got[f].tobytes() == single[f].tobytes(), f"frame {f} differs"
    if kernel == "stack":
        assert rays == sum(w * h + int((s["flags"] & 1).sum()) for s in single)
    # interleaved bands of every frame (rank 1 of 3, 8-row bands; the last band hangs over the image)
    nb = svo.partition.bands_per_rank(h, 3, 8)
    bands = svo.DeviceBuffer(nframes * nb * 8 * w * 32)
    W.trace_rows_frames(cams, prm, 1, 3, nb, 8, bands.ptr)
    svo.lib.svo_stream_synchronize(None)
    gb = bands.to_numpy(svo.HIT_DTYPE, nframes * nb * 8 * w).reshape(nframes, nb, 8, w)
    for f in range(nframes):
        full = single[f].reshape(h, w)
        for k in range(nb):
            r0 = (1 + 3 * k) * 8
            rows = min(8, max(0, h - r0))
            assert gb[f, k, :rows].tobytes() == full[r0:r0 + rows].tobytes(), f"frame {f} band {k}"
            assert not (gb[f, k, rows:]["flags"] & 1).any()


def test_frames_argument_errors(svo, worlds):
    W, O, lo, hi, _ = worlds["c1_depth8"]
    buf = svo.DeviceBuffer(17 * 64 * 64 * 32)
    cams = [svo.default_camera(1, 1, 128, 64, 64) for _ in range(svo.MAX_FRAMES + 1)]
    with pytest.raises(svo.SvoError) as e:
        W.trace_frames(cams, svo.trace_params(), (0, 0, 64, 64), buf.ptr)          # more than SVO_MAX_FRAMES
    assert e.value.code == -1
    mixed = [svo.default_camera(1, 1, 128, 64, 64), svo.default_camera(1, 1, 128, 32, 64)]
    with pytest.raises(svo.SvoError) as e:
        W.trace_frames(mixed, svo.trace_params(), (0, 0, 32, 32), buf.ptr)         # one image size per launch
    assert e.value.code == -1


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["grid_2x1x2_d6", "grid_neg_2x2x2_d5", "depth10"])
@pytest.mark.parametrize("eps,caps,chunk_faces", [
    (0.0, (0, 0, 0), False),                  # EPS 1/8192, caps 1000/1000/1000: creeps of thousands of steps, cut by the caps
    (1.0 / 4096.0, (40, 300, 25), True),      # another power of two; small caps end the creeps in the middle of a run
    (0.0, (20, 0, 60), True),                 # pinned on chunk faces: chunkmarch, treemarch and twigmarch creep together
    (1.0e-4, (0, 0, 0), False),               # not a power of two: the stack kernel's closed form does not apply, the general step does
])
def test_creeping_rays(svo, oracle, worlds, name, kernel, eps, caps, chunk_faces):
    """Rays pinned on lattice planes (src/Traverse.cpp:25-32: escape == -0, t += EPS per step).  The stack kernel takes
    such stretches in closed form (kernel_stack.hip.h, creep block); every record must still equal the oracle's, which
    walks them step by step - including the step caps running out inside a stretch (src/Traverse.cpp:54,79,142)."""
    W, O, lo, hi, s = worlds[name]
    rng = np.random.default_rng(77)
    o, d = creeping_rays(rng, 6000, lo, hi, 128.0 / (1 << s["depth"]), chunk_faces)
    prm = oracle.make_params(shadow=True, eps=eps, caps=caps)
    want, wc = O.trace_rays(o, d, params=prm, counters=True, threads=8)
    steps = wc[:, 1].astype(np.int64) + wc[:, 2] + wc[:, 3]
    assert steps.max() < (1 << 22)            # below the kernels' runaway guard (SVO_ERR_FLAG)
    got = W.chunkmarch(o, d, shadow=True, kernel=_kid(svo, kernel), eps=eps, caps=caps)
    assert_gbuffer_equal(got, want, f"creep/{name}/{kernel}")
    # the list really contains long creeps: rays with far more steps than any ordinary ray of these worlds takes
    assert (steps > 400).sum() >= 5 and (want["flags"] & 1).sum() > 300


def test_fuzz_one_million_adversarial_rays(svo, oracle):
    """A 1 M-ray cut of scripts/fuzz_parity.py: four worlds (negative chunk coordinates, depth 6-11), two lights, both
    kernels, every record against the oracle."""
    threads = 16
    for i, c in enumerate(FUZZ_CASES):
        W = svo.World.generate(c["w"], c["h"], c["d"], 128, c["depth"], chunkcoordmin=c["ccm"])
        n = c["w"] * c["h"] * c["d"]
        O = oracle.OracleWorld.from_chunks([W.chunk(j, copy=False) for j in range(n)], c["w"], c["h"], c["d"], 128, c["ccm"])
        W.upload(0)
        lo = np.array(c["ccm"], float) * 128
        hi = lo + np.array([c["w"], c["h"], c["d"]]) * 128
        o, d = adversarial_rays(np.random.default_rng(1000 + i), 125000, lo, hi)
        for light in ((1.0, -1.0, 0.0), (0.2, -0.9, 0.4)):
            want = O.trace_rays(o, d, params=oracle.make_params(shadow=True, light_dir=light), threads=threads)
            for k in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
                got = W.chunkmarch(o, d, shadow=True, kernel=k, light_dir=light)
                assert_gbuffer_equal(got, want, f"fuzz {c} kernel {k} light {light}")
        W.destroy()


def test_rays_around_the_sure_miss_conditions(svo, oracle):
    """The stack kernel's draining waves do not enter a brick whose march is bound to miss (step_asm_body.inc; src/Traverse.cpp:99-105
    resumes the tree level from the brick's entry point whatever twigmarch did).  Its proof has three conditions - p(t_miss) provably
    outside the node's box, no backward step (|beta_k| EPS 2^22 >= edge, or beta_k = 0), not creeping - and these lists sit on them:
    direction components around the guard's threshold, exactly 0, denormal; origins on and next to brick lattice planes, the planes
    through 0 of worlds with negative coordinates among them.  Short lists too: a launch of a few waves is all drain.  Both
    semantics (tests/test_variants.py runs the same lists with the test forced into every wave-step, variants suremiss / suremiss64)."""
    for c, n in ((FUZZ_CASES[1], 60000), (FUZZ_CASES[2], 60000), (FUZZ_CASES[3], 3000), (FUZZ_CASES[0], 700)):
        W = svo.World.generate(c["w"], c["h"], c["d"], 128, c["depth"], chunkcoordmin=c["ccm"])
        nch = c["w"] * c["h"] * c["d"]
        O = oracle.OracleWorld.from_chunks([W.chunk(j, copy=False) for j in range(nch)], c["w"], c["h"], c["d"], 128, c["ccm"])
        W.upload(0)
        lo = np.array(c["ccm"], float) * 128
        hi = lo + np.array([c["w"], c["h"], c["d"]]) * 128
        edge = 4.0 * 128.0 / 2 ** c["depth"]
        for sem, eps in ((0, 1.0 / 8192), (1, 1.0 / 4096)):
            o, d = guard_boundary_rays(np.random.default_rng(77 + sem), n, lo, hi, edge, eps)
            want = O.trace_rays(o, d, params=oracle.make_params(shadow=True, semantics=sem), threads=16)
            for k in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
                got = W.chunkmarch(o, d, shadow=True, kernel=k, semantics=sem)
                assert_gbuffer_equal(got, want, f"guard {c} semantics {sem} kernel {k}")
        W.destroy()


def test_runaway_guard_flags_both_kernels(svo, oracle, worlds):
    """A ray pinned on a chunk face creeps in chunkmarch, treemarch and twigmarch at once: with caps 1000/1000/6 it takes
    7 M steps, more than the kernels' per-ray bound of 2^22 steps of their own counting.  A kernel that gives such a ray
    up records a miss flagged SVO_ERR_FLAG (the reference, and the oracle, walk on to a plain miss); the packed record
    keeps the flag.  With EPS a power of two the stack kernel takes the creeping stretches in closed form and may finish
    the ray - then exactly as the oracle does; with another EPS both kernels walk it step by step and both give up."""
    W, O, lo, hi, _ = worlds["grid_2x1x2_d6"]
    o = np.array([[128.0, 64.0, 32.0], [128.0, 61.67112731933594, 45.62421417236328], [100.3, 120.0, 77.7]], np.float32)
    d = np.array([[-3.2018779165809974e-06, -0.9999757409095764, -0.006965192500501871],
                  [-2.4640150968480157e-06, -0.2718605697154999, -0.9623366594314575], [0.3, -0.9, 0.1]], np.float32)
    caps = (1000, 1000, 6)
    for eps in (0.0, 1.0e-4):
        want, wc = O.trace_rays(o, d, params=oracle.make_params(caps=caps, eps=eps), counters=True, threads=3)
        steps = wc[:, 1].astype(np.int64) + wc[:, 2] + wc[:, 3]
        assert np.all(steps[:2] > 6_000_000) and np.all((want["flags"][:2] & 1) == 0) and steps[2] < 1000
        got = {}
        for k in KERNELS:
            g = W.chunkmarch(o, d, kernel=_kid(svo, k), caps=caps, eps=eps)
            gave_up = g["flags"][:2] == svo.ERR_FLAG
            if k == "literal" or eps != 0.0:
                assert np.all(gave_up), f"{k}: runaway rays must be misses flagged SVO_ERR_FLAG"
            assert np.all(gave_up | (g["flags"][:2] == 0)), f"{k}: a runaway ray is given up or finished like the oracle (a miss)"
            assert np.all(g["t"][:2] == 0) and np.all(g["material"][:2] == 0)
            assert_gbuffer_equal(g[2:], want[2:], f"ordinary ray beside the runaway ones/{k}")
            got[k] = g
        if eps != 0.0:
            assert got["literal"].tobytes() == got["stack"].tobytes()
    a = svo.DeviceBuffer.from_numpy(got["stack"]); p = svo.DeviceBuffer(3 * 8); b = svo.DeviceBuffer(3 * 32)
    svo.gbuffer_pack(a.ptr, p.ptr, 3); svo.gbuffer_unpack(p.ptr, b.ptr, 3)
    svo.lib.svo_stream_synchronize(None)
    assert np.array_equal(b.to_numpy(svo.HIT_DTYPE, 3)["flags"], got["stack"]["flags"]) and (got["stack"]["flags"][0] & svo.ERR_FLAG)


def test_update_is_ordered_behind_queued_launches(svo, oracle):
    """svo_world_update while launches of the world are queued on a non-blocking stream (the null stream's copies are not
    ordered against such a stream): every launch issued before the update shows the old world, every launch after it the
    new one, none a mixture (World::modify on the GL queue, src/World.cpp:268-274)."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so.7")
    st = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0            # hipStreamNonBlocking
    O = oracle.OracleWorld.generate(2, 1, 1, 128, 7)
    W = svo.World.create([O.chunk(i) for i in range(2)], 2, 1, 1, 128)
    W.upload(0)
    cam = svo.make_camera((120.0, 150.0, -60.0), (0.05, -0.55, 0.83), (0.0, 1.0, 0.0), 60.0, 480, 270)
    prm_o = oracle.make_params(shadow=True)
    before = O.trace_image(cam, params=prm_o, threads=8)
    dt, dw = oracle.Delta(), oracle.Delta()
    oracle.lib.orc_destroy(C.byref(O.w.chunk[0]), oracle.vec3((0, 0, 0)), oracle.vec3((128, 128, 90)), C.byref(dt), C.byref(dw))
    after = O.trace_image(cam, params=prm_o, threads=8)
    assert not np.array_equal(before["flags"], after["flags"])
    prm = svo.trace_params(shadow=True, kernel=svo.KERNEL_STACK)
    n = 24
    bufs = [svo.DeviceBuffer(480 * 270 * 32) for _ in range(2 * n)]
    for b in bufs[:n]:
        W.trace(cam, prm, (0, 0, 480, 270), b.ptr, st.value)             # queued, not waited for
    c = O.chunk(0)
    W.update(0, c, tree_range=(min(dt.left, c["tree"].size), dt.right), twig_range=(min(dw.left, c["twig"].size // 64), dw.right),
             realloc=bool(dt.realloc_ or dw.realloc_))
    for b in bufs[n:]:
        W.trace(cam, prm, (0, 0, 480, 270), b.ptr, st.value)
    svo.lib.svo_stream_synchronize(st.value)
    for i, b in enumerate(bufs):
        assert_gbuffer_equal(b.to_numpy(svo.HIT_DTYPE, 480 * 270), (before if i < n else after), f"launch {i}")
    hip.hipStreamDestroy(st)
    W.destroy()


@pytest.mark.parametrize("kernel", KERNELS)
def test_face_normal_mode(svo, oracle, worlds, kernel):
    """svo_trace_params.normal_mode = SVO_NORMAL_FACE: the entered-face normal (an axis unit vector, never NaN), flagged
    SVO_FACE_NORMAL, equal to the oracle's restatement and to the reference's cubeNormal wherever that one names a face;
    it survives the packed record; mode 0 stays the reference's formula, NaNs and all."""
    W, O, lo, hi, _ = worlds["depth10"]
    cam = svo.default_camera(1, 1, 128, 480, 270)
    want = O.trace_image(cam, params=oracle.make_params(shadow=True, normal_mode=1), threads=8)
    got = W.draw(cam, shadow=True, kernel=_kid(svo, kernel), normal_mode=svo.NORMAL_FACE)
    assert_gbuffer_equal(got, want, f"face normal/{kernel}")
    hit = (got["flags"] & svo.HIT_FLAG) != 0
    assert hit.sum() > 20000 and np.all((got["flags"][hit] & svo.FACE_NORMAL) != 0) and not np.any(got["flags"][~hit] & svo.FACE_NORMAL)
    n = got["normal"][hit]
    assert not np.isnan(n).any()
    assert np.all(np.abs(n).sum(axis=1) == 1.0) and np.all((np.abs(n) == 1.0).sum(axis=1) == 1)       # +-1 on exactly one axis
    ref = W.draw(cam, shadow=True, kernel=_kid(svo, kernel))                                           # mode 0: cubeNormal
    assert not np.any(ref["flags"] & svo.FACE_NORMAL)
    for f in ("t", "material", "chunk", "node", "cell"):
        assert np.array_equal(ref[f], got[f])                                                          # only normal and the flag differ
    rn = ref["normal"][hit]
    face = (~np.isnan(rn).any(axis=1)) & ((np.abs(rn) == 1.0).sum(axis=1) == 1)                        # cubeNormal found one face
    assert np.isnan(rn).any() and face.mean() > 0.5
    assert np.array_equal(rn[face], n[face])
    # packed record round trip
    flat = got.reshape(-1)
    a = svo.DeviceBuffer.from_numpy(flat); p = svo.DeviceBuffer(flat.size * 8); b = svo.DeviceBuffer(flat.size * 32)
    svo.gbuffer_pack(a.ptr, p.ptr, flat.size); svo.gbuffer_unpack(p.ptr, b.ptr, flat.size)
    svo.lib.svo_stream_synchronize(None)
    back = b.to_numpy(svo.HIT_DTYPE, flat.size)
    assert np.array_equal(back["flags"], flat["flags"]) and np.array_equal(back["normal"][hit.reshape(-1)], n)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("depths", [[3, 5, 6, 8], [9, 2, 4, 7]], ids=["3-5-6-8", "9-2-4-7"])
def test_chunks_of_different_depths(svo, oracle, kernel, depths):
    """One world whose chunks have different depths (the reference's Ocroot carries its own depth, src/Octree.h:56-76, and
    its LOD pass re-grows single chunks at another one): lanes of one wave march trees of 1, 3, 4 and 6 branch levels -
    odd and even, i.e. with and without a padded top wide node - and cross from one into the other."""
    # depths[i]: chunk i of the 2x1x2 grid (depth 2: the chunk is one brick or one terminal node)
    gen = {d: svo.World.generate(2, 1, 2, 128, d) for d in sorted(set(depths))}
    chunks = [gen[d].chunk(i) for i, d in enumerate(depths)]
    assert [int(c["depth"]) for c in chunks] == depths
    W = svo.World.create(chunks, 2, 1, 2, 128)
    O = oracle.OracleWorld.from_chunks(chunks, 2, 1, 2, 128, (0, 0, 0))
    W.upload(0)
    assert W.info.exact_geometry
    lo = np.zeros(3); hi = np.array([256.0, 128.0, 256.0])
    rng = np.random.default_rng(99)
    o, d = random_rays(rng, 40000, lo, hi)
    want = O.trace_rays(o, d, threads=8)
    got = W.chunkmarch(o, d, kernel=_kid(svo, kernel))
    hit = (want["flags"] & 1) != 0
    assert hit.sum() > 2000 and len(set(want["chunk"][hit].tolist())) >= 3          # (a depth-2 chunk may be empty air)
    assert_gbuffer_equal(got, want, f"mixed depths rays/{kernel}")
    cam = svo.default_camera(2, 2, 128, 320, 180)
    want = O.trace_image(cam, params=oracle.make_params(shadow=True), threads=8)
    got = W.draw(cam, shadow=True, kernel=_kid(svo, kernel))
    assert_gbuffer_equal(got, want, f"mixed depths frame/{kernel}")
    o2, d2 = adversarial_rays(np.random.default_rng(5), 60000, lo, hi)
    assert_gbuffer_equal(W.chunkmarch(o2, d2, kernel=_kid(svo, kernel)), O.trace_rays(o2, d2, threads=8), f"mixed depths adversarial/{kernel}")
    W.destroy()
    for g in gen.values():
        g.destroy()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("chunksize,depth,ccm", [(32, 6, (0, 0, 0)), (512, 7, (-1, 0, -2)), (2, 5, (3, -1, 0)), (1024, 9, (0, 0, 0))])
def test_power_of_two_chunk_edges(svo, oracle, kernel, chunksize, depth, ccm):
    """Chunk edges other than the reference's 128 (src/World.cpp: CHUNKSIZE): any power of two keeps the geometry exact, so
    the stack kernel marches it - voxels of 1/16 world unit (edge 2, depth 5) up to 2 units (edge 1024, depth 9), world
    boxes off the origin."""
    W = svo.World.generate(2, 1, 2, chunksize, depth, chunkcoordmin=ccm)
    assert W.info.exact_geometry == 1
    chunks = chunks_of(W, 4)
    O = oracle.OracleWorld.from_chunks(chunks, 2, 1, 2, chunksize, ccm)
    W.upload(0)
    lo = np.array(ccm, dtype=np.float64) * chunksize
    hi = lo + np.array([2, 1, 2]) * chunksize
    rng = np.random.default_rng(chunksize + depth)
    for what, (o, d) in (("random", random_rays(rng, 30000, lo, hi)), ("adversarial", adversarial_rays(rng, 60000, lo, hi))):
        want = O.trace_rays(o, d, params=oracle.make_params(shadow=True), threads=8)
        got = W.chunkmarch(o, d, shadow=True, kernel=_kid(svo, kernel))
        assert (want["flags"] & 1).sum() > 1000, what
        assert_gbuffer_equal(got, want, f"chunk edge {chunksize} {what}/{kernel}")
    W.destroy()


def test_update_replaces_a_chunk_by_one_of_another_depth(svo, oracle):
    """svo_world_update with a chunk re-grown at another depth (what the reference's LOD pass does to an Ocroot): the
    pools, the chunk table, the chunk's wide tree and the kernel instantiation (LDS column height) follow - 4 branch
    levels everywhere, then 7 and 1 in two of the chunks."""
    W = svo.World.generate(2, 1, 2, 128, 6)
    other = {d: svo.World.generate(2, 1, 2, 128, d) for d in (9, 3)}
    chunks = chunks_of(W, 4)
    W.upload(0)
    cam = svo.default_camera(2, 2, 128, 320, 180)
    rng = np.random.default_rng(3)
    o, d = adversarial_rays(rng, 50000, np.zeros(3), np.array([256.0, 128.0, 256.0]))
    for step, (i, depth) in enumerate(((None, None), (1, 9), (2, 3))):
        if i is not None:
            chunks[i] = other[depth].chunk(i)
            W.update(i, chunks[i], tree_range=(0, chunks[i]["tree"].size), twig_range=(0, chunks[i]["twig"].size // 64), realloc=True)
            assert W.info.max_chunk_depth == max(int(c["depth"]) for c in chunks)
        O = oracle.OracleWorld.from_chunks(chunks, 2, 1, 2, 128, (0, 0, 0))
        want = O.trace_image(cam, params=oracle.make_params(shadow=True), threads=8)
        for kernel in KERNELS:
            assert_gbuffer_equal(W.draw(cam, shadow=True, kernel=_kid(svo, kernel)), want, f"after update {step}/{kernel}")
            assert_gbuffer_equal(W.chunkmarch(o, d, kernel=_kid(svo, kernel)), O.trace_rays(o, d, threads=8), f"rays after update {step}/{kernel}")
    W.destroy()
    for g in other.values():
        g.destroy()


def test_host_update_walks_in_place_tail_and_repack(svo, oracle, capfd, monkeypatch):
    """svo_world_update from host pools through all three placements of the install path it shares with the device-built chunks
    (shift, edit, compact): chunk 0, depth 4 among depth-7 chunks, is handed larger and larger versions of itself - another seed's
    chunk of the same depth (fits its slot), the chunk at depth 5 (outgrows its slot, fits the pools' tails) and at depth 7 (no room
    at the tails: the world is packed again).  The pools keep their size until the re-pack; svo_world_chunk returns what was sent
    and both kernels match the oracle after every step."""
    monkeypatch.setenv("SVO_BUILD_TIMING", "1")         # the install path names the placement it took on stderr
    gen = {}
    for depth, seed in ((4, 0), (4, 28), (5, 28), (7, 0)):
        g = svo.World.generate(2, 1, 2, 128, depth, seed=seed)
        gen[depth, seed] = chunks_of(g, 4)
        g.destroy()
    chunks = [gen[4, 0][0]] + gen[7, 0][1:]
    W = svo.World.create(chunks, 2, 1, 2, 128)
    W.upload(0)
    capfd.readouterr()
    o, d = random_rays(np.random.default_rng(17), 12000, (0, 0, 0), (256, 128, 256))
    pool = W.info.tree_pool_bytes
    for key, placement in (((4, 28), "in place"), ((5, 28), "tail"), ((7, 0), "re-pack")):
        new = gen[key][0]
        assert new["tree"].size > chunks[0]["tree"].size and new["twig"].size >= chunks[0]["twig"].size
        chunks[0] = new
        W.update(0, new, tree_range=(0, new["tree"].size), twig_range=(0, new["twig"].size // 64))
        err = capfd.readouterr().err
        assert ("chunk 0: in place" in err) == (placement == "in place"), (key, err)
        assert ("chunk 0: outgrew its slot" in err) == (placement != "in place"), (key, err)
        assert ("chunk 0: no room at the tails" in err) == (placement == "re-pack"), (key, err)
        assert (W.info.tree_pool_bytes == pool) == (placement != "re-pack"), key
        for i in range(4):
            got = W.chunk(i)
            assert np.array_equal(got["tree"], chunks[i]["tree"]) and np.array_equal(got["twig"], chunks[i]["twig"]), (key, i)
        O = oracle.OracleWorld.from_chunks(chunks, 2, 1, 2, 128, (0, 0, 0))
        want = O.trace_rays(o, d, params=oracle.make_params(shadow=True), threads=8)
        for k in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
            assert_gbuffer_equal(W.chunkmarch(o, d, shadow=True, kernel=k), want, f"after update {key}/{k}")
    W.destroy()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("band,stride", [(1, 2), (3, 3), (5, 2), (16, 3), (120, 1)])
def test_band_heights_other_than_the_tile_height(svo, oracle, worlds, kernel, band, stride):
    """svo_trace_rows with band heights that are not the stack kernel's 8-row tile height: tiles straddle bands (and the
    padding below the image), every rank's rows still equal the whole frame's."""
    W, O, lo, hi, s = worlds["grid_2x1x2_d6"]
    cam = svo.default_camera(2, 2, 128, 203, 117)
    full = O.trace_image(cam, params=oracle.make_params(shadow=True), threads=8)
    total = (117 + band - 1) // band
    nb = (total + stride - 1) // stride
    for rank in range(stride):
        buf = svo.DeviceBuffer(nb * band * 203 * 32)
        W.trace_rows(cam, svo.trace_params(shadow=True, kernel=_kid(svo, kernel)), rank, stride, nb, band, buf.ptr)
        svo.lib.svo_stream_synchronize(None)
        bands = buf.to_numpy(svo.HIT_DTYPE, nb * band * 203).reshape(nb, band, 203)
        for k in range(nb):
            y0 = (rank + stride * k) * band
            rows = full[y0:y0 + band]
            if rows.shape[0]:
                assert_gbuffer_equal(bands[k, :rows.shape[0]], rows, f"band {band} rank {rank} #{k}/{kernel}")
            assert np.all(bands[k, rows.shape[0]:]["flags"] == 0)


@pytest.mark.parametrize("kernel", KERNELS)
def test_frames_over_a_sub_rectangle(svo, worlds, kernel):
    """svo_trace_frames with a window that is not the whole image (and not tile-aligned): every frame's raster equals the
    same window of a single-frame trace."""
    W, O, lo, hi, _ = worlds["grid_2x1x2_d6"]
    w, h = 171, 93
    rect = (13, 7, 101, 53)
    cams = [svo.make_camera((100.0 + 9.0 * f, 140.0 - 5.0 * f, -30.0 + 4.0 * f), (0.05 * f, -0.5, 0.8), (0.0, 1.0, 0.0), 50.0 + 3 * f, w, h)
            for f in range(5)]
    prm = svo.trace_params(shadow=True, kernel=_kid(svo, kernel))
    n = rect[2] * rect[3]
    allb = svo.DeviceBuffer(len(cams) * n * 32)
    W.trace_frames(cams, prm, rect, allb.ptr)
    svo.lib.svo_stream_synchronize(None)
    got = allb.to_numpy(svo.HIT_DTYPE, len(cams) * n).reshape(len(cams), rect[3], rect[2])
    for f, c in enumerate(cams):
        full = W.draw(c, shadow=True, kernel=_kid(svo, kernel))
        assert got[f].tobytes() == np.ascontiguousarray(full[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]).tobytes(), f"frame {f}"


@pytest.mark.parametrize("kernel", KERNELS)
def test_tiny_images_and_extreme_fields_of_view(svo, oracle, worlds, kernel):
    """Images smaller than one 8x8 tile (down to one pixel) and fields of view of 1 and 170 degrees."""
    W, O, lo, hi, _ = worlds["grid_2x1x2_d6"]
    for (w, h) in ((1, 1), (1, 7), (9, 1), (2, 2), (63, 65), (7, 9)):
        for fov in (1.0, 60.0, 170.0):
            cam = svo.make_camera((130.3, 150.0, -40.0), (0.1, -0.5, 0.85), (0.0, 1.0, 0.0), fov, w, h)
            want = O.trace_image(cam, params=oracle.make_params(shadow=True), threads=4)
            assert_gbuffer_equal(W.draw(cam, shadow=True, kernel=_kid(svo, kernel)), want, f"{w}x{h} fov {fov}/{kernel}")


def test_tile_order_changes_nothing_but_the_schedule(svo, oracle, worlds):
    """svo_trace_params.tile_cost_dev / tile_order_dev: a frame records its tiles' step maxima,
    svo_tile_order sorts the tiles by them, the next frame hands them out in that order - and writes the same records,
    byte for byte, as without an order (and as the oracle).  Also over two frames in one launch."""
    W, O, lo, hi, s = worlds["grid_2x1x2_d6"]
    cam = svo.default_camera(2, 2, 128, 200, 120)
    w, h = cam.width, cam.height
    ntiles = ((w + 7) // 8) * ((h + 7) // 8)
    out = svo.DeviceBuffer(2 * w * h * 32)
    cost = svo.DeviceBuffer.from_numpy(np.full((2, ntiles, 2), 0xDEAD, np.uint32))     # the launch clears what it records into
    order = svo.DeviceBuffer(ntiles * 4)
    prm = svo.trace_params(shadow=True, kernel=svo.KERNEL_STACK, tile_cost_dev=cost.ptr)
    W.trace(cam, prm, (0, 0, w, h), out.ptr)
    svo.lib.svo_stream_synchronize(None)
    plain = out.to_numpy(svo.HIT_DTYPE, w * h).copy()
    c = cost.to_numpy(np.uint32, 2 * ntiles * 2).reshape(2, ntiles, 2)
    assert c[0, :, 0].max() > c[0, :, 0].min() and c[0, :, 1].max() > 0          # (a tile whose rays all miss the world box records nothing)
    assert np.all(c[1] == 0xDEAD)                                           # one frame traced: the second frame's slots untouched
    W.tile_order(cost.ptr, order.ptr, ntiles)
    svo.lib.svo_stream_synchronize(None)
    od = order.to_numpy(np.uint32, ntiles)
    assert np.array_equal(np.sort(od), np.arange(ntiles, dtype=np.uint32))
    key = c[0, :, 0].astype(np.int64) + c[0, :, 1]
    assert np.all(np.diff(key[od]) <= 0), "tiles are handed out by descending cost"
    want = O.trace_image(cam, params=oracle.make_params(shadow=True), threads=8)
    assert_gbuffer_equal(plain.reshape(h, w), want, "plain frame")
    prm2 = svo.trace_params(shadow=True, kernel=svo.KERNEL_STACK, tile_cost_dev=cost.ptr, tile_order_dev=order.ptr)
    W.trace_frames([cam, cam], prm2, (0, 0, w, h), out.ptr)
    svo.lib.svo_stream_synchronize(None)
    both = out.to_numpy(svo.HIT_DTYPE, 2 * w * h)
    assert both[:w * h].tobytes() == plain.tobytes() and both[w * h:].tobytes() == plain.tobytes()
    c2 = cost.to_numpy(np.uint32, 2 * ntiles * 2).reshape(2, ntiles, 2)
    assert np.array_equal(c2[0] > 0, c[0] > 0) and np.array_equal(c2[1] > 0, c2[0] > 0)
    # a reversed order (shortest first) is a schedule like any other
    rev = svo.DeviceBuffer.from_numpy(od[::-1].copy())
    prm3 = svo.trace_params(shadow=True, kernel=svo.KERNEL_STACK, tile_order_dev=rev.ptr)
    W.trace(cam, prm3, (0, 0, w, h), out.ptr)
    svo.lib.svo_stream_synchronize(None)
    assert out.to_numpy(svo.HIT_DTYPE, w * h).tobytes() == plain.tobytes()
    for b in (out, cost, order, rev):
        b.free()


def test_tile_order_calls_on_several_streams_and_a_bad_order(svo, oracle, worlds):
    """(1) svo_tile_order calls of one world on different streams share the world's sort scratch: they are ordered
    behind one another on the device, every call's result is the permutation its own cost array asks for; (2) an entry of
    tile_order_dev that is no tile index makes the launch skip a tile - its pixels stay as they were - and never index out of
    range; every other pixel is the plain frame's."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so.7")
    W, O, lo, hi, s = worlds["grid_2x1x2_d6"]
    ntiles = 40000                                          # a sort long enough to overlap with the next call's
    rng = np.random.default_rng(5)
    streams, costs, orders, keys = [], [], [], []
    for i in range(4):
        h = ctypes.c_void_p()
        assert hip.hipStreamCreateWithFlags(ctypes.byref(h), 1) == 0        # hipStreamNonBlocking
        streams.append(h.value)
        c = rng.integers(0, 5000, (ntiles, 2)).astype(np.uint32)
        keys.append(c[:, 0].astype(np.int64) + c[:, 1])
        costs.append(svo.DeviceBuffer.from_numpy(c))
        orders.append(svo.DeviceBuffer(ntiles * 4))
    for rep in range(3):
        for i in range(4):
            W.tile_order(costs[i].ptr, orders[i].ptr, ntiles, streams[i])
    for st in streams:
        svo.lib.svo_stream_synchronize(st)
    for i in range(4):
        od = orders[i].to_numpy(np.uint32, ntiles)
        assert np.array_equal(np.sort(od), np.arange(ntiles, dtype=np.uint32)), f"stream {i}: not a permutation"
        assert np.all(np.diff(keys[i][od]) <= 0), f"stream {i}: not by descending cost"
        assert np.array_equal(od, np.argsort(-keys[i], kind="stable").astype(np.uint32)), f"stream {i}: not the stable order of its own costs"
    for st in streams:
        hip.hipStreamDestroy(ctypes.c_void_p(st))
    for b in costs + orders:
        b.free()
    # (2) a corrupted order
    cam = svo.default_camera(2, 2, 128, 200, 120)
    w, h = cam.width, cam.height
    tpr = (w + 7) // 8
    nt = tpr * ((h + 7) // 8)
    out = svo.DeviceBuffer(w * h * 32)
    W.trace(cam, svo.trace_params(shadow=True, kernel=svo.KERNEL_STACK), (0, 0, w, h), out.ptr)
    svo.lib.svo_stream_synchronize(None)
    plain = out.to_numpy(svo.HIT_DTYPE, w * h).copy().reshape(h, w)
    od = np.arange(nt, dtype=np.uint32)[::-1].copy()
    lost = [int(od[3]), int(od[100])]
    od[3] = 0xFFFFFFFF; od[100] = nt                        # two entries that name no tile: tiles `lost` are never handed out
    bad = svo.DeviceBuffer.from_numpy(od)
    sentinel = np.full(w * h * 32, 0xAB, np.uint8)
    out2 = svo.DeviceBuffer.from_numpy(sentinel)
    W.trace(cam, svo.trace_params(shadow=True, kernel=svo.KERNEL_STACK, tile_order_dev=bad.ptr), (0, 0, w, h), out2.ptr)
    svo.lib.svo_stream_synchronize(None)
    got = out2.to_numpy(svo.HIT_DTYPE, w * h).copy().reshape(h, w)
    skipped = np.zeros((h, w), bool)
    for t in lost:
        ty, tx = divmod(t, tpr)
        skipped[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = True
    assert got[~skipped].tobytes() == plain[~skipped].tobytes()
    assert np.all(got[skipped].view(np.uint8) == 0xAB), "pixels of the skipped tiles stay unwritten"
    # list mode: the same guard keeps origins / dirs reads inside the list
    o, d = random_rays(np.random.default_rng(6), 64 * 50, lo, hi)
    od_l = np.arange(50, dtype=np.uint32); od_l[7] = 1 << 20
    ol = svo.DeviceBuffer.from_numpy(od_l)
    ob, db = svo.DeviceBuffer.from_numpy(o), svo.DeviceBuffer.from_numpy(d)
    out3 = svo.DeviceBuffer.from_numpy(np.full(64 * 50 * 32, 0xAB, np.uint8))
    W.trace_rays(ob.ptr, db.ptr, 64 * 50, svo.trace_params(kernel=svo.KERNEL_STACK, tile_order_dev=ol.ptr), out3.ptr)
    svo.lib.svo_stream_synchronize(None)
    g3 = out3.to_numpy(svo.HIT_DTYPE, 64 * 50)
    want = O.trace_rays(o, d, params=oracle.make_params(), threads=8)
    keep = np.ones(64 * 50, bool); keep[7 * 64:8 * 64] = False
    assert_gbuffer_equal(g3[keep], want[keep], "list mode around a skipped tile")
    assert np.all(g3[~keep].view(np.uint8) == 0xAB)
    for b in (out, out2, out3, bad, ol, ob, db):
        b.free()


def test_world_rebuilt_from_chunk_files_marches_like_the_oracle(svo, oracle, tmp_path):
    """VERDICT r2 task 8: Ocroot::write -> Ocroot::read (src/Octree.cpp:178-201) -> svo_world_create -> upload -> march.  A
    2x1x2 world with water, negative chunk coordinates, written chunk by chunk, read back and marched by both kernels
    against the oracle over the ORIGINAL pools."""
    ccm = (-1, 0, -1)
    W0 = svo.World.generate(2, 1, 2, 128, 7, chunkcoordmin=ccm)
    chunks = [W0.chunk(i) for i in range(4)]
    for i, c in enumerate(chunks):
        svo.chunk_write(str(tmp_path / f"chunk{i}.bin"), c, treestoragesize=c["tree"].size + 40, twigstoragesize=c["twig"].size // 64 + 3)
    back = [svo.chunk_read(str(tmp_path / f"chunk{i}.bin")) for i in range(4)]
    assert all(b["treestoragesize"] == c["tree"].size + 40 for b, c in zip(back, chunks))
    W = svo.World.create(back, 2, 1, 2, 128, chunkcoordmin=ccm)
    W.upload(0)
    O = oracle.OracleWorld.from_chunks(chunks, 2, 1, 2, 128, ccm)
    rng = np.random.default_rng(31)
    o, d = random_rays(rng, 20000, (-128, 0, -128), (128, 128, 128))
    want = O.trace_rays(o, d, params=oracle.make_params(shadow=True), threads=8)
    for k in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
        assert_gbuffer_equal(W.chunkmarch(o, d, shadow=True, kernel=k), want, f"read-back world, kernel {k}")
    cam = svo.make_camera((0.0, 150.0, -170.0), (0.0, -0.5, 0.866), (0.0, 1.0, 0.0), 60.0, 160, 90)
    assert_gbuffer_equal(W.draw(cam, shadow=True), O.trace_image(cam, params=oracle.make_params(shadow=True), threads=8), "read-back world, frame")
    assert (want["flags"] & 1).mean() > 0.2
    W.destroy(); W0.destroy()


def test_fuzz_under_face_normals(svo, oracle):
    """VERDICT r2 task 8: a cut of the adversarial fuzz with svo_trace_params.normal_mode = SVO_NORMAL_FACE, both kernels."""
    for i, c in enumerate(FUZZ_CASES[:2]):
        W = svo.World.generate(c["w"], c["h"], c["d"], 128, c["depth"], chunkcoordmin=c["ccm"])
        n = c["w"] * c["h"] * c["d"]
        O = oracle.OracleWorld.from_chunks([W.chunk(j, copy=False) for j in range(n)], c["w"], c["h"], c["d"], 128, c["ccm"])
        W.upload(0)
        lo = np.array(c["ccm"], float) * 128
        hi = lo + np.array([c["w"], c["h"], c["d"]]) * 128
        o, d = adversarial_rays(np.random.default_rng(2000 + i), 60000, lo, hi)
        want = O.trace_rays(o, d, params=oracle.make_params(shadow=True, light_dir=(0.2, -0.9, 0.4), normal_mode=1), threads=16)
        for k in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
            got = W.chunkmarch(o, d, shadow=True, kernel=k, light_dir=(0.2, -0.9, 0.4), normal_mode=svo.NORMAL_FACE)
            assert_gbuffer_equal(got, want, f"face-normal fuzz {c} kernel {k}")
            hit = (got["flags"] & 1) != 0
            assert not np.isnan(got["normal"][hit]).any() and np.all((got["flags"][hit] & svo.FACE_NORMAL) != 0)
        W.destroy()


def test_sixteen_frames_per_launch_on_four_streams_against_the_oracle(svo, oracle, worlds):
    """VERDICT r2 task 8: the bench's launch shape at its limit - svo_trace_frames launches of SVO_MAX_FRAMES = 16 frames,
    four of them in flight on four HIP streams - with EVERY frame of every launch checked against the oracle."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so.7")                                 # the runtime libsvo_amd.so is linked against (already loaded)
    W, O, lo, hi, _ = worlds["grid_2x1x2_d6"]
    w, h = 96, 64
    cams = [svo.make_camera((60.0 + 3.1 * f, 120.0 + 0.7 * f, -40.0 + 1.3 * f), (0.02 * (f % 9) - 0.05, -0.45, 0.85), (0.0, 1.0, 0.0), 55.0, w, h)
            for f in range(64)]
    prm = svo.trace_params(shadow=True, kernel=svo.KERNEL_STACK, tiles_per_wave=4)
    streams = []
    for _ in range(4):
        st = C.c_void_p()
        assert hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0     # hipStreamNonBlocking
        streams.append(st)
    bufs = [svo.DeviceBuffer(16 * w * h * 32) for _ in range(4)]
    for s in range(4):
        W.trace_frames(cams[16 * s:16 * s + 16], prm, (0, 0, w, h), bufs[s].ptr, streams[s].value)
    for st in streams:
        assert svo.lib.svo_stream_synchronize(st) == 0
    p = oracle.make_params(shadow=True)
    for s in range(4):
        got = bufs[s].to_numpy(svo.HIT_DTYPE, 16 * w * h).reshape(16, h, w)
        for f in range(16):
            assert_gbuffer_equal(got[f], O.trace_image(cams[16 * s + f], params=p, threads=8), f"launch {s} frame {f}")
    for st in streams:
        hip.hipStreamDestroy(st)
    for b in bufs:
        b.free()


def test_device_buffers_reused_between_worlds_carry_nothing_over(svo, oracle):
    """The library keeps a destroyed world's large device buffers for the next world whose pools they fit (include/svo.h
    svo_device_cache_trim): a world built into recycled buffers - same size, slightly smaller (the 25 % fit rule), after an edit
    that re-packs, host-built and device-built - marches like a world built into fresh ones, and trimming in between changes nothing."""
    rng = np.random.default_rng(77)
    lo, hi = (0.0, 0.0, 0.0), (256.0, 128.0, 256.0)
    o, d = random_rays(rng, 30000, lo, hi)

    def check(W, seed, depth, what):
        O = oracle.OracleWorld.generate(2, 1, 2, 128, depth, seed=seed)
        want = O.trace_rays(o, d, params=oracle.make_params(shadow=True), threads=8)
        for k in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
            assert_gbuffer_equal(W.chunkmarch(o, d, shadow=True, kernel=k), want, f"{what}/{k}")

    svo.lib.svo_device_cache_trim()
    A = svo.World.generate(2, 1, 2, 128, 8, seed=1, build_device=0)
    check(A, 1, 8, "fresh buffers")
    A.destroy()                                             # its pools go to the cache ...
    B = svo.World.generate(2, 1, 2, 128, 8, seed=5, build_device=0)
    check(B, 5, 8, "recycled buffers, other terrain")       # ... and to this world: nothing of world A may show
    B.destroy()
    C = svo.World.generate(2, 1, 2, 128, 8, seed=9)         # host-built, uploaded into recycled buffers
    C.upload(0)
    check(C, 9, 8, "recycled buffers, host-built world")
    C.edit_box(0, svo.EDIT_BUILD, (10.0, 100.0, 10.0), (60.0, 120.0, 60.0), 5)       # (an edit on top: pools re-sent / re-packed)
    C.destroy()
    svo.lib.svo_device_cache_trim()                         # back to the driver: the next world allocates afresh
    D = svo.World.generate(2, 1, 2, 128, 7, seed=5, build_device=0)
    check(D, 5, 7, "after a trim")
    D.destroy()
    E = svo.World.generate(2, 1, 2, 128, 8, seed=3, build_device=0)        # larger than what D left: the cache must not hand out too small a buffer
    check(E, 3, 8, "a larger world after a smaller one")
    E.destroy()
