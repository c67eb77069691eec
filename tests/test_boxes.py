"""svo_shade_boxes, svo_cursor_place and svo_world_edit_cube on the GPU.  The overlay and the cursor are held bit for bit to the host model
(tests/boxes_model.py) on 64 x 48 frames of one small world (the two mixed hit / miss views of tests/hit_voxels_model.py); the cube edit
to the CPU oracle driven by the reference's own loop, corner by corner (src/Main.cpp:321-338); and the interactive loop - trace, shade,
sky, place the cursor, draw the boxes, RGBA8, read the cursor back, destroy - runs end to end on one stream."""
import ctypes as C

import numpy as np
import pytest

import boxes_model as B
import sky_model as S
from helpers import assert_gbuffer_equal, random_rays

pytestmark = pytest.mark.gpu
F = np.float32
W_, H_ = B.IMAGE
N = W_ * H_
FULL = (0, 0, W_, H_)
SENTINEL = F(-7.0)
PAD = 16                                                        # pixels of sentinel behind the image


def sync(svo):
    assert svo.lib.svo_stream_synchronize(None) == 0


def overlay(svo, cam, rect, image, boxes, nboxes=None, **planes):
    """svo_shade_boxes over a copy of `image` ([n][4] float32) with a sentinel behind it -> the image it leaves."""
    n = rect[2] * rect[3]
    image = np.ascontiguousarray(image, F).reshape(n, 4)
    buf = svo.DeviceBuffer.from_numpy(np.concatenate([image.reshape(-1), np.full(PAD * 4, SENTINEL, F)]))
    boxes = np.ascontiguousarray(boxes, B.BOX_DTYPE)
    dev = svo.DeviceBuffer.from_numpy(boxes) if boxes.size else None
    svo.shade_boxes(cam, dev.ptr if dev else None, boxes.size if nboxes is None else nboxes, rect, buf.ptr, **planes)
    sync(svo)
    got = buf.to_numpy(F, (n + PAD) * 4)
    buf.free()
    if dev:
        dev.free()
    assert np.all(got[n * 4:] == SENTINEL), "wrote past w*h pixels"
    return got[:n * 4].reshape(n, 4)


def same(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def differing(a, b):
    return np.nonzero((np.asarray(a, F).view(np.uint32) != np.asarray(b, F).view(np.uint32)).any(axis=1))[0]


class View:
    """One mixed view: its records, svo_shade's image of them, the model's rays and the scene's boxes."""

    def __init__(self, svo, world, cam):
        self.cam = cam
        gbuffer, rgba = svo.DeviceBuffer(N * 32), svo.DeviceBuffer(N * 16)
        world.trace(cam, svo.trace_params(shadow=True), FULL, gbuffer.ptr)
        svo.shade(cam, svo.shade_defaults(), FULL, gbuffer.ptr, rgba.ptr)
        sync(svo)
        self.g = gbuffer.to_numpy(svo.HIT_DTYPE, N)
        self.base = rgba.to_numpy(F, N * 4).reshape(N, 4)
        gbuffer.free()
        rgba.free()
        self.hit = (self.g["flags"] & 1) != 0
        self.eye, self.dirs = B.eye_of(cam), B.camera_dirs(cam)
        self.boxes = B.scene_boxes(cam, self.g)

    def model(self, boxes, **planes):
        return B.shade_boxes(self.base, self.eye, self.dirs, boxes, **planes)


@pytest.fixture(scope="module")
def world(svo):
    import hit_voxels_model as M
    if svo.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    (w, h, d), cs, ccm = B.world_spec()
    W = svo.World.create(M.make_chunks(svo, B.WORLD), w, h, d, cs, ccm)
    W.upload(0)
    yield W
    W.destroy()


@pytest.fixture(scope="module")
def views(svo, world):
    return {name: View(svo, world, cam) for name, cam in B.mixed_cameras(svo, B.WORLD).items()}


def test_the_overlay_equals_the_model_bit_for_bit(svo, views):
    """All four floats of every pixel, for the eight boxes of the scene and for the seven that do not hold the eye; under the latter the
    frame has every kind of pixel (counted on the model's output), and what no fragment passed on is byte for byte what it was."""
    for name, v in views.items():
        assert v.boxes.size == 8
        want, st = v.model(v.boxes)
        got = overlay(svo, v.cam, FULL, v.base, v.boxes)
        bad = differing(got, want)
        assert bad.size == 0, f"{name}: {bad.size} pixels differ, first {bad[:4]} got {got[bad[:4]]} want {want[bad[:4]]}"
        assert np.all(st["passed"] >= 1), "the box that holds the eye covers the frame"
        seven = B.without_eye_box(v.boxes)
        want, st = v.model(seven)
        got = overlay(svo, v.cam, FULL, v.base, seven)
        bad = differing(got, want)
        assert bad.size == 0, f"{name}: {bad.size} pixels differ, first {bad[:4]} got {got[bad[:4]]} want {want[bad[:4]]}"
        have = B.counts(v.hit, st)
        for k, need in B.NEEDED.items():
            assert have[k] >= need, (name, k, have)
        untouched = st["passed"] == 0
        assert untouched.sum() >= 300
        assert np.array_equal(got[untouched].view(np.uint8), v.base[untouched].view(np.uint8)), "a pixel no fragment passed on was written"
        assert np.all(st["passed"][differing(got, v.base)] > 0)
        assert not np.isnan(got).any()


def test_a_sub_rectangle_equals_the_crop(svo, views):
    x0, y0, w, h = rect = (5, 7, 40, 30)
    for name, v in views.items():
        full = overlay(svo, v.cam, FULL, v.base, v.boxes).reshape(H_, W_, 4)
        crop = v.base.reshape(H_, W_, 4)[y0:y0 + h, x0:x0 + w]
        got = overlay(svo, v.cam, rect, crop, v.boxes).reshape(h, w, 4)
        assert same(got, full[y0:y0 + h, x0:x0 + w]), name
        want, _ = B.shade_boxes(crop.reshape(-1, 4), v.eye, B.camera_dirs(v.cam, rect), v.boxes)
        assert same(got.reshape(-1, 4), want), name


def test_no_boxes_write_nothing(svo, views):
    v = views["above"]
    noise = np.random.default_rng(1).random((N, 4)).astype(F)
    assert same(overlay(svo, v.cam, FULL, noise, v.boxes[:0]), noise)
    assert same(overlay(svo, v.cam, FULL, noise, v.boxes, nboxes=0), noise)
    assert same(overlay(svo, v.cam, FULL, noise, v.boxes[6:]), noise)       # behind the eye, hidden: nothing passes


def test_the_list_order_matters(svo, views):
    for name, v in views.items():
        pair = B.translucent_pair(v.boxes)
        a, b = v.model(pair)[0], v.model(pair[::-1])[0]
        assert differing(a, b).size >= 20, name
        assert same(overlay(svo, v.cam, FULL, v.base, pair), a), name
        assert same(overlay(svo, v.cam, FULL, v.base, pair[::-1]), b), name


def test_the_planes_and_a_full_list(svo, views):
    """near / far other than the defaults reach the depth; SVO_MAX_BOXES boxes (the whole staged list) equal the model."""
    v = views["front"]
    planes = dict(near_plane=0.5, far_plane=1000.0)
    want, st = v.model(B.without_eye_box(v.boxes), near=0.5, far=1000.0)
    got = overlay(svo, v.cam, FULL, v.base, B.without_eye_box(v.boxes), **planes)
    assert same(got, want) and (st["passed"] > 0).sum() >= 100
    assert differing(want, v.model(B.without_eye_box(v.boxes))[0]).size >= 100
    rng = np.random.default_rng(7)
    t = np.where(v.hit, v.g["t"], 100.0).astype(np.float64)
    many = []
    for i in range(B.MAX_BOXES):
        k = int(rng.integers(0, N))
        size = float(rng.uniform(2.0, 12.0))
        centre = v.eye.astype(np.float64) + v.dirs[k].astype(np.float64) * t[k] * rng.uniform(0.5, 1.1)
        many.append(B.box(centre - 0.5 * size, size, rng.random(3), float(rng.choice([0.2, 0.5, 1.0])),
                          (B.SOLID, B.CURSOR)[i % 2] | (B.HIDDEN if i % 9 == 2 else 0)))
    many[-1] = B.box(B.forward_point(v.cam, 6.0) - 1.0, 2.0, (0.3, 1.0, 0.3), 0.5, B.CURSOR)     # the list's last box is in view, near the eye
    many = B.box_list(*many)
    want, st = v.model(many)
    got = overlay(svo, v.cam, FULL, v.base, many)
    bad = differing(got, want)
    assert bad.size == 0, f"{bad.size} pixels differ, first {bad[:4]} got {got[bad[:4]]} want {want[bad[:4]]}"
    assert (st["passed"] > 0).sum() >= 300 and (st["passed"] >= 3).sum() >= 20 and (st["failed"] > 0).sum() >= 100
    # the last box of the list counts: hidden, the image differs
    last = many.copy()
    last["style"][-1] |= B.HIDDEN
    assert differing(v.model(last)[0], want).size >= 20
    assert same(overlay(svo, v.cam, FULL, v.base, last), v.model(last)[0])


def test_cursor_place_equals_the_model(svo, world, views):
    """One ray from svo_trace_rays under both kernels: a hit places the box (bmin, size, SVO_BOX_HIDDEN cleared), a miss hides it and
    leaves bmin; colour, alpha and the low style bits are never written."""
    v = views["above"]
    k_hit, k_miss = int(np.nonzero(v.hit)[0][v.hit.sum() // 2]), int(np.nonzero(~v.hit)[0][0])
    start = B.box((1.5, 2.5, 3.5), 9.0, (0.1, 0.2, 0.3), 0.4, B.CURSOR | B.HIDDEN)
    start["_pad"] = (11, 22, 33)
    for kernel in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
        for k, hit in ((k_hit, True), (k_miss, False)):
            o, d = v.eye, v.dirs[k]
            od, dd, rec = svo.DeviceBuffer.from_numpy(o), svo.DeviceBuffer.from_numpy(d), svo.DeviceBuffer(32)
            box = svo.DeviceBuffer.from_numpy(np.concatenate([start.view(np.uint32), np.full(4, 0xDEADBEEF, np.uint32)]))
            world.trace_rays(od.ptr, dd.ptr, 1, svo.trace_params(kernel=kernel), rec.ptr)
            svo.cursor_place(o, d, rec.ptr, 16.0, box.ptr)
            sync(svo)
            record = rec.to_numpy(svo.HIT_DTYPE, 1)[0]
            raw = box.to_numpy(np.uint32, 16)
            assert np.all(raw[12:] == 0xDEADBEEF), "wrote past the box"
            got = raw[:12].view(B.BOX_DTYPE)
            assert bool(record["flags"] & 1) == hit
            want = B.cursor_place(o, d, record, 16.0, start)
            assert got.tobytes() == want.tobytes(), (kernel, hit, got, want)
            if hit:
                assert got["style"][0] == B.CURSOR and got["size"][0] == 16.0 and np.all(np.isfinite(got["bmin"]))
                centre = got["bmin"][0] + F(8.0)
                assert np.allclose(centre, o + d * record["t"], atol=1e-3)
            else:
                assert got["style"][0] == B.CURSOR | B.HIDDEN and np.array_equal(got["bmin"][0], [1.5, 2.5, 3.5]) and got["size"][0] == 9.0
            # a shown box that misses is hidden, a hidden one that hits is shown: start from the other state too
            shown = start.copy()
            shown["style"] = B.CURSOR
            box2 = svo.DeviceBuffer.from_numpy(shown)
            svo.cursor_place(o, d, rec.ptr, 16.0, box2.ptr)
            sync(svo)
            assert box2.to_numpy(B.BOX_DTYPE, 1).tobytes() == B.cursor_place(o, d, record, 16.0, shown).tobytes()
            for b in (od, dd, rec, box, box2):
                b.free()


def reference_modify(oracle, O, op, bmin, size, material, dims, cs, ccm):
    """The reference's loop (src/Main.cpp:321-367) on the oracle's world: one Ocroot edit per corner that passes the test."""
    lo = np.asarray(bmin, F)
    hi = (lo + F(size)).astype(F)
    calls, distinct = B.corner_chunks(bmin, size, dims, cs, ccm)
    for j in calls:
        dt, dw = oracle.Delta(), oracle.Delta()
        root = C.byref(O.w.chunk[j])
        if op in (1, 2):
            oracle.lib.orc_destroy(root, oracle.vec3(lo), oracle.vec3(hi), C.byref(dt), C.byref(dw))
        if op in (0, 2):
            oracle.lib.orc_build(root, oracle.vec3(lo), oracle.vec3(hi), material, C.byref(dt), C.byref(dw))
    return distinct


def pools_equal(O, D, n, what):
    for i in range(n):
        a, b = O.chunk(i), D.chunk(i, copy=False)
        assert a["tree"].size == b["tree"].size and a["twig"].size == b["twig"].size, f"{what}: chunk {i} pool sizes differ"
        assert np.array_equal(a["tree"], b["tree"]), f"{what}: chunk {i} node words differ"
        assert np.array_equal(a["twig"], b["twig"]), f"{what}: chunk {i} bricks differ"


CUBE_EDITS = [
    # (op, bmin, size, material, chunks)
    (0, (120.0, 60.0, 120.0), 16.0, 5, [0, 2, 1, 3]),           # build at the seam corner, in the air
    (1, (118.3, 2.7, 119.1), 17.6, 0, [0, 2, 1, 3]),            # destroy there, through terrain and water, off the lattice
    (2, (120.0, 0.0, 120.0), 16.0, 7, [0, 2, 1, 3]),            # replace there
    (2, (40.3, 10.2, 30.1), 20.0, 3, [0]),                      # inside one chunk
    (0, (250.0, 20.0, 60.0), 12.0, 4, [1]),                     # half outside the world: only the chunk inside
    (1, (-6.0, -6.0, 200.0), 12.0, 0, [2]),
]


def test_edit_cube_equals_the_references_loop(svo, oracle):
    dims, cs, ccm = (2, 1, 2), 128, (0, 0, 0)
    O = oracle.OracleWorld.generate(2, 1, 2, cs, 6)
    D = svo.World.generate(2, 1, 2, cs, 6, build_device=0)
    o, d = random_rays(np.random.default_rng(31), 20000, (0, 0, 0), (256, 128, 256))
    prm = oracle.make_params(shadow=True)
    for k, (op, bmin, size, mat, chunks) in enumerate(CUBE_EDITS):
        want_chunks = reference_modify(oracle, O, op, bmin, size, mat, dims, cs, ccm)
        assert want_chunks == chunks, (k, want_chunks)
        status, got_chunks = D.edit_cube(op, bmin, size, mat)
        assert status == 0 and got_chunks == want_chunks, (k, status, got_chunks)
        pools_equal(O, D, 4, f"after cube edit {k}")
        want = O.trace_rays(o, d, params=prm, threads=8)
        for kern in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
            assert_gbuffer_equal(D.chunkmarch(o, d, shadow=True, kernel=kern), want, f"cube edit {k} / kernel {kern}")
    # a cube that no chunk holds edits nothing and reports none; NULL outputs are allowed
    before = [D.chunk(i) for i in range(4)]
    assert D.edit_cube(svo.EDIT_DESTROY, (400.0, 10.0, 10.0), 8.0) == (0, [])
    assert svo.lib.svo_world_edit_cube(D._h, 0, (C.c_float * 3)(400.0, 10.0, 10.0), 8.0, C.c_uint16(5), None, None) == 0
    for i in range(4):
        assert np.array_equal(before[i]["tree"], D.chunk(i)["tree"]) and np.array_equal(before[i]["twig"], D.chunk(i)["twig"])
    for bad in (dict(op=3, bmin=(1, 1, 1), size=8.0), dict(op=0, bmin=(1, 1, 1), size=0.0), dict(op=0, bmin=(float("nan"), 1, 1), size=8.0)):
        with pytest.raises(svo.SvoError) as e:
            D.edit_cube(bad["op"], bad["bmin"], bad["size"], 5)
        assert e.value.code == -1
    pools_equal(O, D, 4, "after the refused edits")
    D.destroy()
    O.close()


def test_the_interactive_loop_end_to_end(svo, oracle, views):
    """Trace, shade, sky, svo_cursor_place from the centre pixel's record, svo_shade_boxes with the cursor and three markers, RGBA8 - on
    one stream with no synchronisation in between; the frame equals the model pipeline.  Then the key press: the box read back (48
    bytes), svo_world_edit_cube(SVO_EDIT_DESTROY), and the next trace equals the oracle's world with the same cube destroyed."""
    dims, cs, ccm = (2, 1, 2), 128, (0, 0, 0)
    v = views["above"]
    cam = v.cam
    D = svo.World.generate(2, 1, 2, cs, 6)
    D.upload(0)
    O = oracle.OracleWorld.generate(2, 1, 2, cs, 6)
    centre = (H_ // 2) * W_ + W_ // 2
    assert v.hit[centre], "the view ray misses"
    size = 48.0
    faces = S.random_faces(37, 41)
    sky_dev = svo.DeviceBuffer.from_numpy(faces)
    sky = svo.Sky([sky_dev.ptr + f * 37 * 37 * 3 for f in range(6)], 37, svo.SKY_LINEAR)
    cursor = B.box((0, 0, 0), 1.0, (0.8, 0.8, 0.8), 0.2, B.CURSOR | B.HIDDEN)
    boxes = B.box_list(cursor, v.boxes[0:1], v.boxes[1:2], v.boxes[3:4])
    boxes_dev = svo.DeviceBuffer.from_numpy(boxes)
    gbuffer, rgba = svo.DeviceBuffer(N * 32), svo.DeviceBuffer(N * 16)
    out = svo.DeviceBuffer.from_numpy(np.full(N + PAD, 0xDEADBEEF, np.uint32))
    P = svo.shade_defaults()
    prm = svo.trace_params(shadow=True)
    D.trace(cam, prm, FULL, gbuffer.ptr)
    svo.shade(cam, P, FULL, gbuffer.ptr, rgba.ptr)
    svo.shade_sky(cam, sky, FULL, rgba.ptr, gbuffer_ptr=gbuffer.ptr)
    svo.cursor_place(v.eye, v.dirs[centre], gbuffer.ptr + 32 * centre, size, boxes_dev.ptr)
    svo.shade_boxes(cam, boxes_dev.ptr, boxes.size, FULL, rgba.ptr)
    svo.frame_rgba8(rgba.ptr, N, out.ptr)
    sync(svo)
    got = out.to_numpy(np.uint32, N + PAD)
    assert np.all(got[N:] == 0xDEADBEEF)
    got = got[:N].view(np.uint8).reshape(N, 4)
    g = gbuffer.to_numpy(svo.HIT_DTYPE, N)
    assert g.tobytes() == v.g.tobytes()                          # the same world, the same view
    placed = B.cursor_place(v.eye, v.dirs[centre], g[centre], size, cursor)
    model_boxes = B.box_list(placed, boxes[1:])
    image = S.shade_sky(v.base, g, v.dirs, faces, S.LINEAR)
    image, st = B.shade_boxes(image, v.eye, v.dirs, model_boxes)
    want = S.frame_rgba8(image)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} pixels differ, first {bad[:4]} got {got[bad[:4]]} want {want[bad[:4]]}"
    assert (B.shade_boxes(v.base, v.eye, v.dirs, placed)[1]["passed"] > 0).sum() >= 20, "the cursor is not in the frame"
    assert (st["passed"] > 0).sum() >= 100
    # the key press
    back = np.zeros(1, B.BOX_DTYPE)
    assert svo.lib.svo_memcpy_d2h(back.ctypes.data, boxes_dev.ptr, 48) == 0
    assert back.tobytes() == placed.tobytes()
    status, chunks = D.edit_cube(svo.EDIT_DESTROY, back["bmin"][0], float(back["size"][0]))
    want_chunks = reference_modify(oracle, O, svo.EDIT_DESTROY, back["bmin"][0], back["size"][0], 0, dims, cs, ccm)
    assert status == 0 and chunks == want_chunks and len(chunks) >= 1
    D.trace(cam, prm, FULL, gbuffer.ptr)
    sync(svo)
    g2 = gbuffer.to_numpy(svo.HIT_DTYPE, N)
    assert_gbuffer_equal(g2, O.trace_image(cam, params=oracle.make_params(shadow=True)), "after the destroy")
    assert g2.tobytes() != g.tobytes() and not (g2[centre]["flags"] & 1 and g2[centre]["t"] == g[centre]["t"]), "the destroy does not show"
    for b in (sky_dev, boxes_dev, gbuffer, rgba, out):
        b.free()
    D.destroy()
    O.close()
