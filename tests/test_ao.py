"""svo_hit_ao and svo_shade_ao on the GPU: voxel ambient occlusion from the eight lattice cells around each hit's face, both walks (the
tree pool and the wide pool) and both semantics, on the float's bits against the host model tests/ao_model.py - on generated,
mixed-depth, negative-coordinate and hand-made worlds, with see_through, against the composition through svo_world_locate at a
size the Python walk is too slow for, on the rectangles where eight lanes per pixel can go wrong, on records that get no rule, after
an edit, with a cell override; the statuses; and svo_shade_ao against numpy."""
import numpy as np
import pytest

import ao_model as M
import hit_voxels_model as H
import locate_model as L

pytestmark = pytest.mark.gpu

KERNELS = {"literal": 1, "stack": 2}
WATER = 6
F = np.float32
SCENES = [("grid_2x1x2_d8", "default"), ("grid_2x1x2_d8", "low"), ("mixed_7_2_4_5", "default"), ("grid_neg_2x2x2_d5", "default"), ("handmade", "default")]


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32).reshape(-1)


def assert_same_floats(got, want, what):
    bad = np.nonzero(bits(got) != bits(want))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {bits(got).size} floats differ, first at {bad[:5]}: got {np.asarray(got).reshape(-1)[bad[:5]]} want {np.asarray(want).reshape(-1)[bad[:5]]}"


class Scene:
    """One resident world, its chunks and twin for the model, one camera; per (semantics, see_through) the G-buffer W.draw traces, the
    boxes svo_hit_voxels writes for it and the model's floats, computed once."""

    def __init__(self, svo, name, view, image=M.IMAGE):
        self.svo, self.name = svo, name
        if name == "handmade":
            self.chunks, (w, h, d, ccm) = L.handmade_chunks(), L.HANDMADE
        else:
            self.chunks = M.make_chunks(svo, name)
            w, h, d, ccm, _ = M.WORLDS[name]
        self.dims = (w, h, d, ccm)
        self.W = svo.World.create(self.chunks, w, h, d, 128, ccm)
        self.W.upload(0)
        assert self.W.info.exact_geometry == 1 and self.W.info.wide_nodes > 0
        self.twin = L.world_of(self.chunks, w, h, d, 128, ccm)
        self.cam = M.camera(svo, name, view, image)
        self._frames, self._want = {}, {}

    def frame(self, semantics=0, see_through=0):
        key = (semantics, see_through)
        if key not in self._frames:
            g = self.W.draw(self.cam, semantics=semantics, see_through=see_through)
            self._frames[key] = (g, self.W.hit_boxes(g).reshape(g.shape))
        return self._frames[key]

    def want(self, semantics=0, see_through=0, detail=None):
        key = (semantics, see_through)
        if key not in self._want:
            g, v = self.frame(*key)
            d = {}
            ao = M.hit_ao(self.chunks, 128, self.cam, None, g, v, M.TwinOccupancy(self.twin, semantics, see_through), semantics=semantics, detail=d)
            self._want[key] = (ao.reshape(g.shape), d)
        if detail is not None:
            detail.update(self._want[key][1])
        return self._want[key][0]

    def close(self):
        self.W.destroy()


@pytest.fixture(scope="module")
def scenes(svo):
    if svo.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    made = {}

    def scene(name, view="default"):
        if (name, view) not in made:
            made[(name, view)] = Scene(svo, name, view)
        return made[(name, view)]

    yield scene
    for s in made.values():
        s.close()


@pytest.mark.parametrize("semantics", [0, 1])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name,view", SCENES)
def test_ao_equals_the_model(svo, scenes, name, view, kernel, semantics):
    s = scenes(name, view)
    g, v = s.frame(semantics)
    d = {}
    want = s.want(semantics, detail=d)
    dark = int((want < 1).sum())
    print(f"{name}/{view} {kernel} semantics {semantics}: {int(d['on'].sum())} hits, ao < 1 on {dark}, {np.unique(want).size} values")
    assert d["on"].sum() >= 1000 and dark * 4 >= d["on"].sum()
    got = s.W.ao_image(s.cam, g, voxels=v, kernel=KERNELS[kernel], semantics=semantics)
    assert_same_floats(got, want, f"{name}/{view}/{kernel}/semantics {semantics}")
    assert got.min() >= 0.0 and got.max() == 1.0
    if kernel == "stack":                                       # AUTO takes the same walk; None for the boxes means svo_hit_voxels'
        assert_same_floats(s.W.ao_image(s.cam, g, kernel=svo.KERNEL_AUTO, semantics=semantics), want, f"{name}/{view}/auto")


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_see_through_water(svo, scenes, kernel):
    """see_through = 6: the march passes the water, the hits lie under it, and the water's cells do not occlude them."""
    s = scenes("grid_2x1x2_d8", "default")
    g, v = s.frame(0, WATER)
    plain = s.frame(0)[0]
    under = ((plain["material"] == WATER) & ((plain["flags"] & 1) != 0)).sum()
    d = {}
    want = s.want(0, WATER, detail=d)
    wet = M.TwinOccupancy(s.twin)(d["N"].reshape(-1, 3)).reshape(-1, 8) != d["occ"]
    print(f"see_through {kernel}: {int(under)} pixels saw water, {int(wet.sum())} neighbour cells are opened by see_through")
    assert under > 100 and wet.sum() > 100 and not (g["material"] == WATER).any()
    got = s.W.ao_image(s.cam, g, voxels=v, kernel=KERNELS[kernel], see_through=WATER)
    assert_same_floats(got, want, f"see_through/{kernel}")
    assert (bits(s.W.ao_image(s.cam, g, voxels=v, kernel=KERNELS[kernel])) != bits(want)).any(), "see_through is read"


def test_the_composition_through_locate_at_256x192(svo, scenes):
    """What the call replaces: the model's neighbour points through svo_world_locate, the fold of their SOLID bits."""
    s = scenes("grid_2x1x2_d8", "default")
    cam = M.camera(svo, s.name, "default", (256, 192))
    g = s.W.draw(cam)
    v = s.W.hit_boxes(g)
    on, N, fu, fv = M.neighbour_points(s.chunks, 128, cam, None, g, v, M.resolved_eps())
    assert on.sum() > 20000
    for kernel in sorted(KERNELS):
        records = s.W.locate_points(N.reshape(-1, 3), kernel=KERNELS[kernel])
        want = np.ones(on.shape[0], F)
        want[on] = M.fold(((records["flags"] & L.SOLID) != 0).reshape(-1, 8), fu, fv)
        got = s.W.ao_image(cam, g, voxels=v, kernel=KERNELS[kernel])
        assert_same_floats(got, want, f"composition/{kernel}")
    print(f"256 x 192: {int(on.sum())} hits, ao < 1 on {int((want < 1).sum())}")
    assert (want < 1).sum() * 4 >= on.sum()


def sub_image(s, g, v, rect, kernel):
    x0, y0, w, h = rect
    return s.W.ao_image(s.cam, g[y0:y0 + h, x0:x0 + w], rect=rect, voxels=v[y0:y0 + h, x0:x0 + w], kernel=kernel)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_rectangles_where_the_octets_can_go_wrong(svo, scenes, kernel):
    """1 x 1 (one octet of a wave), 13 x 7 (91 pixels: a partial wave and a partial block), 64 x 1, and a rectangle with x0, y0 > 0:
    each equals its region of the full image."""
    s = scenes("grid_2x1x2_d8", "default")
    g, v = s.frame(0)
    full = s.want(0)
    ys, xs = np.nonzero(full < 1)
    y1, x1 = int(ys[ys.size // 2]), int(xs[xs.size // 2])
    row = int(np.argmax((full < 1).sum(axis=1)))
    by, bx = max((((full[y:y + 7, x:x + 13] < 1).sum(), y, x) for y in range(0, 41, 3) for x in range(0, 51, 3)))[1:]
    rects = {"1 x 1": (x1, y1, 1, 1), "13 x 7": (bx, by, 13, 7), "64 x 1": (0, row, 64, 1), "offset": (5, 9, 50, 30), "one column": (x1, 0, 1, 48)}
    for what, (x0, y0, w, h) in rects.items():
        part = full[y0:y0 + h, x0:x0 + w]
        assert (part < 1).any(), what
        assert_same_floats(sub_image(s, g, v, (x0, y0, w, h), KERNELS[kernel]), part, f"{what}/{kernel}")
    # an empty rectangle launches nothing
    s.W.hit_ao(s.cam, svo.trace_params(kernel=KERNELS[kernel]), (3, 3, 0, 5), None, None, None)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_records_that_get_no_rule(svo, scenes, kernel):
    s = scenes("grid_2x1x2_d8", "default")
    g, v = (a.copy() for a in s.frame(0))
    full = s.want(0)
    nchunks = len(s.chunks)
    dark = np.nonzero((full < 1).reshape(-1))[0]
    assert dark.size >= 400 and ((g["flags"] & 1) == 0).sum() > 100        # misses among the pixels, too
    gf, vf = g.reshape(-1), v.reshape(-1)
    err, zeroed, count, far = dark[0:400:4], dark[1:400:4], dark[2:400:4], dark[3:400:4]
    gf["flags"][err] |= H.ERR_FLAG
    vf[zeroed] = np.zeros(1, H.VOXEL_DTYPE)[0]
    vf["chunk"][count] = nchunks
    vf["chunk"][far] = 0xFFFFFFFF
    want = M.hit_ao(s.chunks, 128, s.cam, None, g, v, M.TwinOccupancy(s.twin)).reshape(full.shape)
    gone = np.concatenate([err, zeroed, count, far])
    assert np.all(want.reshape(-1)[gone] == 1.0) and np.all(want[(g["flags"] & 1) == 0] == 1.0) and (want < 1).sum() == dark.size - 400
    assert_same_floats(s.W.ao_image(s.cam, g, voxels=v, kernel=KERNELS[kernel]), want, f"records/{kernel}")


def test_cell_override(svo, scenes):
    """cell = 2 * the finest voxel of the depth-8 chunks (0.5): a lattice of 1."""
    s = scenes("grid_2x1x2_d8", "default")
    g, v = s.frame(0)
    want = M.hit_ao(s.chunks, 128, s.cam, None, g, v, M.TwinOccupancy(s.twin), cell=1.0).reshape(g.shape)
    assert (bits(want) != bits(s.want(0))).sum() > 300 and (want < 1).sum() > 300
    for kernel in sorted(KERNELS):
        assert_same_floats(s.W.ao_image(s.cam, g, voxels=v, kernel=KERNELS[kernel], cell=1.0), want, f"cell 1.0/{kernel}")


def chunk_position(W, i):
    return W.chunk(int(i), copy=False)["position"]


def test_the_call_after_an_edit_sees_the_edit(svo):
    """svo_world_edit_box BUILDs a column of 4 voxels beside a hit on a flat stretch: the model on the fetched chunks still agrees, and
    the floor around the column got darker."""
    name = "grid_2x1x2_d6"
    w, h, d, ccm, _ = M.WORLDS[name]
    W = svo.World.create(M.make_chunks(svo, name), w, h, d, 128, ccm)
    W.upload(0)
    cam = M.camera(svo, name, "default", (128, 96))            # (rays closer together than the column is wide)

    def frame():
        chunks = [W.chunk(i) for i in range(w * h * d)]
        g = W.draw(cam)
        v = W.hit_boxes(g).reshape(g.shape)
        want = M.hit_ao(chunks, 128, cam, None, g, v, M.TwinOccupancy(L.world_of(chunks, w, h, d, 128, ccm))).reshape(g.shape)
        for kernel in sorted(KERNELS):
            assert_same_floats(W.ao_image(cam, g, voxels=v, kernel=KERNELS[kernel]), want, f"edit/{kernel}")
        return g, v, want

    g, v, before = frame()
    # a flat stretch the camera sees: 5 x 5 pixels, all open, all finest voxels of one chunk hit on their top face at one height, away
    # from the chunk's faces
    top = (before == 1) & ((g["flags"] & 1) != 0) & (v["size"] == 2.0) & (g["normal"][..., 1] == 1.0)
    spot = []
    for y in range(2, cam.height - 2):
        for x in range(2, cam.width - 2):
            blk = (slice(y - 2, y + 3), slice(x - 2, x + 3))
            rel = v["bmin"][y, x] - np.array(chunk_position(W, v["chunk"][y, x]), F)
            if top[blk].all() and np.ptp(v["bmin"][blk][..., 1]) == 0 and np.ptp(v["chunk"][blk]) == 0 and rel.min() > 16 and rel.max() < 100:
                spot.append((y, x))
    assert spot, "the camera sees no flat stretch"
    y, x = spot[len(spot) // 2]
    lo = v["bmin"][y, x].astype(np.float64) + np.array([0.0, 2.0, 0.0])
    W.edit_box(int(v["chunk"][y, x]), svo.EDIT_BUILD, lo + 0.25, lo + np.array([2.0, 8.0, 2.0]) - 0.25, 5)
    g2, v2, after = frame()
    dropped = int((after < before).sum())
    print(f"column at {lo} (pixel {x}, {y}): {int((g2['material'] == 5).sum())} pixels see it, ao dropped on {dropped}")
    assert (g2["material"] == 5).sum() > 0 and dropped >= 1
    W.destroy()


def test_statuses_and_refused_calls_write_nothing(svo, scenes):
    s = scenes("grid_2x1x2_d8", "default")
    g, v = s.frame(0)
    n = g.size
    rect = (0, 0, g.shape[1], g.shape[0])
    gd, vd = svo.DeviceBuffer.from_numpy(g), svo.DeviceBuffer.from_numpy(v)
    sentinel = np.full(n, -7.5, F)
    out = svo.DeviceBuffer.from_numpy(sentinel)

    def code(W, *args, **kw):
        with pytest.raises(svo.SvoError) as e:
            W.hit_ao(*args, **kw)
        return e.value.code

    prm = svo.trace_params()
    assert code(s.W, None, prm, rect, gd.ptr, vd.ptr, out.ptr) == -1
    assert code(s.W, s.cam, prm, rect, None, vd.ptr, out.ptr) == -1
    assert code(s.W, s.cam, prm, rect, gd.ptr, None, out.ptr) == -1
    assert code(s.W, s.cam, prm, rect, gd.ptr, vd.ptr, None) == -1
    assert code(s.W, s.cam, prm, (0, 0, -1, 4), gd.ptr, vd.ptr, out.ptr) == -1
    assert code(s.W, s.cam, prm, (-2, 0, 4, 4), gd.ptr, vd.ptr, out.ptr) == -1
    for cell in (-0.5, float("nan"), float("inf")):
        assert code(s.W, s.cam, prm, rect, gd.ptr, vd.ptr, out.ptr, cell=cell) == -1
    assert code(s.W, s.cam, svo.trace_params(see_through=0x10000), rect, gd.ptr, vd.ptr, out.ptr) == -1
    assert code(s.W, s.cam, svo.trace_params(semantics=7), rect, gd.ptr, vd.ptr, out.ptr) == -1
    assert code(s.W, s.cam, svo.trace_params(kernel=9), rect, gd.ptr, vd.ptr, out.ptr) == -1
    # a world that is not resident: bad arguments first, then the residency, also for an empty rectangle
    cold = svo.World.generate(1, 1, 1, 128, 4)
    assert code(cold, s.cam, prm, rect, gd.ptr, vd.ptr, out.ptr, cell=-1.0) == -1
    assert code(cold, s.cam, prm, rect, gd.ptr, vd.ptr, out.ptr) == -5
    assert code(cold, s.cam, prm, (0, 0, 0, 0), None, None, None) == -5
    cold.destroy()
    # chunk size 100: no exact geometry - STACK is refused as svo_world_locate refuses it, AUTO and LITERAL walk the tree pool
    W100 = svo.World.generate(1, 1, 1, 100, 5)
    W100.upload(0)
    assert W100.info.exact_geometry == 0
    assert code(W100, s.cam, svo.trace_params(kernel=svo.KERNEL_STACK), rect, gd.ptr, vd.ptr, out.ptr) == -6
    assert code(W100, s.cam, svo.trace_params(kernel=svo.KERNEL_STACK), (0, 0, 0, 0), None, None, None) == -6
    cam100 = svo.make_camera((50.0, 120.0, -30.0), (0.0, -0.5, 0.866), (0.0, 1.0, 0.0), 60.0, *M.IMAGE)
    g100 = W100.draw(cam100)
    v100 = W100.hit_boxes(g100)
    c100 = [W100.chunk(0)]
    want = M.hit_ao(c100, 100, cam100, None, g100, v100, M.TwinOccupancy(L.world_of(c100, 1, 1, 1, 100)))
    assert (want < 1).sum() > 100
    for kernel in (svo.KERNEL_AUTO, svo.KERNEL_LITERAL):
        assert_same_floats(W100.ao_image(cam100, g100, voxels=v100, kernel=kernel), want, f"size 100/kernel {kernel}")
    W100.destroy()
    svo.lib.svo_stream_synchronize(None)
    assert np.array_equal(out.to_numpy(F, n), sentinel), "a refused call wrote to ao_dev"
    # w*h == 0 is SVO_OK and touches nothing; params == NULL means defaults
    s.W.hit_ao(s.cam, prm, (0, 0, 0, 9), None, None, None)
    s.W.hit_ao(s.cam, None, rect, gd.ptr, vd.ptr, out.ptr)
    svo.lib.svo_stream_synchronize(None)
    assert_same_floats(out.to_numpy(F, n), s.want(0), "params == NULL")
    for b in (gd, vd, out):
        b.free()


def test_shade_ao_equals_numpy(svo, scenes):
    s = scenes("grid_2x1x2_d8", "default")
    g, v = s.frame(0)
    n, rect = g.size, (0, 0, g.shape[1], g.shape[0])
    ao = s.want(0).reshape(-1).copy()
    dark = np.nonzero(ao < 1)[0]
    ao[dark[::50]] = np.nan
    ao[dark[1]] = 0.0
    gd, aod, rgba = svo.DeviceBuffer.from_numpy(g), svo.DeviceBuffer.from_numpy(ao), svo.DeviceBuffer(n * 16)
    shaded = None
    for strength in (0.0, 0.5, 1.0):
        svo.shade(s.cam, svo.shade_defaults(), rect, gd.ptr, rgba.ptr)
        svo.lib.svo_stream_synchronize(None)
        if shaded is None:
            shaded = rgba.to_numpy(F, n * 4).reshape(n, 4)
            hit = (g.reshape(-1)["flags"] & 1) != 0
            assert np.abs(shaded[hit, :3]).sum() > 0 and np.unique(shaded[hit, 3]).size > 100
        svo.shade_ao(aod.ptr, strength, n, rgba.ptr)
        svo.lib.svo_stream_synchronize(None)
        got = rgba.to_numpy(F, n * 4).reshape(n, 4)
        want = M.shade_ao(ao, strength, shaded)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"strength {strength}"
        keep = ~(ao < 1) | (strength == 0.0)                   # ao == 1 (the misses among them) and NaN: the pixel's 16 bytes as they were
        assert np.array_equal(got.view(np.uint32)[keep], shaded.view(np.uint32)[keep])
        assert np.array_equal(got.view(np.uint32)[:, 3], shaded.view(np.uint32)[:, 3]), "the depth float is not written"
        changed = (got.view(np.uint32) != shaded.view(np.uint32)).any(axis=1).sum()
        print(f"strength {strength}: {int(changed)} of {n} pixels changed")
        assert (changed > 500) == (strength > 0.0)
        if strength == 1.0:
            assert np.all(got[dark[1], :3] == 0.0)
    for b in (gd, aod, rgba):
        b.free()
