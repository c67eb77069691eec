"""svo_hit_voxels on the GPU: the box of every hit, bit for bit (the raw 32-byte records, none left out) against the host model
tests/hit_voxels_model.py - records of both march kernels, both semantics, a see-through launch and a ray list, on generated,
mixed-depth and inexact worlds; two checks that do not rest on the model (cubeNormal / the face normal recomputed from the box, and
svo_world_locate at the box's centre); the parent index's lifetime across every kind of change to the pools; and the refusals."""
import numpy as np
import pytest

import hit_voxels_model as M

pytestmark = pytest.mark.gpu
F = np.float32
KERNELS = {"literal": 1, "stack": 2}
EXACT = ["grid_2x1x2_d6", "grid_neg_2x2x2_d5", "mixed_6_2_4_5"]
CASES = [(n, k) for n in EXACT for k in sorted(KERNELS)] + [("inexact_100_d5", "literal")]
EPS = {0: F(1.0 / 8192.0), 1: F(1.0 / 4096.0)}


def raw(records):
    return np.ascontiguousarray(records).view(np.uint8).reshape(-1, 32)


def assert_records_equal(got, want, what):
    bad = np.nonzero((raw(got) != raw(want)).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.shape[0]} records differ, first at {bad[:5]}: got {got[bad[:3]]} want {want[bad[:3]]}"


def check_boxes(W, chunks, records, what, least=300):
    """Every record of `records` through svo_hit_voxels against the model; misses and error records all zero."""
    g = np.ascontiguousarray(records).reshape(-1)
    got = W.hit_boxes(g)
    assert_records_equal(got, M.hit_voxels(chunks, g), what)
    usable = ((g["flags"] & 1) != 0) & ((g["flags"] & M.ERR_FLAG) == 0)
    assert not raw(got)[~usable].any(), f"{what}: a record without a usable hit got a box"
    assert np.all(got["flags"][usable] == 3) and usable.sum() >= least, f"{what}: {int(usable.sum())} hits"
    return got


class Scene:
    def __init__(self, svo, name):
        w, h, d, cs, ccm, _, _ = M.WORLDS[name]
        self.name, self.chunks = name, M.make_chunks(svo, name)
        self.W = svo.World.create(self.chunks, w, h, d, cs, ccm)
        self.W.upload(0)
        self.cams = M.cameras(svo, name)
        self.exact = self.W.info.exact_geometry == 1


@pytest.fixture(scope="module")
def scenes(svo):
    if svo.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    out = {name: Scene(svo, name) for name in M.WORLDS}
    yield out
    for s in out.values():
        s.W.destroy()


@pytest.mark.parametrize("semantics", [0, 1])
@pytest.mark.parametrize("name,kernel", CASES)
def test_boxes_equal_the_model(svo, scenes, name, kernel, semantics):
    s = scenes[name]
    assert s.exact == (name in EXACT)
    for view, cam in s.cams.items():
        g = s.W.draw(cam, kernel=KERNELS[kernel], semantics=semantics)
        check_boxes(s.W, s.chunks, g, f"{name}/{kernel}/semantics {semantics}/{view}")
    o, d = M.ray_list(name)
    g = s.W.chunkmarch(o, d, kernel=KERNELS[kernel], semantics=semantics, shadow=True)
    check_boxes(s.W, s.chunks, g, f"{name}/{kernel}/semantics {semantics}/rays")
    leaf, cell = M.kinds(g)
    assert leaf >= 100 and cell >= 100


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_see_through_records_keep_their_material(svo, scenes, kernel):
    """A see_through = 6 launch: the records name what lies behind the water, and the boxes carry the records' materials."""
    s = scenes["grid_2x1x2_d6"]
    cam = s.cams["above"]
    plain = s.W.draw(cam, kernel=KERNELS[kernel]).reshape(-1)
    g = s.W.draw(cam, kernel=KERNELS[kernel], see_through=6).reshape(-1)
    assert (plain["material"] == 6).sum() > 50 and not (g["material"] == 6).any()
    got = check_boxes(s.W, s.chunks, g, f"see_through/{kernel}")
    assert np.array_equal(got["material"], g["material"])


@pytest.mark.parametrize("normal_mode", [0, 1], ids=["cube", "face"])
@pytest.mark.parametrize("semantics", [0, 1])
@pytest.mark.parametrize("name", sorted(M.WORLDS))
def test_the_normal_follows_from_the_box(svo, scenes, name, semantics, normal_mode):
    """Not the model: cubeNormal(point, bmin, bmin + size) (or the entered-face normal) recomputed in float32 from the returned box
    equals the record's normal bit for bit, NaN lanes equal."""
    s = scenes[name]
    for view, cam in s.cams.items():
        g = s.W.draw(cam, kernel=svo.KERNEL_LITERAL, semantics=semantics, normal_mode=normal_mode).reshape(-1)
        v = s.W.hit_boxes(g)
        on = (v["flags"] & M.INSIDE) != 0
        assert on.sum() >= 300 and np.array_equal(on, (g["flags"] & 1) != 0)
        beta = M.camera_dirs(cam)[on]
        p = M.sample_points(np.array(cam.eye, F)[None], beta, g["t"][on], EPS[semantics])
        cmin = v["bmin"][on]
        cmax = cmin + v["size"][on][:, None]
        want = M.face_normal(p, cmin, cmax, beta) if normal_mode else M.cube_normal(p, cmin, cmax, EPS[semantics])
        got = g["normal"][on]
        nan = np.isnan(want)
        assert np.array_equal(nan, np.isnan(got)), f"{name}/{view}: NaN lanes differ"
        same = (got.view(np.uint32) == want.view(np.uint32)) | nan
        assert same.all(), f"{name}/{view}: {int((~same).any(axis=1).sum())} normals differ from the box's"
        if normal_mode == 0 and view == "above" and name in EXACT:
            assert (~nan).all(axis=1).sum() > 200


@pytest.mark.parametrize("name", EXACT)
def test_locate_at_the_centre_returns_the_voxel(svo, scenes, name):
    """Not the model: on exact geometry svo_world_locate at bmin + size * 0.5f finds the same chunk, node, cell, bmin and size."""
    s = scenes[name]
    for view, cam in s.cams.items():
        g = s.W.draw(cam).reshape(-1)
        v = s.W.hit_boxes(g)
        v = v[(v["flags"] & M.INSIDE) != 0]
        assert v.shape[0] >= 300
        centre = v["bmin"] + (v["size"] * F(0.5))[:, None]
        at = s.W.locate_points(centre)
        for f in ("chunk", "node", "cell", "size"):
            assert np.array_equal(at[f], v[f]), f"{name}/{view}: {f} differs"
        assert np.array_equal(at["bmin"].view(np.uint32), v["bmin"].view(np.uint32))
        assert np.all(at["flags"] == 3)


def test_every_change_to_the_pools_drops_the_index(svo):
    """Trace and get boxes; edit (a DESTROY that orphans blocks, a BUILD that appends blocks), compact, coarsen, shift - after each,
    trace again and compare with the model of the pools as they are now.  A stale index fails these: the appended blocks have no
    parent in it, compacted blocks have moved."""
    name = "grid_2x1x2_d6"
    w, h, d, cs, ccm, depths, _ = M.WORLDS[name]
    W = svo.World.generate(w, h, d, cs, depths[0], chunkcoordmin=ccm)
    W.upload(0)
    cam = M.cameras(svo, name)["above"]
    n = w * h * d

    def stage(what):
        chunks = [W.chunk(i) for i in range(n)]
        for kernel in sorted(KERNELS):
            check_boxes(W, chunks, W.draw(cam, kernel=KERNELS[kernel]), f"{what}/{kernel}")
        return chunks

    before = stage("fresh")
    W.edit_box(0, svo.EDIT_DESTROY, (30.0, 0.0, 20.0), (90.0, 120.0, 70.0))
    W.edit_box(0, svo.EDIT_BUILD, (50.0, 70.0, 30.0), (75.0, 90.0, 55.0), 3)
    edited = stage("edited")
    assert edited[0]["tree"].size > before[0]["tree"].size, "the BUILD appended no blocks"
    _, level = M.parent_map(edited[0])
    assert (level == 0).sum() > 0, "the DESTROY orphaned no blocks"
    g = W.draw(cam).reshape(-1)
    new = (g["chunk"] == 0) & (g["node"] >= before[0]["tree"].size) & ((g["flags"] & 1) != 0)
    assert new.sum() > 20, "no hit on an appended node: a stale index would go unnoticed"
    W.compact(0)
    compacted = stage("compacted")
    assert compacted[0]["tree"].size < edited[0]["tree"].size
    W.coarsen(0)
    assert stage("coarsened")[0]["depth"] == depths[0] - 1
    W.shift((1, 0, 0))
    stage("shifted")
    W.destroy()


def test_ids_that_name_nothing_give_zero_records(svo):
    """chunk == chunk count, node == trees, cell == 64, a LEAF with a cell, a TWIG without one, EMPTY and BRANCH nodes and the nodes
    of an orphan block whose BRANCH word names a live block: all zero, and the valid records in the same buffer unaffected."""
    c = M.handmade_chunk()
    W = svo.World.create([c], 1, 1, 1, 128)
    W.upload(0)

    def hit(chunk, node, cell, material=3, flags=1):
        r = np.zeros(1, M.HIT_DTYPE)
        r[0] = (10.0, (0, 1, 0), material, flags, chunk, node, cell)
        return r

    good = [hit(0, 14, 0xFF), hit(0, 17, 0xFF, 2), hit(0, 23, 27, 28), hit(0, 23, 0, 0x4321), hit(0, 23, 63)]
    bad = [hit(1, 14, 0xFF), hit(0xFFFFFFFF, 14, 0xFF), hit(0, 25, 0xFF), hit(0, 0xFFFFFFFF, 0xFF), hit(0, 23, 64), hit(0, 23, 0xFF), hit(0, 14, 5),
           hit(0, 9, 0xFF), hit(0, 10, 0xFF), hit(0, 0, 0xFF), hit(0, 4, 0xFF), hit(0, 3, 0xFF), hit(0, 14, 0xFF, flags=0),
           hit(0, 14, 0xFF, flags=1 | M.ERR_FLAG)]
    g = np.concatenate([r for pair in zip(bad, (good * 3)[:len(bad)]) for r in pair])
    got = W.hit_boxes(g)
    assert_records_equal(got, M.hit_voxels([c], g), "handmade")
    assert not raw(got)[0::2].any() and np.all(got["flags"][1::2] == 3)
    assert tuple(got[1]["bmin"]) == (64.0, 0.0, 64.0) and got[1]["size"] == 64.0          # the LEAF directly under the root
    k = 2 * 2 + 1                                                                         # the TWIG's cell 27
    assert tuple(got[k]["bmin"]) == (88.0, 48.0, 40.0) and got[k]["size"] == 8.0 and got[k]["material"] == 28
    # n == 0 launches nothing; a second call (the index is warm now) writes the same bytes
    W.hit_voxels(None, 0, None)
    assert_records_equal(W.hit_boxes(g), got, "second call")
    W.destroy()
