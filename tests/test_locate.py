"""svo_world_locate on the GPU: the voxel under each point, both kernels (the tree-pool walk and the wide-pool walk) and both
semantics, bit for bit (the raw 32-byte records) against the host model tests/locate_model.py - on generated, mixed-depth and
hand-made worlds, after every kind of change to the resident world, with see_through, and kernel against kernel at full size.

Run as a script - python tests/test_locate.py <libsvo_hooks.so> - it uploads a world whose wide trees fail to build (the hooks
variant's SVO_TEST_FAIL_WIDE) and checks that SVO_KERNEL_AUTO still answers (one library per process, as tests/variant_check.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import locate_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"literal": 1, "stack": 2}
WATER = 6
F = np.float32


def raw(records):
    return np.ascontiguousarray(records).view(np.uint8).reshape(-1, 32)


def assert_records_equal(got, want, what):
    bad = np.nonzero((raw(got) != raw(want)).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.shape[0]} records differ, first at {bad[:5]}: got {got[bad[:3]]} want {want[bad[:3]]}"


def camera_dirs(cam):
    """The pinhole camera of include/svo.h in numpy float32, row-major (close to the kernels' rays; only used to make points)."""
    px, py = np.meshgrid(np.arange(cam.width, dtype=F), np.arange(cam.height, dtype=F))
    u = (((px + F(0.5)) / F(cam.width)) * F(2) - F(1)) * F(cam.tan_half_x)
    v = (F(1) - ((py + F(0.5)) / F(cam.height)) * F(2)) * F(cam.tan_half_y)
    d = (np.array(cam.forward, F)[None, None] + np.array(cam.right, F)[None, None] * u[..., None]) + np.array(cam.up, F)[None, None] * v[..., None]
    d = d / np.sqrt((d * d).sum(axis=2, dtype=F))[..., None]
    return d.reshape(-1, 3).astype(F)


def surface_points(svo, W, cam, limit=None):
    """o + d * t of a traced frame's hits, and the same nudged by +-EPS along d."""
    g = W.draw(cam).reshape(-1)
    hit = (g["flags"] & 1) != 0
    d, t = camera_dirs(cam)[hit], g["t"][hit]
    if limit is not None and t.size > limit:
        keep = np.random.default_rng(11).choice(t.size, limit, replace=False)
        d, t = d[keep], t[keep]
    o = np.array(cam.eye, F)[None]
    eps = F(1.0 / 8192.0)
    return np.concatenate([o + d * t[:, None], o + d * (t - eps)[:, None], o + d * (t + eps)[:, None]]).astype(F)


class Scene:
    """One resident world, its twin for the model, its point list; the model's records per (semantics, see_through), computed once."""

    def __init__(self, svo, name, chunks, w, h, d, chunksize, ccm, camera=True):
        self.svo, self.name, self.dims = svo, name, (w, h, d, chunksize, ccm)
        self.W = svo.World.create(chunks, w, h, d, chunksize, ccm)
        self.W.upload(0)
        self.twin = M.world_of(chunks, w, h, d, chunksize, ccm)
        lo, hi = M.box_of(w, h, d, chunksize, ccm)
        sets = M.point_sets(name, lo, hi)
        if camera:
            cx, cz = 0.5 * (lo[0] + hi[0]), lo[2] - 40.0
            cam = svo.make_camera((cx, 150.0, cz), (0.0, -0.5, 0.866), (0.0, 1.0, 0.0), 60.0, 64, 48)
            sets["surface"] = surface_points(svo, self.W, cam, 1200)
            assert sets["surface"].shape[0] >= 300, f"{name}: the camera sees no terrain"
        self.points = np.concatenate(list(sets.values()))
        assert self.points.shape[0] <= 20000
        self._want = {}

    def want(self, semantics=0, see_through=0):
        key = (semantics, see_through)
        if key not in self._want:
            self._want[key] = M.locate(self.twin, self.points, semantics, see_through)
        return self._want[key]

    def close(self):
        self.W.destroy()


@pytest.fixture(scope="module")
def scenes(svo):
    if svo.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    out = {}
    for name, (w, h, d, ccm, _) in M.WORLDS.items():
        out[name] = Scene(svo, name, M.make_chunks(svo, name), w, h, d, 128, ccm)
    w, h, d, ccm = M.HANDMADE
    out["handmade"] = Scene(svo, "handmade", M.handmade_chunks(), w, h, d, 128, ccm, camera=False)
    yield out
    for s in out.values():
        s.close()


@pytest.mark.parametrize("semantics", [0, 1])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", sorted(M.WORLDS) + ["handmade"])
def test_records_equal_the_model(svo, scenes, name, kernel, semantics):
    s = scenes[name]
    want = s.want(semantics)
    share = M.classes(want)
    print(f"{name} {kernel} semantics {semantics}: {s.points.shape[0]} points, {share}")
    assert all(share[c] > 0 for c in M.CLASSES)
    assert s.W.info.exact_geometry == 1 and s.W.info.wide_nodes > 0
    got = s.W.locate_points(s.points, kernel=KERNELS[kernel], semantics=semantics)
    assert_records_equal(got, want, f"{name}/{kernel}/semantics {semantics}")
    if kernel == "stack":                                       # AUTO takes the same walk; a second launch writes the same bytes
        assert_records_equal(s.W.locate_points(s.points, kernel=svo.KERNEL_AUTO, semantics=semantics), want, f"{name}/auto")


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", ["grid_2x1x2_d6", "handmade"])
def test_see_through_water(svo, scenes, name, kernel):
    """see_through = 6: the model's records, which are also those of the same world with its material-6 words rewritten to 0.  The
    generator's water (Ocroot::build below y = 6) lives in brick cells only; the hand-made world has a LEAF of material 6 as well."""
    s = scenes[name]
    plain, want = s.want(0), s.want(0, WATER)
    water = (plain["material"] == WATER) & ((plain["flags"] & M.SOLID) != 0)
    share = M.classes(plain[water])
    print(f"see_through {name} {kernel}: {int(water.sum())} of {plain.shape[0]} points lie in material {WATER} ({share})")
    assert water.sum() > 100 and share["solid_cell"] > 0 and (name != "handmade" or share["leaf"] > 0)
    assert not (want["material"] == WATER).any() and np.array_equal(raw(want)[~water], raw(plain)[~water])
    assert not (want["flags"][water] & M.SOLID).any() and np.array_equal(want["node"], plain["node"]) and np.array_equal(want["cell"], plain["cell"])
    got = s.W.locate_points(s.points, kernel=KERNELS[kernel], see_through=WATER)
    assert_records_equal(got, want, f"see_through/{kernel}")
    w, h, d, cs, ccm = s.dims
    dry = svo.World.create([svo.see_through_chunk(s.W.chunk(i), WATER) for i in range(w * h * d)], w, h, d, cs, ccm)
    dry.upload(0)
    assert_records_equal(dry.locate_points(s.points, kernel=KERNELS[kernel]), got, f"rewritten world/{kernel}")
    dry.destroy()
    # a material nothing holds changes nothing
    assert_records_equal(s.W.locate_points(s.points, kernel=KERNELS[kernel], see_through=0xFFFF), plain, f"see_through 0xFFFF/{kernel}")


def check_against_pools(svo, W, points, records, depth_of, chunksize):
    """Every record against the pools fetched with svo_world_chunk: the node is of the record's kind, the material is the word's or the
    cell's, the closed box holds p, size is chunksize / 2^level for an integer level <= depth."""
    inside = (records["flags"] & M.INSIDE) != 0
    assert not raw(records)[~inside].any()
    nchunks = len(depth_of)
    assert records["chunk"][inside].max() < nchunks
    for i in range(nchunks):
        sel = inside & (records["chunk"] == i)
        if not sel.any():
            continue
        c = W.chunk(i, copy=False)
        r, p = records[sel], points[sel].astype(np.float64)
        assert r["node"].max() < c["tree"].size
        word = c["tree"][r["node"]]
        kind, off = word >> 30, word & 0x3FFFFFFF
        cellular, solid = r["cell"] != M.CELL_NONE, (r["flags"] & M.SOLID) != 0
        assert not (kind == 2).any(), "a record names a BRANCH"
        assert np.all(kind[cellular] == 3) and np.all(r["cell"][cellular] < 64)
        assert np.all(solid[kind == 1]) and np.array_equal(r["material"][kind == 1], (off[kind == 1] & 0xFFFF).astype(np.uint16))
        assert not solid[kind == 0].any() and not r["material"][kind == 0].any()
        cells = c["twig"][off[cellular].astype(np.int64) * 64 + r["cell"][cellular]]
        assert np.array_equal(r["material"][cellular], cells) and np.array_equal(solid[cellular], cells != 0)
        lone = (kind == 3) & ~cellular                          # a TWIG without a cell: only on the chunk's max faces
        top = np.array(c["position"], np.float64) + chunksize
        assert np.all((p[lone] == top[None]).any(axis=1)) and not solid[lone].any()
        lo = r["bmin"].astype(np.float64)
        assert np.all((p >= lo) & (p <= lo + r["size"][:, None].astype(np.float64)))
        level = np.log2(chunksize / r["size"].astype(np.float64))
        assert np.all(level == np.round(level)) and level.min() >= 0 and level.max() <= depth_of[i]
        assert np.all(np.where(cellular, level == depth_of[i], level <= depth_of[i] - 2) | lone)
    return int(inside.sum())


def test_kernels_agree_at_full_size(svo):
    """The benchmark's grid at depth 10 (c3small: 4x1x4 chunks; the depth-12 world's pools take tens of seconds to fetch), built on
    the device: 2^21 uniform points and one frame's hit points, LITERAL and STACK byte for byte, every record held against the pools."""
    W = svo.World.generate(4, 1, 4, 128, 10, build_device=0)
    assert W.info.wide_nodes > 0
    rng = np.random.default_rng(2026)
    lo, hi = M.box_of(4, 1, 4, 128, (0, 0, 0))
    cam = svo.default_camera(4, 4, 128, 640, 360)
    sets = {"uniform": M.uniform_points(rng, 1 << 21, lo, hi, 0.05), "surface": surface_points(svo, W, cam)}
    for name, pts in sets.items():
        a = W.locate_points(pts, kernel=svo.KERNEL_LITERAL)
        b = W.locate_points(pts, kernel=svo.KERNEL_STACK)
        assert_records_equal(b, a, f"stack against literal, {name}")
        share = M.classes(a)
        print(f"full size, {name}: {pts.shape[0]} points, {share}")
        assert all(share[c] > 0 for c in M.CLASSES if (c != "outside" or name == "uniform"))       # (a hit point lies inside the world)
        assert check_against_pools(svo, W, pts, a, [10] * 16, 128.0) == pts.shape[0] - share["outside"]
    W.destroy()


def both_kernels_equal_model(svo, W, pts, what, dims=(2, 1, 2)):
    """The resident world as it is now: the model on the chunks svo_world_chunk fetches."""
    w, h, d = dims
    info = W.info
    ccm = tuple(info.chunkcoordmin)
    twin = M.world_of([W.chunk(i) for i in range(w * h * d)], w, h, d, 128, ccm)
    want = M.locate(twin, pts)
    assert info.wide_nodes > 0
    for kernel in (svo.KERNEL_LITERAL, svo.KERNEL_STACK):
        assert_records_equal(W.locate_points(pts, kernel=kernel), want, f"{what}/kernel {kernel}")
    return want


def test_the_world_as_it_is_now(svo):
    W = svo.World.generate(2, 1, 2, 128, 6)
    W.upload(0)
    rng = np.random.default_rng(77)
    lo, hi = M.box_of(2, 1, 2, 128, (0, 0, 0))
    pts = np.concatenate([M.uniform_points(rng, 2500, lo, hi), M.lattice_points(rng, 800, lo, hi, 1.0)])
    blo, bhi = np.array([20.0, 60.0, 20.0]), np.array([50.0, 100.0, 50.0])
    boxed = (blo + 0.25 + rng.random((600, 3)) * (bhi - blo - 0.5)).astype(F)
    pts = np.concatenate([pts, boxed])
    in_box = np.zeros(pts.shape[0], bool)
    in_box[-600:] = True
    before = both_kernels_equal_model(svo, W, pts, "uploaded")
    assert ((before["flags"][in_box] & M.SOLID) == 0).sum() > 100       # the box reaches into the air above the terrain
    # svo_world_edit_box: BUILD fills what was empty, DESTROY empties the box
    W.edit_box(0, svo.EDIT_BUILD, blo, bhi, 5)
    built = both_kernels_equal_model(svo, W, pts, "after BUILD")
    assert np.all((built["flags"][in_box] & M.SOLID) != 0) and (built["material"][in_box] == 5).sum() > 100
    assert np.array_equal(raw(built)[before["chunk"] != 0], raw(before)[before["chunk"] != 0])
    W.edit_box(0, svo.EDIT_DESTROY, blo, bhi)
    gone = both_kernels_equal_model(svo, W, pts, "after DESTROY")
    assert not (gone["flags"][in_box] & M.SOLID).any()
    # svo_world_compact / svo_world_coarsen: the same materials from fewer / coarser nodes
    W.compact(0)
    packed = both_kernels_equal_model(svo, W, pts, "after compact")
    low = pts[:, 1] != 128.0                                    # (on the world's top face a brick without a cell may have become a LEAF)
    assert np.array_equal(packed["material"][low], gone["material"][low]) and np.array_equal(packed["flags"][low], gone["flags"][low])
    W.coarsen(1)
    coarse = both_kernels_equal_model(svo, W, pts, "after coarsen")
    assert W.chunk(1)["depth"] == 5 and coarse["size"][(coarse["chunk"] == 1) & (coarse["cell"] != M.CELL_NONE)].min() == 4.0
    # svo_world_update with realloc: chunk 2 with every brick cell of material 1 repainted
    c = W.chunk(2)
    assert (c["twig"] == 1).sum() > 0
    c["twig"][c["twig"] == 1] = 7
    W.update(2, c, realloc=True)
    painted = both_kernels_equal_model(svo, W, pts, "after update")
    assert (painted["material"] == 7).sum() > 0 and not ((painted["chunk"] == 2) & (painted["material"] == 1) & (painted["cell"] != M.CELL_NONE)).any()
    # svo_world_shift: the window moves, the toroidal index with it
    W.shift((1, 0, 0))
    assert tuple(W.info.chunkcoordmin) == (1, 0, 0)
    moved = pts + np.array([128.0, 0.0, 0.0], F)[None]
    slid = both_kernels_equal_model(svo, W, moved, "after shift")
    assert all(M.classes(slid)[k] > 0 for k in M.CLASSES)
    W.destroy()


def test_statuses_and_inexact_geometry(svo):
    """Chunk size 100: no exact geometry - STACK is refused, AUTO and LITERAL walk the tree pool and equal the model."""
    W = svo.World.generate(1, 1, 1, 100, 6)
    assert W.info.exact_geometry == 0
    twin = M.world_of([W.chunk(0)], 1, 1, 1, 100)
    W.upload(0)
    rng = np.random.default_rng(3)
    lo, hi = M.box_of(1, 1, 1, 100, (0, 0, 0))
    pts = np.concatenate([M.uniform_points(rng, 3000, lo, hi), M.lattice_points(rng, 1000, lo, hi, 100.0 / 64.0), M.SPECIAL])
    for semantics in (0, 1):
        want = M.locate(twin, pts, semantics)
        assert all(M.classes(want)[k] > 0 for k in M.CLASSES)
        for kernel in (svo.KERNEL_AUTO, svo.KERNEL_LITERAL):
            assert_records_equal(W.locate_points(pts, kernel=kernel, semantics=semantics), want, f"size 100/kernel {kernel}/semantics {semantics}")
    with pytest.raises(svo.SvoError) as e:
        W.locate_points(pts, kernel=svo.KERNEL_STACK)
    assert e.value.code == -6
    # n == 0 is SVO_OK and touches nothing; params == NULL means defaults
    W.locate(None, 0, svo.trace_params(), None)
    pd, out = svo.DeviceBuffer.from_numpy(pts), svo.DeviceBuffer(pts.shape[0] * 32)
    W.locate(pd.ptr, pts.shape[0], None, out.ptr)
    svo.lib.svo_stream_synchronize(None)
    assert_records_equal(out.to_numpy(svo.VOXEL_DTYPE, pts.shape[0]), M.locate(twin, pts), "params == NULL")
    with pytest.raises(svo.SvoError) as e:
        W.locate(pd.ptr, 8, svo.trace_params(see_through=0x10000), out.ptr)
    assert e.value.code == -1
    pd.free()
    out.free()
    W.destroy()
    # chunk size 7: the one point where the CPU and the GLSL cell formulas part (tests/test_locate_cpu.py)
    cells = np.arange(1, 65, dtype=np.uint16)
    chunk = dict(position=(0, 0, 0), size=7.0, depth=2, tree=np.array([(3 << 30) | 0], np.uint32), twig=cells)
    W7 = svo.World.create([chunk], 1, 1, 1, 7)
    W7.upload(0)
    twin7 = M.world_of([chunk], 1, 1, 1, 7)
    x = np.nextafter(F(1.75), F(0))
    p7 = np.concatenate([np.array([[x, 0.5, 0.5], [1.75, 0.5, 0.5], [7.0, 7.0, 7.0]], F), M.uniform_points(rng, 500, np.zeros(3), np.full(3, 7.0))])
    got = [W7.locate_points(p7, semantics=sem) for sem in (0, 1)]
    for sem in (0, 1):
        assert_records_equal(got[sem], M.locate(twin7, p7, sem), f"size 7/semantics {sem}")
    assert got[0]["cell"][0] == 0 and got[1]["cell"][0] == 1
    W7.destroy()


def hooks_library():
    return os.path.join(ROOT, "octree-raymarcher_amd", "build", "libsvo_hooks.so")


def test_a_literal_only_world_still_answers():
    """SVO_OK_LITERAL_ONLY (the wide trees could not be built): reached through the hooks variant, in a process of its own."""
    assert os.path.exists(hooks_library()), f"{hooks_library()} missing: __graft_entry__.build() makes it"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), hooks_library()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "literal only: AUTO equals the model" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from variant_check import load
    svo_, _ = load(os.path.abspath(sys.argv[1]))
    if svo_.device_count() < 1:
        print("no HIP device")
        sys.exit(3)
    name_ = "grid_2x1x2_d6"
    w_, h_, d_, ccm_, _ = M.WORLDS[name_]
    chunks_ = M.make_chunks(svo_, name_)
    W_ = svo_.World.create(chunks_, w_, h_, d_, 128, ccm_)
    os.environ["SVO_TEST_FAIL_WIDE"] = "1"
    W_.upload(0)
    del os.environ["SVO_TEST_FAIL_WIDE"]
    assert W_.upload_status == svo_.OK_LITERAL_ONLY and W_.info.wide_nodes == 0
    pts_ = np.concatenate(list(M.point_sets(name_, *M.box_of(w_, h_, d_, 128, ccm_)).values()))
    want_ = M.locate(M.world_of(chunks_, w_, h_, d_, 128, ccm_), pts_)
    for kernel_ in (svo_.KERNEL_AUTO, svo_.KERNEL_LITERAL):
        assert_records_equal(W_.locate_points(pts_, kernel=kernel_), want_, f"literal only/kernel {kernel_}")
    try:
        W_.locate_points(pts_, kernel=svo_.KERNEL_STACK)
        raise AssertionError("SVO_KERNEL_STACK must be refused without a wide pool")
    except svo_.SvoError as e_:
        assert e_.code == -6
    W_.destroy()
    print("literal only: AUTO equals the model")
