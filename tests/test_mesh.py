"""svo_device_grid_add_mesh / svo_device_grid_fill_enclosed (csrc/mesh.hip) on the GPU: the grid the device leaves equals the numpy
model's (tests/mesh_model.py), cell for cell - exact equality of uint16 grids everywhere - with a sentinel behind the grid and the
mesh's arrays untouched; then the way on from the grid: svo_world_chunk_from_grid, both march kernels, one svo_trace_instances
placement.  The shapes are the smallest at which the kernels can still go wrong: triangle counts around the 64 lanes of a wave and
the 256 threads of a block, a grid that is one tile, a triangle that is thousands of tile jobs beside hundreds that are one, 64
writers per grid word, corridors that need hundreds of sweeps."""
import numpy as np
import pytest

import grid_model as G
import instances_model as IM
import mesh_model as M
from helpers import assert_gbuffer_equal
from test_compact_model import same_pools

pytestmark = pytest.mark.gpu

PAD = 64
SENTINEL = np.uint16(0xBEEF)


def zeros(depth):
    n = 1 << depth
    return np.zeros((n, n, n), np.uint16)


class DeviceGrid:
    """A grid in device memory with PAD sentinel cells behind it."""

    def __init__(self, svo, grid):
        self.svo, self.shape, self.depth = svo, grid.shape, G.depth_of(grid) if grid.shape[0] >= 4 else 0
        self.buf = svo.DeviceBuffer.from_numpy(np.concatenate([grid.reshape(-1), np.full(PAD, SENTINEL, np.uint16)]))
        self.ptr = self.buf.ptr

    def read(self):
        cells = self.buf.to_numpy(np.uint16, int(np.prod(self.shape)) + PAD)
        assert np.all(cells[-PAD:] == SENTINEL), "wrote behind the grid"
        return cells[:-PAD].reshape(self.shape)

    def free(self):
        self.buf.free()


def device_add(svo, grid, v, ix, origin=(0.0, 0.0, 0.0), cell=1.0, material=1, materials=None, into=None):
    """svo_device_grid_add_mesh of host arrays: uploads them, checks that the call left them and the sentinel alone, returns the grid
    (or, `into` a DeviceGrid, adds to that one and returns nothing)."""
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    ix = np.ascontiguousarray(ix, np.uint32).reshape(-1, 3)
    D = into if into is not None else DeviceGrid(svo, grid)
    bv, bi = svo.DeviceBuffer.from_numpy(v), svo.DeviceBuffer.from_numpy(ix)
    bm = None if materials is None else svo.DeviceBuffer.from_numpy(np.ascontiguousarray(materials, np.uint16))
    assert svo.device_grid_add_mesh(D.ptr, D.depth, bv.ptr, v.shape[0], bi.ptr, ix.shape[0], origin, cell, material, bm.ptr if bm else None) == svo.SVO_OK
    assert np.array_equal(bv.to_numpy(np.float32, v.size).view(np.uint32), v.reshape(-1).view(np.uint32)), "the vertices were written"
    assert np.array_equal(bi.to_numpy(np.uint32, ix.size), ix.reshape(-1)), "the indices were written"
    if bm:
        assert np.array_equal(bm.to_numpy(np.uint16, ix.shape[0]), np.asarray(materials, np.uint16)), "the materials were written"
        bm.free()
    bv.free(); bi.free()
    if into is not None:
        return None
    out = D.read()
    D.free()
    return out


def device_fill(svo, grid, material):
    D = DeviceGrid(svo, grid)
    count = svo.device_grid_fill_enclosed(D.ptr, D.depth, material)
    out = D.read()
    D.free()
    return out, count


def differs(got, want):
    bad = np.argwhere(got != want)
    return f"{bad.shape[0]} cells differ, first [z, y, x] {bad[:4].tolist()}: got {[int(got[tuple(b)]) for b in bad[:4]]} want {[int(want[tuple(b)]) for b in bad[:4]]}"


def same_grid(got, want, what=""):
    assert np.array_equal(got, want), f"{what}: {differs(got, want)}"


@pytest.fixture(scope="module", autouse=True)
def device(svo):
    if svo.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")


@pytest.mark.parametrize("name", ["sphere5", "sphere5_off", "sphere4", "torus5", "soup2", "soup5", "lattice_cube"])
def test_device_grid_equals_the_model(svo, name):
    depth, v, ix, kw = M.cases()[name]
    want = M.model_grid(name)
    assert want.any()
    same_grid(device_add(svo, zeros(depth), v, ix, **kw), want, name)
    if name == "lattice_cube":
        assert int((want != 0).sum()) == 208


@pytest.fixture(scope="module")
def many():
    """257 triangles at depth 5 and the model's grids of their prefixes (computed once)."""
    v, ix, m = M.soup(11, 257, 32)
    v[:3] = [[3.3, 4.4, 5.5], [9.1, 6.2, 4.3], [5.7, 11.6, 8.2]]              # the first one inside the grid
    return v, ix, m, {k: M.add_mesh(zeros(5), v, ix[:k], materials=m[:k]) for k in (0, 1, 63, 64, 65, 257)}


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_triangle_counts_around_a_wave_and_a_block(svo, many, count):
    v, ix, m, want = many
    assert count == 0 or want[count].any()
    same_grid(device_add(svo, zeros(5), v, ix[:count], materials=m[:count]), want[count], f"{count} triangles")


def test_material_0_and_a_shuffled_order_on_the_device(svo, many):
    v, ix, m, want = many
    pre = np.random.default_rng(2).integers(0, 4, (32, 32, 32)).astype(np.uint16)
    same_grid(device_add(svo, pre, v, ix, material=0), pre, "mesh.material = 0")
    same_grid(device_add(svo, pre, v, ix, materials=np.zeros(257, np.uint16)), pre, "every triangle's material 0")
    some = m.copy()
    some[::2] = 0                                           # every other triangle writes nothing
    model = M.add_mesh(zeros(5), v, ix, materials=some)
    assert model.any() and not np.array_equal(model, want[257])
    same_grid(device_add(svo, zeros(5), v, ix, materials=some), model, "material 0 among others")
    order = np.random.default_rng(9).permutation(257)
    same_grid(device_add(svo, zeros(5), v, ix[order], materials=m[order]), want[257], "shuffled")


def test_dropped_triangles_on_the_device(svo):
    nan, inf = float("nan"), float("inf")
    v = np.array([[2, 2, 2], [9, 3, 4], [4, 10, 6], [6, 6, 6], [3, 3, 3], [4, 4, 4], [5, 5, 5], [nan, 5, 5], [5, inf, 5], [5, 5, -inf]], np.float32)
    ix = np.array([(0, 1, 1), (0, 0, 0), (4, 5, 6), (6, 3, 4), (0, 1, 2), (0, 1, 7), (8, 1, 2), (0, 9, 2), (0, 1, 10), (10, 1, 2), (0, 0xFFFFFFFF, 2),
                   (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (1, 2, 3)], np.uint32)
    want = M.add_mesh(zeros(4), v, ix[[4, 12]], material=9)
    assert want.any()
    same_grid(device_add(svo, zeros(4), v, ix, material=9), want, "dropped among live triangles")
    dead = np.delete(ix, [4, 12], axis=0)
    assert not device_add(svo, zeros(4), v, dead, material=9).any()


def test_depth_2_is_one_tile(svo):
    v = np.array([[-1.0, 0.5, 0.2], [4.5, 1.5, 3.9], [1.0, 5.0, 2.5], [0.3, 0.3, 0.3], [0.6, 0.4, 0.35], [0.4, 0.7, 0.5]], np.float32)
    ix = np.array([(0, 1, 2), (3, 4, 5)], np.uint32)
    mats = np.array([5, 0xFFFF], np.uint16)
    want = M.add_mesh(zeros(2), v, ix, materials=mats)
    assert (want == 5).sum() > 8 and (want == 0xFFFF).sum() >= 1
    same_grid(device_add(svo, zeros(2), v, ix, materials=mats), want, "depth 2")


def test_a_mesh_partly_and_wholly_outside_the_grid(svo):
    v, ix = M.uv_sphere((16.2, 15.8, 16.1), 17.5)           # leaves the grid through all six faces, the corners stay inside
    want = M.add_mesh(zeros(5), v, ix, material=4)
    for face in (want[0], want[-1], want[:, 0], want[:, -1], want[:, :, 0], want[:, :, -1]):
        assert face.any() and not face.all()
    same_grid(device_add(svo, zeros(5), v, ix, material=4), want, "partly outside")
    pre = np.random.default_rng(1).integers(0, 3, (32, 32, 32)).astype(np.uint16)
    for centre in ((100.0, 100.0, 100.0), (-40.0, 16.0, 16.0), (16.0, 16.0, 45.0)):
        v, ix = M.uv_sphere(centre, 10.0)
        same_grid(device_add(svo, pre, v, ix, material=9), pre, f"wholly outside at {centre}")


@pytest.fixture(scope="module")
def split_mesh():
    """Depth 6: one triangle across the whole grid (its cell box is all 16^3 tiles) and 500 triangles smaller than a cell."""
    big = np.array([[-5.0, -3.0, -4.0], [70.0, 66.0, 20.0], [10.0, 68.0, 71.0]], np.float32)
    v, ix, m = M.soup(13, 500, 64, small=0.8)
    v, ix = M.concat((big, np.array([(0, 1, 2)], np.uint32)), (v, ix))
    m = np.concatenate([np.array([500], np.uint16), m])
    want = M.add_mesh(zeros(6), v, ix, materials=m)
    return v, ix, m, want


def test_work_splitting_one_huge_triangle_beside_500_tiny_ones(svo, split_mesh):
    v, ix, m, want = split_mesh
    assert (want == 500).sum() > 2000 and ((want != 0) & (want != 500)).sum() > 300
    got = device_add(svo, zeros(6), v, ix, materials=m)
    same_grid(got, want, "huge + tiny")
    same_grid(device_add(svo, zeros(6), v, ix[::-1], materials=m[::-1]), got, "the same mesh reversed")


@pytest.mark.parametrize("x0,x1", [(3.3, 10.6), (4.2, 11.5)])
def test_the_merge_is_a_maximum_whatever_arrives_first(svo, x0, x1):
    """64 coincident triangles of materials 1 .. 64 over cells that begin at an odd (3 .. 10) or an even x (4 .. 11): 64 writers per
    32-bit word.  Then on a checkerboard of 100: those cells keep 100, the other half of each word holds the model's value."""
    tri = np.array([[x0, 2.2, 3.1], [x1, 4.4, 9.7], [0.5 * (x0 + x1), 12.8, 5.2]], np.float32)
    v = np.tile(tri, (64, 1))
    ix = np.arange(192, dtype=np.uint32).reshape(64, 3)
    mats = np.random.default_rng(4).permutation(64).astype(np.uint16) + 1
    want = M.add_mesh(zeros(4), v[:3], ix[:1], material=64)
    xs = np.nonzero(want.any(axis=(0, 1)))[0]
    assert (xs[0], xs[-1]) == (int(x0), int(x1)) and (want != 0).sum() > 60
    got = device_add(svo, zeros(4), v, ix, materials=mats)
    same_grid(got, want, "64 coincident triangles")
    assert set(np.unique(got)) == {0, 64}
    z, y, x = np.indices(want.shape)
    board = np.where((x + y + z) % 2 == 0, 100, 0).astype(np.uint16)
    want = np.maximum(board, want)
    got = device_add(svo, board, v, ix, materials=mats)
    same_grid(got, want, "on the checkerboard")
    assert (got[board == 100] == 100).all() and set(np.unique(got[board == 0])) == {0, 64}


def test_two_calls_compose(svo):
    depth, v, ix, kw = M.cases()["soup5"]
    D = DeviceGrid(svo, zeros(depth))
    device_add(svo, None, v, ix[:23], materials=kw["materials"][:23], into=D)
    assert not np.array_equal(D.read(), M.model_grid("soup5"))
    device_add(svo, None, v, ix[23:], materials=kw["materials"][23:], into=D)
    same_grid(D.read(), M.model_grid("soup5"), "two calls")
    D.free()


@pytest.mark.parametrize("name", ["shell", "holed", "nested", "full", "empty", "depth2"])
def test_device_fill_equals_the_model(svo, name):
    g = M.fill_cases()[name]
    want = g.copy()
    count = M.fill_enclosed(want, 11)
    got, filled = device_fill(svo, g, 11)
    assert filled == count
    same_grid(got, want, name)
    assert count == {"holed": 0, "full": 0, "empty": 0, "depth2": 7}.get(name, count) and (name not in ("shell", "nested") or count > 3000)


@pytest.fixture(scope="module")
def shell7():
    """A sphere shell at depth 7 (rows of two 64-bit words) and the model's fill of it, computed once."""
    g = M.add_mesh(zeros(7), *M.uv_sphere((64.3, 63.6, 64.2), 50.4, nu=24, nv=16), material=3)
    want = g.copy()
    return g, want, M.fill_enclosed(want, 11)


def test_fill_at_depth_7_where_a_row_is_several_words(svo, shell7):
    """Depth 7: the words per row, the 64 cells per word and the carry between x-neighbour words, which no grid of 32^3 reaches."""
    g, want, count = shell7
    assert count > 400000 and want[64, 64, 63] == 11 and want[64, 64, 64] == 11      # the interior spans the word boundary at x = 63 / 64
    got, filled = device_fill(svo, g, 11)
    assert filled == count
    same_grid(got, want, "sphere shell at depth 7")
    holed = g.copy()
    x = int(np.flatnonzero(g[64, 64])[0])
    holed[64, 64, x:x + 3] = 0                              # a hole through the shell on the -x side: everything is outside
    assert M.fill_enclosed(holed.copy(), 11) == 0
    got, filled = device_fill(svo, holed, 11)
    assert filled == 0
    same_grid(got, holed, "holed shell at depth 7")


@pytest.mark.parametrize("depth,block,at,along", [(5, 16, 4, 0), (5, 16, 4, 1), (5, 24, 4, 2), (6, 16, 24, 0), (6, 16, 24, 2), (7, 16, 56, 0), (7, 16, 56, 1)])
def test_fill_follows_a_serpentine_corridor_to_its_end(svo, depth, block, at, along):
    """A corridor one cell wide through a block^3 cube (this construction gives 735 cells in 16^3 and 2783 in 24^3): open at its mouth
    nothing is filled, sealed every cell is.  Along y or z every cell is a word of its own, so the flood needs a sweep per cell: no
    fixed number of sweeps gets this right.  Depth 6: a row is exactly one 64-bit word.  Depth 7, the cube at cells 56 .. 71: rows of
    two words, and along x every row of the corridor crosses from one word into the next at x = 63 / 64, in both directions."""
    for sealed in (False, True):
        g, path = M.serpentine(depth, block, at, sealed, along)
        assert len(path) > (1000 if block == 24 else 700)
        want = g.copy()
        if sealed:
            want[tuple(np.array(path).T)] = 8
        got, filled = device_fill(svo, g, 8)
        assert filled == (len(path) if sealed else 0)
        same_grid(got, want, f"block {block}, along {along}, sealed {sealed}")


@pytest.fixture(scope="module")
def sphere_world(svo):
    """The sphere voxelised and filled on the device at depth 5, installed from the device pointer as the one chunk of a 32-unit world."""
    depth, v, ix, _ = M.cases()["sphere5"]
    want = M.model_grid("sphere5").copy()
    count = M.fill_enclosed(want, 2)
    D = DeviceGrid(svo, zeros(depth))
    device_add(svo, None, v, ix, material=5, into=D)
    assert svo.device_grid_fill_enclosed(D.ptr, depth, 2) == count
    want[want == 1] = 5
    same_grid(D.read(), want, "voxelised and filled")
    empty = dict(position=(0.0, 0.0, 0.0), size=float(IM.MODEL_SIZE), depth=3, tree=np.zeros(1, np.uint32), twig=np.zeros(0, np.uint16))
    W = svo.World.create([empty], 1, 1, 1, IM.MODEL_SIZE).upload(0)
    assert W.chunk_from_grid(0, D.ptr, depth) == svo.SVO_OK
    D.free()
    yield W, G.chunk_of(want, size=float(IM.MODEL_SIZE))
    W.destroy()


def test_end_to_end_the_chunk_and_its_march(svo, oracle, sphere_world):
    W, chunk = sphere_world
    same_pools(W.chunk(0), chunk, "chunk from the device grid")
    O = oracle.OracleWorld.from_chunks([chunk], 1, 1, 1, IM.MODEL_SIZE)
    cam = svo.make_camera((14.0, 40.0, -22.0), (0.05, -0.5, 0.866), (0.0, 1.0, 0.0), 60.0, 64, 48)
    for semantics in (0, 1):
        want = O.trace_image(cam, params=oracle.make_params(shadow=True, semantics=semantics))
        assert int((want["flags"] & 1).sum()) > 200
        for kernel in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
            assert_gbuffer_equal(W.draw(cam, shadow=True, kernel=kernel, semantics=semantics), want, f"semantics {semantics} / kernel {kernel}")


def test_end_to_end_one_instance_placement(svo, oracle, sphere_world):
    from test_instances import assert_records, assert_words, stage1
    Mw, chunk = sphere_world
    scene = svo.World.generate(2, 1, 2, 128, 6)
    chunks = [scene.chunk(i) for i in range(4)]
    scene.upload(0)
    cam = svo.default_camera(2, 2, 128, 64, 48)
    rect, inst = (0, 0, 64, 48), [IM.instance((94.0, 84.0, 4.0))]              # identity rotation, integer position
    S = dict(W=scene, Mw=Mw, cam=cam, inst=inst)
    ow, om = oracle.OracleWorld.from_chunks(chunks, 2, 1, 2, 128), oracle.OracleWorld.from_chunks([chunk], 1, 1, 1, IM.MODEL_SIZE)
    frame = ow.trace_image(cam, params=oracle.make_params(shadow=True), threads=8).reshape(-1)
    want = IM.trace(oracle, om, IM.world_box((0, 0, 0), (1, 1, 1), IM.MODEL_SIZE), cam, rect, frame, inst, max_rays=64 * 48)
    assert want["stats"][0]["owned"] > 50
    for kernel in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
        got = stage1(svo, S, svo.trace_params(shadow=True, kernel=kernel), rect=rect, max_rays=64 * 48)
        assert got["counts"] == want["counts"]
        assert_words(got["owner"], want["owner"], f"owner, kernel {kernel}")
        assert_records(got["merged"], want["merged"], f"merged, kernel {kernel}")
    scene.destroy()


def test_a_misaligned_grid_is_refused_and_nothing_is_written(svo):
    v, ix = M.lattice_cube()
    D = DeviceGrid(svo, zeros(4))
    bv, bi = svo.DeviceBuffer.from_numpy(v), svo.DeviceBuffer.from_numpy(ix)
    for off in (2, 4, 8):
        with pytest.raises(svo.SvoError) as e:
            svo.device_grid_add_mesh(D.ptr + off, 3, bv.ptr, 8, bi.ptr, 12)
        assert e.value.code == -1
        with pytest.raises(svo.SvoError) as e:
            svo.device_grid_fill_enclosed(D.ptr + off, 3, 1)
        assert e.value.code == -1
    with pytest.raises(svo.SvoError) as e:
        svo.device_grid_fill_enclosed(D.ptr, 4, 0)
    assert e.value.code == -1
    assert not D.read().any()
    assert svo.device_grid_add_mesh(D.ptr, 4, bv.ptr, 8, bi.ptr, 0) == svo.SVO_OK and not D.read().any()
    bv.free(); bi.free(); D.free()
