"""svo_world_chunk_from_grid / svo_world_chunk_to_grid on an uploaded world (csrc/grid.hip): the pools the device builds from a grid
equal the model's (tests/grid_model.py) index for index, the grid read back equals the model's sampling of them, both kernels march
the result as the oracle marches the model's pools, and everything an install must drop or rebuild follows."""
import numpy as np
import pytest

import grid_model as G
import lod_model as M
from helpers import assert_gbuffer_equal, random_rays
from test_compact_model import leaf_centres, same_pools

pytestmark = pytest.mark.gpu

NAMES = ["g2_empty", "g2_leaf", "g2_mixed", "g3", "g5", "g6", "g7"]

def empty_chunk(depth, position=(0.0, 0.0, 0.0)):
    return dict(position=position, size=128.0, depth=depth, tree=np.zeros(1, np.uint32), twig=np.zeros(0, np.uint16))


def empty_world(svo, depths, dims):
    chunks = [empty_chunk(d, (128.0 * (i % dims[0]), 0.0, 0.0)) for i, d in enumerate(depths)]
    return svo.World.create(chunks, *dims, 128).upload(0)


@pytest.mark.parametrize("name", NAMES)
def test_device_pools_equal_the_model_and_the_grid_comes_back(svo, name):
    grid = G.grids()[name]
    want, depth = G.model_chunk(name), G.depth_of(grid)
    W = empty_world(svo, [depth + 3 if depth < 5 else depth - 2], (1, 1, 1))      # a different depth to begin with
    assert W.set_chunk_grid(0, grid) == svo.SVO_OK
    same_pools(W.chunk(0), want, name)
    info = W.info
    assert info.max_chunk_depth == depth and info.exact_geometry == 1
    assert info.total_trees == want["tree"].size and info.total_twigs == want["twig"].size // 64
    for d in (depth, depth - 1, depth + 1):
        if d >= 2:
            assert np.array_equal(W.chunk_grid(0, d), G.pools_to_grid(want, d)), f"{name}: to_grid at depth {d}"
    assert np.array_equal(W.chunk_grid(0, depth), grid)
    W.destroy()


def test_to_grid_reads_every_kind_of_pool(svo):
    """Pools no grid produces: a brick above level depth-2 (the terrain's sparse refinement), blocks an edit orphaned, uniform bricks."""
    W = svo.World.generate(1, 1, 1, 128, 6, coarse_depth=4, refine_box=((0.0, -1e9, -1e9), (40.0, 1e9, 1e9)), build_device=0)
    W.edit_box(0, svo.EDIT_DESTROY, (10.0, 0.0, 10.0), (90.0, 128.0, 70.0))
    W.edit_box(0, svo.EDIT_BUILD, (30.5, 20.0, 30.5), (60.0, 50.0, 66.0), 4)
    c = W.chunk(0)
    for d in (6, 4, 7, 2):
        assert np.array_equal(W.chunk_grid(0, d), G.pools_to_grid(c, d)), f"to_grid at depth {d}"
    W.destroy()


def test_round_trip_of_a_terrain_chunk(svo):
    """to_grid -> from_grid -> to_grid on a generated chunk (depth 6, with water): identical grids, and identical trace records apart
    from the node / cell ids - the rebuilt tree is minimal and numbered breadth-first, the terrain's is neither, so a hit names another
    node; t, normal, material, flags and chunk are compared, bit for bit, under SVO_SEMANTICS_GLSL.
    Under SVO_SEMANTICS_CPU the records cannot be identical, and the test does not ask for it: the CPU march reports a LEAF hit at
    t - EPS and a brick-cell hit at t (src/Traverse.cpp), and the rebuilt tree has a LEAF where the terrain's had a brick of one value
    (and the other way round where the water fill split a node).  The CPU oracle over the two sets of pools shows the same: of this
    camera's 6144 pixels 203 differ in t, each by 1/8192, and 11 of those in their shadow bit.  There material, chunk and the hit bit
    are compared."""
    W = svo.World.generate(1, 1, 1, 128, 6, build_device=0)
    cam = svo.default_camera(1, 1, 128, 96, 64)
    views = [(k, sem) for k in (svo.KERNEL_STACK, svo.KERNEL_LITERAL) for sem in (svo.SEMANTICS_GLSL, svo.SEMANTICS_CPU)]
    before = {v: W.draw(cam, shadow=True, kernel=v[0], semantics=v[1]) for v in views}
    g0 = W.chunk_grid(0, 6)
    assert (g0 == 6).any() and (g0 != 0).sum() > 1000                    # water and terrain
    assert W.set_chunk_grid(0, g0) == svo.SVO_OK
    assert np.array_equal(W.chunk_grid(0, 6), g0)
    same_pools(W.chunk(0), G.chunk_of(g0), "terrain chunk rebuilt from its grid")
    for (k, sem), want in before.items():
        got = W.draw(cam, shadow=True, kernel=k, semantics=sem)
        what = f"kernel {k}, semantics {sem}"
        assert int((want["flags"] & 1).sum()) > 500
        assert np.array_equal(got["material"], want["material"]) and np.array_equal(got["chunk"], want["chunk"]), what
        assert np.array_equal(got["flags"] & 1, want["flags"] & 1), what
        if sem == svo.SEMANTICS_GLSL:
            assert np.array_equal(got["flags"], want["flags"]), what
            assert np.array_equal(got["t"].view(np.uint32), want["t"].view(np.uint32)), what + ": t"
            assert np.array_equal(got["normal"].view(np.uint32), want["normal"].view(np.uint32)), what + ": normal"
    W.destroy()


@pytest.fixture(scope="module")
def two_chunks():
    """The model's chunks of the 2x1x1 parity world: G5 at the origin, G6 beside it."""
    return [G.chunk_of(G.grids()["g5"]), G.chunk_of(G.grids()["g6"], position=(128.0, 0.0, 0.0))]


def parity_world(svo):
    W = empty_world(svo, [3, 2], (2, 1, 1))
    assert W.set_chunk_grid(0, G.grids()["g5"]) == svo.SVO_OK and W.set_chunk_grid(1, G.grids()["g6"]) == svo.SVO_OK
    return W


def test_march_parity_with_the_oracle_over_the_model_pools(svo, oracle, two_chunks):
    W = parity_world(svo)
    assert W.info.exact_geometry == 1 and W.info.max_chunk_depth == 6
    O = oracle.OracleWorld.from_chunks(two_chunks, 2, 1, 1, 128)
    cam = svo.default_camera(2, 1, 128, 64, 48)
    o, d = random_rays(np.random.default_rng(56), 4096, (0, 0, 0), (256, 128, 128))
    for semantics in (0, 1):
        prm = oracle.make_params(shadow=True, semantics=semantics)
        want_image, want_rays = O.trace_image(cam, params=prm), O.trace_rays(o, d, params=prm, threads=8)
        assert int((want_image["flags"] & 1).sum()) > 50 and int((want_rays["flags"] & 1).sum()) > 500
        for kernel in (svo.KERNEL_LITERAL, svo.KERNEL_STACK):           # (the stack kernel is asked for by name: a refusal would raise)
            what = f"semantics {semantics} / kernel {kernel}"
            assert_gbuffer_equal(W.draw(cam, shadow=True, kernel=kernel, semantics=semantics), want_image, "image, " + what)
            assert_gbuffer_equal(W.chunkmarch(o, d, shadow=True, kernel=kernel, semantics=semantics), want_rays, "rays, " + what)
    W.destroy()


def test_the_install_drops_what_was_derived_from_the_old_pools(svo, oracle, two_chunks):
    import hit_voxels_model as HV
    W = empty_world(svo, [3, 2], (2, 1, 1))
    cam = svo.default_camera(2, 1, 128, 64, 48)
    # the parent index and the see-through view are built from the empty world, then the chunks arrive
    empty_records = W.draw(cam, see_through=6, kernel=svo.KERNEL_STACK)
    assert not np.any(empty_records["flags"] & 1)
    assert not np.any(W.hit_boxes(empty_records)["flags"])
    W.set_chunk_grid(0, G.grids()["g5"])
    W.set_chunk_grid(1, G.grids()["g6"])
    O = oracle.OracleWorld.from_chunks([svo.see_through_chunk(c, 6) for c in two_chunks], 2, 1, 1, 128)
    want = O.trace_image(cam, params=oracle.make_params())
    assert int((want["flags"] & 1).sum()) > 50
    for kernel in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
        assert_gbuffer_equal(W.draw(cam, see_through=6, kernel=kernel), want, f"see-through after from_grid / kernel {kernel}")
    records = W.draw(cam, kernel=svo.KERNEL_STACK)
    boxes = W.hit_boxes(records)
    model = HV.hit_voxels(two_chunks, records.reshape(-1))
    assert np.array_equal(boxes.view(np.uint8), model.view(np.uint8)) and int((boxes["flags"] & 1).sum()) > 50
    located = W.locate_points(leaf_centres(5))
    assert np.array_equal(located["material"].reshape(32, 32, 32), G.grids()["g5"])
    W.destroy()


def test_a_replaced_chunk_is_edited_compacted_and_coarsened(svo):
    """The same DESTROY box on the chunk built from G5 and on a world created from the model's pools of G5: equal pools; the edited
    grid is G5 with the box's voxels emptied; compact and coarsen then equal the model's (tests/lod_model.py) on those pools."""
    W = empty_world(svo, [2], (1, 1, 1))
    W.set_chunk_grid(0, G.grids()["g5"])
    R = svo.World.create([G.model_chunk("g5")], 1, 1, 1, 128).upload(0)
    lo, hi = (22.0, 10.0, 30.0), (90.0, 70.0, 101.0)       # off the 4-unit voxel lattice: voxels floor(lo / 4) .. floor(hi / 4) touch the box
    for world in (W, R):
        assert world.edit_box(0, svo.EDIT_DESTROY, lo, hi) == svo.SVO_OK
    edited = R.chunk(0)
    same_pools(W.chunk(0), edited, "DESTROY after from_grid")
    g = G.grids()["g5"].copy()
    g[30 // 4:101 // 4 + 1, 10 // 4:70 // 4 + 1, 22 // 4:90 // 4 + 1] = 0
    assert (g != G.grids()["g5"]).sum() > 100
    assert np.array_equal(W.chunk_grid(0, 5), g) and np.array_equal(G.pools_to_grid(edited, 5), g)
    assert W.compact(0) == svo.SVO_OK
    compacted = M.compact(edited)
    same_pools(W.chunk(0), compacted, "compact after from_grid + edit")
    assert np.array_equal(W.chunk_grid(0, 5), g)
    assert W.coarsen(0) == svo.SVO_OK
    same_pools(W.chunk(0), M.coarsen(compacted, full=False), "coarsen after from_grid + edit + compact")
    assert W.info.max_chunk_depth == 4
    W.destroy(); R.destroy()


def test_one_world_through_every_builder_in_turn(svo):
    """The builders share a world's scratch: the terrain grower and the grid walk the same level arrays, compact / coarsen and the grid
    keep arrays of their own beside them, every one of them writes the edits' pools.  One 2x1x1 world of depth 5, generated on the
    device with water (the grower and the filler have run), takes eight steps that hand those arrays from one builder to the next - to a
    deeper grid after compact, back to the terrain, then to a shallower grid; after each the chunks equal, index for index, what the
    models give for that step alone, and at the end both kernels march the same frame."""
    import ball_model as B
    W = svo.World.generate(2, 1, 1, 128, 5, build_device=0)
    fresh = {x: svo.World.generate(2, 1, 1, 128, 5, chunkcoordmin=(x, 0, 0)) for x in (0, 1)}      # host-generated: what a shift must leave

    def terrain(x, what):
        assert tuple(W.info.chunkcoordmin) == (x, 0, 0), what
        for i in range(2):
            assert W.chunk(i)["position"] == fresh[x].chunk(i)["position"], f"{what}: chunk {i}"
            same_pools(W.chunk(i), fresh[x].chunk(i), f"{what}: chunk {i}")

    def at(i, chunk):
        return dict(chunk, position=W.chunk(i)["position"])

    assert W.shift((1, 0, 0)) == svo.SVO_OK
    terrain(1, "1 shift +x")
    assert W.chunk(0)["position"] == (256.0, 0.0, 0.0)
    assert W.set_chunk_grid(0, G.grids()["g5"]) == svo.SVO_OK
    same_pools(W.chunk(0), G.model_chunk("g5"), "2 grid g5")
    centre, radius = (256.0 + 70.5, 40.0, 61.0), 37.3
    assert W.edit_ball(0, svo.EDIT_DESTROY, centre, radius) == svo.SVO_OK
    carved = B.pools_of(B.edit(B.chunk_of(at(0, G.model_chunk("g5"))), svo.EDIT_DESTROY, B.Ball(centre, radius)))
    assert carved["tree"].size > G.model_chunk("g5")["tree"].size          # the ball split nodes
    same_pools(W.chunk(0), carved, "3 ball")
    assert W.compact(0) == svo.SVO_OK
    same_pools(W.chunk(0), M.compact(carved), "4 compact")
    assert W.set_chunk_grid(0, G.grids()["g6"]) == svo.SVO_OK
    same_pools(W.chunk(0), G.model_chunk("g6"), "5 grid g6 after compact")
    assert W.coarsen(0) == svo.SVO_OK
    same_pools(W.chunk(0), M.coarsen(G.model_chunk("g6"), full=False), "6 coarsen")
    same_pools(W.chunk(1), fresh[1].chunk(1), "6 coarsen: the chunk beside it")
    assert W.shift((-1, 0, 0)) == svo.SVO_OK
    terrain(0, "7 shift -x after the grid")
    assert W.set_chunk_grid(1, G.grids()["g3"]) == svo.SVO_OK
    same_pools(W.chunk(1), G.model_chunk("g3"), "8 grid g3")
    same_pools(W.chunk(0), fresh[0].chunk(0), "8 grid g3: the chunk beside it")
    cam = svo.default_camera(2, 1, 128, 64, 48)
    frame = W.draw(cam, shadow=True, kernel=svo.KERNEL_STACK)
    assert int((frame["flags"] & 1).sum()) > 200
    assert_gbuffer_equal(W.draw(cam, shadow=True, kernel=svo.KERNEL_LITERAL), frame, "the frame at the end, literal against stack")
    W.destroy()
    for F in fresh.values():
        F.destroy()


def test_refused_calls_change_nothing(svo):
    H = svo.World.create([G.model_chunk("g3")], 1, 1, 1, 128)
    buf = svo.DeviceBuffer(8 ** 3 * 2)
    for call in (lambda: H.chunk_from_grid(0, buf.ptr, 3), lambda: H.chunk_to_grid(0, 3, buf.ptr)):
        with pytest.raises(svo.SvoError) as e:
            call()
        assert e.value.code == -5                                       # SVO_ERR_NOT_UPLOADED on a host-only world
    H.upload(0)
    big = svo.DeviceBuffer.from_numpy(G.grids()["g5"])
    for chunk, depth in ((1, 5), (-1, 5), (0, 1), (0, 11)):
        with pytest.raises(svo.SvoError) as e:
            H.chunk_from_grid(chunk, big.ptr, depth)
        assert e.value.code == -1
        with pytest.raises(svo.SvoError) as e:
            H.chunk_to_grid(chunk, depth, big.ptr)
        assert e.value.code == -1
        same_pools(H.chunk(0), G.model_chunk("g3"), "after a refused call")
    assert np.array_equal(H.chunk_grid(0, 3), G.grids()["g3"])
    buf.free(); big.free()
    H.destroy()
