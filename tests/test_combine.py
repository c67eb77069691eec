"""svo_world_chunk_combine (csrc/combine.hip) on the GPU: the pools the device installs, read back with World.chunk, and the count equal
the host form's (csrc/combine.cpp, which tests/test_combine_cpu.py holds against the dense model) index for index - exact equality
everywhere; then what the feature exists for: a mesh put into a terrain chunk and carved out of it, equal to the dense grid route; what
follows the install: svo_world_info, the other chunk, both march kernels; the three places B can live in; depth 12 and 16.  The shapes are
the smallest at which the kernels can still go wrong: depth 2 (the roots a pair of TWIGs), every pairing of node types, results that fold
to one word and results larger than either input, level lists beyond one block and brick candidates across a block border at depth 7."""
import ctypes as C

import numpy as np
import pytest

import combine_model as K
import grid_model as G
import mesh_model as M
import sparse_fill_model as F
import sparse_mesh_model as S
from helpers import assert_gbuffer_equal
from test_combine_cpu import deep_cubes, filled_sphere12
from test_compact_model import same_pools
from test_sparse_fill import check_after, device, put, world      # noqa: F401  (device and world are fixtures)
from test_sparse_mesh import device_build, empty_chunk

pytestmark = pytest.mark.gpu
OPS = list(K.OPS.items())


@pytest.fixture(scope="module")
def model(svo):
    """A one-chunk world on the same device: where B lives when it is a model of its own."""
    MW = svo.World.create([empty_chunk()], 1, 1, 1, 128).upload(0)
    yield MW
    MW.destroy()


def place(W, i, chunk):
    """The host pools of `chunk` become chunk i of the uploaded world, at that chunk's place."""
    W.update(i, dict(chunk, position=(128.0 * i, 0.0, 0.0), size=128.0), (0, chunk["tree"].size), (0, chunk["twig"].size // 64), True)


def combine_and_check(svo, W, other, MW, a, b, what, ops=OPS):
    """Every op of `ops` on (a, b), B in the model world: pools, count, the sentinel chunk, svo_world_info and B after each call."""
    place(MW, 0, b)
    for opname, op in ops:
        want, changed = svo.chunk_combine(a, b, op)
        put(W, a)
        count = W.chunk_combine(0, MW, 0, op)
        print(what, opname, "changed", count, "host form", changed, "node words", want["tree"].size, "bricks", want["twig"].size // 64)
        assert W.combine_status == svo.SVO_OK and count == changed
        check_after(W, other, want, f"{what}, {opname}")
        same_pools(MW.chunk(0), b, f"{what}, {opname}: B")


@pytest.mark.parametrize("name", list(K.pairs()))
def test_device_pools_and_count_equal_the_host_form(svo, world, model, name):
    W, other = world
    a, b = K.pairs()[name]
    combine_and_check(svo, W, other, model, a, b, name)


def test_depth_7_lists_beyond_one_block(svo, world, model):
    W, other = world
    a, b = K.depth7_pair()
    assert a["tree"].size > 8 * 256 and b["tree"].size > 8 * 256 and min(a["twig"].size, b["twig"].size) // 64 > 1024
    combine_and_check(svo, W, other, model, a, b, "depth 7")
    combine_and_check(svo, W, other, model, b, a, "depth 7, swapped", ops=[("max", K.MAX), ("subtract", K.SUBTRACT)])


@pytest.mark.parametrize("name", ["g5_shell", "two_spheres", "untidy_empty", "pairings"])
def test_the_three_places_b_can_live_in_give_the_same_pools(svo, world, model, name):
    W, other = world
    a, b = K.pairs()[name]
    for opname, op in OPS:
        want, changed = svo.chunk_combine(a, b, op)
        put(W, a); place(model, 0, b)                       # B in the model world
        assert W.chunk_combine(0, model, 0, op) == changed
        same_pools(W.chunk(0), want, f"{name}, {opname}: B in the model world")
        same_pools(model.chunk(0), b, "B")
        put(W, a); place(W, 1, b)                           # B as chunk 1 of the same world
        assert W.chunk_combine(0, W, 1, op) == changed
        same_pools(W.chunk(0), want, f"{name}, {opname}: B in the same world")
        same_pools(W.chunk(1), b, "B")
        info = W.info
        assert info.total_trees == want["tree"].size + b["tree"].size and info.total_twigs == (want["twig"].size + b["twig"].size) // 64
        self_want, self_changed = svo.chunk_combine(b, b, op)
        assert W.chunk_combine(1, W, 1, op) == self_changed     # src_chunk == chunk: A = B, read completely before it is replaced
        same_pools(W.chunk(1), self_want, f"{name}, {opname}: B with itself")
        same_pools(W.chunk(0), want, f"{name}, {opname}: the other chunk")
    place(W, 1, other)
    same_pools(W.chunk(1), other, "the sentinel chunk, put back")


def test_two_max_calls_with_two_shells_give_the_two_mesh_chunk(svo, world, model):
    W, other = world
    depth, meshes = S.shared_cases()["two_meshes"]
    put(W, K.one_word(depth, 0))
    for m in meshes:
        assert device_build(svo, model, 0, [m], depth) == svo.SVO_OK
        assert W.chunk_combine(0, model, 0, K.MAX) > 0
    check_after(W, other, svo.chunk_from_mesh(meshes, depth), "MAX of two meshes' shells")
    assert device_build(svo, model, 0, meshes, depth) == svo.SVO_OK
    same_pools(W.chunk(0), model.chunk(0), "... against svo_world_chunk_from_mesh of the two-mesh list")


# ---- the composition the feature exists for, at depth 6 ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def terrain6():
    return F.freeze(G.chunk_of(G.heightfield(6)))


@pytest.fixture(scope="module")
def sphere6():
    v, ix = M.sphere_case(6)
    return [S.mesh(v, ix, material=5)]


def test_a_mesh_added_into_a_terrain_chunk_equals_the_dense_route(svo, world, model, terrain6, sphere6):
    W, other = world
    put(W, terrain6)
    assert device_build(svo, model, 0, sphere6, 6) == svo.SVO_OK
    shell = model.chunk(0)
    changed = W.chunk_combine(0, model, 0, K.MAX)
    # the dense route: to-grid, the mesh rasterised into that grid, from-grid
    dense = svo.World.create([empty_chunk(), other], 2, 1, 1, 128).upload(0)
    put(dense, terrain6)
    v, ix = np.ascontiguousarray(sphere6[0]["vertices"], np.float32), np.ascontiguousarray(sphere6[0]["indices"], np.uint32)
    grid, vd, id_ = svo.DeviceBuffer(64 ** 3 * 2), svo.DeviceBuffer.from_numpy(v), svo.DeviceBuffer.from_numpy(ix)
    dense.chunk_to_grid(0, 6, grid.ptr)
    before = grid.to_numpy(np.uint16, 64 ** 3)
    svo.device_grid_add_mesh(grid.ptr, 6, vd.ptr, v.shape[0], id_.ptr, ix.shape[0], material=5)
    assert changed == int((grid.to_numpy(np.uint16, 64 ** 3) != before).sum()) > 1000
    dense.chunk_from_grid(0, grid.ptr, 6)
    same_pools(W.chunk(0), dense.chunk(0), "mesh MAX terrain against to-grid, add-mesh, from-grid")
    same_pools(model.chunk(0), shell, "the model")
    check_after(W, other, svo.chunk_combine(terrain6, shell, K.MAX)[0], "mesh MAX terrain")
    # the solid carved out of the terrain
    filled = model.chunk_fill_enclosed(0, 9)
    assert filled > 40000
    put(W, terrain6)
    changed = W.chunk_combine(0, model, 0, K.SUBTRACT)
    model.chunk_to_grid(0, 6, grid.ptr)
    gb = grid.to_numpy(np.uint16, 64 ** 3)
    g = K.f(K.SUBTRACT, before, gb).astype(np.uint16)
    assert changed == int((g != before).sum()) > 1000
    assert dense.set_chunk_grid(0, g.reshape(64, 64, 64)) == svo.SVO_OK
    same_pools(W.chunk(0), dense.chunk(0), "terrain SUBTRACT solid against the dense grid route")
    for b in (grid, vd, id_):
        b.free()
    dense.destroy()


@pytest.fixture(scope="module")
def carved6(svo, terrain6, sphere6):
    """The host form's composition: the filled sphere, and the terrain with it carved out."""
    solid = svo.chunk_fill_enclosed(svo.chunk_from_mesh(sphere6, 6), 9)[0]
    return F.freeze(solid), F.freeze(svo.chunk_combine(terrain6, solid, K.SUBTRACT)[0])


def test_the_march_equals_the_oracle_over_the_host_forms_pools(svo, oracle, world, model, terrain6, carved6):
    W, other = world
    solid, carved = carved6
    put(W, terrain6); place(model, 0, solid)
    assert W.chunk_combine(0, model, 0, K.SUBTRACT) > 1000
    O = oracle.OracleWorld.from_chunks([carved, other], 2, 1, 1, 128)
    cam = svo.make_camera((150.0, 140.0, -90.0), (-0.35, -0.3, 0.88), (0.0, 1.0, 0.0), 60.0, 64, 48)
    for semantics in (0, 1):
        want = O.trace_image(cam, params=oracle.make_params(shadow=True, semantics=semantics))
        assert int((want["flags"] & 1).sum()) > 200
        for kernel in (svo.KERNEL_LITERAL, svo.KERNEL_STACK):
            assert_gbuffer_equal(W.draw(cam, shadow=True, kernel=kernel, semantics=semantics), want, f"semantics {semantics} / kernel {kernel}")


def test_a_ray_into_the_carved_hollow_flies_through_to_what_lies_behind(svo, world, model, terrain6, carved6):
    """Straight down the voxel column (32, ., 32) (a cell is 2 world units): before the call the ray stops on the terrain's top, after it
    on the first voxel below the hollow - both read off the dense grids."""
    W, other = world
    solid, carved = carved6
    column = lambda chunk: G.pools_to_grid(chunk, 6)[32, :, 32]
    tops = [int(np.nonzero(column(c))[0].max()) for c in (terrain6, carved)]
    assert tops[1] < tops[0] - 5
    o, d = np.array([[65.0, 200.0, 65.0]], np.float32), np.array([[0.0, -1.0, 0.0]], np.float32)
    put(W, terrain6); place(model, 0, solid)
    for k, chunk in enumerate((terrain6, carved)):
        if k == 1:
            assert W.chunk_combine(0, model, 0, K.SUBTRACT) > 1000
        for kernel in (svo.KERNEL_LITERAL, svo.KERNEL_STACK):
            hit = W.chunkmarch(o, d, kernel=kernel)
            assert int(hit["flags"][0]) & 1 and int(hit["material"][0]) == int(column(chunk)[tops[k]])
            assert abs(float(hit["t"][0]) - (200.0 - 2.0 * (tops[k] + 1))) < 0.01, (k, kernel, float(hit["t"][0]))


# ---- depth 12 and 16 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [12, 16])
def test_deep_cubes_built_on_the_device_equal_the_host_form(svo, world, model, depth):
    W, other = world
    a, b, c = deep_cubes(svo, depth)
    ma, mb, _ = K.cube_meshes(depth)
    assert device_build(svo, model, 0, mb, depth) == svo.SVO_OK and model.chunk_fill_enclosed(0, K.MATERIAL_B) == F.CUBE_FILLED
    same_pools(model.chunk(0), b, "cube B, built on the device")
    for opname, op in OPS:
        want, changed = svo.chunk_combine(a, b, op)
        if op == K.MAX:
            assert device_build(svo, W, 0, ma, depth) == svo.SVO_OK and W.chunk_fill_enclosed(0, K.MATERIAL_A) == F.CUBE_FILLED
            same_pools(W.chunk(0), a, "cube A, built on the device")
        else:
            put(W, a)
        count = W.chunk_combine(0, model, 0, op)
        print(f"depth {depth}, {opname}: changed {count}, {want['tree'].size} node words, {want['twig'].size // 64} bricks")
        assert count == changed == K.CUBE_CHANGED[op]
        check_after(W, other, want, f"depth {depth}, {opname}")         # MAX grows beyond A: svo_world_info still adds up
        same_pools(model.chunk(0), b, "cube B")
    assert svo.chunk_combine(a, b, K.MAX)[0]["tree"].size > a["tree"].size


def test_both_march_kernels_agree_at_depth_12_on_the_cube_minus_the_sphere(svo, world, model):
    W, other = world
    a, _, c = deep_cubes(svo, 12)
    ball = filled_sphere12(svo)
    want, changed = svo.chunk_combine(a, ball, K.SUBTRACT)
    put(W, a); place(model, 0, ball)
    assert W.chunk_combine(0, model, 0, K.SUBTRACT) == changed > 40000
    check_after(W, other, want, "cube12 minus sphere12")
    # the sphere leaves the cube through its high z face (cell c + 257): the camera looks at the hole from outside
    (corner, shape), = S.deep_cases()["sphere12"][2]
    hole = np.array([corner[0] + 28.0, corner[1] + 28.0, c + 257.0]) * (128.0 / 4096.0)
    cam = svo.make_camera(tuple(hole + np.array([0.6, 0.5, 1.6])), (-0.3, -0.25, -0.9), (0.0, 1.0, 0.0), 50.0, 64, 64)
    stack = W.draw(cam, shadow=True, kernel=svo.KERNEL_STACK)
    assert int((stack["flags"] & 1).sum()) > 200 and K.MATERIAL_A in set(np.unique(stack["material"][(stack["flags"] & 1) != 0]).tolist())
    assert_gbuffer_equal(W.draw(cam, shadow=True, kernel=svo.KERNEL_LITERAL), stack, "literal against stack at depth 12")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_both_chunks_as_they_were(svo, world, model):
    W, other = world
    a, b = K.pairs()["g5_shell"]
    put(W, a); place(model, 0, b)

    def unchanged(what, a=a, b=b):
        check_after(W, other, a, what)
        same_pools(model.chunk(0), b, what + ": B")

    call = lambda chunk=0, src=model._h, src_chunk=0, op=0, w=W._h: svo.lib.svo_world_chunk_combine(w, chunk, src, src_chunk, op, None)
    assert [call(w=None), call(src=None), call(chunk=-1), call(chunk=2), call(src_chunk=-1), call(src_chunk=1), call(op=-1), call(op=5)] == [-1] * 8
    unchanged("after the argument errors")
    host_only = svo.World.create([b], 1, 1, 1, 128)         # a model world that is not uploaded
    changed = C.c_uint64(77)
    assert svo.lib.svo_world_chunk_combine(W._h, 0, host_only._h, 0, 0, C.byref(changed)) == -5 and changed.value == 77
    assert svo.lib.svo_world_chunk_combine(host_only._h, 0, W._h, 0, 0, C.byref(changed)) == -5 and changed.value == 77
    assert svo.lib.svo_world_chunk_combine(host_only._h, 0, W._h, 0, 9, None) == -1         # the argument errors come first
    same_pools(host_only.chunk(0), b, "the host-only world")
    host_only.destroy()
    unchanged("after the world that is not uploaded")
    deeper = K.pairs()["two_spheres"][1]                    # depths that differ: 5 against 6, and against the sentinel's 4
    place(model, 0, deeper)
    assert svo.lib.svo_world_chunk_combine(W._h, 0, model._h, 0, 0, C.byref(changed)) == -6 and changed.value == 77
    assert call(src=W._h, src_chunk=1) == -6 and svo.lib.svo_world_chunk_combine(model._h, 0, W._h, 0, 0, None) == -6
    unchanged("after the depths that differ", b=deeper)
    shallow = dict(position=(0.0, 0.0, 0.0), size=128.0, depth=5, tree=np.array([G.node(G.TWIG, 0)], np.uint32), twig=b["twig"][:64].copy())
    place(model, 0, shallow)                                # a brick above level depth-2, as B and as A
    assert svo.lib.svo_world_chunk_combine(W._h, 0, model._h, 0, 0, C.byref(changed)) == -6 and changed.value == 77
    unchanged("after the refused sparsely refined B", b=shallow)
    assert svo.lib.svo_world_chunk_combine(model._h, 0, W._h, 0, 0, C.byref(changed)) == -6 and changed.value == 77
    unchanged("after the refused sparsely refined A", b=shallow)
    place(model, 0, b)
    assert W.chunk_combine(0, model, 0, K.MAX) == svo.chunk_combine(a, b, K.MAX)[1]         # and the worlds still work
    check_after(W, other, svo.chunk_combine(a, b, K.MAX)[0], "after the refusals")
