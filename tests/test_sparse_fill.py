"""svo_world_chunk_fill_enclosed (csrc/sparse_fill.hip) on the GPU: the pools the device installs, read back with World.chunk, and
the count equal the host form's (csrc/sparse_fill.cpp, which tests/test_sparse_fill_cpu.py holds against the model) index for index
- exact equality everywhere; then what follows the install: svo_world_info, the other chunk, both march kernels, an edit that cuts
the solid open, one svo_trace_instances placement.  The shapes are the smallest at which the kernels can still go wrong: depth 2 (the
root a TWIG), corridors one cell wide that need hundreds of sweeps and cross block borders, EMPTY nodes of every size beside bricks,
pools that are not minimal, depth 16's 16-bit corners."""
import ctypes as C

import numpy as np
import pytest

import grid_model as G
import instances_model as IM
import mesh_model as M
import sparse_fill_model as F
import sparse_mesh_model as S
from helpers import assert_gbuffer_equal
from test_compact_model import same_pools
from test_sparse_mesh import device_build, empty_chunk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device(svo):
    if svo.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")


@pytest.fixture(scope="module")
def world(svo):
    """Two chunks side by side: chunk 0 is filled by the tests, chunk 1 (the sentinel) holds the hollow depth-4 sphere and stays."""
    other = dict(S.case_pools("sphere4"), position=(128.0, 0.0, 0.0))
    W = svo.World.create([empty_chunk(), other], 2, 1, 1, 128).upload(0)
    yield W, other
    W.destroy()


def put(W, chunk):
    """The host pools of `chunk` become chunk 0 of the uploaded world."""
    W.update(0, dict(chunk, position=(0.0, 0.0, 0.0), size=128.0), (0, chunk["tree"].size), (0, chunk["twig"].size // 64), True)


def check_after(W, other, want, what):
    same_pools(W.chunk(0), want, what)
    same_pools(W.chunk(1), other, what + ": the other chunk")
    info = W.info
    assert info.total_trees == want["tree"].size + other["tree"].size and info.total_twigs == (want["twig"].size + other["twig"].size) // 64
    assert info.max_chunk_depth == max(int(want["depth"]), int(other["depth"]))


SERPENTINES7 = [f"serpentine7_{a}_{s}" for a in "xyz" for s in ("open", "sealed")]


@pytest.mark.parametrize("name", list(F.grid_cases()) + SERPENTINES7)
def test_device_pools_and_count_equal_the_host_form(svo, world, name):
    W, other = world
    chunk, material = F.case_chunk(name)
    want, filled = svo.chunk_fill_enclosed(chunk, material)
    put(W, chunk)
    count = W.chunk_fill_enclosed(0, material)
    print(name, "filled", count, "host form", filled)
    assert W.fill_status == svo.SVO_OK and count == filled
    if name.endswith("_sealed"):
        assert filled == F.SERPENTINE_CELLS
    check_after(W, other, want, name)
    assert W.chunk_fill_enclosed(0, material) == 0          # a second fill finds nothing and installs the same pools
    check_after(W, other, want, name + ", filled twice")


@pytest.mark.parametrize("name", ["sphere5", "torus5", "two_meshes"])
def test_mesh_then_fill_on_the_device_equals_the_host_composition(svo, world, name):
    W, other = world
    depth, meshes = S.shared_cases()[name]
    want, filled = svo.chunk_fill_enclosed(svo.chunk_from_mesh(meshes, depth), 11)
    assert filled > 0 and device_build(svo, W, 0, meshes, depth) == svo.SVO_OK
    assert W.chunk_fill_enclosed(0, 11) == filled
    check_after(W, other, want, name)


def test_pools_that_are_not_minimal_come_back_minimal_and_in_fifo_order(svo, world):
    W, other = world
    chunk, material = F.untidy_chunk()
    for m in (material, 0xFFFF):
        want, filled = svo.chunk_fill_enclosed(chunk, m)
        put(W, chunk)
        assert W.chunk_fill_enclosed(0, m) == filled == 8
        check_after(W, other, want, f"untidy pool, material {m}")
        assert G.is_minimal(W.chunk(0))


@pytest.mark.parametrize("name", ["sphere12", "sphere16", "cube12", "cube16"])
def test_depth_12_and_16_equal_the_host_form(svo, world, name):
    W, other = world
    depth, meshes = (S.deep_cases()[name][:2] if name.startswith("sphere") else F.deep_cubes()[name][:2])
    want, filled = svo.chunk_fill_enclosed(svo.chunk_from_mesh(meshes, depth), 2)
    assert filled > 20000 and (not name.startswith("cube") or filled == F.CUBE_FILLED)
    assert device_build(svo, W, 0, meshes, depth) == svo.SVO_OK
    before = W.chunk(0)
    count = W.chunk_fill_enclosed(0, 2)
    print(name, "filled", count, "host form", filled)
    assert count == filled
    check_after(W, other, want, name)
    assert want["tree"].size <= before["tree"].size and want["twig"].size <= before["twig"].size


def test_both_march_kernels_agree_at_depth_12_on_the_filled_cube(svo, world):
    W, other = world
    depth, meshes, corner = F.deep_cubes()["cube12"]
    assert device_build(svo, W, 0, meshes, depth) == svo.SVO_OK and W.chunk_fill_enclosed(0, 2) == F.CUBE_FILLED
    centre = (corner + 128.0) * (128.0 / 4096.0)            # of the cube, in world units; its edge is 8
    cam = svo.make_camera((centre - 7.0, centre + 9.0, centre - 16.0), (0.35, -0.45, 0.8), (0.0, 1.0, 0.0), 50.0, 64, 64)
    stack = W.draw(cam, shadow=True, kernel=svo.KERNEL_STACK)
    assert int((stack["flags"] & 1).sum()) > 200 and set(np.unique(stack["material"][(stack["flags"] & 1) != 0])) == {6}
    assert_gbuffer_equal(W.draw(cam, shadow=True, kernel=svo.KERNEL_LITERAL), stack, "literal against stack at depth 12")


@pytest.fixture(scope="module")
def sphere6(svo):
    """The depth-6 sphere: its mesh, and the host form's filled pools."""
    v, ix = M.sphere_case(6)
    meshes = [S.mesh(v, ix, material=5)]
    solid, filled = svo.chunk_fill_enclosed(svo.chunk_from_mesh(meshes, 6), 9)
    assert filled > 40000
    return meshes, F.freeze(solid), filled


def test_the_march_equals_the_oracle_over_the_host_forms_pools(svo, oracle, world, sphere6):
    W, other = world
    meshes, solid, filled = sphere6
    assert device_build(svo, W, 0, meshes, 6) == svo.SVO_OK and W.chunk_fill_enclosed(0, 9) == filled
    O = oracle.OracleWorld.from_chunks([solid, other], 2, 1, 1, 128)
    cam = svo.make_camera((150.0, 140.0, -90.0), (-0.35, -0.3, 0.88), (0.0, 1.0, 0.0), 60.0, 64, 48)
    for semantics in (0, 1):
        want = O.trace_image(cam, params=oracle.make_params(shadow=True, semantics=semantics))
        assert int((want["flags"] & 1).sum()) > 200
        for kernel in (svo.KERNEL_LITERAL, svo.KERNEL_STACK):
            assert_gbuffer_equal(W.draw(cam, shadow=True, kernel=kernel, semantics=semantics), want, f"semantics {semantics} / kernel {kernel}")


def test_an_edit_that_cuts_the_filled_sphere_open_finds_material(svo, world, sphere6):
    """The point of the feature: mesh -> fill -> a ball carved through the centre.  The pools equal, index for index, the same ball
    carved out of the dense path's solid, and a ray into the cut ends on the fill's material."""
    W, other = world
    meshes, solid, filled = sphere6
    assert device_build(svo, W, 0, meshes, 6) == svo.SVO_OK and W.chunk_fill_enclosed(0, 9) == filled
    g = S.zeros(6)
    svo.grid_add_mesh(g, meshes[0]["vertices"], meshes[0]["indices"], material=5)
    assert svo.grid_fill_enclosed(g, 9) == filled
    dense = svo.World.create([empty_chunk(), other], 2, 1, 1, 128).upload(0)
    assert dense.set_chunk_grid(0, g) == svo.SVO_OK
    same_pools(W.chunk(0), dense.chunk(0), "sparse against dense, before the cut")
    centre, radius = (64.0, 64.0, 20.0), 45.0               # world units (a cell is 2): from the sphere's front through its centre
    for world_ in (W, dense):
        assert world_.edit_ball(0, svo.EDIT_DESTROY, centre, radius) == svo.SVO_OK
    same_pools(W.chunk(0), dense.chunk(0), "sparse against dense, after the cut")
    o, d = np.array([[64.5, 64.5, -40.0]], np.float32), np.array([[0.0, 0.0, 1.0]], np.float32)
    for kernel in (svo.KERNEL_LITERAL, svo.KERNEL_STACK):
        hit = W.chunkmarch(o, d, kernel=kernel)
        assert int(hit["flags"][0]) & 1 and int(hit["material"][0]) == 9 and 100.0 < float(hit["t"][0]) < 110.0
        assert_gbuffer_equal(hit, dense.chunkmarch(o, d, kernel=kernel), f"the ray into the cut, kernel {kernel}")
    dense.destroy()
    hollow = svo.World.create([empty_chunk(), other], 2, 1, 1, 128).upload(0)      # without the fill the same ray flies on to the far shell
    assert device_build(svo, hollow, 0, meshes, 6) == svo.SVO_OK and hollow.edit_ball(0, svo.EDIT_DESTROY, centre, radius) == svo.SVO_OK
    far = hollow.chunkmarch(o, d, kernel=svo.KERNEL_LITERAL)
    assert int(far["material"][0]) == 5 and float(far["t"][0]) > 140.0
    hollow.destroy()


def test_one_instance_placement_of_a_filled_model(svo):
    from test_instances import assert_records, assert_words, stage1
    scene = svo.World.generate(2, 1, 2, 128, 6).upload(0)
    cam = svo.default_camera(2, 2, 128, 64, 48)
    rect, inst = (0, 0, 64, 48), [IM.instance((94.0, 84.0, 4.0))]
    model = lambda: svo.World.create([empty_chunk(size=IM.MODEL_SIZE)], 1, 1, 1, IM.MODEL_SIZE).upload(0)
    depth, v, ix, _ = M.cases()["sphere5"]
    sparse, dense = model(), model()
    assert device_build(svo, sparse, 0, [S.mesh(v, ix, material=5)], depth) == svo.SVO_OK and sparse.chunk_fill_enclosed(0, 9) > 0
    g = M.add_mesh(S.zeros(depth), v, ix, material=5)
    M.fill_enclosed(g, 9)
    assert dense.set_chunk_grid(0, g) == svo.SVO_OK
    same_pools(sparse.chunk(0), dense.chunk(0), "the model's pools")
    for kernel in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
        prm = svo.trace_params(shadow=True, kernel=kernel)
        want = stage1(svo, dict(W=scene, Mw=dense, cam=cam, inst=inst), prm, rect=rect, max_rays=64 * 48)
        got = stage1(svo, dict(W=scene, Mw=sparse, cam=cam, inst=inst), prm, rect=rect, max_rays=64 * 48)
        assert want["counts"][0] > 50 and got["counts"] == want["counts"]
        assert_words(got["owner"], want["owner"], f"owner, kernel {kernel}")
        assert_records(got["merged"], want["merged"], f"merged, kernel {kernel}")
    for w in (sparse, dense, scene):
        w.destroy()


def test_refusals_leave_the_pools_as_they_were(svo, world):
    W, other = world
    chunk, material = F.case_chunk("shell")
    put(W, chunk)
    call = lambda chunk=0, material=material, w=W._h: svo.lib.svo_world_chunk_fill_enclosed(w, chunk, material, None)
    assert [call(w=None), call(chunk=-1), call(chunk=2), call(material=0)] == [-1] * 4
    check_after(W, other, chunk, "after the argument errors")
    shallow = dict(position=(0.0, 0.0, 0.0), size=128.0, depth=3, tree=np.array([G.node(G.TWIG, 0)], np.uint32), twig=chunk["twig"][:64].copy())
    put(W, shallow)                                         # a brick above level depth-2: SVO_ERR_UNSUPPORTED, nothing changes
    filled = C.c_uint64(77)
    assert svo.lib.svo_world_chunk_fill_enclosed(W._h, 0, material, C.byref(filled)) == -6 and filled.value == 77
    check_after(W, other, shallow, "after the refused sparsely refined chunk")
    host_only = svo.World.create([chunk], 1, 1, 1, 128)
    assert svo.lib.svo_world_chunk_fill_enclosed(host_only._h, 0, material, None) == -5
    host_only.destroy()
    put(W, chunk)
    assert W.chunk_fill_enclosed(0, material) == F.case_model("shell")[1]       # and the world still works
