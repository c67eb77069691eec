"""svo_world_chunk_from_mesh (csrc/sparse_mesh.hip) on the GPU: the pools the device installs, read back with World.chunk, equal the
host form's (csrc/sparse_mesh.cpp, which tests/test_sparse_mesh_cpu.py holds against the model) index for index - exact equality
everywhere - with the meshes' arrays untouched; then what follows the install: svo_world_info, the other chunk, both march kernels at
depth 12, the dense path's records at depth 6, one svo_trace_instances placement.  The shapes are the smallest at which the kernels
can still go wrong: triangle counts around the 64 lanes of a wave and the 256 threads of a block, depth 2 (one tile, the root a
TWIG), a triangle that is thousands of tile jobs beside hundreds that are one, 64 duplicates per cell, depth 16's 64-bit words."""
import ctypes as C

import numpy as np
import pytest

import grid_model as G
import instances_model as IM
import mesh_model as M
import sparse_mesh_model as S
from helpers import assert_gbuffer_equal
from test_compact_model import same_pools

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device(svo):
    if svo.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")


def device_build(svo, W, chunk, meshes, depth):
    """svo_world_chunk_from_mesh of host arrays: uploads them, checks that the call left them alone, returns the status."""
    bufs, structs, host = [], [], []
    for m in meshes:
        v = np.ascontiguousarray(m["vertices"], np.float32).reshape(-1, 3)
        ix = np.ascontiguousarray(m["indices"], np.uint32).reshape(-1, 3)
        mats = None if m.get("materials") is None else np.ascontiguousarray(m["materials"], np.uint16)
        dev = [svo.DeviceBuffer.from_numpy(a) if a is not None and a.size else None for a in (v, ix, mats)]
        structs.append(svo.Mesh(*[None if b is None else b.ptr for b in dev], v.shape[0], ix.shape[0], m.get("origin", (0.0, 0.0, 0.0)), m.get("cell", 1.0),
                                m.get("material", 1)))
        bufs.append(dev); host.append((v, ix, mats))
    try:
        rc = W.chunk_from_mesh(chunk, structs, depth)
        for dev, arrays in zip(bufs, host):
            for b, a in zip(dev, arrays):
                if b is not None:
                    assert np.array_equal(b.to_numpy(a.dtype, a.size).view(np.uint8), a.reshape(-1).view(np.uint8)), "a mesh array was written"
        return rc
    finally:
        for dev in bufs:
            for b in dev:
                if b is not None:
                    b.free()


def empty_chunk(position=(0.0, 0.0, 0.0), size=128.0):
    return dict(position=position, size=float(size), depth=3, tree=np.zeros(1, np.uint32), twig=np.zeros(0, np.uint16))


@pytest.fixture(scope="module")
def world(svo):
    """Two chunks side by side: chunk 0 is rebuilt by the tests, chunk 1 holds the voxelised depth-4 sphere and stays."""
    other = dict(S.case_pools("sphere4"), position=(128.0, 0.0, 0.0))
    W = svo.World.create([empty_chunk(), other], 2, 1, 1, 128).upload(0)
    yield W, other
    W.destroy()


_host = {}


def host_pools(svo, name, depth, meshes):
    """The host form's pools (computed once per case)."""
    if name not in _host:
        _host[name] = svo.chunk_from_mesh(meshes, depth)
    return _host[name]


def check_info(W, other):
    info, c = W.info, W.chunk(0)
    assert info.total_trees == c["tree"].size + other["tree"].size and info.total_twigs == (c["twig"].size + other["twig"].size) // 64
    assert info.max_chunk_depth == max(int(c["depth"]), int(other["depth"]))


@pytest.mark.parametrize("name", list(S.shared_cases()))
def test_device_pools_equal_the_host_form(svo, world, name):
    W, other = world
    depth, meshes = S.shared_cases()[name]
    want = host_pools(svo, name, depth, meshes)
    assert int(want["tree"][0]) != 0
    assert device_build(svo, W, 0, meshes, depth) == svo.SVO_OK
    same_pools(W.chunk(0), want, name)
    same_pools(W.chunk(0), S.case_pools(name), name + " (the model)")
    same_pools(W.chunk(1), other, "the other chunk")
    check_info(W, other)


@pytest.fixture(scope="module")
def many():
    """257 triangles at depth 5 (tests/test_mesh.py's pattern); the host form's pools of their prefixes are computed on demand."""
    v, ix, m = M.soup(11, 257, 32)
    v[:3] = [[3.3, 4.4, 5.5], [9.1, 6.2, 4.3], [5.7, 11.6, 8.2]]              # the first one inside the grid
    return v, ix, m


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_triangle_counts_around_a_wave_and_a_block(svo, world, many, count):
    W, other = world
    v, ix, m = many
    meshes = [S.mesh(v, ix[:count], materials=m[:count])]
    want = svo.chunk_from_mesh(meshes, 5)
    assert (count == 0) == (want["tree"].tolist() == [0])
    assert device_build(svo, W, 0, meshes, 5) == svo.SVO_OK
    same_pools(W.chunk(0), want, f"{count} triangles")
    if count == 257:                                        # and the order of the triangles does not matter
        order = np.random.default_rng(9).permutation(257)
        assert device_build(svo, W, 0, [S.mesh(v, ix[order], materials=m[order])], 5) == svo.SVO_OK
        same_pools(W.chunk(0), want, "shuffled")
    check_info(W, other)


def test_nothing_to_mark_gives_the_empty_chunk(svo, world):
    W, other = world
    none = S.mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))
    for meshes in ([], [none], [S.dropped_mesh()], [S.mesh(*M.uv_sphere((-40.0, 16.0, 16.0), 10.0))]):
        assert device_build(svo, W, 0, S.shared_cases()["sphere4"][1], 4) == svo.SVO_OK and W.chunk(0)["tree"].size > 1
        assert device_build(svo, W, 0, meshes, 9) == svo.SVO_OK
        c = W.chunk(0)
        assert c["tree"].tolist() == [0] and c["twig"].size == 0 and c["depth"] == 9
        check_info(W, other)
    same_pools(W.chunk(1), other, "the other chunk")


def test_one_huge_triangle_beside_500_tiny_ones_at_depth_7(svo, world):
    """One triangle across the whole grid (its cell box is all 32^3 = 32768 tiles) and 500 triangles smaller than a cell, one tile each
    or a few."""
    W, other = world
    big = np.array([[-5.0, -3.0, -4.0], [140.0, 130.0, 40.0], [20.0, 135.0, 141.0]], np.float32)
    v, ix, m = M.soup(13, 500, 128, small=0.8)
    v, ix = M.concat((big, np.array([(0, 1, 2)], np.uint32)), (v, ix))
    m = np.concatenate([np.array([500], np.uint16), m])
    meshes = [S.mesh(v, ix, materials=m)]
    want = svo.chunk_from_mesh(meshes, 7)
    assert (want["twig"] == 500).sum() > 8000 and ((want["twig"] != 0) & (want["twig"] != 500)).sum() > 300
    assert device_build(svo, W, 0, meshes, 7) == svo.SVO_OK
    same_pools(W.chunk(0), want, "huge + tiny")
    assert device_build(svo, W, 0, [S.mesh(v, ix[::-1], materials=m[::-1])], 7) == svo.SVO_OK
    same_pools(W.chunk(0), want, "the same mesh reversed")


@pytest.mark.parametrize("name", list(S.deep_cases()))
def test_depth_12_and_16_equal_the_host_form(svo, world, name):
    W, other = world
    depth, meshes, _ = S.deep_cases()[name]
    want = host_pools(svo, name, depth, meshes)
    assert want["tree"].size >= 1 + 8 * (depth - 2) and want["twig"].size >= 128
    assert device_build(svo, W, 0, meshes, depth) == svo.SVO_OK
    same_pools(W.chunk(0), want, name)
    same_pools(W.chunk(1), other, "the other chunk")
    check_info(W, other)


def test_both_march_kernels_agree_at_depth_12(svo, world):
    W, other = world
    depth, meshes, wins = S.deep_cases()["sphere12"]
    assert device_build(svo, W, 0, meshes, depth) == svo.SVO_OK and W.info.max_chunk_depth == 12
    corner, shape = wins[0]
    centre = (np.asarray(corner, np.float64) + 28.0) * (128.0 / 4096.0)     # of the sphere, in world units; its radius is 0.75
    cam = svo.make_camera(tuple(centre + np.array([0.4, 0.9, -3.0])), (-0.13, -0.29, 0.95), (0.0, 1.0, 0.0), 40.0, 64, 64)
    stack = W.draw(cam, shadow=True, kernel=svo.KERNEL_STACK)
    assert int((stack["flags"] & 1).sum()) > 200 and set(np.unique(stack["material"][(stack["flags"] & 1) != 0])) == {6}
    assert_gbuffer_equal(W.draw(cam, shadow=True, kernel=svo.KERNEL_LITERAL), stack, "literal against stack at depth 12")


def test_the_records_equal_the_dense_path_at_depth_6(svo, world):
    W, other = world
    v, ix = M.sphere_case(6)
    assert device_build(svo, W, 0, [S.mesh(v, ix, material=5)], 6) == svo.SVO_OK
    sparse = W.chunk(0)
    dense = svo.World.create([empty_chunk(), other], 2, 1, 1, 128).upload(0)
    grid = svo.DeviceBuffer.from_numpy(S.zeros(6))
    bv, bi = svo.DeviceBuffer.from_numpy(v), svo.DeviceBuffer.from_numpy(ix)
    assert svo.device_grid_add_mesh(grid.ptr, 6, bv.ptr, v.shape[0], bi.ptr, ix.shape[0], material=5) == svo.SVO_OK
    assert dense.chunk_from_grid(0, grid.ptr, 6) == svo.SVO_OK
    for b in (grid, bv, bi):
        b.free()
    same_pools(sparse, dense.chunk(0), "sparse against dense pools")
    cam = svo.make_camera((150.0, 140.0, -90.0), (-0.35, -0.3, 0.88), (0.0, 1.0, 0.0), 60.0, 64, 48)
    for kernel in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
        want = dense.draw(cam, shadow=True, kernel=kernel)
        assert int((want["flags"] & 1).sum()) > 200
        assert_gbuffer_equal(W.draw(cam, shadow=True, kernel=kernel), want, f"sparse against dense, kernel {kernel}")
    dense.destroy()


def test_one_instance_placement_of_a_model_built_from_a_mesh(svo):
    from test_instances import assert_records, assert_words, stage1
    scene = svo.World.generate(2, 1, 2, 128, 6).upload(0)
    cam = svo.default_camera(2, 2, 128, 64, 48)
    rect, inst = (0, 0, 64, 48), [IM.instance((94.0, 84.0, 4.0))]              # identity rotation, integer position
    model = lambda: svo.World.create([empty_chunk(size=IM.MODEL_SIZE)], 1, 1, 1, IM.MODEL_SIZE).upload(0)
    # depth 5, where the dense path exists: the same records from both models
    depth, v, ix, _ = M.cases()["sphere5"]
    sparse, dense = model(), model()
    assert device_build(svo, sparse, 0, [S.mesh(v, ix, material=5)], depth) == svo.SVO_OK
    assert dense.set_chunk_grid(0, M.add_mesh(S.zeros(depth), v, ix, material=5)) == svo.SVO_OK
    for kernel in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
        prm = svo.trace_params(shadow=True, kernel=kernel)
        want = stage1(svo, dict(W=scene, Mw=dense, cam=cam, inst=inst), prm, rect=rect, max_rays=64 * 48)
        got = stage1(svo, dict(W=scene, Mw=sparse, cam=cam, inst=inst), prm, rect=rect, max_rays=64 * 48)
        assert want["counts"][0] > 50 and got["counts"] == want["counts"]
        assert_words(got["owner"], want["owner"], f"owner, kernel {kernel}")
        assert_records(got["merged"], want["merged"], f"merged, kernel {kernel}")
    dense.destroy()
    # depth 12: the same sphere in a frame 128 times finer runs, and both kernels agree on it
    v12, ix12 = M.uv_sphere((16.13, 15.79, 16.07), 9.0, nu=48, nv=32)
    assert device_build(svo, sparse, 0, [S.mesh(v12, ix12, cell=1.0 / 128.0, material=5)], 12) == svo.SVO_OK
    assert sparse.info.max_chunk_depth == 12 and sparse.info.total_twigs > 100000
    runs = [stage1(svo, dict(W=scene, Mw=sparse, cam=cam, inst=inst), svo.trace_params(shadow=True, kernel=k), rect=rect, max_rays=64 * 48)
            for k in (svo.KERNEL_STACK, svo.KERNEL_LITERAL)]
    assert runs[0]["counts"][0] > 50 and runs[0]["counts"] == runs[1]["counts"]
    assert_words(runs[0]["owner"], runs[1]["owner"], "owner at depth 12")
    assert_records(runs[0]["merged"], runs[1]["merged"], "merged at depth 12")
    sparse.destroy(); scene.destroy()


def test_refusals_leave_the_pools_as_they_were(svo, world):
    W, other = world
    depth, meshes = S.shared_cases()["torus5"]
    assert device_build(svo, W, 0, meshes, depth) == svo.SVO_OK
    before = W.chunk(0)
    v, ix = M.lattice_cube()
    bv, bi = svo.DeviceBuffer.from_numpy(v), svo.DeviceBuffer.from_numpy(ix)
    good = dict(vertices=bv.ptr, indices=bi.ptr, materials=None, nvertices=8, ntriangles=12, origin=(0.0, 0.0, 0.0), cell=1.0, material=1)
    mesh = lambda **kw: svo.Mesh(**dict(good, **kw))
    call = lambda m, n=1, depth=4, chunk=0: svo.lib.svo_world_chunk_from_mesh(W._h, chunk, None if m is None else C.byref(m), n, depth)
    refused = [call(None), call(mesh(), n=-1), call(mesh(), depth=1), call(mesh(), depth=17), call(mesh(), chunk=2), call(mesh(), chunk=-1),
               call(mesh(vertices=None)), call(mesh(indices=None)), call(mesh(cell=0.0)), call(mesh(cell=float("nan"))), call(mesh(cell=1e-45)),
               call(mesh(origin=(0.0, float("inf"), 0.0)))]
    assert refused == [-1] * len(refused)
    two = (svo.Mesh * 2)(mesh(), mesh(ntriangles=0x7FFFFFFE))            # 2^31 - 1 triangles in the list: refused before any device work
    assert call(two[0], n=2) == -6
    same_pools(W.chunk(0), before, "chunk 0 after the refusals")
    same_pools(W.chunk(1), other, "chunk 1 after the refusals")
    check_info(W, other)
    host_only = svo.World.create([empty_chunk()], 1, 1, 1, 128)
    assert svo.lib.svo_world_chunk_from_mesh(host_only._h, 0, C.byref(mesh()), 1, 4) == -5
    host_only.destroy()
    bv.free(); bi.free()
