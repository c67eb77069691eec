"""svo_chunk_from_mesh (csrc/sparse_mesh.cpp): the tree of a mesh list's shell built without the dense grid, on the host.  Up to the
dense grid's depth the pools equal, index for index, the model's grid_to_pools(add_mesh(zeros)) (tests/grid_model.py,
tests/mesh_model.py); at depth 12 and 16 they are read back cell by cell against the windowed restatement of the rule
(tests/sparse_mesh_model.py).  Every comparison is exact equality.  CPU only."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import grid_model as G
import mesh_model as M
import sparse_mesh_model as S
from test_compact_model import same_pools

NEW = ["svo_chunk_from_mesh", "svo_world_chunk_from_mesh"]


def test_the_library_exports_the_two_symbols(svo):
    out = subprocess.run(["nm", "-D", "--defined-only", svo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in svo.ABI_SYMBOLS and hasattr(svo.lib, name)
        assert re.search(rf" T {name}$", out, flags=re.M)
    assert svo.lib.svo_abi_version() == 4


@pytest.mark.parametrize("name", ["sphere5", "sphere5_off", "sphere4", "torus5", "soup2", "soup5", "lattice_cube", "two_meshes", "coincident"])
def test_host_form_equals_the_model(svo, name):
    depth, meshes = S.shared_cases()[name]
    before = [(m["vertices"].copy(), m["indices"].copy()) for m in meshes]
    want = S.case_pools(name)
    assert int(want["tree"][0]) != 0 and want["twig"].size >= 64                  # (depth 2: the root is the one TWIG)
    same_pools(svo.chunk_from_mesh(meshes, depth), want, name)
    for m, (v, ix) in zip(meshes, before):
        assert np.array_equal(m["vertices"], v) and np.array_equal(m["indices"], ix)
    if name == "coincident":                                # the largest of the 64 materials won in every cell
        assert set(np.unique(want["twig"])) == {0, 64}


def test_a_list_of_meshes_is_their_sum_in_any_order(svo):
    depth, meshes = S.shared_cases()["two_meshes"]
    want = S.case_pools("two_meshes")
    same_pools(svo.chunk_from_mesh(meshes[::-1], depth), want, "reversed list")
    one, _ = S.model_pools(depth, meshes[:1])
    assert one["tree"].size != want["tree"].size or not np.array_equal(one["tree"], want["tree"])
    same_pools(svo.chunk_from_mesh(meshes[:1], depth), one, "the first mesh alone")


def test_no_mesh_and_no_live_triangle_give_the_empty_chunk(svo):
    for meshes in ([], [S.dropped_mesh()], [S.dropped_mesh(), S.mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))],
                   [S.mesh(*M.uv_sphere((-40.0, 16.0, 16.0), 10.0))]):        # the last one: wholly outside the grid, at every depth
        for depth in (2, 5, 16):
            c = svo.chunk_from_mesh(meshes, depth)
            assert c["tree"].tolist() == [0] and c["twig"].size == 0 and c["depth"] == depth
    depth, v, ix, kw = M.cases()["sphere5"]
    same_pools(svo.chunk_from_mesh([S.dropped_mesh(), S.mesh(v, ix, **kw)], depth), S.case_pools("sphere5"), "dropped triangles beside a sphere")


@pytest.mark.parametrize("name", list(S.collapse_cases()))
def test_uniform_blocks_collapse_and_mixed_ones_do_not(svo, name):
    depth, meshes, check = S.collapse_cases()[name]
    want = S.case_pools(name)
    check(want["tree"], want["twig"])                       # the model's pools hold the node this case is about
    assert G.is_minimal(want)
    same_pools(svo.chunk_from_mesh(meshes, depth), want, name)


@pytest.mark.parametrize("name", list(S.deep_cases()))
def test_depth_12_and_16_against_the_windowed_rule(svo, name):
    depth, meshes, _ = S.deep_cases()[name]
    windows = S.deep_windows(name)
    marked = sum(int(np.count_nonzero(a)) for _, a in windows)
    assert marked == 2 if name.startswith("ends") else marked > 5000
    c = svo.chunk_from_mesh(meshes, depth, position=(0.0, 0.0, 0.0), size=128.0)
    assert c["depth"] == depth and c["tree"].size == 1 + 8 * int((c["tree"] >> 30 == G.BRANCH).sum())
    S.check_against_windows(c, windows)
    assert G.is_minimal(c)
    if name.startswith("ends"):                             # the first and the last cell of the grid, material 0xFFFF kept whole
        n = 1 << depth
        assert G.voxel_material(c, 0, 0, 0) == 2 and G.voxel_material(c, n - 1, n - 1, n - 1) == 0xFFFF and c["twig"].size == 128
    W = svo.World.create([c], 1, 1, 1, 128)                 # validate_chunk accepts it
    assert W.info.max_chunk_depth == depth and W.info.total_twigs == c["twig"].size // 64
    W.destroy()


def test_every_refusal_comes_before_any_work(svo):
    v, ix = M.lattice_cube()
    pos = (C.c_float * 3)(0.0, 0.0, 0.0)

    def mesh(**kw):
        a = dict(vertices=v.ctypes.data, indices=ix.ctypes.data, materials=None, nvertices=8, ntriangles=12, origin=(0.0, 0.0, 0.0), cell=1.0, material=1)
        a.update(kw)
        return svo.Mesh(**a)

    def host(m, n=1, depth=4, position=pos, size=128.0, out=True):
        d = svo.ChunkDesc()
        rc = svo.lib.svo_chunk_from_mesh(None if m is None else C.byref(m), n, depth, position, size, C.byref(d) if out else None)
        assert rc == 0 or (not d.tree and not d.twig and d.trees == 0)      # a refusal leaves *out alone
        if rc == 0:
            svo.lib.svo_chunk_free(C.byref(d))
        return rc

    world = svo.World.create([S.case_pools("sphere4")], 1, 1, 1, 128)      # not uploaded
    before = world.chunk(0)
    dev = lambda m, n=1, depth=4, chunk=0, w=world._h: svo.lib.svo_world_chunk_from_mesh(w, chunk, None if m is None else C.byref(m), n, depth)
    assert host(mesh()) == 0
    for call in (host, dev):
        assert call(None) == -1 and call(mesh(), n=-1) == -1 and call(None, n=-1) == -1
        for depth in (0, 1, 17, 0xFFFFFFFF):
            assert call(mesh(), depth=depth) == -1
        assert call(mesh(vertices=None)) == -1 and call(mesh(indices=None)) == -1
        for cell in (0.0, -1.0, float("nan"), float("inf"), 1e-45):
            assert call(mesh(cell=cell)) == -1
        for k in range(3):
            for bad in (float("nan"), float("inf"), -float("inf")):
                o = [0.0, 0.0, 0.0]
                o[k] = bad
                assert call(mesh(origin=o)) == -1
        two = (svo.Mesh * 2)(mesh(), mesh(cell=0.0))        # the second mesh of a list is checked too
        assert call(two[0], n=2) == -1
    assert host(mesh(), out=False) == -1 and host(mesh(), position=None) == -1
    for size in (0.0, -1.0, float("nan"), float("inf")):
        assert host(mesh(), size=size) == -1
    assert dev(mesh(), w=None) == -1 and dev(mesh(), chunk=-1) == -1 and dev(mesh(), chunk=1) == -1
    # past the argument checks: the device form needs a resident world, also for an empty list and at every depth
    assert dev(mesh()) == -5 and dev(None, n=0) == -5 and dev(mesh(), depth=16) == -5
    # the host form: nmeshes == 0 needs no meshes; NULL arrays with zero counts are fine
    assert host(None, n=0) == 0 and host(mesh(vertices=None, indices=None, nvertices=0, ntriangles=0)) == 0
    same_pools(world.chunk(0), before, "the world after the refusals")
    world.destroy()
    with pytest.raises(svo.SvoError) as e:
        svo.chunk_from_mesh([S.mesh(v, ix)], 17)
    assert e.value.code == -1
