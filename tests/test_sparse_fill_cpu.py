"""svo_chunk_fill_enclosed (csrc/sparse_fill.cpp): svo_grid_fill_enclosed's rule applied to a chunk on its tree, on the host.  Up to
the dense grid's depth the pools and the count equal, index for index, the model's chunk_of(fill_enclosed(pools_to_grid(chunk)))
(tests/sparse_fill_model.py); at depth 12 and 16 the result is read back against the windowed model and against cubes whose counts
are known in closed form.  Every comparison is exact equality.  CPU only."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import grid_model as G
import sparse_fill_model as F
import sparse_mesh_model as S
from test_compact_model import same_pools

NEW = ["svo_chunk_fill_enclosed", "svo_world_chunk_fill_enclosed"]


def test_the_library_exports_the_two_symbols(svo):
    out = subprocess.run(["nm", "-D", "--defined-only", svo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in svo.ABI_SYMBOLS and hasattr(svo.lib, name)
        assert re.search(rf" T {name}$", out, flags=re.M)
    assert svo.lib.svo_abi_version() == 4


@pytest.mark.parametrize("name", list(F.grid_cases()))
def test_host_form_equals_the_model(svo, name):
    chunk, material = F.case_chunk(name)
    want, filled = F.case_model(name)
    before = (chunk["tree"].copy(), chunk["twig"].copy())
    got, count = svo.chunk_fill_enclosed(chunk, material)
    print(name, "filled", count, "model", filled)
    same_pools(got, want, name)
    assert count == filled
    assert np.array_equal(chunk["tree"], before[0]) and np.array_equal(chunk["twig"], before[1])      # `in` is unchanged
    if name in ("holed", "full", "empty", "through_faces") or name.endswith("_open"):
        assert filled == 0
        same_pools(got, chunk, name + ": nothing filled, a minimal FIFO input comes back as it was")
    if name.endswith("_sealed"):
        assert filled == F.SERPENTINE_CELLS
    if name in ("shell", "nested", "depth2"):
        assert filled > 0
    again, none = svo.chunk_fill_enclosed(got, material)    # a second fill finds nothing
    same_pools(again, got, name + ", filled twice")
    assert none == 0


@pytest.mark.parametrize("name", ["sphere5", "torus5", "two_meshes"])
def test_mesh_then_fill_equals_the_dense_composition(svo, name):
    depth, meshes = S.shared_cases()[name]
    n = 1 << depth
    g = np.zeros((n, n, n), np.uint16)
    for m in meshes:
        svo.grid_add_mesh(g, m["vertices"], m["indices"], **S.add_kw(m))
    filled = svo.grid_fill_enclosed(g, 11)
    assert filled > 0
    want = svo.chunk_from_grid(g)
    got, count = svo.chunk_fill_enclosed(svo.chunk_from_mesh(meshes, depth), 11)
    same_pools(got, want, name)
    assert count == filled


def test_collapses_are_what_they_claim(svo):
    kind = lambda w: int(w) >> 30
    want, filled = F.case_model("cube_to_one_leaf")
    assert want["tree"].tolist() == [G.node(G.LEAF, 5)] and want["twig"].size == 0 and filled == 216
    want, _ = F.case_model("brick_to_leaf")                 # the brick (0, 0, 0) is child 0 of the root: now a LEAF, no brick is left
    assert kind(want["tree"][0]) == G.BRANCH and int(want["tree"][1]) == G.node(G.LEAF, 5) and want["twig"].size == 0
    want, _ = F.case_model("brick_stays")                   # a second material: the brick stays, its 8 inner cells hold it
    assert kind(want["tree"][1]) == G.TWIG and want["twig"].size == 64 and int((want["twig"] == 6).sum()) == 8 and int((want["twig"] == 5).sum()) == 56
    for name in ("cube_to_one_leaf", "brick_to_leaf", "brick_stays"):
        assert G.is_minimal(F.case_model(name)[0])


def test_pools_that_are_not_minimal_or_not_in_fifo_order_come_back_minimal_and_in_order(svo):
    chunk, material = F.untidy_chunk()
    W = svo.World.create([chunk], 1, 1, 1, 128)             # svo_world_create's validation admits the pool
    W.destroy()
    assert not G.is_minimal(chunk)
    want, filled = F.model_fill(chunk, material)
    assert filled == 8 and G.is_minimal(want)
    got, count = svo.chunk_fill_enclosed(chunk, material)
    same_pools(got, want, "untidy pool")
    assert count == 8
    tidy, none = svo.chunk_fill_enclosed(chunk, 0xFFFF)     # another material: the hollow brick stays, everything else is tidied
    same_pools(tidy, F.model_fill(chunk, 0xFFFF)[0], "untidy pool, another material")
    assert none == 8 and tidy["twig"].size == 64


@pytest.mark.parametrize("name", ["sphere12", "sphere16"])
def test_deep_spheres_against_the_windowed_model(svo, name):
    depth, meshes, _ = S.deep_cases()[name]
    windows, filled = F.filled_windows(name, 9)
    assert filled > 20000
    shell = svo.chunk_from_mesh(meshes, depth)
    got, count = svo.chunk_fill_enclosed(shell, 9)
    print(name, "filled", count, "windowed model", filled)
    assert count == filled and got["depth"] == depth
    S.check_against_windows(got, windows)
    assert G.is_minimal(got)
    assert got["tree"].size <= shell["tree"].size and got["twig"].size <= shell["twig"].size
    W = svo.World.create([got], 1, 1, 1, 128)
    W.destroy()


@pytest.mark.parametrize("name", list(F.deep_cubes()))
def test_deep_cubes_fill_254_cubed_cells(svo, name):
    depth, meshes, corner = F.deep_cubes()[name]
    shell = svo.chunk_from_mesh(meshes, depth)
    assert S.occupied_cells(shell) == F.CUBE_SHELL
    got, count = svo.chunk_fill_enclosed(shell, 2)
    print(name, "filled", count)
    assert count == F.CUBE_FILLED == 16387064
    assert S.occupied_cells(got) == 258 ** 3 and G.is_minimal(got)
    assert F.largest_leaf_edge(got) >= 64
    assert got["tree"].size <= shell["tree"].size and got["twig"].size <= shell["twig"].size
    rng = np.random.default_rng(depth)
    n = 1 << depth
    points = np.concatenate([rng.integers(corner - 8, corner + 264, (300, 3)), rng.integers(0, n, (40, 3)),
                             [[corner - 2, corner, corner], [corner - 1, corner, corner], [corner + 1, corner + 1, corner + 1], [corner + 254, corner + 254, corner + 254],
                              [corner + 255, corner + 9, corner + 9], [corner + 256, corner + 9, corner + 9], [corner + 257, corner + 9, corner + 9], [0, 0, 0], [n - 1, n - 1, n - 1]]])
    seen = set()
    for x, y, z in points.tolist():
        want = F.cube_material(corner, x, y, z, 6, 2)
        seen.add(want)
        assert G.voxel_material(got, x, y, z) == want, (x, y, z)
    assert seen == {0, 2, 6}
    again, none = svo.chunk_fill_enclosed(got, 2)
    same_pools(again, got, name + ", filled twice")
    assert none == 0
    W = svo.World.create([got], 1, 1, 1, 128)               # validate_chunk accepts it
    assert W.info.max_chunk_depth == depth
    W.destroy()


def test_every_refusal_comes_before_any_work(svo):
    chunk, material = F.case_chunk("shell")
    tree, twig = chunk["tree"].copy(), chunk["twig"].copy()

    def desc(tree=tree, twig=twig, depth=5, size=128.0, trees=None, twigs=None):
        d = svo.ChunkDesc()
        d.size, d.depth = size, depth
        d.tree = None if tree is None else tree.ctypes.data_as(C.POINTER(C.c_uint32))
        d.trees = (0 if tree is None else tree.size) if trees is None else trees
        d.twig = None if twig is None else twig.ctypes.data_as(C.POINTER(C.c_uint16))
        d.twigs = (0 if twig is None else twig.size // 64) if twigs is None else twigs
        return d

    def host(d, material=material, out=True, count=True):
        o, filled = svo.ChunkDesc(), C.c_uint64(77)
        rc = svo.lib.svo_chunk_fill_enclosed(None if d is None else C.byref(d), material, C.byref(o) if out else None, C.byref(filled) if count else None)
        assert rc == 0 or (not o.tree and not o.twig and o.trees == 0 and filled.value == 77)       # a refusal leaves *out and the count alone
        if rc == 0:
            svo.lib.svo_chunk_free(C.byref(o))
        return rc

    assert host(desc()) == 0 and host(desc(), count=False) == 0          # filled_out may be NULL
    assert host(None) == -1 and host(desc(), out=False) == -1 and host(desc(), material=0) == -1
    assert host(desc(tree=None)) == -1 and host(desc(twig=None, twigs=twig.size // 64)) == -1 and host(desc(trees=0)) == -1
    d = desc()
    assert svo.lib.svo_chunk_fill_enclosed(C.byref(d), material, C.byref(d), None) == -1          # out may not alias in
    for size in (0.0, -1.0, float("nan"), float("inf")):
        assert host(desc(size=size)) == -1
    # what svo_world_create's validation refuses
    assert host(desc(trees=tree.size - 1)) == -1            # not 1 + 8k node words
    bad = tree.copy(); bad[0] = G.node(G.BRANCH, 0)
    assert host(desc(tree=bad)) == -1                       # a BRANCH that does not point forward
    bad = tree.copy(); bad[0] = G.node(G.BRANCH, tree.size)
    assert host(desc(tree=bad)) == -1                       # ... or beyond the pool
    bad = tree.copy(); bad[int(np.nonzero(tree >> 30 == G.TWIG)[0][0])] = G.node(G.TWIG, twig.size // 64)
    assert host(desc(tree=bad)) == -1                       # a TWIG beyond the bricks
    assert host(desc(depth=3)) == -1                        # BRANCHes below level depth-2
    two = np.array([G.node(G.BRANCH, 1)] + [G.node(G.BRANCH, 9)] * 2 + [0] * 14, np.uint32)
    assert host(desc(tree=two, twig=None, depth=6)) == -1   # a child block referenced twice
    # SVO_ERR_UNSUPPORTED: a depth outside [2, 16], a brick above level depth-2
    one = np.array([G.node(G.LEAF, 3)], np.uint32)
    for depth in (0, 1, 17, 30):
        assert host(desc(tree=one, twig=None, depth=depth)) == -6
    assert host(desc(tree=one, twig=None, depth=16)) == 0
    shallow = np.array([G.node(G.TWIG, 0)], np.uint32)
    assert host(desc(tree=shallow, twig=twig[:64].copy(), depth=2)) == 0 and host(desc(tree=shallow, twig=twig[:64].copy(), depth=3)) == -6
    # the device form: argument errors first, then a world that is not uploaded
    world = svo.World.create([chunk], 1, 1, 1, 128)
    dev = lambda chunk=0, material=material, w=world._h: svo.lib.svo_world_chunk_fill_enclosed(w, chunk, material, None)
    assert dev(w=None) == -1 and dev(chunk=-1) == -1 and dev(chunk=1) == -1 and dev(material=0) == -1
    assert dev() == -5
    same_pools(world.chunk(0), chunk, "the world after the refusals")
    world.destroy()
    with pytest.raises(svo.SvoError) as e:
        svo.chunk_fill_enclosed(chunk, 0)
    assert e.value.code == -1
