"""svo_chunk_from_grid (csrc/grid.cpp) against the numpy model of the rule (tests/grid_model.py), the model against itself and
against the point-query model, and the argument checks of the three grid entry points.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import grid_model as G
import locate_model as LM
from test_compact_model import leaf_centres, same_pools

NAMES = ["g2_empty", "g2_leaf", "g2_mixed", "g3", "g5", "g6", "g7"]


@pytest.mark.parametrize("name", NAMES)
def test_host_builder_equals_the_model(svo, name):
    grid = G.grids()[name]
    want = G.model_chunk(name)
    got = svo.chunk_from_grid(grid, position=(0.0, 0.0, 0.0), size=128.0)
    same_pools(got, want, name)
    assert got["position"] == (0.0, 0.0, 0.0) and got["size"] == 128.0
    W = svo.World.create([got], 1, 1, 1, 128)              # validate_chunk accepts it
    info = W.info
    assert info.total_trees == want["tree"].size and info.total_twigs == want["twig"].size // 64
    assert info.max_chunk_depth == G.depth_of(grid) and info.exact_geometry == 1
    W.destroy()


def test_the_grids_are_what_the_tests_need():
    T = lambda c, i=0: int(c["tree"][i]) >> 30
    assert T(G.model_chunk("g2_empty")) == G.EMPTY and G.model_chunk("g2_empty")["tree"].size == 1
    assert int(G.model_chunk("g2_leaf")["tree"][0]) == G.node(G.LEAF, 7)
    assert T(G.model_chunk("g2_mixed")) == G.TWIG and G.model_chunk("g2_mixed")["twig"].size == 64
    c3 = G.model_chunk("g3")
    assert c3["tree"].size == 9 and c3["twig"].size == 5 * 64
    assert sorted(int(w) for w in c3["tree"][1:] if (int(w) >> 30) != G.TWIG) == sorted([G.node(G.EMPTY), G.node(G.LEAF, 9), G.node(G.LEAF, 0xFFFF)])
    c5 = G.model_chunk("g5")
    assert int(c5["tree"][1 + 5]) == G.node(G.LEAF, 300)                # the 16^3 box: child x=1, y=0, z=1 of the root
    c6, c7 = G.model_chunk("g6"), G.model_chunk("g7")
    assert (c6["tree"].size - 1) // 8 > 256                             # ranks cross thread-block boundaries
    assert c7["twig"].size // 64 > 2000 and c7["tree"].size > 4096      # more than one workgroup, more than one scan tile


@pytest.mark.parametrize("name", NAMES)
def test_model_round_trip_and_resampling(name):
    grid = G.grids()[name]
    c, depth = G.model_chunk(name), G.depth_of(grid)
    assert np.array_equal(G.pools_to_grid(c, depth), grid)
    assert np.array_equal(G.pools_to_grid(c, depth - 1), grid[::2, ::2, ::2])
    assert np.array_equal(G.pools_to_grid(c, depth + 1), np.repeat(np.repeat(np.repeat(grid, 2, 0), 2, 1), 2, 2))
    rng = np.random.default_rng(11)
    for X, Y, Z in rng.integers(0, 1 << depth, (200, 3)):
        assert G.voxel_material(c, int(X), int(Y), int(Z)) == int(grid[Z, Y, X])


@pytest.mark.parametrize("name", NAMES)
def test_pools_are_minimal(name):
    assert G.is_minimal(G.model_chunk(name))


@pytest.mark.parametrize("name", ["g3", "g5"])
def test_point_queries_over_the_model_pools_report_the_grid(name):
    grid = G.grids()[name]
    c, depth = G.model_chunk(name), G.depth_of(grid)
    world = LM.world_of([c], 1, 1, 1, 128)
    r = LM.locate(world, leaf_centres(depth))
    assert np.all(r["flags"] & LM.INSIDE)
    assert np.array_equal(r["material"].reshape(grid.shape), grid)
    assert np.array_equal(((r["flags"] & LM.SOLID) != 0).reshape(grid.shape), grid != 0)      # (a LEAF of this tree is never material 0)


def test_oracle_marches_the_model_pools_of_g5(svo, oracle):
    """The march-parity test on the GPU compares against this world: it must have something to compare."""
    O = oracle.OracleWorld.from_chunks([G.model_chunk("g5")], 1, 1, 1, 128)
    cam = svo.default_camera(1, 1, 128, 64, 48)
    for semantics in (0, 1):
        g = O.trace_image(cam, params=oracle.make_params(shadow=True, semantics=semantics))
        assert int((g["flags"] & 1).sum()) >= 1 and not np.any(g["flags"] & 0x8000)


def test_argument_errors_come_before_any_device_work(svo):
    grid = np.zeros((4, 4, 4), np.uint16)
    pos = (C.c_float * 3)(0, 0, 0)
    d = svo.ChunkDesc()
    f = svo.lib.svo_chunk_from_grid
    assert f(None, 2, pos, 128.0, C.byref(d)) == -1
    assert f(grid.ctypes.data, 2, None, 128.0, C.byref(d)) == -1
    assert f(grid.ctypes.data, 2, pos, 128.0, None) == -1
    for depth in (0, 1, 11, 0xFFFFFFFF):
        assert f(grid.ctypes.data, depth, pos, 128.0, C.byref(d)) == -1
    for size in (0.0, -1.0, float("nan"), float("inf")):
        assert f(grid.ctypes.data, 2, pos, size, C.byref(d)) == -1
    with pytest.raises(ValueError):
        svo.chunk_from_grid(np.zeros((4, 4, 8), np.uint16))
    W = svo.World.create([G.model_chunk("g2_mixed")], 1, 1, 1, 128)
    ptr = 0x1000                                            # a dummy device pointer, never dereferenced
    for call in (lambda w, i, p, dp: svo.lib.svo_world_chunk_from_grid(w, i, p, dp),
                 lambda w, i, p, dp: svo.lib.svo_world_chunk_to_grid(w, i, dp, p, None)):
        assert call(None, 0, ptr, 2) == -1
        assert call(W._h, 0, None, 2) == -1
        assert call(W._h, 0, ptr + 2, 2) == -1              # not 16-byte aligned
        for chunk in (-1, 1):
            assert call(W._h, chunk, ptr, 2) == -1
        for depth in (0, 1, 11):
            assert call(W._h, 0, ptr, depth) == -1
        assert call(W._h, 0, ptr, 2) == -5                  # a host-only world: SVO_ERR_NOT_UPLOADED, behind the argument checks
    with pytest.raises(svo.SvoError) as e:
        W.chunk_from_grid(0, ptr, 2)
    assert e.value.code == -5
    with pytest.raises(svo.SvoError) as e:
        W.chunk_to_grid(0, 2, ptr)
    assert e.value.code == -5
    same_pools(W.chunk(0), G.model_chunk("g2_mixed"), "after the refused calls")
    W.destroy()
