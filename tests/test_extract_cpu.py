"""svo_chunk_extract (csrc/extract.cpp): a cube of N_C^3 cells copied out of chunk A at a cell offset, in one of the 48 orientations of
the cube, into a chunk of depth D_C <= D_A, on the tree, on the host - the stamp's inverse.  Up to the dense grid's depth the pools and
the count equal, index for index, the model's (tests/extract_model.py: the zero-padded window, the header's rule as an index map,
chunk_of) for every case; the header's four identities hold through svo_chunk_stamp and svo_chunk_combine; at depth 12 and 16 windows
of combine_model's solid cube are taken, and their counts follow from the boxes by integer arithmetic.  Every comparison is exact
equality.  CPU only."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import combine_model as K
import extract_model as X
import grid_model as G
import sparse_mesh_model as S
import stamp_model as T
from test_combine_cpu import deep_cubes
from test_compact_model import same_pools

NEW = ["svo_chunk_extract", "svo_world_chunk_extract"]


def test_the_library_exports_the_two_symbols_and_the_constants(svo):
    out = subprocess.run(["nm", "-D", "--defined-only", svo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in svo.ABI_SYMBOLS and hasattr(svo.lib, name)
        assert re.search(rf" T {name}$", out, flags=re.M)
    assert svo.lib.svo_abi_version() == 4
    assert (svo.EXTRACT_MIN_DEPTH, svo.EXTRACT_MAX_DEPTH) == (2, 16)


# ---- the cases against the dense model -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.cases()))
def test_host_form_equals_the_model(svo, name):
    a, offset, orient, depth = X.case(name)
    before = [x.copy() for x in (a["tree"], a["twig"])]
    want, occupied = X.case_model(name)
    got, count = svo.chunk_extract(a, offset, orient, depth, position=(3.0, -2.0, 7.5), size=32.0)
    same_pools(got, want, name)
    assert count == occupied, name
    assert got["position"] == (3.0, -2.0, 7.5) and got["size"] == 32.0 and got["depth"] == depth                   # the frame as given
    assert G.is_minimal(got)
    for x, y in zip((a["tree"], a["twig"]), before):                                # a is unchanged, byte for byte
        assert np.array_equal(x, y)


def test_the_case_list_holds_what_it_claims(svo):
    cases = X.cases()
    assert {d for _, _, _, d in cases.values()} == {2, 3, 4} and {int(X.chunks()[a]["depth"]) for a, _, _, _ in cases.values()} == {4, 6, 7}
    turned = {o: n for n, (a, offset, o, d) in cases.items() if a == "height4" and offset == (5, -3, -2) and d == 3}
    assert set(turned) == set(range(48)) and X.case_model(turned[0])[1] > 200
    assert len({X.case_model(n)[0]["tree"].tobytes() + X.case_model(n)[0]["twig"].tobytes() for n in turned.values()}) == 48      # pairwise distinct
    assert sum(1 for n in cases if X.case_model(n)[1] > 0) >= 100
    assert sum(1 for _, offset, _, _ in cases.values() if 65536 in offset and -65536 in offset) >= 6
    empty = [n for n in cases if X.case_model(n)[0]["tree"].tolist() == [0]]
    assert len(empty) >= 12                                                        # wholly outside, and windows over nothing
    # the root descent meets EMPTY and LEAF above the target level: a g7 window whose neighbourhood is one word
    for a in ("g6", "g7"):
        assert {d for n, (b, _, _, d) in cases.items() if b == a} == {2, 3, 4}
    # an aligned octant is that child's subtree rebuilt
    for a in ("pairings", "height4"):
        ga = G.pools_to_grid(X.chunks()[a], 4)
        assert np.array_equal(G.pools_to_grid(X.case_model(f"{a}_octant_5")[0], 3), ga[8:16, 0:8, 8:16])
        assert np.array_equal(G.pools_to_grid(X.case_model(f"{a}_octant_2")[0], 3), ga[0:8, 8:16, 0:8])


def test_a_leaf_root_a_at_an_odd_offset_leaves_bricks_from_a_one_word_pool(svo):
    a, offset, orient, depth = X.case("leaf_root_at_odd_offset")
    assert a["twig"].size == 0 and a["tree"].size == 1 and offset == (1, 1, 1) and depth == 4
    want, occupied = X.case_model("leaf_root_at_odd_offset")
    got, count = svo.chunk_extract(a, offset, orient, depth)
    assert count == occupied == 15 ** 3
    # the window holds A's cells [1, 16)^3 in its cells [0, 15)^3: every brick that touches cell 15 on an axis is mixed
    assert got["twig"].size // 64 == want["twig"].size // 64 == 4 ** 3 - 3 ** 3 > 0
    assert G.is_minimal(got)


def test_collapses_are_what_they_claim(svo):
    one = lambda got: (got["tree"].tolist(), got["twig"].size)
    for name, word in (("octant4_the_empty_octant", 0), ("octant4_a_full_octant", G.node(G.LEAF, 5)), ("octant4_a_full_octant_turned", G.node(G.LEAF, 5)), ("hole4_the_hole", 0)):
        a, offset, orient, depth = X.case(name)
        got, count = svo.chunk_extract(a, offset, orient, depth)
        assert one(got) == ([word], 0) and count == (512 if word else 0), name
    a, offset, orient, depth = X.case("hole4_the_hole_missed_by_one")
    got, count = svo.chunk_extract(a, offset, orient, depth)
    assert got["tree"].size > 1 and count == 64


# ---- the identities of the header ------------------------------------------------------------------------------------------------------
IDENTITY_CASES = ["pairings_d3_1_3_5_o", "pairings_d4_-3_2_1_o", "height4_d3_5_1_-3_o", "pairings_d2_13_3_2_o", "g6_d4_", "leaf_root_through_one_face"]


def _named(prefix):
    names = [n for n in X.cases() if n.startswith(prefix)]
    assert names, prefix
    return names[0]


@pytest.mark.parametrize("prefix", IDENTITY_CASES)
def test_the_four_identities_through_stamp_and_combine(svo, prefix):
    a, offset, _, depth = X.case(_named(prefix))
    empty = K.one_word(int(a["depth"]), 0)
    for orient in (0, 5, 11, 22, 30, 41, 47):
        c, occupied = svo.chunk_extract(a, offset, orient, depth)
        assert svo.chunk_stamp(a, c, offset, orient, K.OVER)[1] == 0
        assert svo.chunk_stamp(a, c, offset, orient, K.SUBTRACT)[1] == occupied
        same_pools(svo.chunk_stamp(a, c, offset, orient, K.INTERSECT)[0], svo.chunk_stamp(empty, c, offset, orient, K.MAX)[0], f"{prefix}, orient {orient}")
    for name in ("pairings", "height4", "g6"):
        a = X.chunks()[name]
        whole, occupied = svo.chunk_extract(a, (0, 0, 0), 0, int(a["depth"]))
        rebuilt, _ = svo.chunk_combine(a, K.one_word(int(a["depth"]), 0), K.MAX)
        same_pools(whole, rebuilt, f"{name}: the whole chunk, as it lies")
        assert occupied == int(np.count_nonzero(T._grid(a)))


@pytest.mark.parametrize("orient", T.quarter_turns())
def test_a_quarter_turn_applied_four_times_returns_a_rebuilt(svo, orient):
    a = X.chunks()["pairings"]
    ga = G.pools_to_grid(a, 4)
    x = a
    for turn in range(4):
        x, occupied = svo.chunk_extract(x, (0, 0, 0), orient, 4)
        assert occupied == int(np.count_nonzero(ga))
        if turn < 3:
            assert not np.array_equal(G.pools_to_grid(x, 4), ga)
    same_pools(x, svo.chunk_combine(a, K.one_word(4, 0), K.MAX)[0], f"orient {orient}, four times")


# ---- depth 12 and 16 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [12, 16])
def test_deep_windows_of_the_solid_cube(svo, depth):
    a, _, c = deep_cubes(svo, depth)
    before = [x.copy() for x in (a["tree"], a["twig"])]
    wins = X.deep_windows(depth)
    # a depth-8 window at the odd offset c + (129, 65, 33): three faces of the cube cross it
    offset, d, box, inside = wins["across_three_faces"]
    assert d == 8 and all(v % 2 == 1 for v in offset) and T.box_cells(inside) == 128 * 192 * 224
    got, occupied = svo.chunk_extract(a, offset, 0, d)
    print(f"depth {depth} -> 8: occupied {occupied}, {got['tree'].size} node words, {got['twig'].size // 64} bricks; A had {a['tree'].size} and {a['twig'].size // 64}")
    assert occupied == 128 * 192 * 224 == S.occupied_cells(got)
    assert G.is_minimal(got) and got["depth"] == 8
    far = [hi - lo for lo, hi in zip(offset, inside[1])]                          # the cube's far faces in the window's cells: (128, 192, 224)
    assert far == [128, 192, 224]
    for axis in range(3):                                                           # both sides of the three faces that cross the window
        for side in (far[axis] - 1, far[axis]):
            p = [77, 130, 201]
            p[axis] = side
            want = K.MATERIAL_A if all(v < f for v, f in zip(p, far)) else 0
            assert G.voxel_material(got, *p) == want, (axis, p)
    W = svo.World.create([got], 1, 1, 1, 128)                                     # validate_chunk accepts the pools
    assert W.info.max_chunk_depth == 8
    W.destroy()
    mirrored, count = svo.chunk_extract(a, offset, 7, d)                           # every axis flipped: cell d of the window is cell 255 - d of C
    assert count == occupied and G.is_minimal(mirrored)
    assert G.voxel_material(mirrored, 255 - 77, 255 - 130, 255 - 201) == K.MATERIAL_A and G.voxel_material(mirrored, 255 - 77, 255 - 130, 255 - 230) == 0
    for orient in (7, 46):
        turned, count = svo.chunk_extract(a, offset, orient, d)
        assert count == occupied
        assert svo.chunk_stamp(a, turned, offset, orient, K.OVER)[1] == 0 and svo.chunk_stamp(a, turned, offset, orient, K.SUBTRACT)[1] == occupied
    # a depth-10 window that holds the whole cube
    offset, d, box, inside = wins["the_whole_cube"]
    assert d == 10 and T.box_cells(inside) == K.CUBE ** 3
    got, occupied = svo.chunk_extract(a, offset, 13, d)
    assert occupied == 258 ** 3 == S.occupied_cells(got) and G.is_minimal(got) and got["depth"] == 10
    # depth 2 out of the deep chunk (at depth 16 a root descent of 14 levels): on a face of the cube, and wholly inside
    got, occupied = svo.chunk_extract(a, (c + 255, c + 8, c + 8), 0, 2)           # x cells c + 255 and c + 256 are solid, c + 257 and c + 258 are not
    assert occupied == 2 * 4 * 4 and got["twig"].size == 64 and got["tree"].tolist() == [G.node(G.TWIG, 0)]
    assert [int(G.voxel_material(got, x, 1, 2)) for x in range(4)] == [K.MATERIAL_A, K.MATERIAL_A, 0, 0]
    got, occupied = svo.chunk_extract(a, (c + 101, c + 77, c + 33), 29, 2)
    assert occupied == 64 and got["tree"].tolist() == [G.node(G.LEAF, K.MATERIAL_A)] and got["twig"].size == 0
    for x, y in zip((a["tree"], a["twig"]), before):
        assert np.array_equal(x, y)


# ---- inputs and refusals -------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_any_work(svo):
    a = X.chunks()["pairings"]
    ta, ka = a["tree"].copy(), a["twig"].copy()

    def desc(tree=ta, twig=ka, depth=4, size=128.0, trees=None, twigs=None):
        d = svo.ChunkDesc()
        d.size, d.depth = size, depth
        d.tree = None if tree is None else tree.ctypes.data_as(C.POINTER(C.c_uint32))
        d.trees = (0 if tree is None else tree.size) if trees is None else trees
        d.twig = None if twig is None else twig.ctypes.data_as(C.POINTER(C.c_uint16))
        d.twigs = (0 if twig is None else twig.size // 64) if twigs is None else twigs
        return d

    origin = (C.c_float * 3)(0.0, 0.0, 0.0)

    def host(da, depth=3, out=True, count=True, pl=svo.Placement((1, 2, 3), 5), position=origin, size=16.0):
        o, occupied = svo.ChunkDesc(), C.c_uint64(77)
        rc = svo.lib.svo_chunk_extract(None if da is None else C.byref(da), None if pl is None else C.byref(pl), depth, position, size,
                                       C.byref(o) if out else None, C.byref(occupied) if count else None)
        assert rc == 0 or (not o.tree and not o.twig and o.trees == 0 and occupied.value == 77)     # a refusal leaves *out and the count alone
        if rc == 0:
            svo.lib.svo_chunk_free(C.byref(o))
        return rc

    assert host(desc()) == 0 and host(desc(), count=False) == 0                 # occupied_out may be NULL
    assert host(None) == -1 and host(desc(), out=False) == -1 and host(desc(), position=None) == -1
    # the placement
    assert host(desc(), pl=None) == -1 and host(desc(), pl=svo.Placement((0, 0, 0), 48)) == -1 and host(desc(), pl=svo.Placement((0, 0, 0), 0xFFFFFFFF)) == -1
    for axis in range(3):
        for v, rc in ((65537, -1), (-65537, -1), (2 ** 31 - 1, -1), (-2 ** 31, -1), (65536, 0), (-65536, 0)):
            offset = [0, 0, 0]
            offset[axis] = v
            assert host(desc(), pl=svo.Placement(offset, 47)) == rc
    d = desc()
    pl = svo.Placement()
    assert svo.lib.svo_chunk_extract(C.byref(d), C.byref(pl), 3, origin, 16.0, C.byref(d), None) == -1           # out == a
    for bad in (desc(tree=None), desc(twig=None, twigs=ka.size // 64), desc(trees=0)):
        assert host(bad) == -1
    for size in (0.0, -1.0, float("nan"), float("inf")):
        assert host(desc(), size=size) == -1
        assert host(desc(size=size)) == 0                                       # A's frame is not consulted
    # what svo_world_create's validation refuses
    assert host(desc(trees=ta.size - 1)) == -1
    bad = ta.copy(); bad[0] = G.node(G.BRANCH, 0)
    assert host(desc(tree=bad)) == -1
    bad = ta.copy(); bad[0] = G.node(G.BRANCH, ta.size)
    assert host(desc(tree=bad)) == -1
    bad = ta.copy(); bad[int(np.nonzero(ta >> 30 == G.TWIG)[0][0])] = G.node(G.TWIG, ka.size // 64)
    assert host(desc(tree=bad)) == -1
    # SVO_ERR_UNSUPPORTED: C deeper than A, a depth outside [2, 16], a brick above level depth-2
    one = np.array([G.node(G.LEAF, 3)], np.uint32)
    L = lambda depth: desc(tree=one, twig=None, depth=depth)
    assert host(L(5), depth=6) == -6 and host(L(2), depth=16) == -6 and host(L(6), depth=5) == 0 and host(L(16), depth=2) == 0
    for depth in (0, 1, 17, 30):
        assert host(L(depth), depth=depth) == -6 and host(L(16), depth=depth) == -6 and host(L(depth), depth=2) == -6
    assert host(L(16), depth=16, pl=svo.Placement()) == 0 and host(L(2), depth=2) == 0
    shallow = np.array([G.node(G.TWIG, 0)], np.uint32)
    Tw = lambda depth: desc(tree=shallow, twig=ka[:64].copy(), depth=depth)
    assert host(Tw(2), depth=2) == 0 and host(Tw(3), depth=3) == -6 and host(Tw(3), depth=2) == -6 and host(Tw(4), depth=2) == -6
    # the device form: argument errors first, then a world that is not uploaded
    world = svo.World.create([a, dict(K.one_word(3, 0), position=(128.0, 0.0, 0.0))], 2, 1, 1, 128)
    good = svo.Placement((1, 2, 3), 5)

    def dev(chunk=1, src=world._h, src_chunk=0, w=world._h, pl=good):
        occupied = C.c_uint64(77)
        rc = svo.lib.svo_world_chunk_extract(w, chunk, src, src_chunk, None if pl is None else C.byref(pl), C.byref(occupied))
        assert occupied.value == 77
        return rc

    assert dev(w=None) == -1 and dev(src=None) == -1 and dev(chunk=-1) == -1 and dev(chunk=2) == -1 and dev(src_chunk=-1) == -1 and dev(src_chunk=2) == -1
    assert dev(pl=None) == -1 and dev(pl=svo.Placement((0, 0, 0), 48)) == -1 and dev(pl=svo.Placement((0, 65537, 0), 0)) == -1
    assert dev() == -5 and dev(chunk=0, src_chunk=1) == -5                      # not uploaded comes before the depths
    same_pools(world.chunk(0), a, "the world after the refusals")
    same_pools(world.chunk(1), K.one_word(3, 0), "the world after the refusals, the destination")
    world.destroy()
    with pytest.raises(svo.SvoError) as e:
        svo.chunk_extract(a, (0, 0, 0), 48, 3)
    assert e.value.code == -1
