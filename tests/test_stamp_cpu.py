"""svo_chunk_stamp (csrc/stamp.cpp): chunk B placed into chunk A at a cell offset, in one of the 48 orientations of the cube, through
a COMBINE_* rule, on the two trees, on the host.  Up to the dense grid's depth the pools and the count equal, index for index, the
model's (tests/stamp_model.py: numpy transpose and flip, slices, combine_model.f, chunk_of) for every case and all five ops; at depth
12 and 16 a LEAF-root B of depth 8 goes into combine_model's solid cube at an odd offset, and the counts follow from the two boxes by
integer arithmetic.  Every comparison is exact equality.  CPU only."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import combine_model as K
import grid_model as G
import sparse_mesh_model as S
import stamp_model as T
from test_combine_cpu import deep_cubes
from test_compact_model import same_pools

NEW = ["svo_chunk_stamp", "svo_world_chunk_stamp"]
OPS = list(K.OPS.items())


def test_the_library_exports_the_two_symbols_and_the_constants(svo):
    out = subprocess.run(["nm", "-D", "--defined-only", svo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in svo.ABI_SYMBOLS and hasattr(svo.lib, name)
        assert re.search(rf" T {name}$", out, flags=re.M)
    assert svo.lib.svo_abi_version() == 4
    assert (svo.STAMP_MIN_DEPTH, svo.STAMP_MAX_DEPTH, svo.STAMP_ORIENTS, svo.STAMP_OFFSET_LIMIT) == (2, 16, 48, 65536)
    assert C.sizeof(svo.Placement) == 16
    pl = svo.Placement((1, -2, 3), 47)
    assert list(pl.offset) == [1, -2, 3] and pl.orient == 47
    assert len(svo.ORIENT_ROTATIONS) == 24 and svo.ORIENT_ROTATIONS[0] == 0
    assert list(svo.ORIENT_ROTATIONS) == [o for o in range(48) if T.is_rotation(o)]


# ---- the orientations ------------------------------------------------------------------------------------------------------------------
def test_the_48_oriented_grids_are_pairwise_distinct_and_follow_the_rule():
    gb = G.grids()["g3"]
    seen = {T.oriented(gb, o).tobytes() for o in range(48)}
    assert len(seen) == 48
    rng = np.random.default_rng(48)
    for o in range(48):                                     # the header's sentence, cell by cell
        g, pi = T.oriented(gb, o), T.PERMS[o >> 3]
        for d in rng.integers(0, 8, (12, 3)).tolist():
            q = [0, 0, 0]
            for i in range(3):
                q[pi[i]] = 7 - d[i] if (o >> i) & 1 else d[i]
            assert g[d[2], d[1], d[0]] == gb[q[2], q[1], q[0]]
    # the determinant of the cell map, from the permutation matrix and the signs: +1 exactly for ORIENT_ROTATIONS
    for o in range(48):
        m = np.zeros((3, 3))
        for i in range(3):
            m[T.PERMS[o >> 3][i], i] = -1.0 if (o >> i) & 1 else 1.0
        assert (round(float(np.linalg.det(m))) == 1) == T.is_rotation(o)


def test_there_are_six_quarter_turns():
    assert len(T.quarter_turns()) == 6


@pytest.mark.parametrize("orient", T.quarter_turns())
def test_a_quarter_turn_applied_four_times_into_an_empty_chunk_returns_b(svo, orient):
    b = G.model_chunk("g3")
    empty = K.one_word(3, 0)
    x = b
    for turn in range(4):
        x, changed = svo.chunk_stamp(empty, x, (0, 0, 0), orient, K.MAX)
        assert changed == int(np.count_nonzero(G.grids()["g3"]))
        if turn < 3:
            assert not np.array_equal(G.pools_to_grid(x, 3), G.grids()["g3"])
    same_pools(x, b, f"orient {orient}, four times")


# ---- the cases against the dense model, all five ops -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.cases()))
def test_host_form_equals_the_model(svo, name):
    a, b, offset, orient = T.case(name)
    before = [x.copy() for x in (a["tree"], a["twig"], b["tree"], b["twig"])]
    for opname, op in OPS:
        want, changed = T.case_model(name, op)
        got, count = svo.chunk_stamp(a, b, offset, orient, op)
        same_pools(got, want, f"{name}, {opname}")
        assert count == changed, (name, opname)
        assert got["position"] == tuple(a["position"]) and got["size"] == a["size"] and got["depth"] == a["depth"]     # A's frame
    for x, y in zip((a["tree"], a["twig"], b["tree"], b["twig"]), before):                      # a and b are unchanged, byte for byte
        assert np.array_equal(x, y)


def test_the_case_list_holds_what_it_claims():
    cases = T.cases()
    assert {T.chunks()[b]["depth"] for _, b, _, _ in cases.values()} == {2, 3, 4} and {T.chunks()[a]["depth"] for a, _, _, _ in cases.values()} == {4}
    assert {o for _, b, offset, o in cases.values() if b == "b3" and offset == (5, -3, 9)} == set(range(48))
    outside = [n for n, (a, b, offset, o) in cases.items() if not T.placed(np.ones((1 << T.chunks()[b]["depth"],) * 3, np.uint16), 16, offset).any()]
    assert len(outside) >= 9


def test_a_leaf_root_b_at_an_odd_offset_leaves_more_bricks_than_both_inputs_hold(svo):
    a, b, offset, orient = T.case("leaf_root_at_odd_offset")
    assert a["twig"].size == 0 and b["twig"].size == 0 and a["tree"].size == 1 and b["tree"].size == 1 and offset == (1, 1, 1)
    got, changed = svo.chunk_stamp(a, b, offset, orient, K.MAX)
    assert changed == 8 ** 3
    assert got["twig"].size // 64 == 3 ** 3 - 1 > 0 and got["tree"].size > a["tree"].size + b["tree"].size     # every brick [1, 9)^3 touches but the one it holds whole
    assert G.is_minimal(got)


def test_collapses_are_what_they_claim(svo):
    one = lambda got: (got["tree"].tolist(), got["twig"].size)
    for name in ("half_space_completed", "hole_at_odd_offset_completed"):
        a, b, offset, orient = T.case(name)
        got, changed = svo.chunk_stamp(a, b, offset, orient, K.MAX)
        assert one(got) == ([G.node(G.LEAF, 5)], 0) and changed == 512, name
    a, b, offset, orient = T.case("half_space_missed_by_one")
    assert svo.chunk_stamp(a, b, offset, orient, K.MAX)[0]["tree"].size > 1
    a, b, offset, orient = T.case("into_empty")             # SUBTRACT of B where B was stamped with MAX into an empty chunk: EMPTY
    stamped, changed = svo.chunk_stamp(a, b, offset, orient, K.MAX)
    assert changed == int(np.count_nonzero(G.grids()["g3"])) > 0
    got, back = svo.chunk_stamp(stamped, b, offset, orient, K.SUBTRACT)
    assert one(got) == ([0], 0) and back == changed
    got, cleared = svo.chunk_stamp(stamped, b, (16, 0, 0), orient, K.INTERSECT)     # outside B's cube b is 0: INTERSECT clears A
    assert one(got) == ([0], 0) and cleared == changed


@pytest.mark.parametrize("name", ["pairings", "pairings_swapped", "g2_mixed_depth2", "g3_full", "g5_shell", "two_spheres", "untidy_itself", "checkerboards"])
def test_equal_depth_offset_0_orient_0_is_svo_chunk_combine(svo, name):
    a, b = K.pairs()[name]
    for opname, op in OPS:
        want, changed = svo.chunk_combine(a, b, op)
        got, count = svo.chunk_stamp(a, b, (0, 0, 0), 0, op)
        same_pools(got, want, f"{name}, {opname}")
        assert count == changed


def test_the_two_chunk_recipe_equals_the_model_of_the_wide_grid(svo):
    """A model that straddles the border between chunk 0 and its +x neighbour: two calls whose offsets differ by N_A on x."""
    left, right, b = T.chunks()["pairings"], T.chunks()["height4"], T.chunks()["b3"]
    offset, orient = (13, 5, -2), 29
    wide = np.concatenate([G.pools_to_grid(left, 4), G.pools_to_grid(right, 4)], axis=2)        # [z, y, x] of 16 x 16 x 32
    put = np.zeros((16 + 8, 16, 32), np.uint16)             # z from -2 on: room for what lies outside
    put[0:8, 5:13, 13:21] = T.oriented(G.grids()["g3"], orient)
    for opname, op in OPS:
        g = K.f(op, wide, put[2:18]).astype(np.uint16)
        got_l, n_l = svo.chunk_stamp(left, b, offset, orient, op)
        got_r, n_r = svo.chunk_stamp(right, b, (offset[0] - 16, offset[1], offset[2]), orient, op)
        assert np.array_equal(G.pools_to_grid(got_l, 4), g[:, :, :16]) and np.array_equal(G.pools_to_grid(got_r, 4), g[:, :, 16:]), opname
        assert n_l + n_r == int((g != wide).sum())


# ---- depth 12 and 16 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [12, 16])
def test_deep_leaf_root_b_at_an_odd_offset(svo, depth):
    a, _, c = deep_cubes(svo, depth)
    box_a, box_b = T.deep_boxes(depth)
    assert all(v % 2 == 1 for v in box_b[0]) and all(0 <= lo and hi <= 1 << depth for lo, hi in zip(*box_b))
    both = T.box_overlap(box_a, box_b)
    assert T.box_cells(box_b) == 256 ** 3 and T.box_cells(both) == 128 * 192 * 224 and T.box_cells(box_a) == K.CUBE ** 3
    b, offset = T.deep_b(), box_b[0]
    before = [x.copy() for x in (a["tree"], a["twig"])]
    got, changed = svo.chunk_stamp(a, b, offset, 0, K.MAX)
    print(f"depth {depth}: MAX changed {changed}, {got['tree'].size} node words, {got['twig'].size // 64} bricks; A had {a['tree'].size} and {a['twig'].size // 64}")
    assert changed == T.box_cells(box_b)                    # material 5 over empty cells and over A's material 3 alike
    assert G.is_minimal(got) and got["depth"] == depth and got["position"] == tuple(a["position"])
    assert S.occupied_cells(got) == T.box_cells(box_a) + T.box_cells(box_b) - T.box_cells(both)
    for axis in range(3):                                   # both sides of all six faces of B's cube, and of A's
        for box in (box_b, box_a):
            for face in (box[0][axis], box[1][axis]):
                for side in (face - 1, face):
                    p = [box_b[0][0] + 77, box_b[0][1] + 130, box_b[0][2] + 201]
                    p[axis] = side
                    want = T.DEEP_MATERIAL if T.inside(box_b, *p) else K.MATERIAL_A if T.inside(box_a, *p) else 0
                    assert G.voxel_material(got, *p) == want, (axis, p)
    W = svo.World.create([got], 1, 1, 1, 128)               # validate_chunk accepts the pools
    assert W.info.max_chunk_depth == depth
    W.destroy()
    sub, carved = svo.chunk_stamp(a, b, offset, 0, K.SUBTRACT)
    assert carved == T.box_cells(both) and S.occupied_cells(sub) == T.box_cells(box_a) - T.box_cells(both) and G.is_minimal(sub)
    for orient in (17, 46):                                 # a cube of one value is the same in every orientation
        same_pools(svo.chunk_stamp(a, b, offset, orient, K.MAX)[0], got, f"orient {orient}")
    for x, y in zip((a["tree"], a["twig"]), before):
        assert np.array_equal(x, y)


# ---- inputs and refusals -------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_any_work(svo):
    a, b = T.chunks()["pairings"], T.chunks()["b3"]
    ta, ka, tb, kb = a["tree"].copy(), a["twig"].copy(), b["tree"].copy(), b["twig"].copy()

    def desc(tree=ta, twig=ka, depth=4, size=128.0, trees=None, twigs=None):
        d = svo.ChunkDesc()
        d.size, d.depth = size, depth
        d.tree = None if tree is None else tree.ctypes.data_as(C.POINTER(C.c_uint32))
        d.trees = (0 if tree is None else tree.size) if trees is None else trees
        d.twig = None if twig is None else twig.ctypes.data_as(C.POINTER(C.c_uint16))
        d.twigs = (0 if twig is None else twig.size // 64) if twigs is None else twigs
        return d

    B = lambda **kw: desc(**dict(dict(tree=tb, twig=kb, depth=3), **kw))

    def host(da, db, op=K.MAX, out=True, count=True, pl=svo.Placement((1, 2, 3), 5)):
        o, changed = svo.ChunkDesc(), C.c_uint64(77)
        rc = svo.lib.svo_chunk_stamp(None if da is None else C.byref(da), None if db is None else C.byref(db), None if pl is None else C.byref(pl), op,
                                     C.byref(o) if out else None, C.byref(changed) if count else None)
        assert rc == 0 or (not o.tree and not o.twig and o.trees == 0 and changed.value == 77)     # a refusal leaves *out and the count alone
        if rc == 0:
            svo.lib.svo_chunk_free(C.byref(o))
        return rc

    assert host(desc(), B()) == 0 and host(desc(), B(), count=False) == 0       # changed_out may be NULL
    d = desc()
    assert host(d, d) == 0                                                      # a == b is allowed
    assert host(None, B()) == -1 and host(desc(), None) == -1 and host(desc(), B(), out=False) == -1
    assert host(desc(), B(), op=-1) == -1 and host(desc(), B(), op=5) == -1
    # the placement
    assert host(desc(), B(), pl=None) == -1 and host(desc(), B(), pl=svo.Placement((0, 0, 0), 48)) == -1
    assert host(desc(), B(), pl=svo.Placement((0, 0, 0), 0xFFFFFFFF)) == -1
    for axis in range(3):
        for v, rc in ((65537, -1), (-65537, -1), (2 ** 31 - 1, -1), (-2 ** 31, -1), (65536, 0), (-65536, 0)):
            offset = [0, 0, 0]
            offset[axis] = v
            assert host(desc(), B(), pl=svo.Placement(offset, 47)) == rc
    d, e = desc(), B()
    pl = svo.Placement()
    assert svo.lib.svo_chunk_stamp(C.byref(d), C.byref(e), C.byref(pl), 0, C.byref(d), None) == -1
    assert svo.lib.svo_chunk_stamp(C.byref(d), C.byref(e), C.byref(pl), 0, C.byref(e), None) == -1
    for bad in (desc(tree=None), desc(twig=None, twigs=ka.size // 64), desc(trees=0)):
        assert host(bad, B()) == -1 and host(desc(), bad) == -1
    for size in (0.0, -1.0, float("nan"), float("inf")):
        assert host(desc(size=size), B()) == -1
        assert host(desc(), B(size=size)) == 0                                  # B's frame is not consulted
    # what svo_world_create's validation refuses, in a and in b
    assert host(desc(trees=ta.size - 1), B()) == -1 and host(desc(), B(trees=tb.size - 1)) == -1
    bad = tb.copy(); bad[0] = G.node(G.BRANCH, 0)
    assert host(desc(), B(tree=bad)) == -1                  # a BRANCH that does not point forward (the walk's marker word, in a pool)
    bad = tb.copy(); bad[0] = G.node(G.BRANCH, tb.size)
    assert host(desc(), B(tree=bad)) == -1
    bad = ta.copy(); bad[int(np.nonzero(ta >> 30 == G.TWIG)[0][0])] = G.node(G.TWIG, ka.size // 64)
    assert host(desc(tree=bad), B()) == -1
    # SVO_ERR_UNSUPPORTED: B deeper than A, a depth outside [2, 16], a brick above level depth-2
    one = np.array([G.node(G.LEAF, 3)], np.uint32)
    L = lambda depth: desc(tree=one, twig=None, depth=depth)
    assert host(L(5), L(6)) == -6 and host(L(2), L(16)) == -6 and host(L(6), L(5)) == 0 and host(L(16), L(2)) == 0
    for depth in (0, 1, 17, 30):
        assert host(L(depth), L(depth)) == -6 and host(L(16), L(depth)) == -6 and host(L(depth), L(2)) == -6
    assert host(L(16), L(16), pl=svo.Placement()) == 0 and host(L(2), L(2)) == 0
    shallow = np.array([G.node(G.TWIG, 0)], np.uint32)
    Tw = lambda depth: desc(tree=shallow, twig=ka[:64].copy(), depth=depth)
    assert host(Tw(2), Tw(2)) == 0 and host(L(3), Tw(2)) == 0 and host(Tw(3), L(3)) == -6 and host(L(3), Tw(3)) == -6 and host(L(4), Tw(3)) == -6
    # the device form: argument errors first, then a world that is not uploaded
    world = svo.World.create([a, dict(b, position=(128.0, 0.0, 0.0))], 2, 1, 1, 128)
    good = svo.Placement((1, 2, 3), 5)

    def dev(chunk=0, src=world._h, src_chunk=1, op=0, w=world._h, pl=good):
        return svo.lib.svo_world_chunk_stamp(w, chunk, src, src_chunk, None if pl is None else C.byref(pl), op, None)

    assert dev(w=None) == -1 and dev(src=None) == -1 and dev(chunk=-1) == -1 and dev(chunk=2) == -1 and dev(src_chunk=-1) == -1 and dev(src_chunk=2) == -1
    assert dev(op=-1) == -1 and dev(op=5) == -1 and dev(pl=None) == -1 and dev(pl=svo.Placement((0, 0, 0), 48)) == -1 and dev(pl=svo.Placement((0, 65537, 0), 0)) == -1
    assert dev() == -5 and dev(chunk=1, src_chunk=0) == -5                      # not uploaded comes before the depths
    same_pools(world.chunk(0), a, "the world after the refusals")
    same_pools(world.chunk(1), b, "the world after the refusals, the source")
    world.destroy()
    with pytest.raises(svo.SvoError) as e:
        svo.chunk_stamp(a, b, (0, 0, 0), 48, K.MAX)
    assert e.value.code == -1
