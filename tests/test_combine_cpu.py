"""svo_chunk_combine (csrc/combine.cpp): two chunks of one depth combined cell by cell on their trees, on the host.  Up to the dense
grid's depth the pools and the count equal, index for index, the model's chunk_of(f_op(pools_to_grid(A), pools_to_grid(B)))
(tests/combine_model.py) for all five ops; at depth 12 and 16 two solid cubes give counts known in closed form, and the filled deep
sphere carved out of one of them is read back against the windowed model.  Every comparison is exact equality.  CPU only."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import combine_model as K
import grid_model as G
import sparse_fill_model as F
import sparse_mesh_model as S
from test_compact_model import same_pools

NEW = ["svo_chunk_combine", "svo_world_chunk_combine"]
OPS = list(K.OPS.items())


def test_the_library_exports_the_two_symbols_and_the_constants(svo):
    out = subprocess.run(["nm", "-D", "--defined-only", svo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in svo.ABI_SYMBOLS and hasattr(svo.lib, name)
        assert re.search(rf" T {name}$", out, flags=re.M)
    assert svo.lib.svo_abi_version() == 4
    assert (svo.COMBINE_MAX, svo.COMBINE_UNDER, svo.COMBINE_OVER, svo.COMBINE_SUBTRACT, svo.COMBINE_INTERSECT) == (K.MAX, K.UNDER, K.OVER, K.SUBTRACT, K.INTERSECT) == (0, 1, 2, 3, 4)
    assert (svo.COMBINE_MIN_DEPTH, svo.COMBINE_MAX_DEPTH) == (2, 16)


def test_the_models_cell_function_is_the_headers_table():
    a, b = np.array([0, 0, 4, 4, 9, 4]), np.array([0, 7, 0, 7, 2, 4])
    assert K.f(K.MAX, a, b).tolist() == [0, 7, 4, 7, 9, 4] and K.f(K.UNDER, a, b).tolist() == [0, 7, 4, 4, 9, 4]
    assert K.f(K.OVER, a, b).tolist() == [0, 7, 4, 7, 2, 4] and K.f(K.SUBTRACT, a, b).tolist() == [0, 0, 4, 0, 0, 0]
    assert K.f(K.INTERSECT, a, b).tolist() == [0, 0, 0, 4, 9, 4]


# ---- 1 to 4: the pairs against the dense model, all five ops --------------------------------------------------------------------------
@pytest.mark.parametrize("opname,op", OPS)
@pytest.mark.parametrize("name", list(K.pairs()))
def test_host_form_equals_the_model(svo, name, opname, op):
    a, b = K.pairs()[name]
    want, changed = K.pair_model(name, op)
    before = [x.copy() for x in (a["tree"], a["twig"], b["tree"], b["twig"])]
    got, count = svo.chunk_combine(a, b, op)
    print(name, opname, "changed", count, "model", changed, "node words", got["tree"].size, "bricks", got["twig"].size // 64)
    same_pools(got, want, f"{name}, {opname}")
    assert count == changed
    assert got["position"] == tuple(a["position"]) and got["size"] == a["size"]                 # the result keeps A's frame
    for x, y in zip((a["tree"], a["twig"], b["tree"], b["twig"]), before):                      # a and b are unchanged, byte for byte
        assert np.array_equal(x, y)


def _kinds_met(a, b):
    """The (type of A's word, type of B's word, at level depth-2?) of every pair the walk visits."""
    met, maxlevel = set(), int(a["depth"]) - 2
    stack = [(int(a["tree"][0]), int(b["tree"][0]), 0)]
    while stack:
        wa, wb, level = stack.pop()
        met.add((wa >> 30, wb >> 30, level == maxlevel))
        if G.BRANCH in (wa >> 30, wb >> 30):
            kid = lambda t, w, c: int(t[(w & 0x3FFFFFFF) + c]) if w >> 30 == G.BRANCH else w
            stack.extend((kid(a["tree"], wa, c), kid(b["tree"], wb, c), level + 1) for c in range(8))
    return met


def test_the_pairing_cases_hold_every_pairing():
    a, b = K.pairs()["pairings"]
    met = _kinds_met(a, b) | _kinds_met(*K.pairs()["pairings_swapped"])
    for kind in (G.EMPTY, G.LEAF, G.BRANCH):
        assert (kind, G.BRANCH, False) in met and (G.BRANCH, kind, False) in met, kind
    for kind in (G.EMPTY, G.LEAF, G.TWIG):
        assert (kind, G.TWIG, True) in met and (G.TWIG, kind, True) in met, kind
    assert (G.LEAF, G.BRANCH, False) in _kinds_met(*K.pairs()["g5_shell"])


def test_collapses_are_what_they_claim(svo):
    one = lambda got: (got["tree"].tolist(), got["twig"].size)
    a, b = K.pairs()["half_spaces"]
    assert one(svo.chunk_combine(a, b, K.UNDER)[0]) == ([G.node(G.LEAF, 5)], 0)                 # two complementary half-spaces: one word
    a, b = K.pairs()["checkerboards"]
    assert a["twig"].size == 64 and b["twig"].size == 64
    for op in (K.MAX, K.UNDER, K.OVER):                                                         # a LEAF at level depth-2 that chains upwards
        got, changed = svo.chunk_combine(a, b, op)
        assert one(got) == ([G.node(G.LEAF, 5)], 0) and changed == 32
    a, b = K.pairs()["g5_root_leaf"]
    assert one(svo.chunk_combine(a, b, K.MAX)[0]) == ([G.node(G.LEAF, 0xFFFF)], 0)
    a, _ = K.pairs()["g5_itself"]
    got, changed = svo.chunk_combine(a, a, K.SUBTRACT)
    assert one(got) == ([0], 0) and changed == S.occupied_cells(a) > 0
    got, changed = svo.chunk_combine(a, K.pairs()["g5_empty"][1], K.INTERSECT)
    assert one(got) == ([0], 0) and changed == S.occupied_cells(a)


def test_the_result_can_be_larger_than_either_input(svo):
    a, b = K.pairs()["two_spheres"]
    got, changed = svo.chunk_combine(a, b, K.MAX)
    assert changed == S.occupied_cells(b) > 0
    for pool in ("tree", "twig"):
        assert got[pool].size > max(a[pool].size, b[pool].size) and got[pool].size <= a[pool].size + b[pool].size
    assert G.is_minimal(got)


def test_untidy_pools_come_back_minimal_and_in_fifo_order(svo):
    untidy, empty = K.pairs()["untidy_empty"]
    assert not G.is_minimal(untidy)
    tidy = svo.chunk_from_grid(G.pools_to_grid(untidy, 4))
    for op in (K.MAX, K.UNDER, K.OVER, K.SUBTRACT):                                             # as A, against an empty B: A, rebuilt
        got, changed = svo.chunk_combine(untidy, empty, op)
        same_pools(got, tidy, f"untidy against empty, op {op}")
        assert changed == 0 and G.is_minimal(got)
    for op in (K.MAX, K.UNDER, K.OVER):                                                         # as B, into an empty A
        got, changed = svo.chunk_combine(empty, untidy, op)
        same_pools(got, tidy, f"empty against untidy, op {op}")
        assert changed == int(np.count_nonzero(G.pools_to_grid(untidy, 4))) == 696


# ---- 5: algebra on pools -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pairings", "g5_shell", "g3_full", "two_spheres", "untidy_itself"])
def test_algebra_on_pools(svo, name):
    a, b = K.pairs()[name]
    ab, ba = svo.chunk_combine(a, b, K.MAX)[0], svo.chunk_combine(b, a, K.MAX)[0]
    same_pools(ab, ba, "MAX(A, B) = MAX(B, A)")
    same_pools(svo.chunk_combine(a, b, K.UNDER)[0], svo.chunk_combine(b, a, K.OVER)[0], "UNDER(A, B) has the grid of OVER(B, A)")
    aa, changed = svo.chunk_combine(a, a, K.MAX)
    same_pools(aa, svo.chunk_from_grid(G.pools_to_grid(a, int(a["depth"]))), "MAX(A, A) = the rebuilt A")
    assert changed == 0
    same_pools(svo.chunk_combine(svo.chunk_combine(a, b, K.SUBTRACT)[0], b, K.INTERSECT)[0], K.one_word(int(a["depth"]), 0), "(A - B) & B is empty")


def test_two_max_calls_with_two_shells_give_the_two_mesh_chunk(svo):
    depth, meshes = S.shared_cases()["two_meshes"]
    first, second = (svo.chunk_from_mesh([m], depth) for m in meshes)
    empty = K.one_word(depth, 0)
    got = svo.chunk_combine(svo.chunk_combine(empty, first, K.MAX)[0], second, K.MAX)[0]
    same_pools(got, svo.chunk_from_mesh(meshes, depth), "MAX of two meshes' shells")
    same_pools(got, S.case_pools("two_meshes"), "... and the model's pools")


# ---- 6: depth 12 and 16 -----------------------------------------------------------------------------------------------------------
_cubes = {}


def deep_cubes(svo, depth):
    """(A, B, c): the two solid cubes of combine_model at `depth`, from the sparse voxeliser and the sparse fill - computed once."""
    if depth not in _cubes:
        ma, mb, c = K.cube_meshes(depth)
        solid = []
        for meshes, material in ((ma, K.MATERIAL_A), (mb, K.MATERIAL_B)):
            chunk, filled = svo.chunk_fill_enclosed(svo.chunk_from_mesh(meshes, depth), material)
            assert filled == F.CUBE_FILLED and S.occupied_cells(chunk) == K.CUBE ** 3
            solid.append(F.freeze(chunk))
        _cubes[depth] = (solid[0], solid[1], c)
    return _cubes[depth]


@pytest.mark.parametrize("opname,op", OPS)
@pytest.mark.parametrize("depth", [12, 16])
def test_deep_cubes_change_the_cells_the_header_says(svo, depth, opname, op):
    a, b, c = deep_cubes(svo, depth)
    got, changed = svo.chunk_combine(a, b, op)
    print(f"depth {depth}, {opname}: changed {changed}, {got['tree'].size} node words, {got['twig'].size // 64} bricks")
    assert changed == K.CUBE_CHANGED[op]
    assert {K.MAX: 17173512, K.OVER: 17173512, K.UNDER: 11473792, K.INTERSECT: 11473792, K.SUBTRACT: 5699720}[op] == K.CUBE_CHANGED[op]
    assert G.is_minimal(got) and F.largest_leaf_edge(got) >= 64 and got["depth"] == depth
    assert got["tree"].size <= a["tree"].size + b["tree"].size and got["twig"].size <= a["twig"].size + b["twig"].size
    rng, n = np.random.default_rng(depth), 1 << depth
    edges = [c - 2, c - 1, c, c + 30, c + 31, c + 62, c + 63, c + 126, c + 127, c + 128, c + 255, c + 256, c + 257, c + 288, c + 289, c + 320, c + 321, c + 384, c + 385]
    points = np.concatenate([rng.integers(c - 8, c + 392, (300, 3)), rng.choice(edges, (200, 3)), rng.integers(0, n, (30, 3)), [[0, 0, 0], [n - 1, n - 1, n - 1]]])
    seen = set()
    for x, y, z in points.tolist():
        va, vb = K.cube_cells(depth, x, y, z)
        want = int(K.f(op, va, vb))
        seen.add((va, vb))
        assert G.voxel_material(got, x, y, z) == want, (x, y, z)
    assert seen == {(0, 0), (K.MATERIAL_A, 0), (0, K.MATERIAL_B), (K.MATERIAL_A, K.MATERIAL_B)}
    W = svo.World.create([got], 1, 1, 1, 128)               # validate_chunk accepts the pools
    assert W.info.max_chunk_depth == depth
    W.destroy()


def filled_sphere12(svo):
    depth, meshes, _ = S.deep_cases()["sphere12"]
    return svo.chunk_fill_enclosed(svo.chunk_from_mesh(meshes, depth), 9)[0]


def test_the_deep_sphere_carved_out_of_a_cube_matches_the_windowed_model(svo):
    """Cube A holds the depth-12 sphere of sparse_mesh_model but for the sphere's last cells in z.  INTERSECT leaves what lies in the
    sphere's window, so sparse_mesh_model.check_against_windows reads it whole; SUBTRACT leaves the rest of the cube around the window: its
    cells are read node by node (combine_model.window_of) and the rest is counted."""
    a, _, c = deep_cubes(svo, 12)
    ball = filled_sphere12(svo)
    windows, changed = K.sphere12_windows(K.INTERSECT)
    got, count = svo.chunk_combine(a, ball, K.INTERSECT)
    kept = sum(int(np.count_nonzero(r)) for _, r, _ in windows)
    assert kept > 40000 and count == K.CUBE ** 3 - kept
    S.check_against_windows(got, [(corner, r) for corner, r, _ in windows])
    assert G.is_minimal(got)
    windows, changed = K.sphere12_windows(K.SUBTRACT)
    got, count = svo.chunk_combine(a, ball, K.SUBTRACT)
    print("cube12 minus sphere12: changed", count, "windowed model", changed)
    assert count == changed == kept
    for corner, r, _ in windows:
        assert np.array_equal(K.window_of(got, corner, r.shape), r), corner
        assert np.array_equal(K.window_of(got, corner, r.shape)[::9, ::9, ::9], np.array(
            [[[G.voxel_material(got, corner[0] + x, corner[1] + y, corner[2] + z) for x in range(0, r.shape[2], 9)] for y in range(0, r.shape[1], 9)]
             for z in range(0, r.shape[0], 9)]))
    assert S.occupied_cells(got) == K.CUBE ** 3 - changed and G.is_minimal(got)
    W = svo.World.create([got], 1, 1, 1, 128)
    W.destroy()


# ---- 7: inputs and refusals ------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_any_work(svo):
    a, b = K.pairs()["g5_shell"]
    ta, ka, tb, kb = a["tree"].copy(), a["twig"].copy(), b["tree"].copy(), b["twig"].copy()

    def desc(tree=ta, twig=ka, depth=5, size=128.0, trees=None, twigs=None):
        d = svo.ChunkDesc()
        d.size, d.depth = size, depth
        d.tree = None if tree is None else tree.ctypes.data_as(C.POINTER(C.c_uint32))
        d.trees = (0 if tree is None else tree.size) if trees is None else trees
        d.twig = None if twig is None else twig.ctypes.data_as(C.POINTER(C.c_uint16))
        d.twigs = (0 if twig is None else twig.size // 64) if twigs is None else twigs
        return d

    B = lambda **kw: desc(**dict(dict(tree=tb, twig=kb), **kw))

    def host(da, db, op=K.MAX, out=True, count=True):
        o, changed = svo.ChunkDesc(), C.c_uint64(77)
        rc = svo.lib.svo_chunk_combine(None if da is None else C.byref(da), None if db is None else C.byref(db), op, C.byref(o) if out else None,
                                       C.byref(changed) if count else None)
        assert rc == 0 or (not o.tree and not o.twig and o.trees == 0 and changed.value == 77)     # a refusal leaves *out and the count alone
        if rc == 0:
            svo.lib.svo_chunk_free(C.byref(o))
        return rc

    def both(bad):
        """The status of `bad` as a against a good b, which is also its status as b against a good a."""
        rc = host(bad, B())
        assert host(desc(), bad) == rc
        return rc

    assert host(desc(), B()) == 0 and host(desc(), B(), count=False) == 0       # changed_out may be NULL
    d = desc()
    assert host(d, d) == 0                                                      # a == b is allowed
    assert host(None, B()) == -1 and host(desc(), None) == -1 and host(desc(), B(), out=False) == -1
    assert host(desc(), B(), op=-1) == -1 and host(desc(), B(), op=5) == -1
    d, e = desc(), B()
    assert svo.lib.svo_chunk_combine(C.byref(d), C.byref(e), 0, C.byref(d), None) == -1 and svo.lib.svo_chunk_combine(C.byref(d), C.byref(e), 0, C.byref(e), None) == -1
    assert both(desc(tree=None)) == -1 and both(desc(twig=None, twigs=ka.size // 64)) == -1 and both(desc(trees=0)) == -1
    for size in (0.0, -1.0, float("nan"), float("inf")):
        assert host(desc(size=size), B()) == -1
        assert host(desc(), B(size=size)) == 0                                  # B's frame is not consulted
    # what svo_world_create's validation refuses
    assert both(desc(trees=ta.size - 1)) == -1              # not 1 + 8k node words
    bad = ta.copy(); bad[0] = G.node(G.BRANCH, 0)
    assert both(desc(tree=bad)) == -1                       # a BRANCH that does not point forward
    bad = ta.copy(); bad[0] = G.node(G.BRANCH, ta.size)
    assert both(desc(tree=bad)) == -1                       # ... or beyond the pool
    bad = ta.copy(); bad[int(np.nonzero(ta >> 30 == G.TWIG)[0][0])] = G.node(G.TWIG, ka.size // 64)
    assert both(desc(tree=bad)) == -1                       # a TWIG beyond the bricks
    two = np.array([G.node(G.BRANCH, 1)] + [G.node(G.BRANCH, 9)] * 2 + [0] * 14, np.uint32)
    assert both(desc(tree=two, twig=None)) == -1            # a child block referenced twice
    deep = np.array([G.node(G.BRANCH, 1)] + [0] * 8, np.uint32)
    assert host(desc(tree=deep, twig=None, depth=2), B(tree=deep, twig=None, depth=2)) == -1      # a BRANCH below level depth-2
    # SVO_ERR_UNSUPPORTED: depths that differ, a depth outside [2, 16], a brick above level depth-2
    one = np.array([G.node(G.LEAF, 3)], np.uint32)
    L = lambda depth: desc(tree=one, twig=None, depth=depth)
    assert host(L(5), L(6)) == -6 and host(L(16), L(2)) == -6 and host(desc(), L(4)) == -6
    for depth in (0, 1, 17, 30):
        assert host(L(depth), L(depth)) == -6
    assert host(L(16), L(16)) == 0 and host(L(2), L(2)) == 0
    shallow = np.array([G.node(G.TWIG, 0)], np.uint32)
    T = lambda depth: desc(tree=shallow, twig=ka[:64].copy(), depth=depth)
    assert host(T(2), T(2)) == 0 and host(T(3), L(3)) == -6 and host(L(3), T(3)) == -6
    # the device form: argument errors first, then a world that is not uploaded
    b = dict(b, position=(128.0, 0.0, 0.0))
    world = svo.World.create([a, b], 2, 1, 1, 128)
    dev = lambda chunk=0, src=world._h, src_chunk=1, op=0, w=world._h: svo.lib.svo_world_chunk_combine(w, chunk, src, src_chunk, op, None)
    assert dev(w=None) == -1 and dev(src=None) == -1 and dev(chunk=-1) == -1 and dev(chunk=2) == -1 and dev(src_chunk=-1) == -1 and dev(src_chunk=2) == -1
    assert dev(op=-1) == -1 and dev(op=5) == -1
    assert dev() == -5
    same_pools(world.chunk(0), a, "the world after the refusals")
    same_pools(world.chunk(1), b, "the world after the refusals, the source")
    world.destroy()
    with pytest.raises(svo.SvoError) as e:
        svo.chunk_combine(a, b, 9)
    assert e.value.code == -1
