"""What the three host entry points that validate a chunk's pools - svo_world_create, svo_chunk_fill_enclosed and svo_chunk_combine (the
bad pools as a and as b) - answer to one table of small hand-written depth-3 and depth-4 pools: the return code and the whole message.
The three share one forward pass (csrc/chunk_pools.h: pools_walk) and differ in their codes and in when a shallow TWIG outranks a
malformed word; the expected values were recorded from the library before the pass was shared, so the table pins those differences.
An accepted pool leaves no message to compare: its row holds None.  Then the svo_chunk_desc the four producers hand out.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import grid_model as G

E, B, T = G.node(G.EMPTY), (lambda off: G.node(G.BRANCH, off)), (lambda off: G.node(G.TWIG, off))
INVALID, MALFORMED, UNSUPPORTED = -1, -4, -6

# name: (depth, node words, bricks)
CASES = {
    "back_edge":             (4, [B(9)] + [E] * 8 + [B(1)] + [E] * 7, 0),
    "offset_past_the_pool":  (3, [B(9)] + [E] * 8, 0),
    "offset_not_1_plus_8k":  (4, [B(2)] + [E] * 16, 0),
    "block_referenced_twice": (4, [B(1)] + [B(9), B(9)] + [E] * 6 + [E] * 8, 0),
    "branch_at_depth_2":     (3, [B(1)] + [B(9)] + [E] * 7 + [E] * 8, 0),
    "twig_past_the_bricks":  (3, [B(1)] + [T(1)] + [E] * 7, 1),
    "shallow_twig":          (4, [B(1)] + [T(0)] + [E] * 7, 1),
    "shallow_then_malformed": (4, [B(1)] + [T(0), B(2)] + [E] * 6 + [E] * 8, 1),
    "malformed_then_shallow": (4, [B(1)] + [B(2), T(0)] + [E] * 6 + [E] * 8, 1),
    "orphan_garbage":        (4, [B(1)] + [G.node(G.LEAF, 3)] + [E] * 7 + [0xFFFFFFFF] * 8, 0),
}
ENTRIES = ("create", "fill", "combine_a", "combine_b")

FORWARD = "BRANCH offset outside pool or not a forward 8-block"
TWICE, DEEP, BRICK = "child block referenced twice", "BRANCH below level depth-2", "TWIG offset outside brick pool"
SHALLOW = "a TWIG above level depth-2 (a sparsely refined chunk) is not supported"


def _row(why, fill_shallow=False, combine_shallow=False):
    """The four answers to a pool whose first malformed word is `why` (None: none); *_shallow: that entry point answers the shallow TWIG."""
    fill, comb = "svo_chunk_fill_enclosed: ", "svo_chunk_combine: "
    return {
        "create": (MALFORMED, f"svo_world_create: chunk 0: {why}") if why else (0, None),
        "fill": (UNSUPPORTED, fill + SHALLOW) if fill_shallow else (INVALID, fill + why) if why else (0, None),
        "combine_a": (INVALID, comb + f"chunk a: {why}") if why else (UNSUPPORTED, comb + SHALLOW) if combine_shallow else (0, None),
        "combine_b": (INVALID, comb + f"chunk b: {why}") if why else (UNSUPPORTED, comb + SHALLOW) if combine_shallow else (0, None),
    }


EXPECT = {
    "back_edge": _row(FORWARD),
    "offset_past_the_pool": _row(FORWARD),
    "offset_not_1_plus_8k": _row(FORWARD),
    "block_referenced_twice": _row(TWICE),
    "branch_at_depth_2": _row(DEEP),
    "twig_past_the_bricks": _row(BRICK),
    "shallow_twig": _row(None, fill_shallow=True, combine_shallow=True),
    "shallow_then_malformed": _row(FORWARD, fill_shallow=True),
    "malformed_then_shallow": _row(FORWARD),
    "orphan_garbage": _row(None),
}


def _desc(svo, depth, tree, twig):
    d = svo.ChunkDesc()
    d.size, d.depth = 128.0, depth
    d.tree, d.trees = tree.ctypes.data_as(C.POINTER(C.c_uint32)), tree.size
    d.twig, d.twigs = twig.ctypes.data_as(C.POINTER(C.c_uint16)), twig.size // 64
    return d


def observe(svo, name, entry):
    """(return code, message or None) of `entry` for the pools of case `name`."""
    depth, words, bricks = CASES[name]
    tree, twig = np.array(words, np.uint32), (np.arange(64 * bricks, dtype=np.uint16) % 7)
    good_tree, none = np.array([G.node(G.LEAF, 3)], np.uint32), np.zeros(0, np.uint16)
    bad, good, out = _desc(svo, depth, tree, twig), _desc(svo, depth, good_tree, none), svo.ChunkDesc()
    if entry == "create":
        handle = C.c_void_p()
        rc = svo.lib.svo_world_create(C.byref(bad), 1, 1, 1, 1, 128, (C.c_int * 3)(0, 0, 0), C.byref(handle))
        if rc == 0:
            svo.lib.svo_world_destroy(handle)
    elif entry == "fill":
        rc = svo.lib.svo_chunk_fill_enclosed(C.byref(bad), 9, C.byref(out), None)
    else:
        a, b = (bad, good) if entry == "combine_a" else (good, bad)
        rc = svo.lib.svo_chunk_combine(C.byref(a), C.byref(b), 0, C.byref(out), None)
    if rc == 0:
        if entry != "create":
            svo.lib.svo_chunk_free(C.byref(out))
        return 0, None
    assert not out.tree and not out.twig and out.trees == 0                    # a refusal leaves *out alone
    return rc, svo.lib.svo_last_error().decode()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(CASES))
def test_every_entry_point_answers_the_recorded_code_and_message(svo, name, entry):
    got = observe(svo, name, entry)
    print(name, entry, got)
    assert got == EXPECT[name][entry]


def test_the_four_producers_fill_in_every_field_of_the_desc(svo):
    """One tiny input each, all of them without a brick: _pad == 0 over what the caller left there, the caller's position, size and
    depth, and a brick pool that is allocated although it holds nothing."""
    position, size = (C.c_float * 3)(1.0, 2.0, 3.0), 64.0

    def fresh():
        d = svo.ChunkDesc()
        d._pad = 0xDEAD
        return d

    def check(d, depth, who):
        assert d._pad == 0 and tuple(d.position) == (1.0, 2.0, 3.0) and d.size == size and d.depth == depth, who
        assert d.trees == 1 and d.twigs == 0 and bool(d.tree) and bool(d.twig), who
        svo.lib.svo_chunk_free(C.byref(d))

    d = fresh()
    assert svo.lib.svo_chunk_from_grid(np.zeros(4 ** 3, np.uint16).ctypes.data, 2, position, size, C.byref(d)) == 0
    check(d, 2, "svo_chunk_from_grid")
    d = fresh()
    assert svo.lib.svo_chunk_from_mesh(None, 0, 5, position, size, C.byref(d)) == 0
    check(d, 5, "svo_chunk_from_mesh")
    tree, none = np.array([G.node(G.LEAF, 3)], np.uint32), np.zeros(0, np.uint16)
    src = _desc(svo, 3, tree, none)
    src.position[:], src.size = [1.0, 2.0, 3.0], size
    d = fresh()
    assert svo.lib.svo_chunk_fill_enclosed(C.byref(src), 9, C.byref(d), None) == 0
    check(d, 3, "svo_chunk_fill_enclosed")
    other = _desc(svo, 3, tree, none)                                          # (b's frame is not consulted)
    d = fresh()
    assert svo.lib.svo_chunk_combine(C.byref(src), C.byref(other), 0, C.byref(d), None) == 0
    check(d, 3, "svo_chunk_combine")
