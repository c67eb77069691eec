"""svo_world_compact / svo_world_coarsen (Ocroot::defragcopy / Ocroot::lodmm, src/Octree.cpp:445-765) on worlds that are not
uploaded: the host path (csrc/compact.cpp) must leave, index for index, what the test model (tests/lod_model.py, a restatement
of the reference's recursions) leaves.  Chunks come from the oracle's restatement of the reference's edits (orc_build /
orc_destroy append blocks and bricks, leaving garbage behind).  CPU only."""
import ctypes as C

import numpy as np
import pytest

import lod_model as M

B, T, L = 2 << 30, 3 << 30, 1 << 30


def oracle_edit(oracle, O, chunk, op, lo, hi, material):
    """op 0 build, 1 destroy, 2 replace (destroy then build), as svo_world_edit_box."""
    dt, dw = oracle.Delta(), oracle.Delta()
    root = C.byref(O.w.chunk[chunk])
    if op in (1, 2):
        oracle.lib.orc_destroy(root, oracle.vec3(lo), oracle.vec3(hi), C.byref(dt), C.byref(dw))
    if op in (0, 2):
        oracle.lib.orc_build(root, oracle.vec3(lo), oracle.vec3(hi), material, C.byref(dt), C.byref(dw))


def random_edits(oracle, O, chunk, rng, count, depth, origin=(0.0, 0.0, 0.0), size=128.0):
    """`count` random build / destroy / replace boxes, a voxel to half a chunk, on and off the voxel lattice."""
    voxel = size / (1 << depth)
    org = np.asarray(origin, np.float64)
    for _ in range(count):
        op = int(rng.integers(0, 3))
        edge = float(rng.choice([voxel, 3 * voxel, 7.3, 20.0, 64.0]))
        lo = rng.uniform(-4, size - 8, 3)
        if rng.random() < 0.5:
            lo = np.floor(lo / voxel) * voxel
        hi = lo + edge * rng.uniform(0.3, 1.0, 3)
        oracle_edit(oracle, O, chunk, op, (org + lo).astype(np.float32), (org + hi).astype(np.float32), int(rng.integers(1, 8)))


def edited_world(oracle, depth, seed, edits=15, ccm=(0, 0, 0)):
    O = oracle.OracleWorld.generate(1, 1, 1, 128, depth, chunkcoordmin=ccm)
    origin = tuple(128.0 * c for c in ccm)
    random_edits(oracle, O, 0, np.random.default_rng(seed), edits, depth, origin)
    return O


def same_pools(got, want, what):
    assert int(got["depth"]) == int(want["depth"]), f"{what}: depth {got['depth']} != {want['depth']}"
    assert got["tree"].size == want["tree"].size, f"{what}: {got['tree'].size} node words, model {want['tree'].size}"
    assert got["twig"].size == want["twig"].size, f"{what}: {got['twig'].size // 64} bricks, model {want['twig'].size // 64}"
    bad = np.nonzero(got["tree"] != want["tree"])[0]
    assert bad.size == 0, f"{what}: node words differ at {bad[:8]}"
    assert np.array_equal(got["twig"], want["twig"]), f"{what}: bricks differ"


def chunk_dict(tree, twig=(), depth=4, pos=(0.0, 0.0, 0.0)):
    return dict(position=pos, size=128.0, depth=depth, tree=np.array(tree, np.uint32), twig=np.array(twig, np.uint16))


def host_world(svo, chunks, dims=(1, 1, 1), ccm=(0, 0, 0)):
    return svo.World.create(chunks, *dims, 128, ccm)


def leaf_centres(depth, origin=(0.0, 0.0, 0.0), size=128.0):
    n = 1 << depth
    i = (np.arange(n, dtype=np.float32) + np.float32(0.5)) * np.float32(size / n)
    z, y, x = np.meshgrid(i, i, i, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1) + np.asarray(origin, np.float32)


# ---- known answers on hand-written trees -----------------------------------------------------------------------

@pytest.mark.parametrize("name,chunk,want_tree,want_twig", [
    ("uniform brick -> LEAF", chunk_dict([T | 0], [5] * 64, depth=2), [L | 5], []),
    ("uniform empty brick -> EMPTY", chunk_dict([T | 0], [0] * 64, depth=2), [0], []),
    ("8 x LEAF 0 -> EMPTY", chunk_dict([B | 1] + [L | 0] * 8), [0], []),
    ("8 x LEAF 4 -> LEAF 4", chunk_dict([B | 1] + [L | 4] * 8), [L | 4], []),
    ("LEAF 0 alone stays LEAF 0", chunk_dict([B | 1] + [L | 0] + [0] * 7), [B | 1] + [L | 0] + [0] * 7, []),
    ("garbage dropped", chunk_dict([B | 9] + [L | 3] * 8 + [T | 1] + [0] * 6 + [L | 2], [7] * 64 + list(range(64))),
     [B | 1, T | 0] + [0] * 6 + [L | 2], list(range(64))),
    ("a brick referenced twice is copied twice", chunk_dict([B | 1, T | 0, T | 0] + [0] * 6, list(range(64))),
     [B | 1, T | 0, T | 1] + [0] * 6, list(range(64)) * 2),
])
def test_known_answers(svo, name, chunk, want_tree, want_twig):
    got = M.compact(chunk)
    assert got["tree"].tolist() == want_tree, name
    assert got["twig"].tolist() == want_twig, name
    W = host_world(svo, [chunk])
    assert W.compact(0) == svo.SVO_OK
    same_pools(W.chunk(0), got, name)
    W.destroy()


def test_two_level_branch_of_leaves_becomes_a_brick():
    """At level 0 of a depth-6 chunk (three levels above depth-2): a BRANCH whose subtree is two levels of EMPTY / LEAF nodes
    becomes one brick sampled at the cell centres; below a kept BRANCH the brick takes the first brick index."""
    inner = [L | 2, 0, L | 3, 0, 0, 0, 0, 0]
    c = chunk_dict([B | 1, B | 9] + [L | 1] * 7 + inner, depth=6)
    got = M.compact(c)
    assert got["tree"].tolist() == [T | 0]
    cells = got["twig"].reshape(4, 4, 4)            # [z][y][x]
    assert cells[0, 0, 0] == 2 and cells[0, 0, 1] == 0 and cells[0, 1, 0] == 3 and cells[1, 1, 1] == 0
    assert np.all(cells[2:] == 1) and np.all(cells[:, 2:] == 1) and np.all(cells[:, :, 2:] == 1)
    # one level further down: the root stays a BRANCH (its subtree is three levels deep)
    c2 = chunk_dict([B | 1, B | 9] + [T | 0] * 7 + [B | 17] + [L | 1] * 7 + inner, [0] * 63 + [1], depth=8)
    got2 = M.compact(c2)
    assert got2["tree"].tolist() == [B | 1] + [T | k for k in range(8)]
    assert np.array_equal(got2["twig"][:64], got["twig"])


def test_uniform_resampled_brick_folds():
    c = chunk_dict([B | 1, B | 9] + [L | 4] * 7 + [L | 4] * 8, depth=6)
    assert M.compact(c)["tree"].tolist() == [L | 4]


def test_majority_tie_goes_to_the_first_value_seen(svo):
    """A depth-3 chunk coarsened to depth 2: the root (level depth-3) becomes a brick; one cell sees the 2x2x2 cells 7 7 3 3 3 3 7 7
    (z, y, x order: a 4:4 tie) -> 7; another 2 2 2 5 5 5 9 9 -> 2 (3:3 tie, 2 first)."""
    brick = np.zeros(64, np.uint16)
    vals = [7, 7, 3, 3, 3, 3, 7, 7]
    for k, v in enumerate(vals):
        brick[M.word(k & 1, (k >> 1) & 1, k >> 2)] = v
    vals2 = [2, 2, 2, 5, 5, 5, 9, 9]
    for k, v in enumerate(vals2):
        brick[M.word(2 + (k & 1), (k >> 1) & 1, k >> 2)] = v
    c = chunk_dict([B | 1, T | 0, L | 6] + [0] * 6, brick, depth=3)
    for full in (True, False):
        got = M.coarsen(c, full=full)
        assert got["depth"] == 2 and got["tree"].tolist() == [T | 0]
        cells = got["twig"]
        assert cells[M.word(0, 0, 0)] == 7 and cells[M.word(1, 0, 0)] == 2
        assert cells[M.word(2, 0, 0)] == 6 and cells[M.word(3, 1, 1)] == 6 and cells[M.word(0, 2, 0)] == 0
    W = host_world(svo, [c])
    assert W.coarsen(0) == svo.SVO_OK
    same_pools(W.chunk(0), M.coarsen(c), "tie")
    W.destroy()


def test_coarsened_empty_brick_is_kept():
    c = chunk_dict([B | 1] + [0] * 8, depth=3)
    got = M.coarsen(c)
    assert got["tree"].tolist() == [T | 0] and not got["twig"].any()


def test_misra_gries_weighted_counts():
    c = M.MisraGries(2)
    c.count(1, 5); c.count(2, 3); c.count(3, 4)         # no free slot: slot 1 (count 3 < 4) is replaced, all drop by 3
    assert c.keys == [1, 3] and c.A == [2, 1] and c.majority() == 1
    c = M.MisraGries(2)
    c.count(1, 2); c.count(2, 5); c.count(3, 9)         # the search starts at k = 1: slot 0 (count 2) is never replaced
    assert c.keys == [1, 3] and c.A == [-3, 4] and c.majority() == 3


# ---- the model's own properties ---------------------------------------------------------------------------------

def test_compact_keeps_the_material_at_every_leaf_voxel_centre(oracle):
    O = edited_world(oracle, 5, 11, edits=12)
    before = O.chunk(0)
    after = M.compact(before)
    assert after["tree"].size < before["tree"].size
    for p in leaf_centres(5):
        assert M.material_at(before, p) == M.material_at(after, p), p


def test_a_coarsened_cell_is_the_majority_of_its_8_voxels(oracle):
    O = edited_world(oracle, 5, 12, edits=12)
    before = O.chunk(0)
    after = M.coarsen(before)
    assert after["depth"] == 4
    q = np.float32(128.0 / 32)
    offs = [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    for p in leaf_centres(4):
        lo = p - q                                      # the coarse cell's low corner; its 8 voxels' centres at + q/2 + (0|1) q
        vals = [M.material_at(before, lo + np.float32(0.5) * q + np.array(o, np.float32) * q) for o in offs]
        assert M.material_at(after, p) == M.short_majority(vals), p


@pytest.mark.parametrize("depth,seed", [(3, 1), (4, 2), (5, 3), (6, 4)])
def test_short_form_of_the_majority_agrees_with_the_counter(oracle, depth, seed):
    O = edited_world(oracle, depth, seed, edits=10)
    c = O.chunk(0)
    same_pools(M.coarsen(c, full=False), M.coarsen(c, full=True), f"depth {depth}")


# ---- the host path against the model ----------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [2, 3, 4, 5, 6, 7, 8])
def test_host_path_equals_the_model_after_random_edits(svo, oracle, depth):
    O = edited_world(oracle, depth, 100 + depth, edits=15)
    c = O.chunk(0)
    W = host_world(svo, [c])
    assert W.compact(0) == svo.SVO_OK
    same_pools(W.chunk(0), M.compact(c), f"compact, depth {depth}")
    if depth > 2:
        W2 = host_world(svo, [c])
        assert W2.coarsen(0) == svo.SVO_OK
        same_pools(W2.chunk(0), M.coarsen(c, full=depth <= 5), f"coarsen, depth {depth}")
        assert W2.info.max_chunk_depth == depth - 1
        W2.destroy()
    W.destroy()


def test_host_path_negative_chunk_coordinates(svo, oracle):
    O = edited_world(oracle, 6, 7, edits=15, ccm=(-1, 0, -2))
    c = O.chunk(0)
    assert c["position"][0] < 0
    W = host_world(svo, [c], ccm=(-1, 0, -2))
    W.compact(0)
    same_pools(W.chunk(0), M.compact(c), "negative coordinates, compact")
    W.coarsen(0)
    same_pools(W.chunk(0), M.coarsen(M.compact(c), full=False), "negative coordinates, compact then coarsen")
    W.destroy()


def test_host_path_coarse_depth_world(svo):
    """Sparse refinement (coarse_depth): bricks above level depth-2 outside the refine box go through defragcopy unchanged."""
    G = svo.World.generate(2, 1, 1, 128, 7, coarse_depth=4, refine_box=((0, 0, 0), (60, 128, 60)))
    chunks = [G.chunk(i) for i in range(2)]
    G.destroy()
    W = host_world(svo, chunks, dims=(2, 1, 1))
    for i in range(2):
        W.compact(i)
        same_pools(W.chunk(i), M.compact(chunks[i]), f"coarse_depth chunk {i}, compact")
        W.coarsen(i)
        same_pools(W.chunk(i), M.coarsen(M.compact(chunks[i]), full=False), f"coarse_depth chunk {i}, coarsen")
    W.destroy()


def test_repeated_coarsening_down_to_depth_2_then_refusal(svo, oracle):
    O = edited_world(oracle, 6, 5, edits=10)
    c = O.chunk(0)
    W = host_world(svo, [c])
    want = c
    for d in (5, 4, 3, 2):
        assert W.coarsen(0) == svo.SVO_OK
        want = M.coarsen(want, full=d <= 4)
        same_pools(W.chunk(0), want, f"coarsened to depth {d}")
    with pytest.raises(svo.SvoError) as e:
        W.coarsen(0)
    assert e.value.code == -6 and "depth 2" in str(e.value)
    same_pools(W.chunk(0), want, "after the refusal")
    W.destroy()


def test_compacting_an_edited_chunk_gives_fewer_trees(svo, oracle):
    O = edited_world(oracle, 7, 9, edits=25)
    c = O.chunk(0)
    W = host_world(svo, [c])
    before = W.info.total_trees
    W.compact(0)
    assert W.info.total_trees < before
    again = W.chunk(0)
    W.compact(0)                                        # compacting a compacted chunk changes nothing
    same_pools(W.chunk(0), again, "second compact")
    W.destroy()


def test_argument_checks(svo):
    c = chunk_dict([B | 1] + [L | 0] + [0] * 7)
    W = host_world(svo, [c])
    for bad in (-1, 1, 7):
        for f in (W.compact, W.coarsen):
            with pytest.raises(svo.SvoError) as e:
                f(bad)
            assert e.value.code == -1
    assert svo.lib.svo_world_compact(None, 0) == -1 and svo.lib.svo_world_coarsen(None, 0) == -1
    D2 = host_world(svo, [chunk_dict([T | 0], list(range(64)), depth=2)])
    with pytest.raises(svo.SvoError) as e:
        D2.coarsen(0)
    assert e.value.code == -6
    assert D2.chunk(0)["tree"].tolist() == [T | 0] and D2.info.max_chunk_depth == 2
    D2.destroy()
    same_pools(W.chunk(0), dict(c), "untouched")
    W.destroy()
