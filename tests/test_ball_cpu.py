"""svo_world_edit_ball / svo_world_edit_ball_all without a device: the model's skeleton against the Python twin's box edits, the
ball against a pass over all cells (the monotonicity argument of DESIGN.md 6n), known answers, and the argument checks that are
settled before any device work.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import ball_model as B
import grid_model as G

F = np.float32
P = B.P
POSITION = (128.0, 0.0, -128.0)                              # an integer position: the chunk's geometry is exact


def pools_equal(a: P.Chunk, b: P.Chunk, what):
    assert a.trees == b.trees and a.twigs == b.twigs, f"{what}: pool sizes differ"
    assert a.tree == b.tree, f"{what}: node words differ"
    assert np.array_equal(B.pools_of(a)["twig"], B.pools_of(b)["twig"]), f"{what}: bricks differ"
    assert (a.treestoragesize, a.twigstoragesize) == (b.treestoragesize, b.twigstoragesize), f"{what}: storage sizes differ"


# ---- 1. the skeleton against the twin ----------------------------------------------------------------------------------------------
BOXES = [((20, 60, 20), (70, 110, 50)),                      # in the air, on the lattice
         ((0, 0, 0), (128, 45, 30)),                         # a slab through terrain and water
         ((100.3, 2.7, 40.1), (150.9, 70.2, 90.6)),          # off the lattice, beyond the chunk
         ((64, 4, 64), (68, 8, 68)),                         # one voxel of a depth-5 chunk
         ((63.99, 5.99, 63.99), (64.01, 6.01, 64.01)),       # straddles a node corner and the water plane
         ((0, 0, 0), (128, 128, 128)),                       # the whole chunk
         ((500, 500, 500), (600, 600, 600))]                 # misses


@pytest.mark.parametrize("op", [B.BUILD, B.DESTROY, B.REPLACE], ids=["build", "destroy", "replace"])
def test_with_box_predicates_the_model_is_the_twin(svo, op):
    """A run of box edits on one depth-5 chunk, the twin's Chunk.build / destroy / replace and the model side by side."""
    c = svo.World.generate(1, 1, 1, 128, 5).chunk(0)
    twin, model = P.Chunk(c["position"], c["size"], c["depth"], c["tree"], c["twig"]), B.chunk_of(c)
    changed = 0
    for k, (lo, hi) in enumerate(BOXES):
        before = list(twin.tree), [list(b) for b in twin.twig]
        if op == B.BUILD:
            twin.build(lo, hi, 5 + k)
        elif op == B.DESTROY:
            twin.destroy(lo, hi)
        else:
            twin.replace(lo, hi, 5 + k)
        B.edit(model, op, B.Box(lo, hi), 5 + k)
        pools_equal(model, twin, f"op {op}, box {k}")
        changed += before != (twin.tree, twin.twig)
    assert changed >= 4, "the edits changed nothing: the check is empty"


# ---- 2. the ball against a pass over all cells --------------------------------------------------------------------------------------
def balls(depth):
    voxel = 128.0 / (1 << depth)
    x, y, z = POSITION
    return [((x + 64, y + 64, z + 64), 0.3 * voxel),                    # below a voxel, on a corner of eight cells
            ((x + 64 + 0.4 * voxel, y + 30.3, z + 70.9), 0.3 * voxel),  # below a voxel, inside one cell
            ((x + 40, y + 80, z + 24), voxel),                          # on the lattice: tangent cells
            ((x + 41.3, y + 77.7, z + 23.1), 9.6),
            ((x + 64, y + 64, z + 64), 32.0),
            ((x + 100.5, y + 20.25, z + 90.75), 37.3),
            ((x - 10, y + 64, z + 64), 25.0),                           # centre outside, poking in
            ((x + 140, y + 140, z - 12), 40.0),                         # outside a corner
            ((x + 64, y + 64, z + 64), 70.0),                           # cuts every face
            ((x + 60, y + 70, z + 64), 300.0),                          # beyond the chunk: everything
            ((x + 400, y + 64, z + 64), 100.0)]                         # misses


@pytest.fixture(scope="module")
def blobs(svo):
    out = {}
    for depth in (5, 6):
        grid = B.blob_grid(depth, depth)
        chunk = svo.chunk_from_grid(grid, position=POSITION, size=128.0)
        assert B.node_kinds(chunk) == {B.EMPTY, B.LEAF, B.TWIG, B.BRANCH}
        assert np.array_equal(G.pools_to_grid(chunk, depth), grid)
        out[depth] = (grid, chunk)
    return out


@pytest.mark.parametrize("depth", [5, 6])
@pytest.mark.parametrize("op", [B.BUILD, B.DESTROY, B.REPLACE], ids=["build", "destroy", "replace"])
def test_the_ball_edit_changes_exactly_the_touched_cells(svo, blobs, depth, op):
    grid, chunk = blobs[depth]
    n_changed = n_touched_unchanged = n_untouched = 0
    for k, (centre, radius) in enumerate(balls(depth)):
        ball = B.Ball(centre, radius)
        root = B.edit(B.chunk_of(chunk), op, ball, 9)
        got = B.pools_of(root)
        after = G.pools_to_grid(got, depth)
        want, hit = B.brute_force(grid, POSITION, 128.0, op, ball, 9)
        bad = np.argwhere(after != want)
        assert bad.size == 0, f"depth {depth}, op {op}, ball {k}: {len(bad)} cells differ, first (z, y, x) {bad[:4].tolist()}"
        assert np.array_equal(after[~hit], grid[~hit]), "a cell the ball does not touch changed"
        n_changed += int((after != grid).sum())
        n_touched_unchanged += int((hit & (after == grid)).sum())
        n_untouched += int((~hit).sum())
        W = svo.World.create([got], 1, 1, 1, 128, (1, 0, -1))          # svo_world_create's validation accepts the pools
        assert W.info.total_trees == got["tree"].size
        W.destroy()
    assert n_changed > 1000 and n_untouched > 1000
    if op == B.BUILD:
        assert n_touched_unchanged > 1000                       # solid cells a build leaves alone


# ---- 3. known answers ---------------------------------------------------------------------------------------------------------------
def uniform_chunk(word, depth=5):
    return P.Chunk((0, 0, 0), 128.0, depth, [word], [])


def test_a_ball_that_holds_the_chunk():
    big = B.Ball((64, 64, 64), 200.0)
    c = B.edit(uniform_chunk(P.node_make(B.EMPTY, 0)), B.BUILD, big, 7)
    assert c.tree == [P.node_make(B.LEAF, 7)] and c.trees == 1 and c.twigs == 0
    c = B.edit(uniform_chunk(P.node_make(B.LEAF, 3)), B.DESTROY, big)
    assert c.tree == [P.node_make(B.EMPTY, 0)] and c.trees == 1 and c.twigs == 0
    c = B.edit(uniform_chunk(P.node_make(B.LEAF, 3)), B.REPLACE, big, 7)
    assert c.tree == [P.node_make(B.LEAF, 7)] and c.trees == 1
    # the farthest corner decides: sqrt(3) * 64 = 110.85...
    assert B.edit(uniform_chunk(0), B.BUILD, B.Ball((64, 64, 64), 110.9), 7).tree == [P.node_make(B.LEAF, 7)]
    assert B.edit(uniform_chunk(0), B.BUILD, B.Ball((64, 64, 64), 110.8), 7).trees > 1
    # R2 = +inf: everything is touched and inside
    assert B.edit(uniform_chunk(0), B.BUILD, B.Ball((1e30, 0, 0), 3e38), 7).tree == [P.node_make(B.LEAF, 7)]


def test_a_ball_that_misses_changes_nothing(blobs):
    _, chunk = blobs[5]
    for op in (B.BUILD, B.DESTROY, B.REPLACE):
        start = B.chunk_of(chunk)
        for centre, radius in (((POSITION[0] + 400, 64, -64), 100.0), ((POSITION[0] - 8.01, 64, -64), 8.0), ((POSITION[0] + 64, 128 + 6, -128 - 6), 8.4)):
            pools_equal(B.edit(B.chunk_of(chunk), op, B.Ball(centre, radius), 9), start, f"op {op}, ball at {centre}")


def test_tangent_cells_are_edited():
    """Centre (64, 64, 64), radius 8, voxel 4: along each of the six axis directions the cells whose near face lies at distance exactly
    8 are edited (the closed rule), the cells behind them are not, and one ulp less of radius loses them."""
    def built(radius):
        c = B.edit(uniform_chunk(P.node_make(B.EMPTY, 0)), B.BUILD, B.Ball((64, 64, 64), radius), 7)
        return G.pools_to_grid(B.pools_of(c), 5)
    g = built(8.0)
    less = built(np.nextafter(F(8.0), F(0.0)))
    mid = 16                                                    # cell index of coordinate 64
    for axis in range(3):
        for tangent, beyond in ((mid + 2, mid + 3), (mid - 3, mid - 4)):
            for a in (mid - 1, mid):                            # the cells on either side of the lattice planes through the centre
                for b in (mid - 1, mid):
                    at = lambda i: tuple(np.roll([i, a, b], axis))
                    assert g[at(tangent)] == 7 and g[at(beyond)] == 0, (axis, tangent)
                    assert less[at(tangent)] == 0, (axis, tangent)
    lo, hi = B.cell_boxes((0, 0, 0), 128.0, 5)
    assert np.array_equal(g != 0, np.broadcast_to(B.Ball((64, 64, 64), 8.0).touch(lo, hi), g.shape))
    assert int((g != 0).sum()) - int((less != 0).sum()) == 24   # four cells share each of the six tangent faces


def test_the_chunk_list_of_edit_ball_all():
    positions = [(128.0 * x, 0.0, 128.0 * z) for z in range(2) for x in range(2)]      # World::index order of a 2 x 1 x 2 world
    assert B.touched_chunks(positions, 128, B.Ball((64, 64, 64), 10.0)) == [0]
    assert B.touched_chunks(positions, 128, B.Ball((120, 64, 64), 8.0)) == [0, 1]       # tangent to the seam: closed
    assert B.touched_chunks(positions, 128, B.Ball((120, 64, 64), 7.99)) == [0]
    assert B.touched_chunks(positions, 128, B.Ball((128, 64, 128), 1.0)) == [0, 1, 2, 3]
    assert B.touched_chunks(positions, 128, B.Ball((122, 64, 122), 8.0)) == [0, 1, 2]   # the diagonal chunk is sqrt(72) away
    assert B.touched_chunks(positions, 128, B.Ball((128, 300, 128), 100.0)) == []
    assert B.touched_chunks(positions, 128, B.Ball((-500, 64, 64), 1000.0)) == [0, 1, 2, 3]


# ---- 4. argument checks, before any device work ------------------------------------------------------------------------------------
def test_argument_checks_precede_any_device_work(svo):
    H = svo.World.generate(2, 1, 1, 128, 4)                     # not uploaded
    vec = lambda v: (C.c_float * 3)(*v)
    good = vec((10.0, 10.0, 10.0))
    chunks, n = (C.c_int * 4)(*[-7] * 4), C.c_int(-7)
    one = lambda w, chunk, op, c, r: svo.lib.svo_world_edit_ball(w, chunk, op, c, r, C.c_uint16(5))

    def every(w, op, c, r):
        rc = svo.lib.svo_world_edit_ball_all(w, op, c, r, C.c_uint16(5), chunks, 4, C.byref(n))
        assert list(chunks) == [-7] * 4 and n.value == -7, "a refused argument wrote an output"
        return rc

    assert one(None, 0, 0, good, 8.0) == -1 and every(None, 0, good, 8.0) == -1
    assert one(H._h, 0, 0, None, 8.0) == -1 and every(H._h, 0, None, 8.0) == -1
    for chunk in (-1, 2):
        assert one(H._h, chunk, 0, good, 8.0) == -1
    for op in (-1, 3):
        assert one(H._h, 0, op, good, 8.0) == -1 and every(H._h, op, good, 8.0) == -1
    for bad in ((float("nan"), 0.0, 0.0), (0.0, float("nan"), 0.0), (0.0, 0.0, float("nan")), (float("inf"), 0.0, 0.0), (0.0, 0.0, -float("inf"))):
        assert one(H._h, 0, 1, vec(bad), 8.0) == -1 and every(H._h, 1, vec(bad), 8.0) == -1
    for radius in (0.0, -8.0, float("nan"), float("inf")):
        assert one(H._h, 0, 0, good, radius) == -1 and every(H._h, 0, good, radius) == -1
    # then the host world: SVO_ERR_NOT_UPLOADED
    for op in (0, 1, 2):
        assert one(H._h, 0, op, good, 8.0) == -5
    seam = vec((128.0, 64.0, 64.0))
    assert svo.lib.svo_world_edit_ball_all(H._h, 0, seam, 8.0, C.c_uint16(5), chunks, 4, C.byref(n)) == -5
    assert n.value == 2 and list(chunks) == [-7] * 4            # the count needs no device; the list is not written
    assert svo.lib.svo_world_edit_ball_all(H._h, 0, seam, 8.0, C.c_uint16(5), None, 0, None) == -5
    # a list that cannot hold the chunks: refused, the count reported
    n.value = -7
    assert svo.lib.svo_world_edit_ball_all(H._h, 0, seam, 8.0, C.c_uint16(5), chunks, 1, C.byref(n)) == -1
    assert n.value == 2 and list(chunks) == [-7] * 4
    assert svo.lib.svo_world_edit_ball_all(H._h, 0, seam, 8.0, C.c_uint16(5), chunks, 1, None) == -1
    n.value = -7
    assert svo.lib.svo_world_edit_ball_all(H._h, 0, vec((900.0, 64.0, 64.0)), 8.0, C.c_uint16(5), chunks, 0, C.byref(n)) == -5 and n.value == 0
    for call in (lambda: H.edit_ball(0, svo.EDIT_DESTROY, (10, 10, 10), 8.0), lambda: H.edit_ball_all(svo.EDIT_DESTROY, (10, 10, 10), 8.0)):
        with pytest.raises(svo.SvoError) as e:
            call()
        assert e.value.code == -5
    fresh = svo.World.generate(2, 1, 1, 128, 4)
    for i in range(2):
        assert np.array_equal(H.chunk(i)["tree"], fresh.chunk(i)["tree"]) and np.array_equal(H.chunk(i)["twig"], fresh.chunk(i)["twig"])
    H.destroy()
    fresh.destroy()
