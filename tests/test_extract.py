"""svo_world_chunk_extract (csrc/extract.hip) on the GPU: the pools the device installs, read back with World.chunk, and the count equal
the host form's (csrc/extract.cpp, which tests/test_extract_cpu.py holds against the dense model) index for index - exact equality
everywhere; the source is read back unchanged, and what follows the install is checked on both worlds: svo_world_info, the sentinel
chunk, both march kernels.  The source is chunk 0 of the two-chunk world, the shallow destination a chunk of a second small world; the
turn and the shift in place run inside one chunk; the header's identities run through svo_world_chunk_stamp; depth 12 and 16.  The
shapes are the smallest at which the kernels can still go wrong: depth-4, 6 and 7 sources with windows of depth 2, 3 and 4 at every
kind of offset and in all 48 orientations, windows that fold to one word, bricks out of a one-word pool, level lists beyond one block
and brick candidates across a block border at depth 5 and 6."""
import ctypes as C

import numpy as np
import pytest

import combine_model as K
import extract_model as X
import grid_model as G
import sparse_fill_model as F
import stamp_model as T
from helpers import assert_gbuffer_equal
from test_combine import place
from test_combine_cpu import deep_cubes
from test_compact_model import same_pools
from test_sparse_fill import check_after, device, put, world      # noqa: F401  (device and world are fixtures)
from test_sparse_mesh import device_build, empty_chunk

pytestmark = pytest.mark.gpu
STALE = G.node(G.LEAF, 9)                                   # what the destination holds before a call: replaced, never merged


@pytest.fixture(scope="module")
def model(svo):
    """A one-chunk world on the same device: where the extracted chunk goes when it is a model of its own."""
    MW = svo.World.create([empty_chunk()], 1, 1, 1, 128).upload(0)
    yield MW
    MW.destroy()


def model_holds(MW, want, what):
    same_pools(MW.chunk(0), want, what)
    info = MW.info
    assert info.total_trees == want["tree"].size and info.total_twigs == want["twig"].size // 64 and info.max_chunk_depth == int(want["depth"])


def extract_and_check(svo, W, other, MW, a, offset, orient, depth, what):
    """A in chunk 0 of W, C chunk 0 of the model world: pools, count, svo_world_info of both, the sentinel chunk and A."""
    want, occupied = svo.chunk_extract(a, offset, orient, depth)
    put(W, a)
    place(MW, 0, K.one_word(depth, STALE))
    count = MW.chunk_extract(0, W, 0, offset, orient)
    print(what, "occupied", count, "host form", occupied, "node words", want["tree"].size, "bricks", want["twig"].size // 64)
    assert MW.extract_status == svo.SVO_OK and count == occupied
    model_holds(MW, want, what)
    check_after(W, other, a, f"{what}: A")
    return want, occupied


@pytest.mark.parametrize("name", list(X.cases()))
def test_device_pools_and_count_equal_the_host_form(svo, world, model, name):
    W, other = world
    a, offset, orient, depth = X.case(name)
    extract_and_check(svo, W, other, model, a, offset, orient, depth, name)


def test_lists_beyond_one_block_and_brick_candidates_across_block_borders(svo, world, model):
    """The depth-6 shell read at an offset partly outside in a mirrored orientation, and a depth-5 window of the depth-7 terrain at an
    odd offset (a root descent of two levels)."""
    W, other = world
    shell, orient = T.shell6(), 11
    assert not T.is_rotation(orient) and shell["twig"].size // 64 > 1024
    want, _ = extract_and_check(svo, W, other, model, shell, (3, -5, 7), orient, 6, "the depth-6 shell")
    assert want["tree"].size > 8 * 256 and want["twig"].size // 64 > 1024
    want, _ = extract_and_check(svo, W, other, model, G.model_chunk("g7"), (45, 23, 51), 29, 5, "depth 5 out of 7")
    assert want["tree"].size > 256 and want["twig"].size // 64 > 4 * 16           # a list beyond one block, more candidates than one block of k_bricks takes


def test_the_turn_and_the_shift_in_place(svo, world):
    """src == dst and src_chunk == chunk: A is read completely before C is installed."""
    W, other = world
    a = X.chunks()["pairings"]
    for offset, orient in (((0, 0, 0), T.quarter_turns()[0]), ((8, 0, 0), 0), ((-3, 5, 1), 38)):
        want, occupied = svo.chunk_extract(a, offset, orient, 4)
        put(W, a)
        assert W.chunk_extract(0, W, 0, offset, orient) == occupied and W.extract_status == svo.SVO_OK
        check_after(W, other, want, f"in place, offset {offset}, orient {orient}")
    # the shallow destination as the sentinel's neighbour in the same world: chunk 1 out of chunk 0, then chunk 1 put back
    want, occupied = svo.chunk_extract(a, (5, 1, -3), 17, 3)
    put(W, a); place(W, 1, K.one_word(3, STALE))
    assert W.chunk_extract(1, W, 0, (5, 1, -3), 17) == occupied
    same_pools(W.chunk(1), want, "chunk 1 out of chunk 0")
    same_pools(W.chunk(0), a, "chunk 0, the source")
    place(W, 1, other)
    check_after(W, other, a, "the sentinel chunk, put back")


@pytest.mark.parametrize("depth,offset,orient", [(3, (1, 2, -2), 22), (4, (-3, 2, 1), 41), (2, (13, 3, 2), 13)])
def test_the_identities_through_the_device_stamp(svo, world, model, depth, offset, orient):
    W, other = world
    a = X.chunks()["pairings"]
    _, occupied = extract_and_check(svo, W, other, model, a, offset, orient, depth, "C")
    assert W.chunk_stamp(0, model, 0, offset, orient, K.OVER) == 0                  # C back where it came from: nothing to put
    check_after(W, other, svo.chunk_combine(a, K.one_word(4, 0), K.MAX)[0], "OVER: A rebuilt")
    put(W, a)
    assert W.chunk_stamp(0, model, 0, offset, orient, K.SUBTRACT) == occupied
    put(W, a)
    W.chunk_stamp(0, model, 0, offset, orient, K.INTERSECT)
    kept = W.chunk(0)
    put(W, K.one_word(4, 0))
    assert W.chunk_stamp(0, model, 0, offset, orient, K.MAX) == occupied
    check_after(W, other, kept, "INTERSECT into A against MAX into the empty chunk")
    # D_C = D_A, offset 0, orient 0: A rebuilt
    put(W, a); place(model, 0, K.one_word(4, STALE))
    model.chunk_extract(0, W, 0, (0, 0, 0), 0)
    model_holds(model, svo.chunk_combine(a, K.one_word(4, 0), K.MAX)[0], "the whole chunk, as it lies")


# ---- the march --------------------------------------------------------------------------------------------------------------------------
def test_the_march_equals_the_oracle_over_the_host_forms_pools(svo, oracle, world, model):
    W, other = world
    a = F.freeze(G.chunk_of(G.heightfield(6)))
    offset, orient = (13, 9, -5), 19
    want, occupied = extract_and_check(svo, W, other, model, a, offset, orient, 5, "depth 5 out of the depth-6 terrain")
    assert occupied > 5000
    O = oracle.OracleWorld.from_chunks([want], 1, 1, 1, 128)
    cam = svo.make_camera((150.0, 140.0, -90.0), (-0.35, -0.3, 0.88), (0.0, 1.0, 0.0), 60.0, 64, 48)
    for semantics in (0, 1):
        ref = O.trace_image(cam, params=oracle.make_params(shadow=True, semantics=semantics))
        assert int((ref["flags"] & 1).sum()) > 200
        for kernel in (svo.KERNEL_LITERAL, svo.KERNEL_STACK):
            assert_gbuffer_equal(model.draw(cam, shadow=True, kernel=kernel, semantics=semantics), ref, f"semantics {semantics} / kernel {kernel}")


# ---- depth 12 and 16 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [12, 16])
def test_deep_windows_extracted_on_the_device(svo, oracle, world, model, depth):
    W, other = world
    a, _, c = deep_cubes(svo, depth)
    ma, _, _ = K.cube_meshes(depth)
    assert device_build(svo, W, 0, ma, depth) == svo.SVO_OK and W.chunk_fill_enclosed(0, K.MATERIAL_A) == F.CUBE_FILLED
    same_pools(W.chunk(0), a, "cube A, built on the device")
    wins = X.deep_windows(depth)
    offset, d, box, inside = wins["across_three_faces"]
    want, occupied = svo.chunk_extract(a, offset, 0, d)
    place(model, 0, K.one_word(d, STALE))
    count = model.chunk_extract(0, W, 0, offset, 0)
    print(f"depth {depth} -> {d}: occupied {count}, {want['tree'].size} node words, {want['twig'].size // 64} bricks")
    assert count == occupied == T.box_cells(inside) == 128 * 192 * 224
    model_holds(model, want, f"depth {depth} -> {d}")
    check_after(W, other, a, f"depth {depth}: A")
    # the extracted chunk holds the box [0, 128) x [0, 192) x [0, 224) of its 256^3 cells, half a unit each.  One ray straight down
    # onto it ends on A's material in the box's top layer of cells
    cell = 128.0 / 256
    top = 192 * cell
    o = np.array([[40.25, top + 8.0, 60.25]], np.float32)
    down = np.array([[0.0, -1.0, 0.0]], np.float32)
    for kernel in (svo.KERNEL_LITERAL, svo.KERNEL_STACK):
        hit = model.chunkmarch(o, down, kernel=kernel)
        assert int(hit["flags"][0]) & 1 and int(hit["material"][0]) == K.MATERIAL_A
        assert abs(float(hit["t"][0]) - 8.0) < cell, (kernel, float(hit["t"][0]))
    # stack = literal on sixteen rays into the extracted chunk, and both against the oracle over the host form's pools
    rng = np.random.default_rng(depth)
    centre = np.array([32.0, 48.0, 56.0])
    origins = (centre + rng.uniform(-1.0, 1.0, (16, 3)) * 60.0 + np.array([0.0, 150.0, 0.0])).astype(np.float32)
    dirs = centre + rng.uniform(-1.0, 1.0, (16, 3)) * 30.0 - origins
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    stack = model.chunkmarch(origins, dirs, shadow=True, kernel=svo.KERNEL_STACK)
    assert int((stack["flags"] & 1).sum()) >= 8
    assert_gbuffer_equal(model.chunkmarch(origins, dirs, shadow=True, kernel=svo.KERNEL_LITERAL), stack, f"literal against stack, out of depth {depth}")
    O = oracle.OracleWorld.from_chunks([want], 1, 1, 1, 128)
    cam = svo.make_camera((150.0, 140.0, -90.0), (-0.35, -0.3, 0.88), (0.0, 1.0, 0.0), 60.0, 32, 24)
    ref = O.trace_image(cam, params=oracle.make_params(shadow=True))
    assert int((ref["flags"] & 1).sum()) > 50
    for kernel in (svo.KERNEL_LITERAL, svo.KERNEL_STACK):
        assert_gbuffer_equal(model.draw(cam, shadow=True, kernel=kernel), ref, f"the march out of depth {depth} / kernel {kernel}")
    # the whole cube in a depth-10 window, turned; depth 2 on a face of the cube and wholly inside (at depth 16 a descent of 14 levels)
    for offset, orient, d, cells in ((wins["the_whole_cube"][0], 13, 10, 258 ** 3), ((c + 255, c + 8, c + 8), 0, 2, 32), ((c + 101, c + 77, c + 33), 29, 2, 64)):
        want, occupied = svo.chunk_extract(a, offset, orient, d)
        place(model, 0, K.one_word(d, STALE))
        assert model.chunk_extract(0, W, 0, offset, orient) == occupied == cells
        model_holds(model, want, f"depth {depth} -> {d} at {offset}")
    check_after(W, other, a, f"depth {depth}: A at the end")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_both_chunks_as_they_were(svo, world, model):
    W, other = world
    a = X.chunks()["pairings"]
    stale = K.one_word(3, STALE)
    put(W, a); place(model, 0, stale)
    good = svo.Placement((5, -3, 9), 22)

    def unchanged(what, a=a, c=stale):
        check_after(W, other, a, what)
        model_holds(model, c, what + ": C")

    def call(chunk=0, src=W._h, src_chunk=0, w=model._h, pl=good):
        occupied = C.c_uint64(77)
        rc = svo.lib.svo_world_chunk_extract(w, chunk, src, src_chunk, None if pl is None else C.byref(pl), C.byref(occupied))
        assert rc == 0 or occupied.value == 77
        return rc

    assert [call(w=None), call(src=None), call(chunk=-1), call(chunk=1), call(src_chunk=-1), call(src_chunk=2)] == [-1] * 6
    assert [call(pl=None), call(pl=svo.Placement((0, 0, 0), 48)), call(pl=svo.Placement((65537, 0, 0), 0)), call(pl=svo.Placement((0, 0, -65537), 0))] == [-1] * 4
    unchanged("after the argument errors")
    host_only = svo.World.create([a], 1, 1, 1, 128)         # a source world that is not uploaded
    assert call(src=host_only._h) == -5 and call(w=host_only._h, src=W._h) == -5
    assert call(w=host_only._h, src=W._h, pl=None) == -1    # the argument errors come first
    same_pools(host_only.chunk(0), a, "the host-only world")
    host_only.destroy()
    unchanged("after the world that is not uploaded")
    deeper = K.one_word(5, STALE)                           # C deeper than A: that direction is the stamp
    place(model, 0, deeper)
    assert call() == -6
    unchanged("after the deeper C", c=deeper)
    shallow = dict(position=(0.0, 0.0, 0.0), size=128.0, depth=4, tree=np.array([G.node(G.TWIG, 0)], np.uint32), twig=a["twig"][:64].copy())
    put(W, shallow)                                         # a brick above level depth-2 in A: met by the root's descent, and by the walk
    for c in (stale, K.one_word(4, STALE)):
        place(model, 0, c)
        assert call() == -6
        unchanged("after the refused sparsely refined A", a=shallow, c=c)
    put(W, a); place(model, 0, stale)
    want, occupied = svo.chunk_extract(a, (5, -3, 9), 22, 3)
    assert model.chunk_extract(0, W, 0, (5, -3, 9), 22) == occupied             # and the worlds still work
    model_holds(model, want, "after the refusals")
    check_after(W, other, a, "after the refusals: A")
