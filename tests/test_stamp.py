"""svo_world_chunk_stamp (csrc/stamp.hip) on the GPU: the pools the device installs, read back with World.chunk, and the count equal the
host form's (csrc/stamp.cpp, which tests/test_stamp_cpu.py holds against the dense model) index for index - exact equality everywhere;
what follows the install: svo_world_info, the other chunk, both march kernels; the three places B can live in; the two-chunk recipe;
depth 12 and 16.  The shapes are the smallest at which the kernels can still go wrong: depth-4 A with B of depth 2, 3 and 4 at every
kind of offset and in all 48 orientations, results that fold to one word and results larger than both inputs, level lists beyond one
block and brick candidates across a block border at depth 7."""
import ctypes as C

import numpy as np
import pytest

import combine_model as K
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
OPS = list(K.OPS.items())


@pytest.fixture(scope="module")
def model(svo):
    """A one-chunk world on the same device: where B lives when it is a model of its own."""
    MW = svo.World.create([empty_chunk()], 1, 1, 1, 128).upload(0)
    yield MW
    MW.destroy()


def stamp_and_check(svo, W, other, MW, a, b, offset, orient, what, ops=OPS):
    """Every op of `ops` on (a, b) at the placement, B in the model world: pools, count, the sentinel chunk, svo_world_info and B."""
    place(MW, 0, b)
    for opname, op in ops:
        want, changed = svo.chunk_stamp(a, b, offset, orient, op)
        put(W, a)
        count = W.chunk_stamp(0, MW, 0, offset, orient, op)
        print(what, opname, "changed", count, "host form", changed, "node words", want["tree"].size, "bricks", want["twig"].size // 64)
        assert W.stamp_status == svo.SVO_OK and count == changed
        check_after(W, other, want, f"{what}, {opname}")
    same_pools(MW.chunk(0), b, f"{what}: B")


@pytest.mark.parametrize("name", list(T.cases()))
def test_device_pools_and_count_equal_the_host_form(svo, world, model, name):
    W, other = world
    a, b, offset, orient = T.case(name)
    stamp_and_check(svo, W, other, model, a, b, offset, orient, name)


def test_depth_6_shell_into_depth_7_lists_beyond_one_block(svo, world, model):
    """Odd offset, partly outside, a mirror: the level lists pass 256 entries and the brick candidates cross a block border."""
    W, other = world
    a, b = G.model_chunk("g7"), T.shell6()
    offset, orient = (77, 21, -13), 11
    assert not T.is_rotation(orient) and a["tree"].size > 8 * 256 and b["tree"].size > 8 * 256 and b["twig"].size // 64 > 1024
    stamp_and_check(svo, W, other, model, a, b, offset, orient, "depth 6 into 7")
    stamp_and_check(svo, W, other, model, K.one_word(7, 0), b, (1, 1, 1), 0, "depth 6 into an empty 7", ops=[("max", K.MAX)])


def test_the_three_places_b_can_live_in_give_the_same_pools(svo, world, model):
    W, other = world
    a, b, offset, orient = T.chunks()["pairings"], T.chunks()["b3"], (7, 2, 9), 22
    for opname, op in OPS:
        want, changed = svo.chunk_stamp(a, b, offset, orient, op)
        put(W, a); place(model, 0, b)                       # B in the model world
        assert W.chunk_stamp(0, model, 0, offset, orient, op) == changed
        same_pools(W.chunk(0), want, f"{opname}: B in the model world")
        same_pools(model.chunk(0), b, "B")
        put(W, a); place(W, 1, b)                           # B as chunk 1 of the same world
        assert W.chunk_stamp(0, W, 1, offset, orient, op) == changed
        same_pools(W.chunk(0), want, f"{opname}: B in the same world")
        same_pools(W.chunk(1), b, "B")
        info = W.info
        assert info.total_trees == want["tree"].size + b["tree"].size and info.total_twigs == (want["twig"].size + b["twig"].size) // 64
        self_want, self_changed = svo.chunk_stamp(b, b, (3, -1, 2), orient, op)
        assert W.chunk_stamp(1, W, 1, (3, -1, 2), orient, op) == self_changed     # src_chunk == chunk: A = B, read completely before it is replaced
        same_pools(W.chunk(1), self_want, f"{opname}: B into itself")
        same_pools(W.chunk(0), want, f"{opname}: the other chunk")
    place(W, 1, other)
    same_pools(W.chunk(1), other, "the sentinel chunk, put back")


def test_the_two_chunk_recipe_equals_the_model_of_the_wide_grid(svo, world, model):
    """A model that straddles the border between chunk 0 and its +x neighbour: two calls whose offsets differ by N_A on x; both chunks'
    to_grid equal the dense model of the 32-wide grid."""
    W, other = world
    left, right, b = T.chunks()["pairings"], T.chunks()["height4"], T.chunks()["b3"]
    offset, orient = (13, 5, -2), 29
    wide = np.concatenate([G.pools_to_grid(left, 4), G.pools_to_grid(right, 4)], axis=2)
    there = np.zeros((16 + 8, 16, 32), np.uint16)           # z from -2 on: room for what lies outside
    there[0:8, 5:13, 13:21] = T.oriented(G.grids()["g3"], orient)
    grid = svo.DeviceBuffer(16 ** 3 * 2)
    place(model, 0, b)
    for opname, op in OPS:
        g = K.f(op, wide, there[2:18]).astype(np.uint16)
        put(W, left); place(W, 1, right)
        n = W.chunk_stamp(0, model, 0, offset, orient, op) + W.chunk_stamp(1, model, 0, (offset[0] - 16, offset[1], offset[2]), orient, op)
        assert n == int((g != wide).sum())
        for i in (0, 1):
            W.chunk_to_grid(i, 4, grid.ptr)
            assert np.array_equal(grid.to_numpy(np.uint16, 16 ** 3).reshape(16, 16, 16), g[:, :, 16 * i:16 * i + 16]), (opname, i)
    grid.free()
    place(W, 1, other)
    same_pools(W.chunk(1), other, "the sentinel chunk, put back")


# ---- the march --------------------------------------------------------------------------------------------------------------------------
def test_the_march_equals_the_oracle_over_the_host_forms_pools(svo, oracle, world, model):
    W, other = world
    a, b = F.freeze(G.chunk_of(G.heightfield(6))), T.chunks()["b4"]
    offset, orient = (21, 30, 11), 19
    want, changed = svo.chunk_stamp(a, b, offset, orient, K.OVER)
    put(W, a); place(model, 0, b)
    assert W.chunk_stamp(0, model, 0, offset, orient, K.OVER) == changed > 500
    O = oracle.OracleWorld.from_chunks([want, other], 2, 1, 1, 128)
    cam = svo.make_camera((150.0, 140.0, -90.0), (-0.35, -0.3, 0.88), (0.0, 1.0, 0.0), 60.0, 64, 48)
    for semantics in (0, 1):
        ref = O.trace_image(cam, params=oracle.make_params(shadow=True, semantics=semantics))
        assert int((ref["flags"] & 1).sum()) > 200
        for kernel in (svo.KERNEL_LITERAL, svo.KERNEL_STACK):
            assert_gbuffer_equal(W.draw(cam, shadow=True, kernel=kernel, semantics=semantics), ref, f"semantics {semantics} / kernel {kernel}")


# ---- depth 12 and 16 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [12, 16])
def test_deep_leaf_root_b_stamped_on_the_device(svo, world, model, depth):
    W, other = world
    a, _, c = deep_cubes(svo, depth)
    ma, _, _ = K.cube_meshes(depth)
    box_a, box_b = T.deep_boxes(depth)
    b, offset = T.deep_b(), box_b[0]
    place(model, 0, b)
    assert device_build(svo, W, 0, ma, depth) == svo.SVO_OK and W.chunk_fill_enclosed(0, K.MATERIAL_A) == F.CUBE_FILLED
    same_pools(W.chunk(0), a, "cube A, built on the device")
    want, changed = svo.chunk_stamp(a, b, offset, 0, K.MAX)
    count = W.chunk_stamp(0, model, 0, offset, 0, K.MAX)
    print(f"depth {depth}: MAX changed {count}, {want['tree'].size} node words, {want['twig'].size // 64} bricks")
    assert count == changed == T.box_cells(box_b) == 256 ** 3
    check_after(W, other, want, f"depth {depth}, MAX")
    same_pools(model.chunk(0), b, "B")
    # one ray straight down onto the stamped cube: it ends on B's material in the cube's top layer of cells, whose upper face lies at
    # y = box_b[1][1] cells.  The march's epsilon (1/8192) is below a cell (128 / 2^depth >= 1/512), so t lies within one cell of the face
    cell = 128.0 / (1 << depth)
    top = box_b[1][1] * cell
    o = np.array([[(box_b[0][0] + 100.5) * cell, top + 8.0, (box_b[0][2] + 100.5) * cell]], np.float32)
    d = np.array([[0.0, -1.0, 0.0]], np.float32)
    for kernel in (svo.KERNEL_LITERAL, svo.KERNEL_STACK):
        hit = W.chunkmarch(o, d, kernel=kernel)
        assert int(hit["flags"][0]) & 1 and int(hit["material"][0]) == T.DEEP_MATERIAL
        assert abs(float(hit["t"][0]) - (float(o[0, 1]) - top)) < cell, (kernel, float(hit["t"][0]))
    # stack = literal on a few rays around the two cubes
    centre = (np.array(box_b[0]) + 90.0) * cell
    rng = np.random.default_rng(depth)
    origins = (centre + rng.uniform(-1.0, 1.0, (16, 3)) * 400.0 * cell + np.array([0.0, 500.0 * cell, 0.0])).astype(np.float32)
    dirs = centre + rng.uniform(-1.0, 1.0, (16, 3)) * 150.0 * cell - origins
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    stack = W.chunkmarch(origins, dirs, shadow=True, kernel=svo.KERNEL_STACK)
    assert int((stack["flags"] & 1).sum()) >= 8
    assert_gbuffer_equal(W.chunkmarch(origins, dirs, shadow=True, kernel=svo.KERNEL_LITERAL), stack, f"literal against stack at depth {depth}")
    put(W, a)
    want, changed = svo.chunk_stamp(a, b, offset, 0, K.SUBTRACT)
    assert W.chunk_stamp(0, model, 0, offset, 0, K.SUBTRACT) == changed == T.box_cells(T.box_overlap(box_a, box_b))
    check_after(W, other, want, f"depth {depth}, SUBTRACT")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_both_chunks_as_they_were(svo, world, model):
    W, other = world
    a, b, offset, orient = T.case("into_empty")
    a = T.chunks()["pairings"]
    put(W, a); place(model, 0, b)
    good = svo.Placement(offset, orient)

    def unchanged(what, a=a, b=b):
        check_after(W, other, a, what)
        same_pools(model.chunk(0), b, what + ": B")

    def call(chunk=0, src=model._h, src_chunk=0, op=0, w=W._h, pl=good):
        changed = C.c_uint64(77)
        rc = svo.lib.svo_world_chunk_stamp(w, chunk, src, src_chunk, None if pl is None else C.byref(pl), op, C.byref(changed))
        assert rc == 0 or changed.value == 77
        return rc

    assert [call(w=None), call(src=None), call(chunk=-1), call(chunk=2), call(src_chunk=-1), call(src_chunk=1), call(op=-1), call(op=5)] == [-1] * 8
    assert [call(pl=None), call(pl=svo.Placement((0, 0, 0), 48)), call(pl=svo.Placement((65537, 0, 0), 0)), call(pl=svo.Placement((0, 0, -65537), 0))] == [-1] * 4
    unchanged("after the argument errors")
    host_only = svo.World.create([b], 1, 1, 1, 128)         # a model world that is not uploaded
    assert call(src=host_only._h) == -5 and call(w=host_only._h, src=W._h) == -5
    assert call(w=host_only._h, src=W._h, op=9) == -1       # the argument errors come first
    same_pools(host_only.chunk(0), b, "the host-only world")
    host_only.destroy()
    unchanged("after the world that is not uploaded")
    deeper = K.pairs()["g5_shell"][0]                       # B deeper than A: 5 into 4, and A into the depth-3 model
    place(model, 0, deeper)
    assert call() == -6
    unchanged("after the deeper B", b=deeper)
    place(model, 0, b)
    assert call(w=model._h, src=W._h) == -6
    unchanged("after the deeper B, the other way")
    shallow = dict(position=(0.0, 0.0, 0.0), size=128.0, depth=4, tree=np.array([G.node(G.TWIG, 0)], np.uint32), twig=a["twig"][:64].copy())
    place(model, 0, shallow)                                # a brick above level depth-2, as B and as A
    assert call() == -6
    unchanged("after the refused sparsely refined B", b=shallow)
    assert call(w=model._h, src=W._h) == -6
    unchanged("after the refused sparsely refined A", b=shallow)
    place(model, 0, b)
    want, changed = svo.chunk_stamp(a, b, offset, orient, K.MAX)
    assert W.chunk_stamp(0, model, 0, offset, orient, K.MAX) == changed         # and the worlds still work
    check_after(W, other, want, "after the refusals")
