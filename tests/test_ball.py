"""Ball edits on the device (svo_world_edit_ball / svo_world_edit_ball_all; csrc/builder.hip: DeviceFiller over a BallRegion).  After
every edit the chunk's pools must equal, index for index, what the host model (tests/ball_model.py: the twin's depth-first edit with the
ball's touch / inside) leaves, and the march over the edited world must equal the oracle's over the model's pools."""
import ctypes as C
import time

import numpy as np
import pytest

import ball_model as B
import grid_model as G
from helpers import assert_gbuffer_equal, random_rays

pytestmark = pytest.mark.gpu
F = np.float32


def same_pools(model, D, i, what):
    a, b = B.pools_of(model), D.chunk(i, copy=False)
    assert a["tree"].size == b["tree"].size and a["twig"].size == b["twig"].size, \
        f"{what}: chunk {i} pool sizes differ: {a['tree'].size} / {a['twig'].size // 64} against {b['tree'].size} / {b['twig'].size // 64}"
    assert np.array_equal(a["tree"], b["tree"]), f"{what}: chunk {i} node words differ"
    assert np.array_equal(a["twig"], b["twig"]), f"{what}: chunk {i} bricks differ"


EDITS = [
    # (op, chunks, centre, radius, material)
    (0, (0,), (45.0, 85.0, 35.0), 14.5, 5),                     # build in the air above the terrain
    (1, (0,), (60.0, 8.0, 40.0), 22.0, 0),                      # destroy through terrain and water
    (2, (0, 1), (127.3, 20.7, 60.1), 25.4, 5),                  # replace across the chunk seam, off the lattice, both chunks
    (0, (1,), (180.4, 90.3, 33.6), 0.3, 7),                     # radius below one voxel, in the air
    (1, (1,), (200.5, 3.5, 50.5), 0.45, 0),                     # ... and inside the ground
    (1, (1,), (192.0, 64.0, 64.0), 120.0, 0),                   # a ball that swallows a whole chunk: its root ends EMPTY ...
    (0, (1,), (192.0, 64.0, 64.0), 120.0, 3),                   # ... and one LEAF
    (1, (1,), (180.25, 60.5, 60.125), 3.3, 0),                  # a small hole in the solid chunk: splits all the way down
    (0, (0,), (500.0, 500.0, 500.0), 50.0, 5),                  # misses: nothing changes
    (0, (0,), (64.0, 64.0, 64.0), 8.0, 2),                      # on the lattice: cells tangent to the ball are edited
    (2, (0,), (-10.0, 30.0, 64.0), 18.0, 4),                    # a centre outside the world, poking in
]


def test_edit_ball_equals_the_model(svo, oracle):
    D = svo.World.generate(2, 1, 1, 128, 7, build_device=0)
    M = [B.chunk_of(D.chunk(i)) for i in range(2)]
    o, d = random_rays(np.random.default_rng(41), 20000, (0, 0, 0), (256, 128, 128))
    prm = oracle.make_params(shadow=True)
    for k, (op, chunks, centre, radius, mat) in enumerate(EDITS):
        before = [B.pools_of(m) for m in M]
        for i in chunks:
            B.edit(M[i], op, B.Ball(centre, radius), mat)
            assert D.edit_ball(i, op, centre, radius, mat) == 0
        for i in range(2):
            same_pools(M[i], D, i, f"after edit {k}")
        pools = [B.pools_of(m) for m in M]
        changed = any(not np.array_equal(a[f], b[f]) for a, b in zip(before, pools) for f in ("tree", "twig"))
        assert changed == (k != 8), f"edit {k}"
        O = oracle.OracleWorld.from_chunks(pools, 2, 1, 1, 128)
        want = O.trace_rays(o, d, params=prm, threads=8)
        for kern in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
            assert_gbuffer_equal(D.chunkmarch(o, d, shadow=True, kernel=kern), want, f"edit {k} / kernel {kern}")
        if k == 5:
            assert M[1].tree[0] == B.P.node_make(B.EMPTY, 0)
        if k == 6:
            assert M[1].tree[0] == B.P.node_make(B.LEAF, 3)
    D.destroy()


_libc = C.CDLL(None)
_libc.malloc.restype = C.c_void_p
_libc.malloc.argtypes = [C.c_size_t]


def oracle_box_edit(oracle, root, op, lo, hi, material):
    """The C oracle's orc_destroy / orc_build (as tests/test_gpu_edits.py applies them) on the model's evolving pools: they are handed
    over in buffers the oracle may grow, and read back."""
    tree, twig = B.pools_of(root)["tree"], B.pools_of(root)["twig"]
    r = oracle.Root()
    r.position, r.size, r.depth = oracle.vec3(root.position), float(root.size), root.depth
    r.trees, r.twigs = tree.size, twig.size // 64
    r.treestoragesize, r.twigstoragesize = root.treestoragesize, root.twigstoragesize
    tp, wp = _libc.malloc(r.treestoragesize * 4), _libc.malloc(r.twigstoragesize * 128)
    C.memmove(tp, tree.ctypes.data, tree.nbytes)
    C.memmove(wp, twig.ctypes.data, twig.nbytes)
    r.tree, r.twig = C.cast(tp, C.POINTER(C.c_uint32)), C.cast(wp, C.POINTER(C.c_uint16))
    dt, dw = oracle.Delta(), oracle.Delta()
    if op in (1, 2):
        oracle.lib.orc_destroy(C.byref(r), oracle.vec3(lo), oracle.vec3(hi), C.byref(dt), C.byref(dw))
    if op in (0, 2):
        oracle.lib.orc_build(C.byref(r), oracle.vec3(lo), oracle.vec3(hi), material, C.byref(dt), C.byref(dw))
    root.tree = np.ctypeslib.as_array(r.tree, shape=(r.trees,)).tolist()
    root.twig = list(np.ctypeslib.as_array(r.twig, shape=(r.twigs, 64)).copy()) if r.twigs else []
    root.treestoragesize, root.twigstoragesize = r.treestoragesize, r.twigstoragesize
    oracle.lib.orc_root_free(C.byref(r))


@pytest.mark.parametrize("depth,seed,rmax", [(6, 1, 40.0), (9, 2, 6.0)])
def test_random_sequences_of_box_and_ball_edits(svo, oracle, depth, seed, rmax):
    """Forty edits on one chunk, boxes (the C oracle) and balls (the model) mixed - they share the filler's scratch and the install
    path: pools equal after every tenth edit and at the end."""
    rng = np.random.default_rng(seed)
    D = svo.World.generate(1, 1, 1, 128, depth, build_device=0)
    M = B.chunk_of(D.chunk(0))
    voxel = 128.0 / (1 << depth)
    kinds = []
    for k in range(40):
        op = int(rng.integers(0, 3))
        mat = int(rng.integers(1, 8))
        on_lattice = rng.random() < 0.5
        if rng.random() < 0.5:
            edge = float(rng.choice([voxel, 3 * voxel, 7.3, 20.0, 64.0]))
            lo = rng.uniform(-4, 120, 3)
            if on_lattice:
                lo = np.floor(lo / voxel) * voxel
            lo, hi = lo.astype(F), (lo + edge * rng.uniform(0.3, 1.0, 3)).astype(F)
            oracle_box_edit(oracle, M, op, lo, hi, mat)
            assert D.edit_box(0, op, lo, hi, mat) == 0
            kinds.append("box")
        else:
            radius = float(rng.choice([0.4 * voxel, voxel, 2.5 * voxel, rmax * rng.uniform(0.3, 1.0)]))
            c = rng.uniform(-4, 132, 3)
            if on_lattice:
                c = np.floor(c / voxel) * voxel
            B.edit(M, op, B.Ball(c.astype(F), radius), mat)
            assert D.edit_ball(0, op, c.astype(F), radius, mat) == 0
            kinds.append("ball")
        if k % 10 == 9:
            same_pools(M, D, 0, f"depth {depth}, after edit {k} ({' '.join(kinds[-10:])})")
    assert min(kinds.count("box"), kinds.count("ball")) >= 10
    D.destroy()


BALLS_ALL = [
    # (op, centre, radius, material, chunks)
    (0, (40.0, 70.0, 50.0), 12.0, 5, [0]),                      # inside one chunk
    (1, (128.0, 20.0, 128.0), 21.5, 0, [0, 1, 2, 3]),           # on the corner the four chunks share
    (2, (120.0, 30.0, 60.0), 8.0, 7, [0, 1]),                   # tangent to the seam: the closed rule
    (2, (122.0, 30.0, 122.0), 8.0, 4, [0, 1, 2]),               # the diagonal chunk is sqrt(72) away
    (0, (100.3, 64.2, 100.1), 150.0, 3, [0, 1, 2, 3]),          # wider than a chunk
    (1, (-30.0, 60.0, 200.0), 35.5, 0, [2]),                    # a centre outside the world
    (0, (128.0, 300.0, 128.0), 100.0, 5, []),                   # misses
]


def test_edit_ball_all_on_a_2x1x2_world(svo):
    D = svo.World.generate(2, 1, 2, 128, 6, build_device=0)
    M = [B.chunk_of(D.chunk(i)) for i in range(4)]
    positions = [D.chunk(i)["position"] for i in range(4)]
    vec = lambda v: (C.c_float * 3)(*v)
    for k, (op, centre, radius, mat, chunks) in enumerate(BALLS_ALL):
        ball = B.Ball(centre, radius)
        want = B.touched_chunks(positions, 128, ball)
        assert want == chunks, (k, want)
        for i in want:
            B.edit(M[i], op, ball, mat)
        status, got = D.edit_ball_all(op, centre, radius, mat)
        assert status == 0 and got == want, (k, status, got)
        for i in range(4):
            same_pools(M[i], D, i, f"after ball {k}")
    # a list that cannot hold the chunks: refused, the count reported, nothing edited
    out, n = (C.c_int * 4)(*[-7] * 4), C.c_int(-7)
    corner = vec((128.0, 40.0, 128.0))
    assert svo.lib.svo_world_edit_ball_all(D._h, 1, corner, 30.0, C.c_uint16(0), out, 3, C.byref(n)) == -1
    assert n.value == 4 and list(out) == [-7] * 4
    for i in range(4):
        same_pools(M[i], D, i, "after the refused call")
    # no list at all
    n.value = -7
    assert svo.lib.svo_world_edit_ball_all(D._h, 1, corner, 30.0, C.c_uint16(0), None, 0, C.byref(n)) == 0 and n.value == 4
    assert svo.lib.svo_world_edit_ball_all(D._h, 0, corner, 12.0, C.c_uint16(6), None, 0, None) == 0
    for i in range(4):
        B.edit(M[i], 1, B.Ball((128.0, 40.0, 128.0), 30.0))
        B.edit(M[i], 0, B.Ball((128.0, 40.0, 128.0), 12.0), 6)
        same_pools(M[i], D, i, "after the calls without a list")
    with pytest.raises(svo.SvoError) as e:
        D.edit_ball_all(3, (1, 1, 1), 8.0)
    assert e.value.code == -1
    D.destroy()


@pytest.mark.parametrize("op", [0, 1, 2], ids=["build", "destroy", "replace"])
def test_the_edited_chunk_as_a_grid_and_compacted(svo, op):
    """Another path to the same voxels: svo_world_chunk_to_grid of the edited chunk equals the model's pools expanded and the rule
    applied to every cell of the grid read before the edit; svo_world_compact then leaves the same voxels."""
    D = svo.World.generate(1, 1, 1, 128, 6, build_device=0)
    c = D.chunk(0)
    before = D.chunk_grid(0, 6)
    ball = B.Ball((70.0, 12.0, 60.0), 27.3)
    model = B.edit(B.chunk_of(c), op, ball, 9)
    assert D.edit_ball(0, op, (70.0, 12.0, 60.0), 27.3, 9) == 0
    want = G.pools_to_grid(B.pools_of(model), 6)
    brute, hit = B.brute_force(before, c["position"], 128.0, op, ball, 9)
    assert np.array_equal(want, brute) and int((brute != before).sum()) > 500 and int((~hit).sum()) > 500
    assert np.array_equal(D.chunk_grid(0, 6), want)
    assert D.compact(0) == 0
    assert np.array_equal(D.chunk_grid(0, 6), want)
    D.destroy()


def test_edit_ball_on_a_benchmark_chunk(svo):
    """A depth-12 chunk of the benchmark's world: destroy / build / replace of a ball of radius 8 against edit_box of its bounding cube,
    medians over ten places each, in one process.  The times are printed, the statuses asserted."""
    worlds = {shape: svo.World.generate(1, 1, 1, 128, 12, build_device=0) for shape in ("ball", "box")}       # the same terrain under both
    rng = np.random.default_rng(12)
    centres = np.column_stack([rng.uniform(16, 112, 12), rng.uniform(4, 30, 12), rng.uniform(16, 112, 12)]).astype(F)
    r = F(8.0)
    times = {}
    for name, op in (("destroy", svo.EDIT_DESTROY), ("build", svo.EDIT_BUILD), ("replace", svo.EDIT_REPLACE)):
        for shape, W in worlds.items():
            ts = []
            for c in centres:
                t0 = time.perf_counter()
                rc = W.edit_ball(0, op, c, r, 5) if shape == "ball" else W.edit_box(0, op, c - r, c + r, 5)
                assert svo.lib.svo_stream_synchronize(None) == 0
                ts.append(time.perf_counter() - t0)
                assert rc in (svo.SVO_OK, svo.OK_LITERAL_ONLY)
            times[name, shape] = float(np.median(ts[2:])) * 1e3       # the first two calls size the scratch
    print("\ndepth-12 chunk, medians of 10: " + ", ".join(f"{n} {s} {times[n, s]:.3f} ms" for n, s in times))
    for W in worlds.values():
        W.destroy()
