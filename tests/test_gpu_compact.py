"""svo_world_compact / svo_world_coarsen on an uploaded world (csrc/compact.hip: Ocroot::defragcopy / Ocroot::lodmm as three
level-synchronous sweeps, the pools never visit the host).  The device result must equal, index for index, the test model
(tests/lod_model.py) and the host path (csrc/compact.cpp); both kernels must march the result as the oracle marches the pools read
back; edits, launches on other streams and the world's bookkeeping must follow."""
import time

import numpy as np
import pytest

import lod_model as M
from helpers import assert_gbuffer_equal, random_rays
from test_compact_model import oracle_edit, random_edits, same_pools

pytestmark = pytest.mark.gpu

EDITS = [   # the edit list of tests/test_gpu_edits.py: (op, chunks, lo, hi, material)
    (0, (0,), (20, 60, 20), (70, 110, 50), 5),
    (1, (0,), (0, 0, 0), (128, 45, 30), 0),
    (2, (0, 1), (100.3, 10.7, 40.1), (150.9, 70.2, 90.6), 5),
    (0, (1,), (130.0, 0.0, 0.0), (131.0, 128.0, 1.0), 7),
    (1, (1,), (128, 0, 0), (256, 128, 128), 0),
    (0, (1,), (128, 0, 0), (256, 128, 128), 3),
    (1, (1,), (180.25, 60.5, 60.125), (181.0, 61.0, 61.5), 0),
    (0, (0,), (500, 500, 500), (600, 600, 600), 5),
    (2, (0,), (63.99, 5.99, 63.99), (64.01, 6.01, 64.01), 2),
]


def march_equals_oracle(svo, oracle, D, dims, rays, what):
    n = dims[0] * dims[1] * dims[2]
    O = oracle.OracleWorld.from_chunks([D.chunk(i) for i in range(n)], *dims, 128)
    o, d = rays
    want = O.trace_rays(o, d, params=oracle.make_params(shadow=True), threads=8)
    for kern in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
        assert_gbuffer_equal(D.chunkmarch(o, d, shadow=True, kernel=kern), want, f"{what} / kernel {kern}")
    return want


def test_device_equals_the_model_after_the_edit_list(svo, oracle):
    O = oracle.OracleWorld.generate(2, 1, 1, 128, 7)
    D = svo.World.generate(2, 1, 1, 128, 7, build_device=0)
    for op, chunks, lo, hi, mat in EDITS:
        for i in chunks:
            oracle_edit(oracle, O, i, op, lo, hi, mat)
            D.edit_box(i, op, lo, hi, mat)
    for i in range(2):
        c = O.chunk(i)
        assert D.compact(i) == svo.SVO_OK
        want = M.compact(c)
        same_pools(D.chunk(i), want, f"edit list, chunk {i}, compact")
        assert D.coarsen(i) == svo.SVO_OK
        same_pools(D.chunk(i), M.coarsen(want, full=False), f"edit list, chunk {i}, coarsen")
    D.destroy()


@pytest.mark.parametrize("depth,seed", [(6, 1), (9, 2), (11, 3)])
def test_device_equals_the_model_after_random_edits(svo, oracle, depth, seed):
    O = oracle.OracleWorld.generate(1, 1, 1, 128, depth)
    D = svo.World.generate(1, 1, 1, 128, depth, build_device=0)
    rng = np.random.default_rng(seed)
    state = rng.bit_generator.state
    random_edits(oracle, O, 0, rng, 40, depth)
    rng.bit_generator.state = state                     # the same boxes again, on the device
    voxel = 128.0 / (1 << depth)
    for _ in range(40):
        op = int(rng.integers(0, 3))
        edge = float(rng.choice([voxel, 3 * voxel, 7.3, 20.0, 64.0]))
        lo = rng.uniform(-4, 120, 3)
        if rng.random() < 0.5:
            lo = np.floor(lo / voxel) * voxel
        hi = lo + edge * rng.uniform(0.3, 1.0, 3)
        D.edit_box(0, op, lo.astype(np.float32), hi.astype(np.float32), int(rng.integers(1, 8)))
    c = O.chunk(0)
    same_pools(D.chunk(0), c, f"depth {depth}: the edits themselves")
    D2 = svo.World.generate(1, 1, 1, 128, depth, build_device=0)
    D2.update(0, c, realloc=True)
    assert D.compact(0) == svo.SVO_OK
    want = M.compact(c)
    same_pools(D.chunk(0), want, f"depth {depth}, compact")
    assert D.info.total_trees == want["tree"].size
    assert D.coarsen(0) == svo.SVO_OK
    same_pools(D.chunk(0), M.coarsen(want, full=False), f"depth {depth}, compact then coarsen")
    assert D2.coarsen(0) == svo.SVO_OK                  # coarsen straight from the edited pools
    same_pools(D2.chunk(0), M.coarsen(c, full=False), f"depth {depth}, coarsen")
    rays = random_rays(np.random.default_rng(seed + 100), 20000, (0, 0, 0), (128, 128, 128))
    march_equals_oracle(svo, oracle, D, (1, 1, 1), rays, f"depth {depth} compacted + coarsened")
    D.destroy(); D2.destroy()


def test_device_equals_the_host_path_on_c3_chunks(svo):
    """C3's world (4x1x4, depth 12, built on the device): chunks compacted / coarsened on the device equal the host path's result on
    the same pools; status SVO_OK (the wide trees are rebuilt); max_chunk_depth follows coarsening.  Times are printed."""
    W = svo.World.generate(4, 1, 4, 128, 12, build_device=0)
    for i in (0, 5):
        src = W.chunk(i)
        H = svo.World.create([src], 1, 1, 1, 128)
        t0 = time.time(); assert H.compact(0) == svo.SVO_OK; t1 = time.time()
        t2 = time.time(); assert W.compact(i) == svo.SVO_OK; t3 = time.time()
        a, b = W.chunk(i, copy=False), H.chunk(0, copy=False)
        same_pools(a, b, f"C3 chunk {i}, compact")
        print(f"\nC3 chunk {i}: {src['tree'].size} nodes / {src['twig'].size // 64} bricks -> {a['tree'].size} / {a['twig'].size // 64};"
              f" compact host {t1 - t0:.3f} s, device {t3 - t2:.3f} s")
        t0 = time.time(); assert H.coarsen(0) == svo.SVO_OK; t1 = time.time()
        t2 = time.time(); assert W.coarsen(i) == svo.SVO_OK; t3 = time.time()
        a, b = W.chunk(i, copy=False), H.chunk(0, copy=False)
        same_pools(a, b, f"C3 chunk {i}, coarsen")
        print(f"C3 chunk {i} coarsened: {a['tree'].size} / {a['twig'].size // 64}; coarsen host {t1 - t0:.3f} s, device {t3 - t2:.3f} s")
        H.destroy()
    assert W.info.max_chunk_depth == 12
    for i in range(16):
        if i not in (0, 5):
            assert W.coarsen(i) == svo.SVO_OK
    assert W.info.max_chunk_depth == 11
    cam = svo.make_camera((256.3, 150.0, -40.0), (0.0, -0.5, 0.866), (0.0, 1.0, 0.0), 60.0, 320, 180)
    g = W.draw(cam, shadow=True)
    assert (g["flags"] & 1).sum() > 1000
    W.destroy()


def test_mixed_depths_march_equal_to_the_oracle_and_edits_follow(svo, oracle):
    """Compact and coarsen a mix of chunks (depths 8, 7, 6 in one world), march primary + shadow rays and a camera with both kernels
    against the oracle over the pools read back; then an edit on a compacted chunk still marches equal."""
    D = svo.World.generate(2, 1, 2, 128, 8, build_device=0)
    rng = np.random.default_rng(77)
    for i in range(4):
        x0 = (i % 2) * 128.0
        z0 = (i // 2) * 128.0
        D.edit_box(i, svo.EDIT_DESTROY, (x0 + 10, 0, z0 + 10), (x0 + 70, 40, z0 + 50))
        D.edit_box(i, svo.EDIT_BUILD, (x0 + 30, 30, z0 + 30), (x0 + 90, 90, z0 + 80), int(rng.integers(1, 8)))
    assert D.compact(0) == svo.SVO_OK
    assert D.coarsen(1) == svo.SVO_OK
    assert D.coarsen(2) == svo.SVO_OK and D.coarsen(2) == svo.SVO_OK
    assert D.compact(3) == svo.SVO_OK and D.coarsen(3) == svo.SVO_OK
    assert [D.chunk(i, copy=False)["depth"] for i in range(4)] == [8, 7, 6, 7] and D.info.max_chunk_depth == 8
    rays = random_rays(np.random.default_rng(5), 30000, (0, 0, 0), (256, 128, 256))
    march_equals_oracle(svo, oracle, D, (2, 1, 2), rays, "mixed depths")
    O = oracle.OracleWorld.from_chunks([D.chunk(i) for i in range(4)], 2, 1, 2, 128)
    cam = svo.default_camera(2, 2, 128, 96, 64)
    want = O.trace_image(cam, params=oracle.make_params(shadow=True))
    for kern in (svo.KERNEL_STACK, svo.KERNEL_LITERAL):
        assert_gbuffer_equal(D.draw(cam, shadow=True, kernel=kern), want, f"camera / kernel {kern}")
    D.edit_box(0, svo.EDIT_REPLACE, (40.5, 20.25, 40.5), (80.0, 70.0, 60.0), 4)
    D.edit_box(2, svo.EDIT_DESTROY, (20.0, 0.0, 150.0), (60.0, 60.0, 200.0))
    march_equals_oracle(svo, oracle, D, (2, 1, 2), rays, "edits after compact / coarsen")
    D.destroy()


def test_launches_issued_before_coarsen_see_the_old_world(svo, oracle):
    """Launches queued on a non-blocking stream before svo_world_coarsen march the old pools (node indices included), launches
    after it the new ones."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so.7")
    st = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0            # hipStreamNonBlocking
    D = svo.World.generate(1, 1, 1, 128, 8, build_device=0)
    cam = svo.default_camera(1, 1, 128, 256, 256)
    prm_o = oracle.make_params(shadow=True)
    before = oracle.OracleWorld.from_chunks([D.chunk(0)], 1, 1, 1, 128).trace_image(cam, params=prm_o, threads=8)
    prm = svo.trace_params(shadow=True, kernel=svo.KERNEL_STACK)
    n = 8
    bufs = [svo.DeviceBuffer(256 * 256 * 32) for _ in range(2 * n)]
    for b in bufs[:n]:
        D.trace(cam, prm, (0, 0, 256, 256), b.ptr, st.value)             # queued, not waited for
    assert D.coarsen(0) == svo.SVO_OK
    for b in bufs[n:]:
        D.trace(cam, prm, (0, 0, 256, 256), b.ptr, st.value)
    svo.lib.svo_stream_synchronize(st.value)
    after = oracle.OracleWorld.from_chunks([D.chunk(0)], 1, 1, 1, 128).trace_image(cam, params=prm_o, threads=8)
    assert not np.array_equal(before["node"], after["node"])
    for k, b in enumerate(bufs):
        assert_gbuffer_equal(b.to_numpy(svo.HIT_DTYPE, 256 * 256), before if k < n else after, f"launch {k}")
        b.free()
    hip.hipStreamDestroy(st)
    D.destroy()
