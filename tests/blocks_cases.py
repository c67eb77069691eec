#!/usr/bin/env python3
"""The worlds, ray lists and images of tests/test_gpu_blocks.py, and the march of them through ONE build of the library in its own
process (the binding loads one library per process, like tests/variant_check.py).  Test infrastructure.

    python tests/blocks_cases.py <path to libsvo_*.so> <reference.npz>

marches everything with the stack kernel and compares the records with the oracle's, which the test computed once and stored in
<reference.npz>.  exit 0 = every check passed.

What is marched are the blocks of k_trace_stack around its march step (kernel_stack.hip.h): the chunk step (chunk index and chunk
tables), tile generation (camera rasters through every entry point) and the hit resolve (node and cell ids, materials, normals).
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHUNK = 128
RAYS = 4096

# ---- chunk step: grids with a dimension that is no power of two, negative chunk coordinates, and 72 chunks - more than the
# 64 (large pools: 126) entries of the chunk table in LDS, so that the table is read from global memory.  (name, dims, depth, ccm)
GRID_WORLDS = [("3x1x2", (3, 1, 2), 4, (0, 0, 0)), ("3x1x2neg", (3, 1, 2), 4, (-2, 0, -1)), ("2x2x2neg", (2, 2, 2), 4, (-1, -1, -1)),
               ("9x1x8", (9, 1, 8), 3, (-4, 0, 3))]
# ---- tile generation: rasters whose last tiles are ragged in one or both directions, on a 2x1x2 world of depth 6
TILE_WORLD = ((2, 1, 2), 6, (0, 0, 0))
TILE_IMAGES = [(40, 24), (37, 21)]
TILE_RECT_X0, TILE_RECT_Y0 = 5, 3       # the rectangle that does not start at 0: (5, 3) to the image's lower right corner
BAND, RANKS = 8, 3
# ---- hit resolve
HIT_DEPTH = 5                           # 32 cells per axis: tree levels 0 - 3, bricks of 4^3 cells below level 3
HIT_MODES = [(nm, sh) for nm in (0, 1) for sh in (False, True)]     # (normal mode, shadow ray)


def box_of(dims, ccm):
    lo = np.array(ccm, np.float64) * CHUNK
    return lo, lo + np.array(dims, np.float64) * CHUNK


def lattice_plane_rays(rng, n, lo, hi):
    """Origins with one to three coordinates exactly on a chunk lattice plane (multiples of the chunk edge, the world's faces among
    them), generic directions and, for a quarter, axis-parallel ones: the chunk step's floor(p / chunksize) is taken at exact
    multiples, on either side of 0, and a ray runs along the seam between chunks."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    o = lo + rng.random((n, 3)) * (hi - lo)
    for j in range(n):
        for a in rng.permutation(3)[: rng.integers(1, 4)]:
            o[j, a] = np.round(o[j, a] / CHUNK) * CHUNK
    d = rng.normal(size=(n, 3))
    q = n // 4
    ax = rng.integers(0, 3, q)
    d[:q] = 0.0
    d[np.arange(q), ax] = rng.choice([-1.0, 1.0], q)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


def grid_lists(name, dims, ccm):
    sys.path.insert(0, HERE)
    from helpers import random_rays
    rng = np.random.default_rng(9000 + sum(ord(c) for c in name))
    lo, hi = box_of(dims, ccm)
    return {"random": random_rays(rng, RAYS, lo, hi), "lattice": lattice_plane_rays(rng, RAYS, lo, hi)}


def grid_camera(svo, dims, ccm):
    lo, hi = box_of(dims, ccm)
    eye = (float(lo[0] + 0.31 * (hi[0] - lo[0])) + 0.37, float(hi[1]) + 40.0, float(lo[2]) - 35.0)
    return svo.make_camera(eye, (0.12, -0.55, 0.83), (0.0, 1.0, 0.0), 70.0, 45, 27)


def tile_cameras(svo, w, h):
    return [svo.make_camera((100.0 + 23.0 * f, 140.0 - 6.0 * f, -30.0 + 5.0 * f), (0.06 * f, -0.5, 0.8), (0.0, 1.0, 0.0), 55.0 + 4.0 * f, w, h)
            for f in range(3)]


def hit_chunks(svo):
    """Two chunks of depth 5 from grids.  Chunk 0 is one material throughout: its root is a LEAF, level 0.  Chunk 1, below y = 16:
    4^3 blocks that are solid (LEAF nodes at the deepest level), of several materials (a brick whose bmat entry is 0xFFFF: the
    material is read from the brick itself), of one material with holes (a brick with one material) or empty, and one solid 8^3
    block (a LEAF one level up)."""
    n = 1 << HIT_DEPTH
    rng = np.random.default_rng(31)
    solid = np.full((n, n, n), 7, np.uint16)
    g = np.zeros((n, n, n), np.uint16)                       # [z, y, x]
    for bz in range(0, n, 4):
        for by in range(0, 16, 4):
            for bx in range(0, n, 4):
                kind = rng.integers(0, 4)
                blk = g[bz:bz + 4, by:by + 4, bx:bx + 4]
                if kind == 1:
                    blk[:] = rng.integers(1, 6)
                elif kind == 2:
                    blk[:] = rng.integers(1, 6, (4, 4, 4))
                    blk[rng.random((4, 4, 4)) < 0.3] = 0
                elif kind == 3:
                    blk[:] = rng.integers(1, 6)
                    blk[rng.random((4, 4, 4)) < 0.5] = 0
    g[8:16, 8:16, 8:16] = 9
    return [svo.chunk_from_grid(solid, position=(0.0, 0.0, 0.0), size=float(CHUNK)),
            svo.chunk_from_grid(g, position=(float(CHUNK), 0.0, 0.0), size=float(CHUNK))]


def hit_lists():
    from helpers import random_rays
    rng = np.random.default_rng(77)
    o, d = random_rays(rng, RAYS, (0.0, 0.0, 0.0), (2.0 * CHUNK, 1.0 * CHUNK, 1.0 * CHUNK), inside_frac=0.3)
    # half of them come down on chunk 1 from above, where its blocks are
    k = RAYS // 2
    o[:k, 0] = CHUNK + rng.random(k) * CHUNK
    o[:k, 1] = 70.0 + rng.random(k) * 50.0
    o[:k, 2] = rng.random(k) * CHUNK
    d[:k, 1] = -np.abs(d[:k, 1]) - 0.3
    d[:k] /= np.linalg.norm(d[:k], axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


def hit_camera(svo):
    return svo.make_camera((150.3, 118.0, -30.0), (0.1, -0.6, 0.8), (0.0, 1.0, 0.0), 65.0, 45, 27)


# ---- the oracle's records of everything above (computed once by the test)
def reference(svo, ob):
    ref = {}
    for name, dims, depth, ccm in GRID_WORLDS:
        W = svo.World.generate(*dims, CHUNK, depth, chunkcoordmin=ccm)
        O = ob.OracleWorld.from_chunks([W.chunk(i) for i in range(dims[0] * dims[1] * dims[2])], *dims, CHUNK, ccm)
        W.destroy()
        prm = ob.make_params(shadow=True)
        for lname, (o, d) in grid_lists(name, dims, ccm).items():
            ref[f"grid/{name}/{lname}"] = O.trace_rays(o, d, params=prm, threads=8)
            ref[f"grid/{name}/{lname}/rays"] = np.array([O.last_rays], np.int64)
        ref[f"grid/{name}/image"] = O.trace_image(grid_camera(svo, dims, ccm), params=prm, threads=8)
        ref[f"grid/{name}/image/rays"] = np.array([O.last_rays], np.int64)
    dims, depth, ccm = TILE_WORLD
    W = svo.World.generate(*dims, CHUNK, depth, chunkcoordmin=ccm)
    O = ob.OracleWorld.from_chunks([W.chunk(i) for i in range(4)], *dims, CHUNK, ccm)
    W.destroy()
    for (w, h) in TILE_IMAGES:
        for f, cam in enumerate(tile_cameras(svo, w, h)):
            ref[f"tile/{w}x{h}/{f}"] = O.trace_image(cam, params=ob.make_params(shadow=True), threads=8)
            ref[f"tile/{w}x{h}/{f}/rays"] = np.array([O.last_rays], np.int64)
            rect = (TILE_RECT_X0, TILE_RECT_Y0, w - TILE_RECT_X0, h - TILE_RECT_Y0)
            ref[f"tile/{w}x{h}/{f}/rect"] = O.trace_image(cam, rect=rect, params=ob.make_params(shadow=True), threads=8)
            ref[f"tile/{w}x{h}/{f}/rect/rays"] = np.array([O.last_rays], np.int64)
    O = ob.OracleWorld.from_chunks(hit_chunks(svo), 2, 1, 1, CHUNK)
    o, d = hit_lists()
    for nm, sh in HIT_MODES:
        prm = ob.make_params(shadow=sh, normal_mode=nm)
        ref[f"hit/{nm}/{int(sh)}/list"] = O.trace_rays(o, d, params=prm, threads=8)
        ref[f"hit/{nm}/{int(sh)}/image"] = O.trace_image(hit_camera(svo), params=prm, threads=8)
    return ref


# ---- the marches
def march_grids(svo, ref):
    from helpers import assert_gbuffer_equal
    for name, dims, depth, ccm in GRID_WORLDS:
        W = svo.World.generate(*dims, CHUNK, depth, chunkcoordmin=ccm)
        W.upload(0)
        for lname, (o, d) in grid_lists(name, dims, ccm).items():
            got = W.chunkmarch(o, d, shadow=True, kernel=svo.KERNEL_STACK)
            assert_gbuffer_equal(got, ref[f"grid/{name}/{lname}"], f"grid {name}/{lname}")
            assert W.last_ray_count() == int(ref[f"grid/{name}/{lname}/rays"][0]), f"grid {name}/{lname}: ray count"
        got = W.draw(grid_camera(svo, dims, ccm), shadow=True, kernel=svo.KERNEL_STACK)
        assert_gbuffer_equal(got, ref[f"grid/{name}/image"], f"grid {name}/image")
        assert W.last_ray_count() == int(ref[f"grid/{name}/image/rays"][0]), f"grid {name}/image: ray count"
        W.destroy()


def march_tiles(svo, ref):
    from helpers import assert_gbuffer_equal
    dims, depth, ccm = TILE_WORLD
    W = svo.World.generate(*dims, CHUNK, depth, chunkcoordmin=ccm)
    W.upload(0)
    sync = lambda: svo.lib.svo_stream_synchronize(None)
    for (w, h) in TILE_IMAGES:
        what = f"tile {w}x{h}"
        cams = tile_cameras(svo, w, h)
        full = [ref[f"tile/{w}x{h}/{f}"] for f in range(3)]
        rays = [int(ref[f"tile/{w}x{h}/{f}/rays"][0]) for f in range(3)]
        prm = svo.trace_params(shadow=True, kernel=svo.KERNEL_STACK)
        # svo_trace, one camera per launch
        for f, cam in enumerate(cams):
            assert_gbuffer_equal(W.draw(cam, shadow=True, kernel=svo.KERNEL_STACK), full[f], f"{what} trace, camera {f}")
            assert W.last_ray_count() == rays[f], f"{what} trace, camera {f}: ray count"
        # svo_trace_frames: three cameras in one launch, the whole raster and a rectangle that does not start at 0
        out = svo.DeviceBuffer(3 * w * h * 32)
        W.trace_frames(cams, prm, (0, 0, w, h), out.ptr)
        sync()
        plain = out.to_numpy(svo.HIT_DTYPE, 3 * w * h).copy().reshape(3, h, w)
        for f in range(3):
            assert_gbuffer_equal(plain[f], full[f], f"{what} trace_frames, frame {f}")
        assert W.last_ray_count() == sum(rays), f"{what} trace_frames: ray count"
        rw, rh = w - TILE_RECT_X0, h - TILE_RECT_Y0
        W.trace_frames(cams, prm, (TILE_RECT_X0, TILE_RECT_Y0, rw, rh), out.ptr)
        sync()
        part = out.to_numpy(svo.HIT_DTYPE, 3 * rw * rh).reshape(3, rh, rw)
        for f in range(3):
            assert_gbuffer_equal(part[f], ref[f"tile/{w}x{h}/{f}/rect"], f"{what} trace_frames, rectangle, frame {f}")
            assert part[f].tobytes() == plain[f][TILE_RECT_Y0:, TILE_RECT_X0:].tobytes(), f"{what}: the rectangle is a cut of the frame"
        assert W.last_ray_count() == sum(int(ref[f"tile/{w}x{h}/{f}/rect/rays"][0]) for f in range(3)), f"{what} rectangle: ray count"
        # svo_trace_rows_frames: every rank's 8-row bands of the three frames, the padding bands below the image included
        nb = svo.partition.bands_per_rank(h, RANKS, BAND) + 1      # (one band more than the image has for any rank: all padding)
        bands = svo.DeviceBuffer(3 * nb * BAND * w * 32)
        for rank in range(RANKS):
            W.trace_rows_frames(cams, prm, rank, RANKS, nb, BAND, bands.ptr)
            sync()
            gb = bands.to_numpy(svo.HIT_DTYPE, 3 * nb * BAND * w).reshape(3, nb, BAND, w)
            for f in range(3):
                for k in range(nb):
                    r0 = (rank + RANKS * k) * BAND
                    rows = min(BAND, max(0, h - r0))
                    assert gb[f, k, :rows].tobytes() == plain[f][r0:r0 + rows].tobytes(), f"{what} rank {rank} frame {f} band {k}"
                    assert not (gb[f, k, rows:]["flags"] & 1).any(), f"{what} rank {rank} frame {f} band {k}: padding rows hold no hit"
        bands.free()
        # the caller's tile order together with the tile costs: the same records, byte for byte, and the same ray count
        tpr = (w + 7) // 8
        nt = tpr * ((h + 7) // 8)
        cost = svo.DeviceBuffer.from_numpy(np.zeros((3, nt, 2), np.uint32))
        order = np.arange(nt, dtype=np.uint32)[::-1].copy()
        od = svo.DeviceBuffer.from_numpy(order)
        prm_o = svo.trace_params(shadow=True, kernel=svo.KERNEL_STACK, tile_cost_dev=cost.ptr, tile_order_dev=od.ptr)
        W.trace_frames(cams, prm_o, (0, 0, w, h), out.ptr)
        sync()
        assert out.to_numpy(svo.HIT_DTYPE, 3 * w * h).tobytes() == plain.tobytes(), f"{what}: records with and without a tile order"
        assert W.last_ray_count() == sum(rays), f"{what} ordered: ray count"
        c = cost.to_numpy(np.uint32, 3 * nt * 2).reshape(3, nt, 2)
        hits_per_frame = [int((full[f]["flags"] & 1).sum()) for f in range(3)]
        assert all(c[f, :, 0].max() > 0 for f in range(3) if hits_per_frame[f]), f"{what}: every frame records its tiles' costs"
        # ... and with one entry that names no tile: that tile is never handed out, its pixels stay as they were
        lost = int(order[2])
        order[2] = nt + 5
        bad = svo.DeviceBuffer.from_numpy(order)
        out1 = svo.DeviceBuffer.from_numpy(np.full(w * h * 32, 0xAB, np.uint8))
        prm_b = svo.trace_params(shadow=True, kernel=svo.KERNEL_STACK, tile_cost_dev=cost.ptr, tile_order_dev=bad.ptr)
        W.trace(cams[1], prm_b, (0, 0, w, h), out1.ptr)
        sync()
        got = out1.to_numpy(svo.HIT_DTYPE, w * h).copy().reshape(h, w)
        skipped = np.zeros((h, w), bool)
        ty, tx = divmod(lost, tpr)
        skipped[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = True
        assert got[~skipped].tobytes() == plain[1][~skipped].tobytes(), f"{what}: every tile but the skipped one"
        assert np.all(got[skipped].view(np.uint8) == 0xAB), f"{what}: the skipped tile stays unwritten"
        for b in (out, out1, cost, od, bad):
            b.free()
    W.destroy()


def march_hits(svo, ref):
    from helpers import assert_gbuffer_equal
    W = svo.World.create(hit_chunks(svo), 2, 1, 1, CHUNK)
    W.upload(0)
    o, d = hit_lists()
    for nm, sh in HIT_MODES:
        got = W.chunkmarch(o, d, shadow=sh, kernel=svo.KERNEL_STACK, normal_mode=nm)
        assert_gbuffer_equal(got, ref[f"hit/{nm}/{int(sh)}/list"], f"hit resolve list, normal mode {nm}, shadow {sh}")
        got = W.draw(hit_camera(svo), shadow=sh, kernel=svo.KERNEL_STACK, normal_mode=nm)
        assert_gbuffer_equal(got, ref[f"hit/{nm}/{int(sh)}/image"], f"hit resolve image, normal mode {nm}, shadow {sh}")
    W.destroy()


def march_all(svo, ref):
    march_grids(svo, ref)
    march_tiles(svo, ref)
    march_hits(svo, ref)


if __name__ == "__main__":
    lib_path, ref_path = os.path.abspath(sys.argv[1]), sys.argv[2]
    os.environ["SVO_AMD_LIB"] = lib_path
    for p in (HERE, ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    svo = importlib.import_module("octree-raymarcher_amd")
    assert os.path.samefile(svo.LIB_PATH, lib_path)
    if svo.device_count() < 1:
        print("no HIP device"); sys.exit(3)
    march_all(svo, np.load(ref_path, allow_pickle=False))
    print("blocks: chunk grids, tile generation and hit resolve: every record equal to the oracle's")
