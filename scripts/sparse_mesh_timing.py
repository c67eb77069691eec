"""Wall time of the dense path (svo_device_grid_add_mesh + svo_world_chunk_from_grid) and of svo_world_chunk_from_mesh on the same
meshes at depths 8, 9, 10, and of the sparse call alone at depths 12, 14, 16 (with SVO_BUILD_TIMING the library prints the tile jobs,
the overlaps, the cells and the working bytes of each call on stderr).  Both paths are complete at their return: wall time around
the second call of each.  A report, not a gate; profiles/sparse_mesh.txt and DESIGN.md 6za quote it.
  python scripts/sparse_mesh_timing.py"""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
svo = importlib.import_module("octree-raymarcher_amd")
import mesh_model as M

def fast_sphere(centre, radius, nu, nv):
    th = np.pi * np.arange(1, nv) / nv
    ph = 2 * np.pi * np.arange(nu) / nu
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(nu))], -1).reshape(-1, 3)
    verts = np.concatenate([[[0, 0, 1.0]], ring, [[0, 0, -1.0]]])
    r = lambda a, k: 1 + (a - 1) * nu + k % nu
    k = np.arange(nu)
    tris = [np.stack([np.zeros(nu, int), r(1, k), r(1, k + 1)], -1)]
    for a in range(1, nv - 1):
        tris += [np.stack([r(a, k), r(a + 1, k), r(a + 1, k + 1)], -1), np.stack([r(a, k), r(a + 1, k + 1), r(a, k + 1)], -1)]
    tris.append(np.stack([np.full(nu, len(verts) - 1), r(nv - 1, k + 1), r(nv - 1, k)], -1))
    return (np.asarray(centre) + radius * verts).astype(np.float32), np.concatenate(tris).astype(np.uint32)

def wall(f):
    svo.lib.svo_stream_synchronize(None)
    t = time.perf_counter(); f(); return (time.perf_counter() - t) * 1e3

empty = dict(position=(0.0, 0.0, 0.0), size=128.0, depth=3, tree=np.zeros(1, np.uint32), twig=np.zeros(0, np.uint16))
W = svo.World.create([empty, dict(empty, position=(128.0, 0.0, 0.0))], 2, 1, 1, 128).upload(0)

def upload(v, ix, mats):
    bv, bi = svo.DeviceBuffer.from_numpy(v), svo.DeviceBuffer.from_numpy(ix)
    bm = None if mats is None else svo.DeviceBuffer.from_numpy(mats)
    return bv, bi, bm

print("== dense path against the sparse call, ms wall, second call of each ==", flush=True)
for depth in (8, 9, 10):
    n = 1 << depth
    for name, (v, ix, mats) in (("uv-sphere 168 tri", (*M.sphere_case(depth), None)), ("soup 100k tri", M.soup(21, 100000, n, small=2.0))):
        bv, bi, bm = upload(v, ix, mats)
        grid = svo.DeviceBuffer(n ** 3 * 2)
        def dense():
            svo.device_grid_add_mesh(grid.ptr, depth, bv.ptr, v.shape[0], bi.ptr, ix.shape[0], material=5, materials_ptr=bm.ptr if bm else None)
            W.chunk_from_grid(0, grid.ptr, depth)
        mesh = svo.Mesh(bv.ptr, bi.ptr, bm.ptr if bm else None, v.shape[0], ix.shape[0], (0.0, 0.0, 0.0), 1.0, 5)
        sparse = lambda: W.chunk_from_mesh(0, [mesh], depth)
        td = []
        for _ in range(2):
            W.chunk_to_grid(1, depth, grid.ptr)             # chunk 1 is empty: clears the grid on the device, outside the timing
            td.append(wall(dense))
        a = W.chunk(0)
        ts = [wall(sparse), wall(sparse)]
        b = W.chunk(0)
        same = np.array_equal(a["tree"], b["tree"]) and np.array_equal(a["twig"], b["twig"])
        print(f"depth {depth:2d} {name:18s} dense {td[1]:9.2f} ms  sparse {ts[1]:9.2f} ms  pools equal: {same}  ({b['tree'].size} words, {b['twig'].size // 64} bricks)", flush=True)
        for x in (bv, bi, bm, grid):
            if x: x.free()

print("== the sparse call beyond the dense grid (SVO_BUILD_TIMING prints overlaps, cells, working bytes on stderr) ==", flush=True)
os.environ["SVO_BUILD_TIMING"] = "1"
for depth, radius, at, nu, nv in ((12, 1597.0, 0.5, 192, 128), (14, 3195.0, 0.5, 512, 384), (16, 3195.0, 0.7, 512, 384)):
    n = 1 << depth
    for name, (v, ix, mats) in ((f"uv-sphere r={radius:.0f} cells {2 * nu * (nv - 1)} tri", (*fast_sphere((at * n + 0.13, at * n - 0.21, at * n + 0.07), radius, nu, nv), None)),
                                ("soup 100k tri", M.soup(21, 100000, n, small=2.0))):
        bv, bi, bm = upload(v, ix, mats)
        mesh = svo.Mesh(bv.ptr, bi.ptr, bm.ptr if bm else None, v.shape[0], ix.shape[0], (0.0, 0.0, 0.0), 1.0, 5)
        sparse = lambda: W.chunk_from_mesh(0, [mesh], depth)
        ts = [wall(sparse), wall(sparse)]
        info = W.info
        print(f"depth {depth:2d} {name:40s} sparse {ts[1]:9.2f} ms (first call {ts[0]:9.2f})  {info.total_trees} words, {info.total_twigs} bricks", flush=True)
        sys.stderr.flush()
        for x in (bv, bi, bm):
            if x: x.free()
W.destroy()
