"""Wall time of svo_world_chunk_fill_enclosed on the shells of the spheres of scripts/sparse_mesh_timing.py: at depths 8, 9, 10
against the dense route (svo_world_chunk_to_grid + svo_device_grid_fill_enclosed + svo_world_chunk_from_grid, the pools compared), at
depths 12, 14, 16 alone (with SVO_BUILD_TIMING the library prints the sweeps, the cells filled and the working bytes of each call on
stderr).  Every call is complete at its return; the shell is rebuilt (outside the timing) before each timed call, the first timed call
is dropped and the best of the next three is reported.  A report, not a gate; profiles/sparse_fill.txt and DESIGN.md 6zb quote it.
  python scripts/sparse_fill_timing.py [--only DEPTH]     (--only: one sparse call at that depth and nothing else, for a kernel trace)"""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
os.environ["SVO_BUILD_TIMING"] = "1"
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

def best_of_3_after_the_first(prepare, f):
    times = []
    for _ in range(4):
        prepare()
        times.append(wall(f))
    return min(times[1:])

empty = dict(position=(0.0, 0.0, 0.0), size=128.0, depth=3, tree=np.zeros(1, np.uint32), twig=np.zeros(0, np.uint16))
W = svo.World.create([empty, dict(empty, position=(128.0, 0.0, 0.0))], 2, 1, 1, 128).upload(0)
DEEP = {12: (1597.0, 0.5, 192, 128), 14: (3195.0, 0.5, 512, 384), 16: (3195.0, 0.7, 512, 384)}

def deep_mesh(depth):
    radius, at, nu, nv = DEEP[depth]
    n = 1 << depth
    return fast_sphere((at * n + 0.13, at * n - 0.21, at * n + 0.07), radius, nu, nv)

if len(sys.argv) > 2 and sys.argv[1] == "--only":
    depth = int(sys.argv[2])
    v, ix = deep_mesh(depth)
    bv, bi = svo.DeviceBuffer.from_numpy(v), svo.DeviceBuffer.from_numpy(ix)
    W.chunk_from_mesh(0, [svo.Mesh(bv.ptr, bi.ptr, None, v.shape[0], ix.shape[0], (0.0, 0.0, 0.0), 1.0, 5)], depth)
    print(f"depth {depth}: {W.chunk_fill_enclosed(0, 9)} cells filled", flush=True)
    W.destroy()
    sys.exit(0)

print("== dense route against the sparse fill, ms wall, best of 3 after the first ==", flush=True)
for depth in (8, 9, 10):
    n = 1 << depth
    v, ix = M.sphere_case(depth)
    bv, bi = svo.DeviceBuffer.from_numpy(v), svo.DeviceBuffer.from_numpy(ix)
    mesh = svo.Mesh(bv.ptr, bi.ptr, None, v.shape[0], ix.shape[0], (0.0, 0.0, 0.0), 1.0, 5)
    grid = svo.DeviceBuffer(n ** 3 * 2)
    shell = lambda: W.chunk_from_mesh(0, [mesh], depth)
    counts = {}
    def dense():
        W.chunk_to_grid(0, depth, grid.ptr)
        counts["dense"] = svo.device_grid_fill_enclosed(grid.ptr, depth, 9)
        W.chunk_from_grid(0, grid.ptr, depth)
    def sparse():
        counts["sparse"] = W.chunk_fill_enclosed(0, 9)
    td = best_of_3_after_the_first(shell, dense)
    a = W.chunk(0)
    ts = best_of_3_after_the_first(shell, sparse)
    b = W.chunk(0)
    same = np.array_equal(a["tree"], b["tree"]) and np.array_equal(a["twig"], b["twig"]) and counts["dense"] == counts["sparse"]
    print(f"depth {depth:2d} uv-sphere 168 tri  dense route {td:9.2f} ms  sparse fill {ts:9.2f} ms  pools and counts equal: {same}  "
          f"({counts['sparse']} cells filled; {b['tree'].size} words, {b['twig'].size // 64} bricks)", flush=True)
    sys.stderr.flush()
    for x in (bv, bi, grid):
        x.free()

print("== the sparse fill beyond the dense grid (SVO_BUILD_TIMING prints sweeps, cells filled, working bytes on stderr) ==", flush=True)
# per depth its own sphere of DESIGN.md 6za and, at 14 and 16, the depth-12 one again at that depth's centre (the host form fills it too:
# the counts are compared)
for depth, (radius, at, nu, nv), check in [(d, DEEP[d], d == 12) for d in (12, 14, 16)] + [(d, (DEEP[12][0], DEEP[d][1]) + DEEP[12][2:], True) for d in (14, 16)]:
    n = 1 << depth
    v, ix = fast_sphere((at * n + 0.13, at * n - 0.21, at * n + 0.07), radius, nu, nv)
    bv, bi = svo.DeviceBuffer.from_numpy(v), svo.DeviceBuffer.from_numpy(ix)
    mesh = svo.Mesh(bv.ptr, bi.ptr, None, v.shape[0], ix.shape[0], (0.0, 0.0, 0.0), 1.0, 5)
    counts = {}
    def sparse():
        counts["sparse"] = W.chunk_fill_enclosed(0, 9)
    W.chunk_from_mesh(0, [mesh], depth)
    shell = W.info
    ts = best_of_3_after_the_first(lambda: W.chunk_from_mesh(0, [mesh], depth), sparse)
    info = W.info
    host = ""
    if check:
        h = svo.chunk_from_mesh([dict(vertices=v, indices=ix, material=5)], depth)
        host = f"  host form: shell {h['tree'].size} words, {h['twig'].size // 64} bricks, {svo.chunk_fill_enclosed(h, 9)[1]} cells filled"
    print(f"depth {depth:2d} uv-sphere r={radius:.0f} cells {ix.shape[0]} tri  sparse fill {ts:9.2f} ms  {counts['sparse']} cells filled  "
          f"shell {shell.total_trees} words, {shell.total_twigs} bricks -> {info.total_trees} words, {info.total_twigs} bricks{host}", flush=True)
    sys.stderr.flush()
    for x in (bv, bi):
        x.free()
W.destroy()
