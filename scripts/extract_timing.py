"""Wall time of svo_world_chunk_extract: a window of depth D - 2 at an odd offset, in the mirrored orientation 11, out of a generated
terrain chunk of depth D = 8, 9, 10 (the window put across the terrain's surface) into the chunk of a second world, beside the dense
route on the same inputs in the same run (svo_world_chunk_to_grid of A, one torch slice, flip and permute, one svo_world_chunk_from_grid; the pools compared), and at depths 12
and 16 - where no dense route exists - a depth-10 window at an odd offset out of the solid cube of tests/combine_model.py with the
filled depth-10 sphere stamped onto its far corner (with SVO_BUILD_TIMING the library prints the entries, the node words in and out and
the working bytes of each call on stderr).  Every call is complete at its return; the destination is put back (outside the timing)
before each timed call, the first timed call is dropped and the best of the next three is reported.  A report, not a gate;
profiles/extract.txt and DESIGN.md 6zf quote it.
  python scripts/extract_timing.py [--only DEPTH]     (--only: one call out of the chunk of that depth and nothing else, for a kernel trace)"""
import importlib, os, sys, time
import numpy as np
import torch                                                # (before the library: both share one HIP runtime)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
os.environ["SVO_BUILD_TIMING"] = "1"
svo = importlib.import_module("octree-raymarcher_amd")
import combine_model as K
import mesh_model as M
import stamp_model as T

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
model = svo.World.create([empty], 1, 1, 1, 128).upload(0)

def stale(W, depth):
    """The destination before a call: one LEAF word at the result's depth."""
    W.update(0, dict(empty, depth=depth, tree=np.array([(1 << 30) | 9], np.uint32)), (0, 1), (0, 0), True)

def device_mesh(m):
    v, ix = np.ascontiguousarray(m["vertices"], np.float32), np.ascontiguousarray(m["indices"], np.uint32)
    bv, bi = svo.DeviceBuffer.from_numpy(v), svo.DeviceBuffer.from_numpy(ix)
    return svo.Mesh(bv.ptr, bi.ptr, None, v.shape[0], ix.shape[0], m.get("origin", (0.0, 0.0, 0.0)), m.get("cell", 1.0), m.get("material", 1)), (bv, bi)

def solid(W, meshes, depth, material):
    structs, bufs = zip(*[device_mesh(m) for m in meshes])
    W.chunk_from_mesh(0, list(structs), depth)
    W.chunk_fill_enclosed(0, material)
    for pair in bufs:
        for b in pair:
            b.free()

def deep(W, depth):
    """Cube A of combine_model at `depth` with the filled depth-10 UV sphere stamped onto its far corner; returns the odd offset of a
    depth-10 window that holds most of both."""
    solid(W, K.cube_meshes(depth)[0], depth, K.MATERIAL_A)
    v, ix = M.sphere_case(10)
    solid(model, [dict(vertices=v, indices=ix, material=5)], 10, 9)
    c = K.DEEP[depth][0]
    W.chunk_stamp(0, model, 0, (c - 255, c - 255, c - 255), 0, svo.COMBINE_MAX)
    return (c - 251, c - 253, c - 249)

MIRROR = 11                                                 # (x,z,y) with x and y flipped: a mirror
if len(sys.argv) > 2 and sys.argv[1] == "--only":
    depth = int(sys.argv[2])
    W = svo.World.create([empty], 1, 1, 1, 128).upload(0)
    offset = deep(W, depth)
    stale(model, 10)
    print(f"depth {depth}: {model.chunk_extract(0, W, 0, offset, MIRROR)} cells occupied", flush=True)
    W.destroy(); model.destroy()
    sys.exit(0)

def turned(window, orient):
    """G_C of a [z, y, x] torch window: what tests/stamp_model.oriented turns back into the window."""
    xyz = window.permute(2, 1, 0)
    flips = [i for i in range(3) if (orient >> i) & 1]
    if flips:
        xyz = xyz.flip(flips)
    inverse = [0, 0, 0]
    for i, p in enumerate(T.PERMS[orient >> 3]):
        inverse[p] = i
    return xyz.permute(*inverse).permute(2, 1, 0).contiguous()

print(f"== dense route against svo_world_chunk_extract (orient {MIRROR}, odd offset), ms wall, best of 3 after the first ==", flush=True)
for depth in (8, 9, 10):
    n, nc = 1 << depth, 1 << (depth - 2)
    W = svo.World.generate(1, 1, 1, 128, depth).upload(0)
    terrain = W.chunk(0)
    # (x, y, z), odd on every axis; y puts the window across the terrain's surface: of the odd heights tried (outside the timing),
    # the one whose window is nearest to half full
    x0, z0 = n // 2 - nc // 2 + 1, n // 2 - nc // 2 - 5
    stale(model, depth - 2)
    fill = {y: model.chunk_extract(0, W, 0, (x0, y, z0), MIRROR) for y in range(1, n - nc, nc // 4)}
    offset = (x0, min(fill, key=lambda y: abs(fill[y] - nc ** 3 // 2)), z0)
    ga = torch.empty(n ** 3, dtype=torch.int16, device="cuda")               # (the materials here are below 2^15)
    def dense():
        W.chunk_to_grid(0, depth, ga.data_ptr())
        svo.lib.svo_stream_synchronize(None)                # (torch runs on a stream of its own)
        gc = turned(ga.view(n, n, n)[offset[2]:offset[2] + nc, offset[1]:offset[1] + nc, offset[0]:offset[0] + nc], MIRROR)
        torch.cuda.synchronize()
        model.chunk_from_grid(0, gc.data_ptr(), depth - 2)
        svo.lib.svo_stream_synchronize(None)
    counts = {}
    def sparse():
        counts["occupied"] = model.chunk_extract(0, W, 0, offset, MIRROR)
    td = best_of_3_after_the_first(lambda: stale(model, depth - 2), dense)
    a = model.chunk(0)
    ts = best_of_3_after_the_first(lambda: stale(model, depth - 2), sparse)
    b = model.chunk(0)
    same = np.array_equal(a["tree"], b["tree"]) and np.array_equal(a["twig"], b["twig"])
    print(f"depth {depth:2d} terrain {terrain['tree'].size} words, {terrain['twig'].size // 64} bricks  window of depth {depth - 2} at {offset}  dense route {td:9.2f} ms  "
          f"extract {ts:9.2f} ms  pools equal: {same}  {counts['occupied']} cells occupied  ({b['tree'].size} words, {b['twig'].size // 64} bricks out)", flush=True)
    sys.stderr.flush()
    del ga
    torch.cuda.empty_cache()
    W.destroy()

print("== beyond the dense grid: a depth-10 window out of the solid cube with the depth-10 sphere on its corner (SVO_BUILD_TIMING prints entries, node words, working bytes on stderr) ==", flush=True)
W = svo.World.create([empty], 1, 1, 1, 128).upload(0)
for depth in (12, 16):
    offset = deep(W, depth)
    source = W.info
    counts = {}
    def sparse():
        counts["occupied"] = model.chunk_extract(0, W, 0, offset, MIRROR)
    ts = best_of_3_after_the_first(lambda: stale(model, 10), sparse)
    info = model.info
    print(f"depth {depth:2d} cube of 258 cells and sphere of depth 10, window of depth 10 at {offset}  extract {ts:9.2f} ms  {counts['occupied']} cells occupied  "
          f"{source.total_trees} words, {source.total_twigs} bricks -> {info.total_trees} words, {info.total_twigs} bricks", flush=True)
    sys.stderr.flush()
W.destroy(); model.destroy()
