"""Wall time of svo_world_chunk_stamp (MAX): the UV sphere of scripts/sparse_fill_timing.py, filled, at depth D - 2, stamped at an odd
offset into a generated terrain chunk of depth D = 8, 9, 10, beside the dense route on the same inputs (svo_world_chunk_to_grid of A and
of B, one torch slice-assign, one svo_world_chunk_from_grid; the pools compared), once more in a mirrored orientation, and at depths 12
and 16 - where no dense route exists - the depth-10 sphere into the solid cube of tests/combine_model.py (with SVO_BUILD_TIMING the
library prints the entries, the node words in and out and the working bytes of each call on stderr).  Every call is complete at its
return; chunk A is put back (outside the timing) before each timed call, the first timed call is dropped and the best of the next three
is reported.  A report, not a gate; profiles/stamp.txt and DESIGN.md 6ze quote it.
  python scripts/stamp_timing.py [--only DEPTH]     (--only: one MAX call into the cube of that depth and nothing else, for a kernel trace)"""
import importlib, os, sys, time
import numpy as np
import torch                                                # (before the library: both share one HIP runtime)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
os.environ["SVO_BUILD_TIMING"] = "1"
svo = importlib.import_module("octree-raymarcher_amd")
import combine_model as K
import mesh_model as M

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

def put(W, chunk):
    W.update(0, dict(chunk, position=(0.0, 0.0, 0.0), size=128.0), (0, chunk["tree"].size), (0, chunk["twig"].size // 64), True)

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

def sphere(depth):
    """The filled UV sphere at `depth` becomes the model world's chunk."""
    v, ix = M.sphere_case(depth)
    solid(model, [dict(vertices=v, indices=ix, material=5)], depth, 9)

def deep(W, depth):
    """Cube A of combine_model at `depth`, the depth-10 sphere as B; returns the odd offset that puts the sphere's centre on the cube's
    far corner (c + 257), so that an eighth of the sphere and the cube overlap."""
    solid(W, K.cube_meshes(depth)[0], depth, K.MATERIAL_A)
    sphere(10)
    c = K.DEEP[depth][0]
    return (c - 255, c - 255, c - 255)

if len(sys.argv) > 2 and sys.argv[1] == "--only":
    depth = int(sys.argv[2])
    W = svo.World.create([empty], 1, 1, 1, 128).upload(0)
    offset = deep(W, depth)
    print(f"depth {depth}: {W.chunk_stamp(0, model, 0, offset, 0, svo.COMBINE_MAX)} cells changed", flush=True)
    W.destroy(); model.destroy()
    sys.exit(0)

MIRROR = 11                                                 # (x,z,y) with x and y flipped: a mirror
print("== dense route against svo_world_chunk_stamp (MAX, odd offset), ms wall, best of 3 after the first ==", flush=True)
for depth in (8, 9, 10):
    n, nb = 1 << depth, 1 << (depth - 2)
    W = svo.World.generate(1, 1, 1, 128, depth).upload(0)
    terrain = W.chunk(0)
    sphere(depth - 2)
    offset = (n // 2 - nb // 2 + 1, n // 4 + 3, n // 2 - nb // 2 - 5)        # (x, y, z), odd on every axis
    ga, gb = torch.empty(n ** 3, dtype=torch.int16, device="cuda"), torch.empty(nb ** 3, dtype=torch.int16, device="cuda")     # (the materials here are below 2^15)
    def dense():
        W.chunk_to_grid(0, depth, ga.data_ptr())
        model.chunk_to_grid(0, depth - 2, gb.data_ptr())
        svo.lib.svo_stream_synchronize(None)                # (torch runs on a stream of its own)
        part = ga.view(n, n, n)[offset[2]:offset[2] + nb, offset[1]:offset[1] + nb, offset[0]:offset[0] + nb]
        part.copy_(torch.maximum(part, gb.view(nb, nb, nb)))
        torch.cuda.synchronize()
        W.chunk_from_grid(0, ga.data_ptr(), depth)
    counts = {}
    def sparse(orient=0):
        counts["changed"] = W.chunk_stamp(0, model, 0, offset, orient, svo.COMBINE_MAX)
    td = best_of_3_after_the_first(lambda: put(W, terrain), dense)
    a = W.chunk(0)
    ts = best_of_3_after_the_first(lambda: put(W, terrain), sparse)
    b = W.chunk(0)
    tm = best_of_3_after_the_first(lambda: put(W, terrain), lambda: sparse(MIRROR))
    same = np.array_equal(a["tree"], b["tree"]) and np.array_equal(a["twig"], b["twig"])
    print(f"depth {depth:2d} terrain {terrain['tree'].size} words, {terrain['twig'].size // 64} bricks  filled uv-sphere of depth {depth - 2} at {offset}  dense route {td:9.2f} ms  "
          f"stamp {ts:9.2f} ms  mirrored {tm:9.2f} ms  pools equal: {same}  ({b['tree'].size} words, {b['twig'].size // 64} bricks out)", flush=True)
    sys.stderr.flush()
    del ga, gb
    torch.cuda.empty_cache()
    W.destroy()

print("== beyond the dense grid: the depth-10 sphere into the solid cube (SVO_BUILD_TIMING prints entries, node words, working bytes on stderr) ==", flush=True)
W = svo.World.create([empty], 1, 1, 1, 128).upload(0)
for depth in (12, 16):
    offset = deep(W, depth)
    cube = W.chunk(0)
    for name, op in (("MAX", svo.COMBINE_MAX), ("SUBTRACT", svo.COMBINE_SUBTRACT)):
        counts = {}
        def sparse():
            counts["changed"] = W.chunk_stamp(0, model, 0, offset, MIRROR, op)
        ts = best_of_3_after_the_first(lambda: put(W, cube), sparse)
        info = W.info
        print(f"depth {depth:2d} cube of 258 cells, sphere of depth 10 at {offset} {name:8s} stamp {ts:9.2f} ms  {counts['changed']} cells changed  "
              f"{cube['tree'].size} words, {cube['twig'].size // 64} bricks -> {info.total_trees} words, {info.total_twigs} bricks", flush=True)
        sys.stderr.flush()
W.destroy(); model.destroy()
