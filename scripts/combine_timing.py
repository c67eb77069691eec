"""Wall time of svo_world_chunk_combine (MAX and SUBTRACT): the UV sphere of scripts/sparse_fill_timing.py, filled, against a generated
terrain chunk at depths 8, 9, 10, beside the dense route on the same inputs (two svo_world_chunk_to_grid, one elementwise torch kernel,
one svo_world_chunk_from_grid; the pools compared), and the two solid cubes of tests/combine_model.py at depths 12 and 16 alone (with
SVO_BUILD_TIMING the library prints the entries, the output and the working bytes of each call on stderr).  Every call is complete at
its return; the terrain chunk is put back (outside the timing) before each timed call, the first timed call is dropped and the best of
the next three is reported.  A report, not a gate; profiles/combine.txt and DESIGN.md 6zc quote it.
  python scripts/combine_timing.py [--only DEPTH]     (--only: one MAX call on the cubes of that depth and nothing else, for a kernel trace)"""
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

def cubes(W, depth):
    ma, mb, _ = K.cube_meshes(depth)
    solid(W, ma, depth, K.MATERIAL_A)
    solid(model, mb, depth, K.MATERIAL_B)

if len(sys.argv) > 2 and sys.argv[1] == "--only":
    depth = int(sys.argv[2])
    W = svo.World.create([empty], 1, 1, 1, 128).upload(0)
    cubes(W, depth)
    print(f"depth {depth}: {W.chunk_combine(0, model, 0, svo.COMBINE_MAX)} cells changed", flush=True)
    W.destroy(); model.destroy()
    sys.exit(0)

OPS = (("MAX", svo.COMBINE_MAX, lambda a, b: torch.maximum(a, b, out=a)), ("SUBTRACT", svo.COMBINE_SUBTRACT, lambda a, b: a.masked_fill_(b != 0, 0)))

print("== dense route against svo_world_chunk_combine, ms wall, best of 3 after the first ==", flush=True)
for depth in (8, 9, 10):
    n = 1 << depth
    W = svo.World.generate(1, 1, 1, 128, depth).upload(0)
    terrain = W.chunk(0)
    v, ix = M.sphere_case(depth)
    solid(model, [dict(vertices=v, indices=ix, material=5)], depth, 9)
    ga, gb = (torch.empty(n ** 3, dtype=torch.int16, device="cuda") for _ in range(2))      # (the materials here are below 2^15)
    for name, op, kernel in OPS:
        def dense():
            W.chunk_to_grid(0, depth, ga.data_ptr())
            model.chunk_to_grid(0, depth, gb.data_ptr())
            svo.lib.svo_stream_synchronize(None)            # (torch runs on a stream of its own)
            kernel(ga, gb)
            torch.cuda.synchronize()
            W.chunk_from_grid(0, ga.data_ptr(), depth)
        counts = {}
        def sparse():
            counts["changed"] = W.chunk_combine(0, model, 0, op)
        td = best_of_3_after_the_first(lambda: put(W, terrain), dense)
        a = W.chunk(0)
        ts = best_of_3_after_the_first(lambda: put(W, terrain), sparse)
        b = W.chunk(0)
        same = np.array_equal(a["tree"], b["tree"]) and np.array_equal(a["twig"], b["twig"])
        print(f"depth {depth:2d} terrain {terrain['tree'].size} words, {terrain['twig'].size // 64} bricks {name:8s} filled uv-sphere  dense route {td:9.2f} ms  "
              f"combine {ts:9.2f} ms  pools equal: {same}  ({counts['changed']} cells changed; {b['tree'].size} words, {b['twig'].size // 64} bricks)", flush=True)
        sys.stderr.flush()
    del ga, gb
    torch.cuda.empty_cache()
    W.destroy()

print("== the two solid cubes beyond the dense grid (SVO_BUILD_TIMING prints entries, output, working bytes on stderr) ==", flush=True)
W = svo.World.create([empty], 1, 1, 1, 128).upload(0)
for depth in (12, 16):
    cubes(W, depth)
    cube = W.chunk(0)
    for name, op, _ in OPS:
        counts = {}
        def sparse():
            counts["changed"] = W.chunk_combine(0, model, 0, op)
        ts = best_of_3_after_the_first(lambda: put(W, cube), sparse)
        info = W.info
        print(f"depth {depth:2d} cubes of 258 cells {name:8s} combine {ts:9.2f} ms  {counts['changed']} cells changed (closed form {K.CUBE_CHANGED[op]})  "
              f"{cube['tree'].size} words, {cube['twig'].size // 64} bricks -> {info.total_trees} words, {info.total_twigs} bricks", flush=True)
        sys.stderr.flush()
W.destroy(); model.destroy()
