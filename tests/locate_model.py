"""Host model of svo_world_locate (include/svo.h): steps 1-7 of the call, one point at a time, on top of the Python twin of the
reference's CPU path (oracle/svo_oracle_py.py) - its World.index_float / World.index, traverse, is_inside_cube, twig_word and
trunc_int are imported, not restated.  Test infrastructure: the only yardstick the device kernels are held against."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import svo_oracle_py as P                                   # noqa: E402

f32 = np.float32
INSIDE, SOLID = 1, 2                                        # SVO_LOCATE_INSIDE / SVO_LOCATE_SOLID
CELL_NONE = P.CELL_NONE
VOXEL_DTYPE = np.dtype([("bmin", "<f4", (3,)), ("size", "<f4"), ("material", "<u2"), ("flags", "<u2"),
                        ("chunk", "<u4"), ("node", "<u4"), ("cell", "<u4")])
CLASSES = ("outside", "empty", "leaf", "solid_cell", "empty_cell")


def world_of(chunks, w, h, d, chunksize, chunkcoordmin=(0, 0, 0)):
    """The twin's World over chunk dicts (position, size, depth, tree, twig) in World::index() order."""
    return P.World([P.Chunk(c["position"], c["size"], c["depth"], c["tree"], c["twig"]) for c in chunks], w, h, d, chunksize, chunkcoordmin)


def world_box(world):                                       # chunkmin / chunkmax of chunkmarch, src/Traverse.cpp:129-133
    ccm, cs = world.chunkcoordmin, f32(world.chunksize)
    ics = int(cs)
    chunkmin = P.vec3(ccm[0] * ics, ccm[1] * ics, ccm[2] * ics)
    chunkmax = P.vmuls(P.vec3(ccm[0] + world.width, ccm[1] + world.height, ccm[2] + world.depth), cs)
    return chunkmin, chunkmax


def locate_one(world, p, semantics=0, see_through=0, box=None):
    """-> None (the all-zero record) or (bmin, size, material, flags, chunk, node, cell)."""
    p = P.vec3(*p)
    chunkmin, chunkmax = box or world_box(world)
    if not P.is_inside_cube(p, chunkmin, chunkmax):         # 1. the world box (closed; NaN and inf fail)
        return None
    q = world.index_float(p)                                # 2. the chunk, and the check of src/Traverse.cpp:154
    i = world.index(q[0], q[1], q[2])
    root = world.chunk[i]
    cmin = root.position
    if not P.is_inside_cube(p, cmin, P.vadds(cmin, f32(world.chunksize))):
        return None
    bmin, size, node = P.traverse(p, root)                  # 3. the descent
    word = root.tree[node]
    kind = P.node_type(word)
    material, cell, solid = 0, CELL_NONE, False
    if kind == P.LEAF:                                      # 5.
        material, solid = P.node_offset(word) & 0xFFFF, True
    elif kind == P.TWIG:                                    # 6.
        leafsize = size / f32(1 << P.TWIG_LEVELS)
        d = P.vsub(p, bmin)
        v = P.vmuls(d, f32(1.0) / leafsize) if semantics == 1 else P.vdivs(d, leafsize)
        off = (P.trunc_int(v[0]), P.trunc_int(v[1]), P.trunc_int(v[2]))
        if P.is_inside_cube(P.vec3(*off), P._IMIN, P._IMAX):
            cell = P.twig_word(*off)
            bmin = P.vadd(bmin, P.vmuls(P.vec3(*off), leafsize))
            size = leafsize
            material = root.twig[P.node_offset(word)][cell]
            solid = material != 0
    else:
        assert kind == P.EMPTY                              # 4.
    if see_through and solid and material == see_through:   # 7.
        material, solid = 0, False
    return bmin, size, material, INSIDE | (SOLID if solid else 0), i, node, cell


def locate(world, points, semantics=0, see_through=0):
    """VOXEL_DTYPE[n]: the records svo_world_locate writes for `points` ([n][3] float32)."""
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(pts.shape[0], VOXEL_DTYPE)
    box = world_box(world)
    for k in range(pts.shape[0]):
        r = locate_one(world, pts[k], semantics, see_through, box)
        if r is not None:
            out[k] = (np.array(r[0], np.float32), r[1], r[2], r[3], r[4], r[5], r[6])
    return out


def classes(records):
    """Points per class of CLASSES (by the records alone: a LEAF has SVO_CELL_NONE and SOLID, ...)."""
    r = np.asarray(records)
    inside = (r["flags"] & INSIDE) != 0
    solid = (r["flags"] & SOLID) != 0
    cellular = r["cell"] != CELL_NONE
    return {"outside": int((~inside).sum()), "empty": int((inside & ~solid & ~cellular).sum()), "leaf": int((inside & solid & ~cellular).sum()),
            "solid_cell": int((inside & solid & cellular).sum()), "empty_cell": int((inside & ~solid & cellular).sum())}


# ---- the point sets of the GPU tests (tests/test_locate.py) and of the input-condition test (tests/test_locate_cpu.py) -----------
def box_of(w, h, d, chunksize, ccm):
    lo = np.array(ccm, np.float64) * chunksize
    return lo, lo + np.array([w, h, d], np.float64) * chunksize


def uniform_points(rng, n, lo, hi, margin=0.1):
    """Uniform in the box grown by `margin` of its extent on every side."""
    ext = hi - lo
    return (lo - margin * ext + rng.random((n, 3)) * (1.0 + 2.0 * margin) * ext).astype(np.float32)


def lattice_points(rng, n, lo, hi, pitch=1.0):
    """Points whose coordinates are multiples of `pitch`, the box's faces, edges and corners among them (and one plane beyond)."""
    cells = np.round((hi - lo) / pitch).astype(np.int64)
    q = np.stack([rng.integers(-1, cells[a] + 2, n) for a in range(3)], axis=1)
    k = n // 4                                              # a quarter on faces / edges / corners of the chunk lattice
    ax = rng.integers(0, 3, k)
    big = max(1, int(round(128.0 / pitch)))
    q[np.arange(k), ax] = np.round(q[np.arange(k), ax] / big) * big
    k2 = n // 16                                            # ... and on the world's own faces
    for a in range(3):
        q[k:k + k2, a] = np.where(rng.random(k2) < 0.5, q[k:k + k2, a], rng.choice([0, cells[a]], k2))
    return (lo + q * pitch).astype(np.float32)


SPECIAL = np.array([[np.nan, 1.0, 1.0], [1.0, np.nan, 1.0], [1.0, 1.0, np.nan], [np.inf, 1.0, 1.0], [1.0, -np.inf, 1.0], [1.0, 1.0, np.inf],
                    [np.nan, np.nan, np.nan], [-np.inf, np.inf, 1.0], [-0.0, -0.0, -0.0], [1e-45, 1e-45, 1e-45], [3.4e38, 1.0, 1.0]], np.float32)


# the worlds of the GPU tests: name -> (w, h, d, chunkcoordmin, depth of every chunk in World::index() order)
WORLDS = {
    "grid_2x1x2_d6": (2, 1, 2, (0, 0, 0), [6] * 4),                    # tests/golden/grid_2x1x2_depth6.npz's world
    "grid_neg_2x2x2_d5": (2, 2, 2, (-1, -1, -1), [5] * 8),             # tests/golden/grid_neg_2x2x2_depth5.npz's (odd branch levels: a padded top wide node)
    "c1_depth8": (1, 1, 1, (0, 0, 0), [8]),                            # tests/golden/c1_depth8_single.npz's
    "mixed_7_2_4_5": (2, 1, 2, (0, 0, 0), [7, 2, 4, 5]),               # 5, 0, 2 and 3 branch levels: pad 1, 2, 0, 1
}


def make_chunks(svo, name):
    """The chunk dicts of WORLDS[name], generated on the host by the library (bit-identical to the twin's: tests/test_golden.py)."""
    w, h, d, ccm, depths = WORLDS[name]
    gen = {}
    for depth in sorted(set(depths)):
        W = svo.World.generate(w, h, d, 128, depth, chunkcoordmin=ccm)
        gen[depth] = [W.chunk(i) for i in range(w * h * d)]
        W.destroy()
    return [gen[depth][i] for i, depth in enumerate(depths)]


L_, B_, T_ = 1 << 30, 2 << 30, 3 << 30


def handmade_chunks():
    """A 2x1x1 world of 128-unit chunks at chunkcoordmin (-1, 0, 0): chunk 0 is one TWIG (depth 2, 32-unit cells, every third cell
    solid, material 1 + cell % 5), chunk 1 a BRANCH (depth 3) over EMPTY, LEAF 3, TWIG, TWIG, LEAF 6, EMPTY, BRANCH-free rest."""
    b0 = np.array([(1 + c % 5) if c % 3 == 0 else 0 for c in range(64)], np.uint16)
    b1 = np.array([6 if c % 2 else 0 for c in range(64)], np.uint16)
    b2 = np.array([2 if (c >> 4) < 2 else 0 for c in range(64)], np.uint16)
    c0 = dict(position=(-128.0, 0.0, 0.0), size=128.0, depth=2, tree=np.array([T_ | 0], np.uint32), twig=b0)
    tree1 = np.array([B_ | 1, 0, L_ | 3, T_ | 0, T_ | 1, L_ | 6, 0, L_ | 0x10002, 0], np.uint32)
    c1 = dict(position=(0.0, 0.0, 0.0), size=128.0, depth=3, tree=tree1, twig=np.concatenate([b1, b2]))
    return [c1, c0]                                         # World::index(): chunk coordinate x = -1 has linear index 1


HANDMADE = (2, 1, 1, (-1, 0, 0))


def point_sets(name, lo, hi, n=1600):
    """name -> the point lists every world is queried with (surface points are added by the GPU test, which traces a frame)."""
    rng = np.random.default_rng(sum(name.encode()) + 2707)
    return {"uniform": uniform_points(rng, 2 * n, lo, hi), "lattice": lattice_points(rng, n, lo, hi, 1.0),
            "half_lattice": lattice_points(rng, n, lo, hi, 0.5), "special": SPECIAL}
