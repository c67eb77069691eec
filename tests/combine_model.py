"""What the chunk CSG's tests share (svo_chunk_combine / svo_world_chunk_combine, include/svo.h): the dense model -
grid_model.pools_to_grid of both chunks, the numpy form of f_op, grid_model.chunk_of, and the count of cells that differ from A's -,
the named pairs (A, B) of equal depth that a dense grid reaches, and for depth 12 and 16 two solid cubes whose counts are known in
closed form and a windowed model of one of them against the filled deep sphere of sparse_mesh_model.  Test infrastructure."""
import numpy as np

import grid_model as G
import mesh_model as M
import sparse_fill_model as F
import sparse_mesh_model as S

MAX, UNDER, OVER, SUBTRACT, INTERSECT = range(5)
OPS = {"max": MAX, "under": UNDER, "over": OVER, "subtract": SUBTRACT, "intersect": INTERSECT}


def f(op, a, b):
    """f_op of include/svo.h on arrays (or ints) of cell values."""
    a, b = np.asarray(a), np.asarray(b)
    zero = np.zeros_like(a)
    return {MAX: lambda: np.maximum(a, b), UNDER: lambda: np.where(a != 0, a, b), OVER: lambda: np.where(b != 0, b, a),
            SUBTRACT: lambda: np.where(b != 0, zero, a), INTERSECT: lambda: np.where(b != 0, a, zero)}[op]()


def model_combine(a, b, op):
    """(the combined chunk by the definition, how many cells differ from A's): dense grids at the chunks' own depth (<= 7 here)."""
    depth = int(a["depth"])
    assert int(b["depth"]) == depth
    ga, gb = G.pools_to_grid(a, depth), G.pools_to_grid(b, depth)
    g = f(op, ga, gb).astype(np.uint16)
    return G.chunk_of(g, a["position"], a["size"]), int((g != ga).sum())


# ---- the pairs a dense grid reaches --------------------------------------------------------------------------------------------------
def _pairing_grids():
    """Depth 4, so that the root's children (8^3) sit above level depth-2 and their children (4^3) at it.  A: octant 0 EMPTY, octant 1 a
    LEAF, octant 2 a BRANCH over one EMPTY, one LEAF and six TWIG blocks, the rest EMPTY.  B: octants 0, 1, 2 BRANCHes whose blocks are
    EMPTY, LEAF and TWIG in turn - every pairing of the two levels occurs, and in the swapped pair in the other order."""
    rng = np.random.default_rng(44)
    a, b = np.zeros((16, 16, 16), np.uint16), np.zeros((16, 16, 16), np.uint16)
    a[0:8, 0:8, 8:16] = 7                                   # octant 1 (x high)
    a[0:8, 8:16, 0:8] = rng.choice(np.array([0, 3, 9], np.uint16), (8, 8, 8))   # octant 2 (y high)
    a[0:4, 8:12, 0:4] = 0
    a[0:4, 8:12, 4:8] = 9
    for z0, y0, x0 in ((0, 0, 0), (0, 0, 8), (0, 8, 0)):
        b[z0:z0 + 8, y0:y0 + 8, x0:x0 + 8] = rng.choice(np.array([0, 5, 9, 300], np.uint16), (8, 8, 8))
        b[z0:z0 + 4, y0:y0 + 4, x0:x0 + 4] = 0                      # one EMPTY block
        b[z0 + 4:z0 + 8, y0:y0 + 4, x0:x0 + 4] = 5                  # one LEAF block
    b[0:4, 8:12, 4:8] = rng.choice(np.array([0, 12], np.uint16), (4, 4, 4))     # a TWIG of B on the LEAF block of A's octant 2
    return a, b


def _ball(depth, centre, radius, material):
    n = 1 << depth
    i = np.arange(n) + 0.5
    z, y, x = np.meshgrid(i, i, i, indexing="ij")
    r2 = (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2
    return np.where(r2 <= radius * radius, material, 0).astype(np.uint16)


def _checkerboards():
    """Depth 4: A is material 5 everywhere but in the block [0, 4)^3, where it holds the even cells of a checkerboard; B holds the odd
    cells of that block and nothing else.  Together the block is a LEAF at level depth-2, and the chain of equal LEAFs reaches the root."""
    i = np.arange(4)
    even = (i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2 == 0
    a, b = np.full((16, 16, 16), 5, np.uint16), np.zeros((16, 16, 16), np.uint16)
    a[0:4, 0:4, 0:4] = np.where(even, 5, 0)
    b[0:4, 0:4, 0:4] = np.where(even, 0, 5)
    return a, b


def one_word(depth, word):
    return F.freeze(dict(position=(0.0, 0.0, 0.0), size=128.0, depth=depth, tree=np.array([word], np.uint32), twig=np.zeros(0, np.uint16)))


_pairs = {}


def pairs():
    """name -> (A, B): chunks of equal depth, computed once, left unchanged.  Sections 1 to 5 of the CPU test and the GPU test's pools
    against the host form run over all of them."""
    if _pairs:
        return _pairs
    chunk = lambda g: F.freeze(G.chunk_of(g))
    grids, fills = G.grids(), M.fill_cases()
    filled = {}
    for name in ("shell", "nested", "depth2"):
        g = fills[name].copy()
        M.fill_enclosed(g, 11)
        filled[name] = g
    P = _pairs
    # 1. every node-type pairing
    pa, pb = _pairing_grids()
    P["pairings"], P["pairings_swapped"] = (chunk(pa), chunk(pb)), (chunk(pb), chunk(pa))
    for name in ("g2_empty", "g2_leaf", "g2_mixed"):
        P[f"{name}_depth2"] = (G.model_chunk(name), chunk(fills["depth2"]))
    P["depth2_g2_mixed"] = (chunk(fills["depth2"]), G.model_chunk("g2_mixed"))
    P["g2_mixed_depth2_filled"] = (G.model_chunk("g2_mixed"), chunk(filled["depth2"]))
    P["g3_full"], P["full_g3"] = (G.model_chunk("g3"), chunk(fills["full"])), (chunk(fills["full"]), G.model_chunk("g3"))
    P["g3_empty"], P["empty_g3"] = (G.model_chunk("g3"), chunk(fills["empty"])), (chunk(fills["empty"]), G.model_chunk("g3"))
    P["g5_shell"], P["shell_g5"] = (G.model_chunk("g5"), chunk(fills["shell"])), (chunk(fills["shell"]), G.model_chunk("g5"))
    P["g5_shell_filled"], P["nested_filled_g5"] = (G.model_chunk("g5"), chunk(filled["shell"])), (chunk(filled["nested"]), G.model_chunk("g5"))
    P["g5_nested"], P["g5_holed"] = (G.model_chunk("g5"), chunk(fills["nested"])), (G.model_chunk("g5"), chunk(fills["holed"]))
    # 2. collapses
    half = np.zeros((16, 16, 16), np.uint16)
    half[:, :, 0:8] = 5
    other = np.where(half == 0, 5, 0).astype(np.uint16)
    P["half_spaces"] = (chunk(half), chunk(other))
    P["checkerboards"] = tuple(chunk(g) for g in _checkerboards())
    P["g5_root_leaf"] = (G.model_chunk("g5"), one_word(5, G.node(G.LEAF, 0xFFFF)))
    P["g5_itself"] = (G.model_chunk("g5"), G.model_chunk("g5"))
    P["g5_empty"] = (G.model_chunk("g5"), one_word(5, 0))
    # 3. growth
    P["two_spheres"] = (chunk(_ball(6, (16.0, 16.0, 16.0), 12.3, 3)), chunk(_ball(6, (47.0, 48.0, 46.0), 12.3, 5)))
    # 4. untidy inputs
    untidy = F.untidy_chunk()[0]
    P["untidy_empty"], P["empty_untidy"], P["untidy_itself"] = (untidy, one_word(4, 0)), (one_word(4, 0), untidy), (untidy, untidy)
    P["untidy_leaf0"] = (untidy, one_word(4, G.node(G.LEAF, 0)))           # LEAF | 0 is empty however it is stored
    return P


def depth7_pair():
    """The depth-7 pair of the GPU test: the level lists pass 256 entries and the brick candidates cross a block border."""
    return F.freeze(G.chunk_of(np.where(_ball(7, (64.0, 60.0, 66.0), 40.0, 6) != _ball(7, (64.0, 60.0, 66.0), 36.0, 6), 6, 0).astype(np.uint16))), G.model_chunk("g7")


_models = {}


def pair_model(name, op):
    """(the model's chunk, the count) of a pair under op - computed once, left unchanged."""
    if (name, op) not in _models:
        a, b = pairs()[name]
        want, changed = model_combine(a, b, op)
        _models[(name, op)] = (F.freeze(want), changed)
    return _models[(name, op)]


# ---- depth 12 and 16: two solid cubes -----------------------------------------------------------------------------------------------
CUBE = 258                                                  # the closed rule: a box mesh of 256 cells marks 258 per axis, from corner - 1 on
SHIFT = (128, 64, 32)                                       # B's min corner relative to A's
OVERLAP = 130 * 194 * 226
CUBE_CHANGED = {MAX: CUBE ** 3, OVER: CUBE ** 3, UNDER: CUBE ** 3 - OVERLAP, INTERSECT: CUBE ** 3 - OVERLAP, SUBTRACT: OVERLAP}
MATERIAL_A, MATERIAL_B = 3, 5
DEEP = {12: (2880, (0.0, 0.0, 0.0), 1.0), 16: (47104, (10.0, -20.0, 30.0), 0.25)}      # depth -> (A's corner c, a multiple of 64; the meshes' frame)


def cube_meshes(depth):
    """(A's mesh list, B's mesh list, c): 12-triangle boxes of edge 256 cells with min corners (c, c, c) and c + SHIFT."""
    c, origin, cell = DEEP[depth]
    out = []
    for shift, material in (((0, 0, 0), MATERIAL_A), (SHIFT, MATERIAL_B)):
        lo = np.asarray(origin, np.float64) + (c + np.asarray(shift, np.float64)) * cell
        v, ix = M.box_mesh(lo, lo + 256 * cell)
        out.append([S.mesh(v, ix, origin=origin, cell=cell, material=material)])
    return out[0], out[1], c


def cube_cells(depth, x, y, z):
    """(a, b): what the two solid cubes hold at voxel (x, y, z)."""
    c = DEEP[depth][0]
    inside = lambda lo: all(l - 1 <= p < l + 257 for p, l in zip((x, y, z), lo))
    return (MATERIAL_A if inside((c, c, c)) else 0), (MATERIAL_B if inside(tuple(c + s for s in SHIFT)) else 0)


def window_of(chunk, corner, shape):
    """The [z, y, x] array of the chunk's finest voxels from `corner` (x, y, z) on, node by node: what sparse_mesh_model's
    check_against_windows reads cell by cell."""
    tree, twig = chunk["tree"], chunk["twig"]
    out = np.zeros(shape, np.uint16)
    lo, hi = np.asarray(corner), np.asarray(corner) + np.asarray(shape)[::-1]
    stack = [(0, np.zeros(3, np.int64), 1 << int(chunk["depth"]))]
    while stack:
        i, p, e = stack.pop()
        if (p + e <= lo).any() or (p >= hi).any():
            continue
        w = int(tree[i])
        kind, off = w >> 30, w & 0x3FFFFFFF
        if kind == G.BRANCH:
            stack.extend((off + c, p + np.array([c & 1, (c >> 1) & 1, c >> 2]) * (e // 2), e // 2) for c in range(8))
            continue
        if kind == G.EMPTY:
            continue
        a, b = np.maximum(p, lo), np.minimum(p + e, hi)
        view = out[a[2] - lo[2]:b[2] - lo[2], a[1] - lo[1]:b[1] - lo[1], a[0] - lo[0]:b[0] - lo[0]]
        if kind == G.LEAF:
            view[...] = off & 0xFFFF
        else:                                               # a TWIG at level depth-2: e == 4
            cells = np.asarray(twig[off * 64:off * 64 + 64]).reshape(4, 4, 4)
            view[...] = cells[a[2] - p[2]:b[2] - p[2], a[1] - p[1]:b[1] - p[1], a[0] - p[0]:b[0] - p[0]]
    return out


def sphere12_windows(op):
    """The windowed model of cube A (depth 12) combined with the filled deep sphere of sparse_mesh_model: [(corner, array)] of the
    expected cells in the sphere's windows, and how many of them differ from A's.  Outside the windows B is empty."""
    out, changed = [], 0
    for corner, b in F.filled_windows("sphere12", 9)[0]:
        zs, ys, xs = (np.arange(corner[k], corner[k] + b.shape[2 - k]) for k in (2, 1, 0))
        c = DEEP[12][0]
        inside = lambda v: (v >= c - 1) & (v < c + 257)
        a = np.where(inside(zs)[:, None, None] & inside(ys)[None, :, None] & inside(xs)[None, None, :], MATERIAL_A, 0).astype(np.uint16)
        r = f(op, a, b).astype(np.uint16)
        changed += int((r != a).sum())
        r.setflags(write=False)
        out.append((corner, r, a))
    return out, changed
