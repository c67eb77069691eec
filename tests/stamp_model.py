"""What the stamp's tests share (svo_chunk_stamp / svo_world_chunk_stamp, include/svo.h): the dense model - grid_model.pools_to_grid of
both chunks, B turned with numpy transpose and flip and placed on slices, combine_model.f, grid_model.chunk_of, and the count of cells
that differ from A's -, the named cases (A, B, offset, orient) a dense grid reaches, and for depth 12 and 16 the boxes of the deep
cases, whose counts follow from integer arithmetic.  Test infrastructure."""
import numpy as np

import combine_model as K
import grid_model as G
import sparse_fill_model as F

PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))        # pi(0), pi(1), pi(2); axis 0 is x
ODD_PERMS = (1, 2, 5)


def is_rotation(orient):
    return ((orient >> 3 in ODD_PERMS) + bin(orient & 7).count("1")) % 2 == 0


def oriented(gb, orient):
    """B' as a [z, y, x] grid: cell d of B' is cell q of B, q[pi(i)] = N_B - 1 - d_i if flips bit i else d_i."""
    xyz = np.asarray(gb).transpose(2, 1, 0)                 # [x, y, z]: array axis i is cell axis i
    out = np.transpose(xyz, PERMS[orient >> 3])             # out[d] = xyz[q] with q[pi(i)] = d_i
    out = np.flip(out, [i for i in range(3) if (orient >> i) & 1])
    return np.ascontiguousarray(out.transpose(2, 1, 0))


def quarter_turns():
    """The proper orientations that are the identity after four applications and not after two: the six quarter turns."""
    probe = np.arange(8).reshape(2, 2, 2)
    out = []
    for o in range(48):
        twice = oriented(oriented(probe, o), o)
        if is_rotation(o) and not np.array_equal(twice, probe) and np.array_equal(oriented(oriented(twice, o), o), probe):
            out.append(o)
    return out


def placed(gb_oriented, n_a, offset):
    """The [z, y, x] grid of A's size that holds B' with its cube starting at A's cell `offset` (x, y, z) and 0 elsewhere."""
    n_b = gb_oriented.shape[0]
    out = np.zeros((n_a,) * 3, np.uint16)
    dst, src = [], []
    for o in (offset[2], offset[1], offset[0]):             # z, y, x
        lo, hi = max(o, 0), min(o + n_b, n_a)
        if lo >= hi:
            return out
        dst.append(slice(lo, hi))
        src.append(slice(lo - o, hi - o))
    out[tuple(dst)] = gb_oriented[tuple(src)]
    return out


_grids = {}


def _grid(chunk):
    key = id(chunk["tree"])
    if key not in _grids:
        _grids[key] = (chunk, G.pools_to_grid(chunk, int(chunk["depth"])))    # (the chunk is kept: its id stays its own)
    return _grids[key][1]


def model_stamp(a, b, offset, orient, op):
    """(the stamped chunk by the definition, how many cells differ from A's): dense grids at the chunks' own depths (<= 7 here)."""
    ga = _grid(a)
    g = K.f(op, ga, placed(oriented(_grid(b), orient), ga.shape[0], offset)).astype(np.uint16)
    return G.chunk_of(g, a["position"], a["size"]), int((g != ga).sum())


# ---- the cases a dense grid reaches ---------------------------------------------------------------------------------------------------
_cases = {}
_chunks = {}


def chunks():
    """name -> chunk: the As (depth 4) and the Bs (depth 2, 3, 4) of the case list - computed once, left unchanged."""
    if not _chunks:
        chunk = lambda g: F.freeze(G.chunk_of(g))
        pa, pb = K.pairs()["pairings"]
        octant = np.full((16, 16, 16), 5, np.uint16)        # material 5 but for one octant / one 8^3 hole at an odd corner: [z, y, x]
        octant[0:8, 0:8, 8:16] = 0
        hole = np.full((16, 16, 16), 5, np.uint16)
        hole[6:14, 5:13, 3:11] = 0
        _chunks.update(pairings=pa, height4=chunk(G.heightfield(4)), empty4=K.one_word(4, 0), octant4=chunk(octant), hole4=chunk(hole),
                       b2=G.model_chunk("g2_mixed"), b3=G.model_chunk("g3"), b4=pb,
                       leaf3=K.one_word(3, G.node(G.LEAF, 5)), leaf2=K.one_word(2, G.node(G.LEAF, 5)))
    return _chunks


def cases():
    """name -> (A's name, B's name, offset (x, y, z), orient): B of depth 2, 3 and 4 into a depth-4 A."""
    if _cases:
        return _cases
    P = _cases
    k = 0

    def add(a, b, offset, orient=None, name=None):
        nonlocal k
        k += 1
        o = (k * 7) % 48 if orient is None else orient
        name = name or f"{a}_{b}_{offset[0]}_{offset[1]}_{offset[2]}_o{o}"
        assert name not in P
        P[name] = (a, b, tuple(offset), o)

    for b, n_b in (("b2", 4), ("b3", 8), ("b4", 16)):
        add("pairings", b, (0, 0, 0), 0)                                        # all zero, as it lies
        add("pairings", b, (0, 0, 0))
        add("pairings", b, (4, 8, 12 if n_b == 4 else 0))                       # multiples of 4 (depth 2: exactly an aligned brick)
        add("pairings", b, (16 - n_b, 0, 16 - n_b))                             # B's cube exactly fills an aligned sub-cube
        add("pairings", b, (1, 3, 5))                                           # odd
        add("pairings", b, (7, 2, 9))
        add("pairings", b, (-3, 2, 1)); add("pairings", b, (2, -5, 3)); add("pairings", b, (1, 2, -2))     # partly outside, low side
        add("pairings", b, (13, 3, 2)); add("pairings", b, (3, 14, 2)); add("pairings", b, (6, 1, 15))     # ... high side
        add("pairings", b, (-1, -1, 17 - n_b))
        add("pairings", b, (16, 0, 0)); add("pairings", b, (0, -n_b, 3)); add("pairings", b, (65536, -65536, 5))   # wholly outside
        for offset in ((0, 0, 0), (4, -4, 8), (5, 1, -3), (9, 11, 2)):
            add("height4", b, offset)
    for orient in range(48):                                                    # all 48 on one asymmetric B, partly outside on two axes
        add("pairings", "b3", (5, -3, 9), orient)
    add("empty4", "leaf3", (1, 1, 1), 0, "leaf_root_at_odd_offset")             # more bricks than twigs_A + twigs_B
    add("pairings", "leaf2", (3, 9, 6), 13)
    add("octant4", "leaf3", (8, 0, 0), 0, "half_space_completed")               # folds to one word
    add("hole4", "leaf3", (3, 5, 6), 38, "hole_at_odd_offset_completed")        # ... through the bricks
    add("octant4", "leaf3", (8, 1, 0), 0, "half_space_missed_by_one")
    add("empty4", "b3", (3, 5, 6), 21, "into_empty")
    return P


def case(name):
    a, b, offset, orient = cases()[name]
    return chunks()[a], chunks()[b], offset, orient


def shell6():
    """The depth-6 sphere shell of the GPU test: more than 1024 bricks."""
    i = np.arange(64) + 0.5
    z, y, x = np.meshgrid(i, i, i, indexing="ij")
    r2 = (x - 31.0) ** 2 + (y - 33.0) ** 2 + (z - 30.0) ** 2
    return F.freeze(G.chunk_of(np.where((r2 <= 29.0 ** 2) & (r2 > 25.5 ** 2), np.where(x > y, 6, 9), 0).astype(np.uint16)))


_models = {}


def case_model(name, op):
    """(the model's chunk, the count) of a case under op - computed once, left unchanged."""
    if (name, op) not in _models:
        a, b, offset, orient = case(name)
        want, changed = model_stamp(a, b, offset, orient, op)
        _models[(name, op)] = (F.freeze(want), changed)
    return _models[(name, op)]


# ---- depth 12 and 16: a LEAF-root B of depth 8 into combine_model's cube A ----------------------------------------------------------
DEEP_B_DEPTH, DEEP_MATERIAL = 8, 5
DEEP_SHIFT = (129, 65, 33)                                  # B's cube starts at c + DEEP_SHIFT: odd on every axis (c is a multiple of 64)


def deep_boxes(depth):
    """(A's box, B's box) as ((x0, y0, z0), (x1, y1, z1)), half open, in cells: the solid cube of combine_model (258 cells from c - 1
    on) and the cube of B (256 cells from c + DEEP_SHIFT on)."""
    c = K.DEEP[depth][0]
    lo_b = tuple(c + s for s in DEEP_SHIFT)
    return ((c - 1,) * 3, (c + 257,) * 3), (lo_b, tuple(v + (1 << DEEP_B_DEPTH) for v in lo_b))


def box_cells(box):
    return int(np.prod([max(hi - lo, 0) for lo, hi in zip(*box)], dtype=object))


def box_overlap(p, q):
    return tuple(max(a, b) for a, b in zip(p[0], q[0])), tuple(min(a, b) for a, b in zip(p[1], q[1]))


def inside(box, x, y, z):
    return all(lo <= v < hi for v, lo, hi in zip((x, y, z), *box))


def deep_b():
    return K.one_word(DEEP_B_DEPTH, G.node(G.LEAF, DEEP_MATERIAL))
