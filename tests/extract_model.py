"""What the extract's tests share (svo_chunk_extract / svo_world_chunk_extract, include/svo.h): the dense model - grid_model.pools_to_grid
of A, the zero-padded window [offset, offset + N_C)^3, the header's rule as an index map, grid_model.chunk_of, and the count of cells
that are not 0 -, the named cases (A, offset, orient, D_C) a dense grid reaches, and for depth 12 and 16 the windows of the deep cases,
whose counts follow from integer arithmetic.  The model asserts once per result that stamp_model.oriented(G_C, orient) is the window:
the extract is the stamp's inverse.  Test infrastructure."""
import numpy as np

import combine_model as K
import grid_model as G
import sparse_fill_model as F
import stamp_model as T


def window(ga, n_c, offset):
    """The [z, y, x] grid of n_c^3 cells that starts at A's cell `offset` (x, y, z); what lies outside A reads 0."""
    n_a = ga.shape[0]
    out = np.zeros((n_c,) * 3, np.uint16)
    dst, src = [], []
    for o in (offset[2], offset[1], offset[0]):             # z, y, x
        lo, hi = max(o, 0), min(o + n_c, n_a)
        if lo >= hi:
            return out
        src.append(slice(lo, hi))
        dst.append(slice(lo - o, hi - o))
    out[tuple(dst)] = ga[tuple(src)]
    return out


def extracted_grid(w, orient):
    """G_C of the window w, the header's rule as an index map: for every d, G_C[q] = w[d] with q[pi(i)] = N_C - 1 - d_i if flips bit i
    else d_i."""
    n = w.shape[0]
    d = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")        # d[i]: cell axis i (0 is x), each [n, n, n]
    q = [None, None, None]
    for i in range(3):
        q[T.PERMS[orient >> 3][i]] = n - 1 - d[i] if (orient >> i) & 1 else d[i]
    gc = np.zeros_like(w)
    gc[q[2], q[1], q[0]] = w[d[2], d[1], d[0]]              # grids are [z, y, x]
    assert np.array_equal(T.oriented(gc, orient), w)        # C, oriented the way the stamp orients B, is the window
    return gc


def model_extract(a, offset, orient, depth, position=(0.0, 0.0, 0.0), size=128.0):
    """(the extracted chunk by the definition, how many of its cells are not 0): dense grids (A's depth <= 7 here)."""
    gc = extracted_grid(window(T._grid(a), 1 << depth, offset), orient)
    return G.chunk_of(gc, position, size), int(np.count_nonzero(gc))


# ---- the cases a dense grid reaches ---------------------------------------------------------------------------------------------------
_cases = {}
_chunks = {}


def chunks():
    """name -> chunk: the As of the case list - computed once, left unchanged."""
    if not _chunks:
        S = T.chunks()
        _chunks.update(pairings=S["pairings"], height4=S["height4"], octant4=S["octant4"], hole4=S["hole4"], g6=G.model_chunk("g6"), g7=G.model_chunk("g7"),
                       leaf4=K.one_word(4, G.node(G.LEAF, 5)))
    return _chunks


def cases():
    """name -> (A's name, offset (x, y, z), orient, D_C)."""
    if _cases:
        return _cases
    P = _cases
    k = 0

    def add(a, offset, depth, orient=None, name=None):
        nonlocal k
        k += 1
        o = (k * 7) % 48 if orient is None else orient
        name = name or f"{a}_d{depth}_{offset[0]}_{offset[1]}_{offset[2]}_o{o}"
        assert name not in P
        P[name] = (a, tuple(offset), o, depth)

    for depth in (2, 3, 4):                                                     # depth 2: the root entry is itself the brick candidate
        n_c = 1 << depth
        add("pairings", (0, 0, 0), depth, 0)                                    # all zero, as it lies
        add("pairings", (0, 0, 0), depth)
        add("pairings", (4, 8, 12 if n_c == 4 else 0), depth)                   # multiples of 4
        add("pairings", (1, 3, 5), depth)                                       # odd
        add("pairings", (7, 2, 9), depth)
        add("pairings", (-3, 2, 1), depth); add("pairings", (2, -5, 3), depth); add("pairings", (1, 2, -2), depth)     # partly outside, low side
        add("pairings", (13, 3, 2), depth); add("pairings", (3, 14, 2), depth); add("pairings", (6, 1, 15), depth)     # ... beyond the far side
        add("pairings", (-1, -1, 17 - n_c), depth)
        add("pairings", (16, 0, 0), depth); add("pairings", (0, -n_c, 3), depth); add("pairings", (65536, -65536, 5), depth)   # wholly outside
        add("pairings", (5, 65536, -65536), depth)
        for offset in ((0, 0, 0), (4, -4, 8), (5, 1, -3), (9, 11, 2)):
            add("height4", offset, depth)
    for a in ("pairings", "height4"):                                           # an aligned octant: that child's subtree rebuilt
        add(a, (8, 0, 8), 3, 0, f"{a}_octant_5")
        add(a, (0, 8, 0), 3, 0, f"{a}_octant_2")
    for orient in range(48):                                                    # all 48 at one offset, partly outside on two axes
        add("height4", (5, -3, -2), 3, orient)
    for a in ("g6", "g7"):                                                      # a root descent of 2 .. 5 levels, past EMPTY and LEAF
        n_a = 1 << G.model_chunk(a)["depth"]
        for depth in (2, 3, 4):
            add(a, (n_a // 2 - 3, n_a * 13 // 32, n_a // 2 + 6), depth)
            add(a, (n_a // 4, n_a // 2, 8), depth)
            add(a, (n_a - 5, 2, n_a // 2), depth)
        add(a, (0, 0, 0), 2); add(a, (n_a - 4, n_a - 4, n_a - 4), 2)
    add("leaf4", (1, 1, 1), 4, 0, "leaf_root_at_odd_offset")                    # bricks from a one-word pool
    add("leaf4", (-3, 5, 0), 3, 17, "leaf_root_through_one_face")
    add("octant4", (8, 0, 0), 3, 0, "octant4_the_empty_octant")                 # windows that fold to one word
    add("octant4", (0, 0, 0), 3, 0, "octant4_a_full_octant")
    add("octant4", (0, 0, 8), 3, 9, "octant4_a_full_octant_turned")
    add("hole4", (3, 5, 6), 3, 38, "hole4_the_hole")
    add("hole4", (3, 5, 7), 3, 38, "hole4_the_hole_missed_by_one")
    return P


def case(name):
    a, offset, orient, depth = cases()[name]
    return chunks()[a], offset, orient, depth


_models = {}


def case_model(name):
    """(the model's chunk, the count) of a case - computed once, left unchanged."""
    if name not in _models:
        a, offset, orient, depth = case(name)
        want, occupied = model_extract(a, offset, orient, depth)
        _models[name] = (F.freeze(want), occupied)
    return _models[name]


# ---- depth 12 and 16: windows of combine_model's cube (solid [c - 1, c + 257)^3) --------------------------------------------------------
def deep_windows(depth):
    """name -> (offset, D_C, the window's box, the box of the cube inside it), boxes half open in A's cells."""
    c = K.DEEP[depth][0]
    cube = ((c - 1,) * 3, (c + 257,) * 3)
    out = {}
    for name, lo, d in (("across_three_faces", tuple(c + s for s in T.DEEP_SHIFT), 8), ("the_whole_cube", (c - 383, c - 255, c - 127), 10)):
        box = (lo, tuple(v + (1 << d) for v in lo))
        out[name] = (lo, d, box, T.box_overlap(cube, box))
    return out
