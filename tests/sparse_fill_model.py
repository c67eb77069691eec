"""What the sparse interior fill's tests share (svo_chunk_fill_enclosed / svo_world_chunk_fill_enclosed, include/svo.h): the model -
grid_model.chunk_of(mesh_model.fill_enclosed(grid_model.pools_to_grid(chunk))) - the cases a dense grid reaches, and for depth 12 and 16
a windowed model: the windows of sparse_mesh_model.add_mesh_windows filled with mesh_model.fill_enclosed.  A window whose outermost
cell layer is empty in the shell is surrounded by empty cells that connect to the chunk's faces (everything outside the windows is
empty), so the window's own faces stand for the outside and its fill is the global one.  Test infrastructure."""
import numpy as np

import grid_model as G
import mesh_model as M
import sparse_mesh_model as S


def model_fill(chunk, material):
    """(the filled chunk by the definition, how many cells were filled): a dense grid at the chunk's own depth (<= 7 here)."""
    g = G.pools_to_grid(chunk, int(chunk["depth"])).copy()
    filled = M.fill_enclosed(g, material)
    return G.chunk_of(g, chunk["position"], chunk["size"]), filled


def freeze(chunk):
    chunk["tree"].setflags(write=False)
    chunk["twig"].setflags(write=False)
    return chunk


# ---- the cases a dense grid reaches: name -> (chunk, material) -----------------------------------------------------------------
def _sphere_through_the_faces(depth=5):
    """A sphere shell larger than the grid's inscribed sphere: it leaves through all six faces, nothing is enclosed."""
    n = 1 << depth
    i = np.arange(n) + 0.5
    z, y, x = np.meshgrid(i, i, i, indexing="ij")
    r = np.sqrt((x - n / 2) ** 2 + (y - n / 2) ** 2 + (z - n / 2) ** 2)
    return np.where((r > 0.55 * n) & (r < 0.62 * n), 4, 0).astype(np.uint16)


def hollow_cube(depth, lo, hi, material):
    """[lo, hi) of material with [lo + 1, hi - 1) cut out."""
    n = 1 << depth
    g = np.zeros((n, n, n), np.uint16)
    g[lo:hi, lo:hi, lo:hi] = material
    g[lo + 1:hi - 1, lo + 1:hi - 1, lo + 1:hi - 1] = 0
    return g


def grid_cases():
    """name -> (grid, material): every grid of mesh_model.fill_cases(), the serpentines, the sphere that leaves the grid, the collapses."""
    out = {name: (g, 9 if name != "depth2" else 2) for name, g in M.fill_cases().items()}
    for depth in (5, 6):
        for along in (0, 1, 2):
            for sealed in (False, True):
                out[f"serpentine{depth}_{'xyz'[along]}_{'sealed' if sealed else 'open'}"] = (M.serpentine(depth, 16, 4, sealed, along)[0], 8)
    out["through_faces"] = (_sphere_through_the_faces(), 2)
    out["cube_to_one_leaf"] = (hollow_cube(3, 0, 8, 5), 5)              # the shell's own material: the whole chunk one LEAF
    brick = np.zeros((8, 8, 8), np.uint16)
    brick[0:4, 0:4, 0:4] = 5
    brick[1:3, 1:3, 1:3] = 0                                            # one brick with 8 enclosed cells
    out["brick_to_leaf"] = (brick, 5)
    out["brick_stays"] = (brick, 6)
    return out


SERPENTINE_CELLS = 735                                      # the corridor of a 16^3 block


def serpentine7(along, sealed):
    """Depth 7, the cube at cells 56 .. 71: the corridor crosses the block borders at 64 and bricks on both sides exchange face bits."""
    return M.serpentine(7, 16, 56, sealed, along)[0], 8


_chunks = {}


def case_chunk(name):
    """(the input chunk of a grid case, material) - computed once, left unchanged."""
    if name not in _chunks:
        if name.startswith("serpentine7"):
            _, a, s = name.split("_")
            g, material = serpentine7("xyz".index(a), s == "sealed")
        else:
            g, material = grid_cases()[name]
        _chunks[name] = (freeze(G.chunk_of(g)), material)
    return _chunks[name]


_models = {}


def case_model(name):
    """(the model's filled chunk, the count) of a grid case - computed once, left unchanged."""
    if name not in _models:
        chunk, material = case_chunk(name)
        want, filled = model_fill(chunk, material)
        _models[name] = (freeze(want), filled)
    return _models[name]


def untidy_chunk():
    """A depth-4 pool that svo_world_create's validation admits and that is neither minimal nor in FIFO order: the root's child blocks
    are stored in swapped order (child 0's block behind child 1's), one BRANCH has eight EMPTY children, one brick holds one value, one
    LEAF carries material 0, and a hollow 4^3 brick encloses 8 cells.  (chunk, material)"""
    B, L, T = G.BRANCH, G.LEAF, G.TWIG
    tree = np.zeros(1 + 8 * 3, np.uint32)
    tree[0] = G.node(B, 1)
    tree[1] = G.node(B, 17)                                 # child 0 -> the block at 17 (behind child 1's at 9)
    tree[2] = G.node(B, 9)                                  # child 1 -> eight EMPTY children
    tree[3] = G.node(L, 0)                                  # LEAF | 0: empty however it is stored
    tree[4] = G.node(L, 7)
    tree[17] = G.node(T, 1)                                 # brick 1: the hollow one
    tree[18] = G.node(T, 0)                                 # brick 0: one value
    tree[19] = G.node(L, 7)
    hollow = np.full((4, 4, 4), 7, np.uint16)
    hollow[1:3, 1:3, 1:3] = 0
    twig = np.concatenate([np.full(64, 3, np.uint16), hollow.reshape(64)])
    return freeze(dict(position=(0.0, 0.0, 0.0), size=128.0, depth=4, tree=tree, twig=twig)), 7


# ---- depth 12 and 16 ---------------------------------------------------------------------------------------------------------------
CUBE_EDGE = 256                                             # the deep cubes: box_mesh of this many cells, min corner a multiple of 64
CUBE_SHELL, CUBE_FILLED = 258 ** 3 - 254 ** 3, 254 ** 3


def deep_cubes():
    """name -> (depth, meshes, corner in cells): the closed rule marks the cell layers on both sides of every face, so the shell is the
    258^3 box from corner - 1 on, one cell thick, and encloses 254^3 cells."""
    out = {}
    for depth, corner, origin, cell in ((12, 2112, (0.0, 0.0, 0.0), 1.0), (16, 47104, (10.0, -20.0, 30.0), 0.25)):
        lo = np.asarray(origin, np.float64) + corner * cell
        v, ix = M.box_mesh(lo, lo + CUBE_EDGE * cell)
        out[f"cube{depth}"] = (depth, [S.mesh(v, ix, origin=origin, cell=cell, material=6)], corner)
    return out


def cube_material(corner, x, y, z, shell, fill):
    """What the filled deep cube holds at voxel (x, y, z): the shell's material, the fill's, or 0."""
    d = [c - (corner - 1) for c in (x, y, z)]
    if any(c < 0 or c >= 258 for c in d):
        return 0
    return shell if any(c < 2 or c >= 256 for c in d) else fill


_windows = {}


def filled_windows(name, material):
    """The windowed model of a deep sphere case of sparse_mesh_model, filled: [(corner, array)], how many cells - computed once."""
    if (name, material) not in _windows:
        out, total = [], 0
        for corner, arr in S.deep_windows(name):
            a = arr.copy()
            rim = np.ones(a.shape, bool)
            rim[1:-1, 1:-1, 1:-1] = False
            assert not a[rim].any(), "the window's outermost cell layer must be empty in the shell"
            total += M.fill_enclosed(a, material)
            a.setflags(write=False)
            out.append((corner, a))
        _windows[(name, material)] = (out, total)
    return _windows[(name, material)]


def largest_leaf_edge(chunk) -> int:
    """The edge in voxels of the largest LEAF the root reaches (0: none)."""
    tree, best, stack = chunk["tree"], 0, [(0, 1 << int(chunk["depth"]))]
    while stack:
        i, e = stack.pop()
        w = int(tree[i])
        if w >> 30 == G.LEAF:
            best = max(best, e)
        elif w >> 30 == G.BRANCH:
            stack.extend(((w & 0x3FFFFFFF) + c, e // 2) for c in range(8))
    return best
