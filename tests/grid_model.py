"""numpy model of "the tree of a grid" and of the grid of a tree (include/svo.h: svo_chunk_from_grid, svo_world_chunk_from_grid,
svo_world_chunk_to_grid), written from the rule in the header, and the grids every grid test uses.  Test infrastructure: the yardstick
the host builder (csrc/grid.cpp) and the device kernels (csrc/grid.hip) are held against.

A grid is a [z, y, x] uint16 array of N = 2^depth cells per axis, 0 = empty."""
from collections import deque

import numpy as np

EMPTY, LEAF, BRANCH, TWIG = 0, 1, 2, 3


def node(kind: int, offset: int = 0) -> int:
    return (kind << 30) | (offset & 0x3FFFFFFF)


def depth_of(grid) -> int:
    n = grid.shape[0]
    assert grid.shape == (n, n, n) and n >= 4 and n & (n - 1) == 0
    return n.bit_length() - 1


def grid_to_pools(grid):
    """(tree uint32[], twig uint16[]) of the grid: the FIFO walk from the root, a node judged by the min and max of the cells it covers."""
    grid = np.asarray(grid, np.uint16)
    depth, n = depth_of(grid), grid.shape[0]
    lo, hi = [], []                                         # per level L: min / max of every node's cells, [z, y, x] of 2^L per axis
    for L in range(depth - 1):
        k, e = 1 << L, n >> L
        blocks = grid.reshape(k, e, k, e, k, e)
        lo.append(blocks.min(axis=(1, 3, 5)))
        hi.append(blocks.max(axis=(1, 3, 5)))
    tree, twig = [0], []
    queue = deque([(0, 0, 0, 0, 0)])                        # (level, x, y, z, slot): x, y, z the node's integer corner in cells
    branches = 0
    while queue:
        L, x, y, z, slot = queue.popleft()
        e = n >> L
        a, b = int(lo[L][z // e, y // e, x // e]), int(hi[L][z // e, y // e, x // e])
        if a == b:
            tree[slot] = node(LEAF, a) if a else node(EMPTY)
        elif L == depth - 2:
            tree[slot] = node(TWIG, len(twig))
            twig.append(grid[z:z + 4, y:y + 4, x:x + 4].reshape(64))     # cz*16 + cy*4 + cx
        else:
            first = 1 + 8 * branches
            branches += 1
            tree[slot] = node(BRANCH, first)
            tree.extend([0] * 8)
            h = e // 2
            for c in range(8):
                queue.append((L + 1, x + (c & 1) * h, y + ((c >> 1) & 1) * h, z + (c >> 2) * h, first + c))
    assert len(tree) == 1 + 8 * branches
    return np.array(tree, np.uint32), (np.concatenate(twig) if twig else np.zeros(0, np.uint16)).astype(np.uint16)


def chunk_of(grid, position=(0.0, 0.0, 0.0), size=128.0) -> dict:
    tree, twig = grid_to_pools(grid)
    return dict(position=tuple(float(v) for v in position), size=float(size), depth=depth_of(np.asarray(grid)), tree=tree, twig=twig)


def voxel_material(chunk, X, Y, Z) -> int:
    """The material of the chunk's finest voxel (X, Y, Z): the descent from the root by integer coordinates."""
    tree, twig, lg = chunk["tree"], chunk["twig"], int(chunk["depth"])
    i = 0
    while True:
        w = int(tree[i])
        kind, off = w >> 30, w & 0x3FFFFFFF
        if kind == EMPTY:
            return 0
        if kind == LEAF:
            return off & 0xFFFF
        if kind == TWIG:
            c = lg - 2
            return int(twig[off * 64 + ((Z >> c) & 3) * 16 + ((Y >> c) & 3) * 4 + ((X >> c) & 3)])
        lg -= 1
        i = off + (((X >> lg) & 1) | ((Y >> lg) & 1) << 1 | ((Z >> lg) & 1) << 2)


def pools_to_grid(chunk, depth):
    """[z, y, x] grid of 2^depth cells per axis: cell x reports voxel x << (D - depth) (depth <= D) or x >> (depth - D)."""
    D, n = int(chunk["depth"]), 1 << depth
    fine = np.zeros((1 << D,) * 3, np.uint16)               # the chunk at its own depth, node by node
    tree, twig = chunk["tree"], chunk["twig"]
    stack = [(0, 0, 0, 0, 1 << D)]
    while stack:
        i, x, y, z, e = stack.pop()
        w = int(tree[i])
        kind, off = w >> 30, w & 0x3FFFFFFF
        if kind == LEAF:
            fine[z:z + e, y:y + e, x:x + e] = off & 0xFFFF
        elif kind == TWIG:
            c = e // 4
            cells = np.asarray(twig[off * 64:off * 64 + 64]).reshape(4, 4, 4)
            fine[z:z + e, y:y + e, x:x + e] = np.repeat(np.repeat(np.repeat(cells, c, 0), c, 1), c, 2)
        elif kind == BRANCH:
            h = e // 2
            for c in range(8):
                stack.append((off + c, x + (c & 1) * h, y + ((c >> 1) & 1) * h, z + (c >> 2) * h, h))
    idx = np.arange(n)
    idx = idx << (D - depth) if depth <= D else idx >> (depth - D)
    return fine[np.ix_(idx, idx, idx)]


# ---- the grids of the tests (seeded: the same for every test) ----------------------------------------------------------------------
MATERIALS = (1, 5, 6, 300, 0xFFFF)


def g2():
    """depth 2, the root at level depth-2: EMPTY, LEAF and TWIG."""
    rng = np.random.default_rng(2)
    return {"g2_empty": np.zeros((4, 4, 4), np.uint16), "g2_leaf": np.full((4, 4, 4), 7, np.uint16),
            "g2_mixed": rng.integers(0, 4, (4, 4, 4)).astype(np.uint16)}


def g3():
    """depth 3: one octant all 0xFFFF, one all zero, one a uniform 4^3 of material 9 (a LEAF at brick level), five mixed."""
    rng = np.random.default_rng(3)
    g = rng.choice(np.array([0, 1, 5, 300], np.uint16), (8, 8, 8)).astype(np.uint16)
    g[0:4, 0:4, 0:4] = 0xFFFF
    g[0:4, 0:4, 4:8] = 0
    g[4:8, 4:8, 0:4] = 9
    return g


def g5():
    """depth 5: random boxes over an empty background, one box aligned to a 16^3 node (a LEAF above brick level) and one 8^3 node filled
    by two materials."""
    rng = np.random.default_rng(5)
    g = np.zeros((32, 32, 32), np.uint16)
    for _ in range(14):
        lo = rng.integers(0, 28, 3)
        hi = np.minimum(lo + rng.integers(1, 12, 3), 32)
        g[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = MATERIALS[int(rng.integers(0, len(MATERIALS)))]
    g[16:32, 0:16, 16:32] = 300                             # node (x 16, y 0, z 16) of level 1
    g[0:8, 24:32, 8:12] = 5                                 # node (x 8, y 24, z 0) of level 2: its x halves differ
    g[0:8, 24:32, 12:16] = 0xFFFF
    return g


def g6():
    """depth 6: a sphere shell plus 2 % single voxels: some level holds more than 256 frontier nodes."""
    rng = np.random.default_rng(6)
    i = np.arange(64) + 0.5
    z, y, x = np.meshgrid(i, i, i, indexing="ij")
    r = np.sqrt((x - 31.0) ** 2 + (y - 33.0) ** 2 + (z - 30.0) ** 2)
    g = np.where((r > 20.0) & (r < 24.0), 6, 0).astype(np.uint16)
    dots = rng.random((64, 64, 64)) < 0.02
    g[dots] = rng.choice(np.array(MATERIALS, np.uint16), int(dots.sum()))
    return g


def heightfield(depth, seed=7):
    """A heightfield of layered materials with caves (spheres cut out): [z, y, x]."""
    rng = np.random.default_rng(seed)
    n = 1 << depth
    i = np.arange(n) / n
    zz, xx = np.meshgrid(i, i, indexing="ij")
    h = 0.35 + 0.12 * np.sin(7.0 * xx + 1.3) * np.cos(5.0 * zz) + 0.06 * np.sin(23.0 * xx * zz + 0.4) + 0.03 * np.cos(41.0 * zz + 17.0 * xx)
    top = (h * n).astype(np.int64)[:, None, :]              # [z, 1, x]
    y = np.arange(n)[None, :, None]
    g = np.where(y < top - 6, 1, np.where(y < top - 1, 5, np.where(y < top, 300, 0))).astype(np.uint16)
    for _ in range(12):
        c = rng.integers(n // 8, n - n // 8, 3)
        rad = int(rng.integers(n // 32 + 2, n // 10 + 3))
        lo, hi = np.maximum(c - rad, 0), np.minimum(c + rad + 1, n)
        sz, sy, sx = (np.arange(lo[a], hi[a]) - c[a] for a in (2, 1, 0))
        ball = sz[:, None, None] ** 2 + sy[None, :, None] ** 2 + sx[None, None, :] ** 2 <= rad * rad
        view = g[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
        view[ball] = 0
    return g


def g7():
    """depth 7: terrain with caves - 2 M cells, several thousand bricks."""
    return heightfield(7)


_cache = {}


def grids():
    """name -> grid, every test grid."""
    if not _cache:
        _cache.update(g2())
        _cache.update({"g3": g3(), "g5": g5(), "g6": g6(), "g7": g7()})
        for g in _cache.values():
            g.setflags(write=False)
    return _cache


_pools = {}


def model_chunk(name) -> dict:
    """The model's chunk of grids()[name] at the origin, size 128 - computed once, shared, left unchanged."""
    if name not in _pools:
        c = chunk_of(grids()[name])
        c["tree"].setflags(write=False)
        c["twig"].setflags(write=False)
        _pools[name] = c
    return _pools[name]


def is_minimal(chunk) -> bool:
    """No reachable BRANCH with eight equal EMPTY / LEAF children, no reachable brick of one value."""
    tree, twig = chunk["tree"], chunk["twig"]
    stack = [0]
    while stack:
        w = int(tree[stack.pop()])
        kind, off = w >> 30, w & 0x3FFFFFFF
        if kind == TWIG and np.unique(twig[off * 64:off * 64 + 64]).size == 1:
            return False
        if kind == BRANCH:
            kids = [int(v) for v in tree[off:off + 8]]
            if all((k >> 30) in (EMPTY, LEAF) for k in kids) and len(set(kids)) == 1:
                return False
            stack.extend(range(off, off + 8))
    return True
