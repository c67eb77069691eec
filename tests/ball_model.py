"""Host model of svo_world_edit_ball / svo_world_edit_ball_all (include/svo.h): the depth-first edit of the Python twin
(oracle/svo_oracle_py.py: _destroy_cube / _build_cube) stated once with the region as a pair of predicates - touch(box) where the twin
asks cubes_intersect(box, region), inside(box) where it asks cube_is_inside(region, box).  With Box the model is the twin's
Chunk.build / destroy / replace (tests/test_ball_cpu.py holds it to that, pools index for index); with Ball it is the definition the
device edit is held against.  numpy float32, one rounding per operation; the 64 cells of a brick are judged at once.
Test infrastructure: the twin's helpers are imported, not restated."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import svo_oracle_py as P                                   # noqa: E402

f32 = np.float32
BUILD, DESTROY, REPLACE = 0, 1, 2                           # SVO_EDIT_BUILD / _DESTROY / _REPLACE
EMPTY, LEAF, BRANCH, TWIG = P.EMPTY, P.LEAF, P.BRANCH, P.TWIG
_CELL = np.arange(P.TWIG_SIZE, dtype=f32)


class Box:
    """The closed box [lo, hi]: the twin's own predicates (src/Traverse.cpp:173-185)."""

    def __init__(self, lo, hi):
        self.lo, self.hi = P.vec3(*lo), P.vec3(*hi)

    def touch(self, bmin, bmax):
        r = (bmax[0] >= self.lo[0]) & (bmax[1] >= self.lo[1]) & (bmax[2] >= self.lo[2])
        return r & (self.hi[0] >= bmin[0]) & (self.hi[1] >= bmin[1]) & (self.hi[2] >= bmin[2])

    def inside(self, bmin, bmax):
        r = (bmin[0] >= self.lo[0]) & (bmin[1] >= self.lo[1]) & (bmin[2] >= self.lo[2])
        return r & (self.hi[0] >= bmax[0]) & (self.hi[1] >= bmax[1]) & (self.hi[2] >= bmax[2])


class Ball:
    """The closed ball |p - centre| <= radius; R2 = radius * radius in float."""

    def __init__(self, centre, radius):
        self.c = P.vec3(*centre)
        self.r2 = f32(radius) * f32(radius)

    def touch(self, bmin, bmax):
        d = []
        for a in range(3):
            near = bmin[a] - self.c[a]
            far = self.c[a] - bmax[a]
            d.append(np.where(near > 0, near, np.where(far > 0, far, f32(0))))
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= self.r2

    def inside(self, bmin, bmax):
        f = []
        for a in range(3):
            u, v = self.c[a] - bmin[a], bmax[a] - self.c[a]
            f.append(np.where(u < v, v, u))
        return (f[0] * f[0] + f[1] * f[1]) + f[2] * f[2] <= self.r2


def chunk_of(c) -> P.Chunk:
    """A twin Chunk over a chunk dict (position, size, depth, tree, twig); its bricks are rows of one uint16 array, replaced whole by
    the edits, so that a chunk of millions of cells costs no Python loop."""
    root = P.Chunk(c["position"], c["size"], c["depth"])
    root.tree = np.asarray(c["tree"], dtype=np.uint32).tolist()
    root.twig = list(np.array(c["twig"], dtype=np.uint16).reshape(-1, 64))
    root.treestoragesize, root.twigstoragesize = max(16, root.trees), max(16, root.twigs)
    return root


def pools_of(root: P.Chunk) -> dict:
    twig = np.concatenate([np.asarray(b, dtype=np.uint16) for b in root.twig]) if root.twigs else np.zeros(0, np.uint16)
    return dict(position=tuple(float(v) for v in root.position), size=float(root.size), depth=root.depth,
                tree=np.array(root.tree, dtype=np.uint32), twig=twig)


def _new_brick(root, offset, value):
    if root.twigs >= root.twigstoragesize:
        root.twigstoragesize *= 2
    root.tree[offset] = P.node_make(TWIG, root.twigs)
    root.twig.append(np.full(64, value, np.uint16))


def _split(root, offset, child):
    if root.trees + 8 >= root.treestoragesize:
        root.treestoragesize *= 2
    root.tree[offset] = P.node_make(BRANCH, root.trees)
    root.tree.extend([child] * 8)


def _cells_touched(region, bmin, size):
    """touch of the 64 cell boxes of the brick at bmin, in brick order (z * 16 + y * 4 + x)."""
    leafsize = size / f32(1 << P.TWIG_LEVELS)
    step = _CELL * leafsize
    lo = (bmin[0] + step[None, None, :], bmin[1] + step[None, :, None], bmin[2] + step[:, None, None])
    hi = (lo[0] + leafsize, lo[1] + leafsize, lo[2] + leafsize)
    return np.broadcast_to(region.touch(lo, hi), (4, 4, 4)).reshape(64)


def _visit(root, offset, bmin, size, depth, region, build, material):
    """One visit of the depth-first edit.  build: EMPTY nodes take the material (whole if inside, else cut open), LEAF nodes stay;
    destroy: whatever lies inside goes, LEAF nodes the region cuts are cut open, EMPTY nodes stay.  A node cut open becomes a brick at
    level depth - 2, a BRANCH above it, and is visited again."""
    bmax = P.vadds(bmin, size)
    if not bool(region.touch(bmin, bmax)):
        return
    t = root.tree[offset]
    kind = P.node_type(t)
    cut = EMPTY if build else LEAF                          # the node kind the region cuts open
    if kind == (LEAF if build else EMPTY):
        return
    if kind == cut or not build:
        if bool(region.inside(bmin, bmax)):
            root.tree[offset] = P.node_make(LEAF, material) if build else P.node_make(EMPTY, 0)
            return
    if kind == cut:
        if depth == root.depth - P.TWIG_LEVELS:
            _new_brick(root, offset, 0 if build else P.node_offset(t) & 0xFFFF)
        else:
            _split(root, offset, P.node_make(EMPTY, 0) if build else P.node_make(LEAF, P.node_offset(t)))
        _visit(root, offset, bmin, size, depth, region, build, material)
    elif kind == TWIG:
        cells = np.array(root.twig[P.node_offset(t)], dtype=np.uint16)
        hit = _cells_touched(region, bmin, size)
        if build:
            cells[hit & (cells == 0)] = material
        else:
            cells[hit] = 0
        root.twig[P.node_offset(t)] = cells
    else:
        half = size * f32(0.5)
        for i in range(8):
            _visit(root, P.node_offset(t) + i, P.vadd(bmin, P.vmuls(P.vec3(*P.cut(i)), half)), half, depth + 1, region, build, material)


def edit(root: P.Chunk, op, region, material=0):
    """op applied to the twin Chunk in place: replace is destroy then build."""
    if op in (DESTROY, REPLACE):
        _visit(root, 0, root.position, root.size, 0, region, False, 0)
    if op in (BUILD, REPLACE):
        _visit(root, 0, root.position, root.size, 0, region, True, int(material))
    return root


def touched_chunks(positions, chunksize, ball):
    """svo_world_edit_ball_all's list: the chunks whose box [position, position + chunksize] the ball touches, ascending."""
    out = []
    for j, pos in enumerate(positions):
        lo = P.vec3(*pos)
        if bool(ball.touch(lo, P.vadds(lo, f32(chunksize)))):
            out.append(j)
    return out


def cell_boxes(position, size, depth):
    """(lo, hi) of every finest cell of a chunk on exact geometry, broadcastable to [z, y, x]."""
    n = 1 << depth
    voxel = f32(size) / f32(n)
    step = np.arange(n, dtype=f32) * voxel
    lo = (f32(position[0]) + step[None, None, :], f32(position[1]) + step[None, :, None], f32(position[2]) + step[:, None, None])
    return lo, (lo[0] + voxel, lo[1] + voxel, lo[2] + voxel)


def brute_force(grid, position, size, op, region, material=0):
    """The rule applied to every cell of a dense [z, y, x] grid: what the pruned recursion must leave."""
    depth = grid.shape[0].bit_length() - 1
    lo, hi = cell_boxes(position, size, depth)
    hit = np.broadcast_to(region.touch(lo, hi), grid.shape)
    out = grid.copy()
    if op in (DESTROY, REPLACE):
        out[hit] = 0
    if op in (BUILD, REPLACE):
        out[hit & (out == 0)] = material
    return out, hit


def blob_grid(depth, seed):
    """A [z, y, x] grid of random solid balls of several materials, with one node-aligned block filled and one emptied: its tree
    holds EMPTY, LEAF, TWIG and BRANCH nodes."""
    rng = np.random.default_rng(seed)
    n = 1 << depth
    i = np.arange(n) + 0.5
    z, y, x = np.meshgrid(i, i, i, indexing="ij")
    g = np.zeros((n, n, n), np.uint16)
    for _ in range(7):
        c = rng.uniform(0, n, 3)
        r = rng.uniform(n / 10, n / 4)
        g[(x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= r * r] = int(rng.integers(1, 8))
    q = n // 4
    g[0:q, 2 * q:3 * q, q:2 * q] = 3
    g[2 * q:3 * q, 0:q, 3 * q:4 * q] = 0
    return g


def node_kinds(chunk) -> set:
    """The kinds of the nodes reachable from the root of a chunk dict."""
    kinds, stack = set(), [0]
    while stack:
        w = int(chunk["tree"][stack.pop()])
        kinds.add(w >> 30)
        if (w >> 30) == BRANCH:
            stack.extend(range(w & 0x3FFFFFFF, (w & 0x3FFFFFFF) + 8))
    return kinds
