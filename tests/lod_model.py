"""Test model of Ocroot::defragcopy / Ocroot::lodmm (src/Octree.cpp:445-765) and MisraGriesCounter (src/MisraGries.h): plain
Python / numpy on pool dicts (tree: uint32 node words, twig: uint16 cells, 64 per brick, depth).  It does not import the library.

The recursions are restated as the reference runs them: nodes written into a growing pool, a folded subtree's blocks and bricks
taken back by resetting the counters (their words stay readable), a resampled brick read back with `descend` at the cell centres,
lodmm's cells counted by `density` into a weighted Misra-Gries counter (the reference is built without NDEBUG, so the
`assert(density(...))` call does run).  Float arithmetic is float32, as in the reference.

`coarsen(..., full=False)` computes lodmm's cells by the short form the library uses (one child: its value; one 2x2x2 block of
brick cells: the most frequent value, ties to the first in z, y, x order); the CPU tests check that it agrees with the full form.
"""
from __future__ import annotations

import numpy as np

EMPTY, LEAF, BRANCH, TWIG = 0, 1, 2, 3
TWIG_LEVELS, TWIG_SIZE, TWIG_WORDS = 2, 4, 64
F = np.float32


def ntype(w) -> int:
    return int(w) >> 30


def noff(w) -> int:
    return int(w) & 0x3FFFFFFF


def node(t, off=0) -> int:
    return (t << 30) | (int(off) & 0x3FFFFFFF)


def word(x, y, z) -> int:
    return z * 16 + y * 4 + x


def branch(gx, gy, gz) -> int:
    return int(gx) + 2 * int(gy) + 4 * int(gz)


class MisraGries:
    """MisraGriesCounter<K> with the weighted count(i, n) (its replacement search starts at k = 1) and majority()."""

    def __init__(self, k=8):
        self.k = k
        self.empty()

    def empty(self):
        self.A = [0] * self.k
        self.keys = [0] * self.k

    def count(self, i, n):
        assert n > 0
        for k in range(self.k):
            if self.keys[k] == i and self.A[k] != 0:
                self.A[k] += n
                return self.A[k]
        for k in range(self.k):
            if self.A[k] == 0:
                self.keys[k], self.A[k] = i, n
                return n
        d, r = n, -1
        for k in range(1, self.k):
            if self.A[k] < d:
                r, d = k, self.A[k]
        if r != -1:
            self.keys[r], self.A[r] = i, n
        for k in range(self.k):
            self.A[k] -= d
        return 0

    def majority(self):
        i = 0
        for k in range(1, self.k):
            if self.A[k] > self.A[i]:
                i = k
        return self.keys[i]


def _vec(v):
    return np.asarray(v, dtype=F)


def descend(tree, twig, offset, cmin, size, p) -> int:
    """The reference's descend(): material at point p under node `offset` whose cube is [cmin, cmin + size]."""
    cmin, p, size = _vec(cmin), _vec(p), F(size)
    while True:
        t = int(tree[offset])
        if ntype(t) == EMPTY:
            return 0
        if ntype(t) == LEAF:
            return noff(t) & 0xFFFF
        if ntype(t) == TWIG:
            leafsize = F(size / F(1 << TWIG_LEVELS))
            i = ((p - cmin) / leafsize).astype(np.int32)
            return int(twig[noff(t) * TWIG_WORDS + word(int(i[0]), int(i[1]), int(i[2]))])
        half = F(size * F(0.5))
        geq = p >= (cmin + half).astype(F)
        offset = noff(t) + branch(*geq)
        cmin = (cmin + geq.astype(F) * half).astype(F)
        size = half


def _cubes_intersect(a0, a1, b0, b1) -> bool:
    return bool(np.all(a1 >= b0) and np.all(b1 >= a0))


def density(tree, twig, offset, bmin, size, cmin, cmax, c: MisraGries, n: int) -> int:
    """The reference's density(): every node under `offset` that the box [cmin, cmax] touches counted with weight n / 8^level."""
    t = int(tree[offset])
    if ntype(t) == EMPTY:
        c.count(0, n)
        return 1
    if ntype(t) == LEAF:
        c.count(noff(t), n)
        return 1
    if ntype(t) == TWIG:
        leafsize = F(F(size) / F(1 << TWIG_LEVELS))
        lo = np.clip(((cmin - bmin) / leafsize).astype(F), F(0), F(TWIG_SIZE))
        hi = np.clip(((cmax - bmin) / leafsize).astype(F), F(0), F(TWIG_SIZE))
        m = n // (1 << (TWIG_LEVELS * 3))
        z = int(lo[2])
        while F(z) < hi[2]:
            y = int(lo[1])
            while F(y) < hi[1]:
                x = int(lo[0])
                while F(x) < hi[0]:
                    c.count(int(twig[noff(t) * TWIG_WORDS + word(x, y, z)]), m)
                    x += 1
                y += 1
            z += 1
        return TWIG_LEVELS
    half = F(F(size) * F(0.5))
    d = 0
    for i in range(8):
        g = np.array([i & 1, (i >> 1) & 1, (i >> 2) & 1], dtype=F)
        nmin = (bmin + g * half).astype(F)
        nmax = (nmin + half).astype(F)
        if _cubes_intersect(cmin, cmax, nmin, nmax):
            d = max(d, density(tree, twig, noff(t) + i, nmin, half, cmin, cmax, c, n // 8))
    return d + 1


def short_majority(values) -> int:
    """Most frequent value, ties to the first seen."""
    values = list(values)
    best, best_n = values[0], 0
    for v in values:
        k = values.count(v)
        if k > best_n:
            best, best_n = v, k
    return best


class _Pools:
    def __init__(self):
        self.tree = [0]
        self.twig = []            # one np.uint16[64] per brick (a taken-back brick's cells stay until overwritten)
        self.trees, self.twigs = 1, 0

    def put(self, i, w):
        while len(self.tree) <= i:
            self.tree.extend([0] * max(len(self.tree), 8))
        self.tree[i] = w

    def add_brick(self, cells):
        i = self.twigs
        self.twigs += 1
        if len(self.twig) <= i:
            self.twig.append(None)
        self.twig[i] = np.array(cells, dtype=np.uint16)
        return i

    def flat_twig(self):
        return np.concatenate(self.twig[:self.twigs]).astype(np.uint16) if self.twigs else np.zeros(0, np.uint16)


class _Rebuild:
    def __init__(self, chunk, full=True):
        self.ft = np.asarray(chunk["tree"], dtype=np.uint32)
        self.fw = np.asarray(chunk["twig"], dtype=np.uint16)
        self.depth = int(chunk["depth"])
        self.full = full
        self.to = _Pools()

    def make_twig(self, t, cells) -> int:
        cells = np.asarray(cells, dtype=np.uint16)
        if np.all(cells == cells[0]):
            x = int(cells[0])
            self.to.put(t, node(EMPTY if not x else LEAF, x))
            return 1
        self.to.put(t, node(TWIG, self.to.add_brick(cells)))
        return TWIG_LEVELS + 1

    def defragcopy(self, f, t) -> int:
        w = int(self.ft[f])
        if ntype(w) == EMPTY:
            self.to.put(t, node(EMPTY, 0))
            return 1
        if ntype(w) == LEAF:
            self.to.put(t, node(LEAF, noff(w)))
            return 1
        if ntype(w) == TWIG:
            return self.make_twig(t, self.fw[noff(w) * 64:(noff(w) + 1) * 64])
        to = self.to
        trees, twigs = to.trees, to.twigs
        i = to.trees
        to.put(t, node(BRANCH, i))
        to.trees += 8
        maxd = 0
        for j in range(8):
            maxd = max(maxd, self.defragcopy(noff(w) + j, i + j))
        if maxd == 1:
            t0, x = ntype(to.tree[i]), noff(to.tree[i])
            if all(ntype(to.tree[i + j]) == t0 and noff(to.tree[i + j]) == x for j in range(1, 8)):
                to.trees, to.twigs = trees, twigs
                to.put(t, node(EMPTY if not x else LEAF, x))
                return 1
        if maxd == TWIG_LEVELS:
            to.trees, to.twigs = trees, twigs
            # descend on the copy at the cell centres: node t is still BRANCH i, and nothing under it is a brick (that returns 3)
            cells = np.zeros(64, np.uint16)
            for z in range(4):
                for y in range(4):
                    for x in range(4):
                        p = np.array([x, y, z], dtype=F) * F(0.25) + F(0.125)
                        cells[word(x, y, z)] = descend(to.tree, None, t, (0, 0, 0), 1.0, p)
            return self.make_twig(t, cells)
        return maxd + 1

    def lod_cells(self, f):
        cells = np.zeros(64, np.uint16)
        if self.full:
            eps = F(1.0 / 256.0)
            c = MisraGries(8)
            for z in range(4):
                for y in range(4):
                    for x in range(4):
                        lo = (np.array([x, y, z], dtype=F) * F(0.25)).astype(F)
                        hi = (lo + F(0.25)).astype(F)
                        c.empty()
                        density(self.ft, self.fw, f, np.zeros(3, F), F(1.0), (lo + eps).astype(F), (hi - eps).astype(F), c, 1 << 9)
                        cells[word(x, y, z)] = c.majority() & 0xFFFF
            return cells
        w = int(self.ft[f])
        for z in range(4):
            for y in range(4):
                for x in range(4):
                    ch = int(self.ft[noff(w) + branch(x >> 1, y >> 1, z >> 1)])
                    if ntype(ch) != TWIG:
                        cells[word(x, y, z)] = noff(ch) & 0xFFFF if ntype(ch) == LEAF else 0
                        continue
                    b = self.fw[noff(ch) * 64:(noff(ch) + 1) * 64]
                    x0, y0, z0 = (x & 1) * 2, (y & 1) * 2, (z & 1) * 2
                    vals = [int(b[word(x0 + dx, y0 + dy, z0 + dz)]) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
                    cells[word(x, y, z)] = short_majority(vals)
        return cells

    def lodmm(self, f, t, level):
        w = int(self.ft[f])
        if ntype(w) != BRANCH:
            self.defragcopy(f, t)
            return
        to = self.to
        if level == (self.depth - 1) - TWIG_LEVELS:
            to.put(t, node(TWIG, to.add_brick(self.lod_cells(f))))
            return
        pos = to.trees
        to.put(t, node(BRANCH, pos))
        to.trees += 8
        for i in range(8):
            self.lodmm(noff(w) + i, pos + i, level + 1)

    def result(self, chunk, depth):
        to = self.to
        return {"position": tuple(chunk["position"]), "size": chunk["size"], "depth": depth,
                "tree": np.array(to.tree[:to.trees], dtype=np.uint32), "twig": to.flat_twig()}


def compact(chunk) -> dict:
    """Ocroot::defragcopy of a pool dict."""
    r = _Rebuild(chunk)
    r.defragcopy(0, 0)
    return r.result(chunk, int(chunk["depth"]))


def coarsen(chunk, full=True) -> dict:
    """Ocroot::lodmm of a pool dict (depth -> depth - 1); full=False: the short form of the cells (see the module's doc)."""
    assert int(chunk["depth"]) > TWIG_LEVELS
    r = _Rebuild(chunk, full=full)
    r.lodmm(0, 0, 0)
    return r.result(chunk, int(chunk["depth"]) - 1)


def material_at(chunk, p) -> int:
    """descend from the root of a pool dict at a point in chunk coordinates."""
    return descend(np.asarray(chunk["tree"], np.uint32), np.asarray(chunk["twig"], np.uint16), 0,
                   _vec(chunk["position"]), F(chunk["size"]), _vec(p))
