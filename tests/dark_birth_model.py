"""dark_birth_model.py — the hit block's "dark at birth" test in float32 — TEST INFRASTRUCTURE.

A primary hit on a cell of brick B whose shadow origin the hit block locates in an OCCUPIED cell of B is shadowed: the
reference's shadow march samples the origin itself first (t = 0 in chunkmarch, treemarch and twigmarch), locates B and that
cell by the same arithmetic and returns a hit there, after one chunk step, one tree step and one brick cell.  The test is
the brick step's: every difference `p - Blo` >= 0, every cell coordinate <= 3, the cell's bit set in the brick's mask.

Premises (DarkBirthModel.enabled): a finite shadow direction, a power-of-two chunk size and no world corner with a negative
coordinate (World::index puts a point at, or one float above, a negative multiple of the chunk size into the chunk below).
The rule needs no prepared light and no eps premise: it holds where §6t and §6u are off (the device's default leaves it off below
eps = 2u for a test's sake, DESIGN §6v "Host"; the model states the rule).

`faults` plants the mistakes that tests/test_dark_birth_cpu.py must catch.
"""
from __future__ import annotations

import math

import numpy as np

import brick_clearance_model as BM

P = BM.P
f32 = np.float32
FAULTS = ("clamp", "transposed", "other_brick", "no_premises")


class DarkBirthModel:
    def __init__(self, chunks, dims, chunksize, light_dir, chunkcoordmin=(0, 0, 0), eps=P.EPS, faults=()):
        assert all(f in FAULTS for f in faults), faults
        self.faults = frozenset(faults)
        self.geo = BM.BrickClearanceModel(chunks, dims, chunksize, light_dir, chunkcoordmin, eps=eps)     # chunks, twig_nodes, locate, march_lit
        self.chunks, self.sdir, self.eps = self.geo.chunks, self.geo.sdir, self.geo.eps
        m, _ = math.frexp(float(chunksize))
        self.enabled = (all(math.isfinite(float(v)) for v in self.sdir) and m == 0.5 and all(v >= 0 for v in chunkcoordmin)) or "no_premises" in self.faults
        self._nodes, self._frames = {}, {}

    def twig_nodes(self, ci):
        if ci not in self._nodes:
            self._nodes[ci] = self.geo.twig_nodes(ci)
        return self._nodes[ci]

    def cells(self, ci, offset):
        """The 64 words of TWIG node `offset` of chunk ci."""
        ch = self.chunks[ci]
        if "other_brick" in self.faults:                    # the brick stored next to the located one
            nodes = self.twig_nodes(ci)
            k = [n[0] for n in nodes].index(offset)
            offset = nodes[(k + 1) % len(nodes)][0]
        return ch.twig[ch.tree[offset] & 0x3FFFFFFF]

    def dark(self, origins, ci, offset, blo, size):
        """The hit block's verdict for shadow origins [N,3] of primary hits in TWIG node `offset` (box blo, edge size) of chunk ci,
        with its float32 expressions -> bool [N]: located in an occupied cell of that brick."""
        o = np.asarray(origins, f32).reshape(-1, 3)
        if not self.enabled:
            return np.zeros(len(o), bool)
        inv_res = f32(1.0) / (f32(size) * f32(0.25))        # (a power of two: exact)
        d = o - np.asarray(blo, f32)[None, :]
        f = d * inv_res
        with np.errstate(invalid="ignore"):
            u = np.where(np.isfinite(f), f, f32(-1.0)).astype(np.int64)      # (int)f, truncation
        ok = (d >= 0).all(axis=1)                           # (the difference's sign: a voxel above 1 takes a denormal difference below 0 to -0)
        if "clamp" in self.faults:
            u = np.minimum(u, 3)
        ok &= (u <= 3).all(axis=1)
        u = np.clip(u, 0, 3)
        word = u[:, 0] * 16 + u[:, 1] * 4 + u[:, 2] if "transposed" in self.faults else u[:, 2] * 16 + u[:, 1] * 4 + u[:, 0]
        return ok & (np.asarray(self.cells(ci, offset))[word] != 0)

    def dark_at_hit(self, origin, hit_chunk, hit_node):
        """The same for one primary hit known by its record (chunk, node): the frame is that of the TWIG node."""
        frame = self._frames.get(hit_chunk)
        if frame is None:
            frame = self._frames[hit_chunk] = {off: (lo, size) for off, lo, size in self.twig_nodes(hit_chunk)}
        if hit_node not in frame:
            return False
        return bool(self.dark([origin], hit_chunk, hit_node, *frame[hit_node])[0])


def model_of(oracle_world, dims, chunksize, light_dir, chunkcoordmin=(0, 0, 0), faults=(), eps=P.EPS):
    """DarkBirthModel over an oracle_binding.OracleWorld."""
    n = dims[0] * dims[1] * dims[2]
    return DarkBirthModel([oracle_world.chunk(i) for i in range(n)], dims, chunksize, light_dir, chunkcoordmin, eps=eps, faults=faults)
