"""brick_clearance_model.py — float64 model of the per-brick "every empty cell is clear" flag — TEST INFRASTRUCTURE.

clearance_model.py decides, per EMPTY reference node, whether a shadow ray that has located it is lit whatever it does
afterwards, and takes every brick for occupied.  This model asks the same question of the EMPTY CELLS of a brick: a TWIG
node B gets the flag when, for every empty cell c of B, nothing occupied meets R1(c) ∪ R2(c) of §6t with c in the place of
C.  Occupied means every LEAF node and every occupied cell of every brick, B's own among them.  A shadow ray whose origin
is located in an empty cell of a flagged brick is lit: the stack kernel's hit block settles it without a step.

Premises beside §6t's (BrickClearanceModel.brick_enabled): no world corner has a negative coordinate, the chunk size is a
power of two and no voxel is smaller than u, the float32 spacing at the largest corner coordinate.  Every lattice plane is
then a float, `p - bmin` of a sample p inside a brick is exact and so is its quotient by the voxel size: the cell that
twigmarch locates a sample in contains it, with no tolerance.

`faults` plants the mistakes that tests/test_brick_clearance_cpu.py must catch.
"""
from __future__ import annotations

import math

import numpy as np

import clearance_model as CM

P = CM.P
f32 = np.float32
EMPTY, LEAF, BRANCH, TWIG = CM.EMPTY, CM.LEAF, CM.BRANCH, CM.TWIG
BRICK_FAULTS = ("own_cells", "bricks_empty", "no_neighbour")
FLAG_BIT = 0x8000                                   # bit 15 of the device's bmat word


def _cell_box(blo, leaf, k):
    lo = (blo[0] + leaf * (k & 3), blo[1] + leaf * ((k >> 2) & 3), blo[2] + leaf * (k >> 4))
    return lo, (lo[0] + leaf, lo[1] + leaf, lo[2] + leaf)


class BrickClearanceModel(CM.ClearanceModel):
    def __init__(self, chunks, dims, chunksize, light_dir, chunkcoordmin=(0, 0, 0), eps=P.EPS, faults=()):
        assert all(f in BRICK_FAULTS for f in faults), faults
        super().__init__(chunks, dims, chunksize, light_dir, chunkcoordmin, eps, faults=tuple(f for f in faults if f in CM.FAULTS))
        self.bfaults = frozenset(faults)
        m, _ = math.frexp(float(chunksize))
        voxel = min(float(c.size) / (1 << c.depth) for c in self.chunks)
        self.brick_enabled = self.enabled and all(v >= 0 for v in self.ccm) and m == 0.5 and voxel >= self.u
        self._bmemo, self._all = {}, None

    # ------------------------------------------------------------------ every occupied box of the world, once
    def _boxes(self):
        """lo[N,3], hi[N,3], chunk[N], node[N] (the TWIG node's offset for a brick cell, -1 for a LEAF node) of everything occupied."""
        if self._all is None:
            lo, size, chunk, node = [], [], [], []
            for cj, ch in enumerate(self.chunks):
                stack = [(0, ch.lo, float(ch.size))]
                while stack:
                    off, l, sz = stack.pop()
                    w = ch.tree[off]
                    kind = w >> 30
                    if kind == LEAF:
                        lo.append(l); size.append(sz); chunk.append(cj); node.append(-1)
                    elif kind == TWIG:
                        leaf = sz * 0.25
                        for k in np.nonzero(ch.twig[w & 0x3FFFFFFF])[0].tolist():
                            lo.append(_cell_box(l, leaf, k)[0]); size.append(leaf); chunk.append(cj); node.append(off)
                    elif kind == BRANCH:
                        h, base = sz * 0.5, w & 0x3FFFFFFF
                        for i in range(8):
                            stack.append((base + i, (l[0] + h * (i & 1), l[1] + h * ((i >> 1) & 1), l[2] + h * ((i >> 2) & 1)), h))
            lo = np.array(lo, np.float64).reshape(-1, 3)
            self._all = (lo, lo + np.array(size, np.float64).reshape(-1, 1), np.array(chunk, np.int64), np.array(node, np.int64))
        return self._all

    # ------------------------------------------------------------------ the region of a cell (or of a whole brick) against many boxes
    def _prism_v(self, lo, hi, clo, chi, d):
        """ClearanceModel._prism for cells clo / chi [E,3] against boxes lo / hi [M,3], the same float64 expressions -> [E,M]."""
        shape = (len(clo), len(lo))
        ok = np.ones(shape, bool)
        l0, l1, slack = np.zeros(shape), np.full(shape, np.inf), 1e-9
        for a in range(3):
            blo, bhi, s = lo[None, :, a] - chi[:, a, None] - d, hi[None, :, a] - clo[:, a, None] + d, self.s[a]
            if s == 0.0:
                ok &= ~((blo > 0.0) | (bhi < 0.0))
            else:
                t0, t1 = blo / s, bhi / s
                t0, t1 = np.minimum(t0, t1), np.maximum(t0, t1)
                l0, l1 = np.maximum(l0, t0 - slack), np.minimum(l1, t1 + slack)
        return ok & (l0 <= l1)

    def _meets_v(self, lo, hi, own, clo, chi, inner_lo, inner_hi):
        """R1(c) ∪ R2(c) of §6t for the cells [clo, chi) [E,3] against boxes lo / hi [M,3] (own: in the cells' chunk) -> bool [E,M]."""
        clo, chi = np.asarray(clo, np.float64).reshape(-1, 3), np.asarray(chi, np.float64).reshape(-1, 3)
        shape = (len(clo), len(lo))
        exact, grown, inner = np.broadcast_to(own, shape).copy(), np.ones(shape, bool), own.copy()
        for a in range(3):
            s = self.s[a]
            g = 0.0 if s == 0.0 else self.d2
            if s >= 0.0:
                exact &= hi[None, :, a] > clo[:, a, None]
                grown &= hi[None, :, a] >= clo[:, a, None] - g
            if s <= 0.0:
                exact &= lo[None, :, a] < chi[:, a, None]
                grown &= lo[None, :, a] <= chi[:, a, None] + g
            inner &= (lo[:, a] >= inner_lo[a]) & (hi[:, a] <= inner_hi[a])
        return (exact & self._prism_v(lo, hi, clo, chi, self.d1)) | (~inner[None, :] & grown & self._prism_v(lo, hi, clo, chi, self.d2))

    def _candidates(self, ci, offset, blo, bhi):
        """Every occupied box that meets the region of B's whole box, which contains the region of each of its cells."""
        home = self.chunks[ci]
        inner_lo = tuple(v + self.d2 for v in home.lo)
        inner_hi = tuple(v - self.d2 for v in home.hi)
        lo, hi, chunk, node = self._boxes()
        own = chunk == ci
        mine = own & (node == offset)
        keep = np.ones(len(lo), bool)
        if "no_neighbour" in self.bfaults:
            keep &= own
        if "own_cells" in self.bfaults:
            keep &= ~mine
        if "bricks_empty" in self.bfaults:
            keep &= mine | (node < 0)
        for a in range(3):                              # (R1 and R2 both lie in the grown octant: a cheap first cut, then the full test)
            g = 0.0 if self.s[a] == 0.0 else self.d2
            if self.s[a] >= 0.0:
                keep &= hi[:, a] >= blo[a] - g
            if self.s[a] <= 0.0:
                keep &= lo[:, a] <= bhi[a] + g
        keep = np.nonzero(keep)[0]
        lo, hi, own = lo[keep], hi[keep], own[keep]
        keep = self._meets_v(lo, hi, own, blo, bhi, inner_lo, inner_hi)[0]
        return (lo[keep], hi[keep], own[keep]), inner_lo, inner_hi

    def clear_cells(self, ci, offset, lo, size):
        """-> (empty cells of TWIG node `offset` of chunk ci, those of them whose way to the light is clear), as cell indices."""
        key = (ci, offset)
        r = self._bmemo.get(key)
        if r is None:
            home = self.chunks[ci]
            cells = home.twig[home.tree[offset] & 0x3FFFFFFF]
            empty = [k for k in range(64) if cells[k] == 0]
            clear = []
            if self.brick_enabled and empty:
                blo = tuple(float(v) for v in lo)
                size = float(size)
                cand, inner_lo, inner_hi = self._candidates(ci, offset, blo, (blo[0] + size, blo[1] + size, blo[2] + size))
                boxes = [_cell_box(blo, size * 0.25, k) for k in empty]
                met = self._meets_v(*cand, [b[0] for b in boxes], [b[1] for b in boxes], inner_lo, inner_hi).any(axis=1)
                clear = [k for k, m in zip(empty, met) if not m]
            r = self._bmemo[key] = (empty, clear)
        return r

    def brick_flag(self, ci, offset, lo, size):
        """Does TWIG node `offset` of chunk ci get the flag?  Every empty cell clear (a brick without one: yes, and never asked)."""
        if not self.brick_enabled:
            return False
        empty, clear = self.clear_cells(ci, offset, lo, size)
        return len(empty) == len(clear)

    def twig_nodes(self, ci):
        """(offset, lo, size) of every TWIG node of chunk ci that traverse() can reach."""
        ch = self.chunks[ci]
        out, stack = [], [(0, ch.lo, float(ch.size))]
        while stack:
            off, lo, sz = stack.pop()
            w = ch.tree[off]
            kind = w >> 30
            if kind == TWIG:
                out.append((off, lo, sz))
            elif kind == BRANCH:
                h, base = sz * 0.5, w & 0x3FFFFFFF
                for i in range(8):
                    stack.append((base + i, (lo[0] + h * (i & 1), lo[1] + h * ((i >> 1) & 1), lo[2] + h * ((i >> 2) & 1)), h))
        return out

    def flagged_bricks(self, stored_only=False):
        """Bricks that get the flag; stored_only: those whose 16-bit word has room for it (what the device pass counts)."""
        return sum(1 for ci in range(len(self.chunks)) for off, lo, sz in self.twig_nodes(ci)
                   if self.brick_flag(ci, off, lo, sz) and not (stored_only and self.bmat_word(ci, off) == 0xFFFF))

    def bmat_word(self, ci, offset):
        """The device's 16-bit word of the brick without the flag: its one material, 0 if empty, 0xFFFF if it holds several or
        its one material does not leave bit 15 free."""
        ch = self.chunks[ci]
        mats = np.unique(ch.twig[ch.tree[offset] & 0x3FFFFFFF])
        mats = mats[mats != 0]
        if len(mats) == 0:
            return 0
        return int(mats[0]) if len(mats) == 1 and int(mats[0]) < FLAG_BIT else 0xFFFF

    # ------------------------------------------------------------------ where a shadow ray starts
    def locate(self, origin):
        """The first tree step of the shadow ray from `origin`, with the reference's arithmetic (chunkmarch, treemarch and
        twigmarch at t = 0): -> None outside the world, or dict(chunk, node, kind, bmin, size, cell) - cell is the brick cell
        the origin is located in (None: not a TWIG node, or outside 0..3)."""
        world = self.world
        p = P.vec3(*origin)
        chunksize = f32(world.chunksize)
        ccm = world.chunkcoordmin
        chunkmin = P.vec3(ccm[0] * world.chunksize, ccm[1] * world.chunksize, ccm[2] * world.chunksize)
        chunkmax = P.vmuls(P.vec3(ccm[0] + world.width, ccm[1] + world.height, ccm[2] + world.depth), chunksize)
        if not P.is_inside_cube(p, chunkmin, chunkmax):
            return None
        q = world.index_float(p)
        i = world.index(q[0], q[1], q[2])
        root = world.chunk[i]
        if not P.is_inside_cube(p, root.position, P.vadds(root.position, chunksize)):
            return None
        bmin, size, offset = P.traverse(p, root)
        kind = root.tree[offset] >> 30
        cell = None
        if kind == TWIG and P.is_inside_cube(p, bmin, P.vadds(bmin, size)):
            leafsize = size / f32(1 << P.TWIG_LEVELS)
            v = P.vdivs(P.vsub(p, bmin), leafsize)
            off = (P.trunc_int(v[0]), P.trunc_int(v[1]), P.trunc_int(v[2]))
            if all(0 <= o <= 3 for o in off):
                cell = P.twig_word(*off)
        return dict(chunk=i, node=offset, kind=kind, bmin=bmin, size=size, cell=cell)

    def settles(self, origin, hit_chunk, hit_node):
        """What the hit block's test finds for the shadow ray of a primary hit in brick (hit_chunk, hit_node):
        -> (origin located in the hit brick, in an empty cell of it, and the brick is flagged)."""
        at = self.locate(origin)
        if at is None or at["kind"] != TWIG or at["cell"] is None or (at["chunk"], at["node"]) != (hit_chunk, hit_node):
            return False, False, False
        ch = self.chunks[hit_chunk]
        empty = ch.twig[ch.tree[hit_node] & 0x3FFFFFFF][at["cell"]] == 0
        return True, bool(empty), bool(empty) and self.brick_flag(hit_chunk, hit_node, at["bmin"], at["size"])


def model_of(oracle_world, dims, chunksize, light_dir, chunkcoordmin=(0, 0, 0), faults=(), eps=P.EPS):
    """BrickClearanceModel over an oracle_binding.OracleWorld."""
    n = dims[0] * dims[1] * dims[2]
    return BrickClearanceModel([oracle_world.chunk(i) for i in range(n)], dims, chunksize, light_dir, chunkcoordmin, eps=eps, faults=faults)
