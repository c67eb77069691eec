"""clearance_model.py — float64 model of the "clear way to the light" predicate — TEST INFRASTRUCTURE.

A shadow ray carries one bit into its record: whether some later sample lands in an occupied cell.  An EMPTY reference
node C is CLEAR for a light when no sample that the reference's march (src/Traverse.cpp) can take after one located in C can
be located in a LEAF or TWIG node; a shadow ray that has located a clear cell is lit whatever it does afterwards.  The
model decides that per EMPTY node with two sweeps over the oracle's chunks:

    R1  C's own chunk, the samples of the treemarch invocation that located C:
        the exact octant of C (per axis: q >= lo(C) where s > 0, q < hi(C) where s < 0, lo <= q < hi where s == 0)
        intersected with the prism  C + {lambda s, lambda >= 0}  grown by D1 = 4 u;
    R2  every chunk, the samples of all later invocations:
        octant and prism both grown by D2 = (8 / S_MIN + 6 + 4 (gw + gh + gd + 2)) u, boxes closed, minus the part of C's
        own chunk that lies deeper than D2 inside it (a later invocation re-enters that chunk only at the face it left by).

u is the float32 spacing at the largest |coordinate| of a world corner.  The rule has premises (ClearanceModel.enabled):
every component of the shadow direction is 0 or at least S_MIN in magnitude, and eps >= 2 u and a power of two.  A brick
counts as occupied whatever its cells hold.  DESIGN §6t has the derivation; `faults` plants the mistakes that
tests/test_light_clearance_cpu.py must catch.

march_lit() re-marches one ray with the reference's arithmetic (the functions of oracle/svo_oracle_py.py, float32 scalars)
and reports, beside the oracle's step counters, the step at which the ray first located a clear cell.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import svo_oracle_py as P  # noqa: E402

f32 = np.float32
EMPTY, LEAF, BRANCH, TWIG = 0, 1, 2, 3
S_MIN = 1.0 / 64.0
FAULTS = ("no_delta", "wrong_way", "brick_empty", "no_neighbour")


def shadow_dir(light_dir):
    """A.sdir of the kernel = the oracle's normalize(-light_dir), float32."""
    return P.normalize(P.vec3(-f32(light_dir[0]), -f32(light_dir[1]), -f32(light_dir[2])))


class _Chunk:
    """What svo_oracle_py's traverse / twigmarch read of a chunk, over the arrays of OracleWorld.chunk(i)."""

    def __init__(self, c):
        self.position = P.vec3(*c["position"])
        self.size = f32(c["size"])
        self.depth = int(c["depth"])
        self.tree = np.asarray(c["tree"], np.uint32).tolist()
        self.twig = np.asarray(c["twig"], np.uint16).reshape(-1, 64)
        self.lo = tuple(float(v) for v in self.position)
        self.hi = tuple(v + float(self.size) for v in self.lo)


class ClearanceModel:
    def __init__(self, chunks, dims, chunksize, light_dir, chunkcoordmin=(0, 0, 0), eps=P.EPS, faults=()):
        assert all(f in FAULTS for f in faults), faults
        self.faults = frozenset(faults)
        self.chunks = [_Chunk(c) for c in chunks]
        self.dims, self.chunksize, self.ccm = tuple(dims), int(chunksize), tuple(chunkcoordmin)
        self.world = P.World(self.chunks, dims[0], dims[1], dims[2], chunksize, chunkcoordmin)
        self.sdir = shadow_dir(light_dir)
        self.s = tuple(float(v) for v in self.sdir)
        self.eps = f32(eps)
        corners = [abs(float((self.ccm[a] + k * dims[a]) * chunksize)) for a in range(3) for k in (0, 1)]
        self.u = float(np.spacing(f32(max(max(corners), 1.0))))
        self.d1 = 4.0 * self.u
        self.d2 = (8.0 / S_MIN + 6.0 + 4.0 * (sum(dims) + 2)) * self.u
        if "no_delta" in self.faults:
            self.d1 = self.d2 = 0.0
        if "wrong_way" in self.faults:
            self.d1, self.d2 = -self.d1, -self.d2
        m, e = math.frexp(float(self.eps))
        self.enabled = (all(v == 0.0 or abs(v) >= S_MIN for v in self.s) and all(math.isfinite(v) for v in self.s)
                        and m == 0.5 and float(self.eps) >= 2.0 * self.u)
        self._memo = {}

    # ------------------------------------------------------------------ the region tests (float64, boxes as lo / hi tuples)
    def _prism(self, blo, bhi, clo, chi, d):
        """Does the closed box [blo, bhi] meet C + {lambda s, lambda >= 0} grown by d?  One slab test of the ray {lambda s}
        against [blo - chi - d, bhi - clo + d]; the quotients' rounding (1e-16 relative) is covered by `slack`."""
        l0, l1, slack = 0.0, math.inf, 1e-9
        for a in range(3):
            lo, hi, s = blo[a] - chi[a] - d, bhi[a] - clo[a] + d, self.s[a]
            if s == 0.0:
                if lo > 0.0 or hi < 0.0:
                    return False
            else:
                t0, t1 = lo / s, hi / s
                if t0 > t1:
                    t0, t1 = t1, t0
                l0, l1 = max(l0, t0 - slack), min(l1, t1 + slack)
        return l0 <= l1

    def _octant_exact(self, blo, bhi, clo, chi):
        """Is some point that traverse() locates in node B inside C's octant?  Cells are half open, so every test is strict."""
        for a in range(3):
            s = self.s[a]
            if s >= 0.0 and not bhi[a] > clo[a]:
                return False
            if s <= 0.0 and not blo[a] < chi[a]:
                return False
        return True

    def _octant_grown(self, blo, bhi, clo, chi, d):
        for a in range(3):
            s = self.s[a]
            g = 0.0 if s == 0.0 else d                    # a zero component never moves the sample: no drift on that axis
            if s >= 0.0 and not bhi[a] >= clo[a] - g:
                return False
            if s <= 0.0 and not blo[a] <= chi[a] + g:
                return False
        return True

    def _occupied(self, ch, meets):
        """Stack walk: does a LEAF or TWIG node of chunk `ch` satisfy meets(lo, hi)?"""
        tree = ch.tree
        stack = [(0, ch.lo, float(ch.size))]
        while stack:
            off, lo, sz = stack.pop()
            hi = (lo[0] + sz, lo[1] + sz, lo[2] + sz)
            if not meets(lo, hi):
                continue
            w = tree[off]
            kind = w >> 30
            if kind == EMPTY:
                continue
            if kind == TWIG and "brick_empty" in self.faults and not ch.twig[w & 0x3FFFFFFF].all():
                continue
            if kind != BRANCH:
                return True
            h, base = sz * 0.5, w & 0x3FFFFFFF
            for i in range(8):
                stack.append((base + i, (lo[0] + h * (i & 1), lo[1] + h * ((i >> 1) & 1), lo[2] + h * ((i >> 2) & 1)), h))
        return False

    def is_clear(self, ci, offset, lo, size):
        """EMPTY node `offset` of chunk `ci` with box [lo, lo + size): may a shadow ray retire on locating it?"""
        if not self.enabled:
            return False
        key = (ci, offset)
        r = self._memo.get(key)
        if r is None:
            r = self._memo[key] = self._sweep(ci, tuple(float(v) for v in lo), float(size))
        return r

    def _sweep(self, ci, clo, size):
        chi = (clo[0] + size, clo[1] + size, clo[2] + size)
        home = self.chunks[ci]
        d1, d2 = self.d1, self.d2
        if self._occupied(home, lambda lo, hi: self._octant_exact(lo, hi, clo, chi) and self._prism(lo, hi, clo, chi, d1)):
            return False
        inner_lo = tuple(v + d2 for v in home.lo)
        inner_hi = tuple(v - d2 for v in home.hi)

        def r2(lo, hi, own):
            if own and all(lo[a] >= inner_lo[a] and hi[a] <= inner_hi[a] for a in range(3)):
                return False
            return self._octant_grown(lo, hi, clo, chi, d2) and self._prism(lo, hi, clo, chi, d2)

        for cj, ch in enumerate(self.chunks):
            if cj != ci and "no_neighbour" in self.faults:
                continue
            if self._occupied(ch, lambda lo, hi, own=(cj == ci): r2(lo, hi, own)):
                return False
        return True

    def empty_nodes(self, ci):
        """(offset, lo, size) of every EMPTY node of chunk ci that traverse() can reach."""
        ch = self.chunks[ci]
        out, stack = [], [(0, ch.lo, float(ch.size))]
        while stack:
            off, lo, sz = stack.pop()
            w = ch.tree[off]
            kind = w >> 30
            if kind == EMPTY:
                out.append((off, lo, sz))
            elif kind == BRANCH:
                h, base = sz * 0.5, w & 0x3FFFFFFF
                for i in range(8):
                    stack.append((base + i, (lo[0] + h * (i & 1), lo[1] + h * ((i >> 1) & 1), lo[2] + h * ((i >> 2) & 1)), h))
        return out

    # ------------------------------------------------------------------ the reference's march, with a look at every tree step
    def march_lit(self, origin, caps=(1000, 1000, 1000)):
        """chunkmarch (src/Traverse.cpp:127-171) of the shadow ray from `origin`, step for step as oracle/svo_oracle_py.py.
        -> dict(hit, tree_steps, brick_cells, chunk_descs, first_clear): first_clear is the 1-based count of steps (tree
        steps + brick cells) taken when the ray first located a clear cell, or None."""
        world, eps, beta = self.world, self.eps, self.sdir
        alpha = P.vec3(*origin)
        cnt = P.Counters()
        res = dict(hit=False, first_clear=None, first_clear_chunk_descs=None)
        chunksize = f32(world.chunksize)
        ccm = world.chunkcoordmin
        chunkmin = P.vec3(ccm[0] * world.chunksize, ccm[1] * world.chunksize, ccm[2] * world.chunksize)
        chunkmax = P.vmuls(P.vec3(ccm[0] + world.width, ccm[1] + world.height, ccm[2] + world.depth), chunksize)

        def finish():
            res.update(tree_steps=cnt.tree_steps, brick_cells=cnt.brick_cells, chunk_descs=cnt.chunk_descs)
            return res

        t = f32(0.0)
        if not P.is_inside_cube(alpha, chunkmin, chunkmax):
            tnear, intersect = P.intersect_cube(alpha, beta, chunkmin, chunkmax)
            t = tnear + eps
            if not intersect:
                return finish()
        for _ in range(caps[0]):
            p = P.vadd(alpha, P.vmuls(beta, t))
            if not P.is_inside_cube(p, chunkmin, chunkmax):
                return finish()
            q = world.index_float(p)
            i = world.index(q[0], q[1], q[2])
            cnt.chunk_descs += 1
            root = world.chunk[i]
            cmin = root.position
            cmax = P.vadds(cmin, chunksize)
            if not P.is_inside_cube(p, cmin, cmax):
                return finish()
            # treemarch (src/Traverse.cpp:74-113)
            a, tt = p, f32(0.0)
            for _ in range(caps[1]):
                pp = P.vadd(a, P.vmuls(beta, tt))
                if not P.is_inside_cube(pp, cmin, cmax):
                    break
                cnt.tree_steps += 1
                bmin, size, offset = P.traverse(pp, root, cnt)
                word = root.tree[offset]
                kind = word >> 30
                if kind == EMPTY:
                    if res["first_clear"] is None and self.is_clear(i, offset, bmin, size):
                        res["first_clear"] = cnt.tree_steps + cnt.brick_cells
                        res["first_clear_chunk_descs"] = cnt.chunk_descs
                elif kind == LEAF:
                    res["hit"] = True
                    return finish()
                else:
                    leafsize = size / f32(1 << P.TWIG_LEVELS)
                    hit = P.twigmarch(pp, beta, bmin, size, leafsize, root.twig[word & 0x3FFFFFFF], eps, caps[2], cnt)[0]
                    if hit:
                        res["hit"] = True
                        return finish()
                tt = tt + (P.cube_escape_distance(pp, beta, bmin, P.vadds(bmin, size)) + eps)
            t = t + (P.cube_escape_distance(p, beta, cmin, cmax) + eps)
        return finish()


def model_of(oracle_world, dims, chunksize, light_dir, chunkcoordmin=(0, 0, 0), faults=(), eps=P.EPS):
    """ClearanceModel over an oracle_binding.OracleWorld."""
    n = dims[0] * dims[1] * dims[2]
    return ClearanceModel([oracle_world.chunk(i) for i in range(n)], dims, chunksize, light_dir, chunkcoordmin, eps=eps, faults=faults)


def shadow_origins(cam_rays, records, eps=P.EPS):
    """The hit block's shadow origin of every primary hit: alpha + beta * (t - eps), float32 (oracle trace_one)."""
    out = []
    for (alpha, beta), rec in zip(cam_rays, records):
        out.append(P.vadd(alpha, P.vmuls(beta, f32(rec["t"]) - f32(eps))))
    return out
