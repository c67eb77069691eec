"""Host model of svo_hit_ao and svo_shade_ao (include/svo.h): steps 1-7 of the rule in numpy float32, one numpy operation per float
operation of the rule, vectorised over the pixels, with the occupancy of the neighbour cells as a plug-in `occupancy(points) -> bool[n]`.
The default occupancy is locate_model.locate_one on the Python twin of the reference's CPU path; rays come from
hit_voxels_model.camera_dirs, boxes from hit_voxels_model.hit_voxels.  Test infrastructure: the yardstick the kernels are held against;
also the scenes of the GPU tests, so that the CPU tests can check them for occlusion of every kind."""
import numpy as np

import hit_voxels_model as H
import locate_model as L

F = np.float32
# (a, b) of neighbour j, and per corner (sa, sb) the neighbours s1 = occ(sa, 0), s2 = occ(0, sb), cn = occ(sa, sb)
NEIGHBOURS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))
CORNERS = {(-1, -1): (3, 1, 0), (1, -1): (4, 1, 2), (-1, 1): (3, 6, 5), (1, 1): (4, 6, 7)}
IMAGE = (64, 48)


class TwinOccupancy:
    """occupancy(points) from locate_model.locate_one; `chunks` keeps the chunk of each point of the last call (-1: no record)."""

    def __init__(self, twin, semantics=0, see_through=0):
        self.twin, self.semantics, self.see_through, self.box = twin, semantics, see_through, L.world_box(twin)
        self.chunks = np.zeros(0, np.int64)

    def __call__(self, points):
        solid = np.zeros(points.shape[0], bool)
        self.chunks = np.full(points.shape[0], -1, np.int64)
        for i, p in enumerate(points):
            r = L.locate_one(self.twin, p, self.semantics, self.see_through, self.box)
            if r is not None:
                solid[i], self.chunks[i] = (r[3] & L.SOLID) != 0, r[4]
        return solid


def resolved_eps(eps=0.0, semantics=0):
    return F(eps) if eps != 0.0 else F(1.0 / 4096.0) if semantics == 1 else F(1.0 / 8192.0)


def neighbour_points(chunks, chunksize, cam, rect, records, voxels, eps, cell=0.0):
    """Steps 1-5 up to the points: -> (on, N, fu, fv) - on: bool[n], the pixels that get the rule (the others get 1.0f); N: [m][8][3]
    the neighbour points of the m pixels that are on; fu, fv: [m]."""
    g, vx = np.ascontiguousarray(records).reshape(-1), np.ascontiguousarray(voxels).reshape(-1)
    n = g.shape[0]
    on = ((g["flags"] & H.HIT_FLAG) != 0) & ((g["flags"] & H.ERR_FLAG) == 0) & ((vx["flags"] & H.INSIDE) != 0) & (vx["chunk"] < len(chunks))
    with np.errstate(all="ignore"):
        d = H.camera_dirs(cam, rect)[on]
        o = np.broadcast_to(np.array(cam.eye, F)[None], d.shape)
        P = H.sample_points(o, d, g["t"][on], F(eps))                            # 1.
        lo = vx["bmin"][on]
        hi = (lo + vx["size"][on][:, None]).astype(F)
        face = H.face_normal(P, lo, hi, d)                                      # 2.
        rows = np.arange(P.shape[0])
        k = np.abs(face).argmax(axis=1)
        sgn = face[rows, k]
        if cell > 0.0:                                                          # 3.
            e = np.full(P.shape[0], F(cell), F)
        else:
            depth = np.array([c["depth"] for c in chunks], np.int64)[vx["chunk"][on].astype(np.int64)]
            e = np.ldexp(F(chunksize), -depth).astype(F)
        u, v = np.where(k == 0, 1, 0), np.where(k == 2, 1, 2)                   # 4.
        ru, rv = P[rows, u] / e, P[rows, v] / e
        gu, gv = np.floor(ru), np.floor(rv)
        fu, fv = ru - gu, rv - gv
        Q = np.zeros_like(P)
        Q[rows, u] = (gu + F(0.5)) * e
        Q[rows, v] = (gv + F(0.5)) * e
        Q[rows, k] = np.where(sgn > 0, hi[rows, k], lo[rows, k]) + sgn * (e * F(0.5))
        finite = np.isfinite(ru) & np.isfinite(rv)
        N = np.repeat(Q[:, None, :], 8, axis=1)                                 # 5.
        for j, (a, b) in enumerate(NEIGHBOURS):
            N[rows, j, u] = Q[rows, u] + F(a) * e
            N[rows, j, v] = Q[rows, v] + F(b) * e
    idx = np.nonzero(on)[0]
    on = np.zeros(n, bool)
    on[idx[finite]] = True
    assert N.dtype == F and fu.dtype == F
    return on, N[finite], fu[finite], fv[finite]


def corner_levels(occ):
    """Step 6: occ bool[m][8] -> {(sa, sb): level int[m]}."""
    out = {}
    for c, (s1, s2, cn) in CORNERS.items():
        a, b, d = occ[:, s1].astype(np.int64), occ[:, s2].astype(np.int64), occ[:, cn].astype(np.int64)
        out[c] = np.where((a & b) != 0, 0, 3 - (a + b + d))
    return out


def fold(occ, fu, fv):
    """Steps 6 and 7: occ bool[m][8] -> ao float32[m]."""
    A = {c: lv.astype(F) / F(3) for c, lv in corner_levels(occ).items()}
    l0 = A[(-1, -1)] + (A[(1, -1)] - A[(-1, -1)]) * fu
    l1 = A[(-1, 1)] + (A[(1, 1)] - A[(-1, 1)]) * fu
    out = l0 + (l1 - l0) * fv
    assert out.dtype == F
    return out


def hit_ao(chunks, chunksize, cam, rect, records, voxels, occupancy, eps=0.0, semantics=0, cell=0.0, detail=None):
    """float32[n]: what svo_hit_ao writes.  `detail`, a dict, receives on, N, occ, fu, fv."""
    on, N, fu, fv = neighbour_points(chunks, chunksize, cam, rect, records, voxels, resolved_eps(eps, semantics), cell)
    occ = np.asarray(occupancy(N.reshape(-1, 3)), bool).reshape(-1, 8)
    out = np.ones(on.shape[0], F)
    out[on] = fold(occ, fu, fv)
    if detail is not None:
        detail.update(on=on, N=N, occ=occ, fu=fu, fv=fv)
    return out


def shade_ao(ao, strength, rgba):
    """What svo_shade_ao leaves of rgba ([n][4] float32)."""
    ao, out = np.asarray(ao, F).reshape(-1), np.array(rgba, F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        f = F(1) - F(strength) * (F(1) - ao)
        write = ~np.isnan(f) & (f != F(1))
        out[write, :3] = (out[write, :3] * f[write, None]).astype(F)
    return out


# ---- the scenes of the GPU tests (tests/test_ao.py) and of the input-condition test (tests/test_ao_cpu.py) ------------------------
# name -> (w, h, d, chunkcoordmin, depth of every chunk in World::index() order); chunk size 128
WORLDS = dict(L.WORLDS)
WORLDS["grid_2x1x2_d8"] = (2, 1, 2, (0, 0, 0), [8] * 4)


def make_chunks(svo, name):
    w, h, d, ccm, depths = WORLDS[name]
    gen = {}
    for depth in sorted(set(depths)):
        W = svo.World.generate(w, h, d, 128, depth, chunkcoordmin=ccm)
        gen[depth] = [W.chunk(i) for i in range(w * h * d)]
        W.destroy()
    return [gen[depth][i] for i, depth in enumerate(depths)]


def camera(svo, name, view="default", image=IMAGE):
    """default: from above and in front of the world's front face (brick cells of the surface); low: level with the terrain (its cut:
    LEAF nodes)."""
    w, h, d, ccm, _ = WORLDS[name] if name in WORLDS else L.HANDMADE + (None,)
    lo, hi = L.box_of(w, h, d, 128, ccm)
    cx, cz = 0.5 * (lo[0] + hi[0]), lo[2] - 40.0
    if name == "handmade":
        return svo.make_camera((cx + 9.0, 190.0, cz - 60.0), (0.05, -0.55, 0.8), (0.0, 1.0, 0.0), 60.0, *image)
    if view == "low":
        return svo.make_camera((cx, 30.0, cz), (0.0, -0.2, 0.98), (0.0, 1.0, 0.0), 60.0, *image)
    return svo.make_camera((cx, 150.0, cz), (0.0, -0.5, 0.866), (0.0, 1.0, 0.0), 60.0, *image)
