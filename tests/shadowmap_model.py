"""Host model of svo_shadowmap_render / svo_shadowmap_apply (include/svo.h): the texel rays and the projection rebuilt in numpy float32
with the header's expressions, the rays marched by the unchanged CPU oracle, depth = where(usable, t, inf).  Every step is specified in
separately rounded float, so the GPU tests compare with this bit for bit.  Test infrastructure of tests/test_shadowmap*.py."""
import numpy as np

import local_shadows_model as LM

HIT, SHADOW_TRACED, SHADOWED, ERR = 1, 2, 4, 1 << 15
F = np.float32
S = float(np.sqrt(0.5))

# the scene of tests/test_local_shadows.py under the default directional light, normalize(1, -1, 0)
LIGHT = dict(direction=(S, -S, 0.0), right=(0.0, 0.0, 1.0), up=(S, S, 0.0), origin=(128.0 - 300.0 * S, 40.0 + 300.0 * S, 128.0))
MAP_A = dict(size=64, half=160.0, bias=8.0)
MAP_B = dict(size=128, half=100.0, bias=4.0)


def make_map(svo, size, half, depth_ptr=None, light=LIGHT):
    """A svo.ShadowMap of size x size texels and half extents `half` for `light`."""
    m = svo.ShadowMap()
    for name in ("origin", "direction", "right", "up"):
        getattr(m, name)[:] = [float(F(c)) for c in light[name]]
    m.half_width = m.half_height = half
    m.width = m.height = size
    m.depth_dev = depth_ptr
    return m


def _vec(a):
    return np.array(list(a), F)


def texel_rays(m):
    """(origins, dirs) of every texel, row-major (row 0 at +up): u, v and o as the header writes them, numpy rounding every float32
    operation on its own."""
    w, h = int(m.width), int(m.height)
    i = (np.arange(w, dtype=F) + F(0.5))
    j = (np.arange(h, dtype=F) + F(0.5))
    u = ((i / F(w)) * F(2.0) - F(1.0)) * F(m.half_width)
    v = (F(1.0) - (j / F(h)) * F(2.0)) * F(m.half_height)
    uu, vv = np.tile(u, h), np.repeat(v, w)
    o = (_vec(m.origin)[None, :] + _vec(m.right)[None, :] * uu[:, None]) + _vec(m.up)[None, :] * vv[:, None]
    d = np.repeat(_vec(m.direction)[None, :], w * h, axis=0)
    assert o.dtype == F and d.dtype == F and u.dtype == F and v.dtype == F
    return o, d


def depth_image(oracle, ow, m, semantics=0, stats=None, **params):
    """The depth image svo_shadowmap_render writes: float32 [height, width], +inf where the texel's ray has no usable hit."""
    o, d = texel_rays(m)
    rec = ow.trace_rays(o, d, params=oracle.make_params(shadow=False, semantics=semantics, **params), threads=8)
    ok = LM.usable(rec)
    if stats is not None:
        stats.update(texels=int(ok.size), hit=float(ok.mean()), runaways=int(np.count_nonzero(rec["flags"] & ERR)))
    return np.where(ok, rec["t"], F(np.inf)).astype(F).reshape(int(m.height), int(m.width))


def project(m, P):
    """(s, fu, fv, inside, i, j) of points P [n, 3]: the header's expressions; i, j are 0 outside the map."""
    with np.errstate(all="ignore"):
        q = (P.astype(F) - _vec(m.origin)[None, :]).astype(F)
        dot = lambda b: ((q[:, 0] * F(b[0]) + q[:, 1] * F(b[1])) + q[:, 2] * F(b[2])).astype(F)
        s, a, b = dot(m.direction), dot(m.right), dot(m.up)
        w, h = F(m.width), F(m.height)
        fu = (((a / F(m.half_width)) + F(1.0)) * F(0.5)) * w
        fv = ((F(1.0) - (b / F(m.half_height))) * F(0.5)) * h
        inside = (fu >= 0) & (fu < w) & (fv >= 0) & (fv < h)
        i = np.where(inside, np.floor(fu), 0).astype(np.int64)
        j = np.where(inside, np.floor(fv), 0).astype(np.int64)
    assert s.dtype == F and fu.dtype == F and fv.dtype == F
    return s, fu, fv, inside, i, j


def lookup(m, depth, P, bias):
    """(occluded, inside) per point: inside && depth[j, i] < s - bias."""
    s, _, _, inside, i, j = project(m, P)
    with np.errstate(all="ignore"):
        occluded = inside & (depth[j, i] < (s - F(bias)).astype(F))
    return occluded, inside


def sample_points(oracle, cam, rect, frame, semantics=0):
    """(usable, P) of a frame's records: P = o + d * (t - eps), where the shadow ray would start."""
    rec = np.asarray(frame).reshape(-1)
    o, d = LM.camera_rays(oracle, cam, rect)
    return LM.usable(rec), LM.sample_points(o, d, rec, LM.resolved_eps(semantics))


def expected(oracle, cam, rect, frame, m, depth, bias, semantics=0, stats=None):
    """The records svo_shadowmap_apply leaves: `frame` (the oracle's svo_trace records of the rectangle) with SHADOW_TRACED set and
    SHADOWED rewritten on every usable hit."""
    want = np.array(frame, copy=True).reshape(-1)
    sel, P = sample_points(oracle, cam, rect, want, semantics)
    occluded, inside = lookup(m, depth, P, bias)
    if stats is not None:
        stats.update(hits=int(sel.sum()), shadowed=float(occluded[sel].mean()), lit=float((~occluded)[sel].mean()), outside=int((sel & ~inside).sum()))
    bits = np.where(occluded, SHADOWED, 0).astype(np.uint16) | np.uint16(SHADOW_TRACED)
    want["flags"] = np.where(sel, (want["flags"] & ~np.uint16(SHADOWED)) | bits, want["flags"])
    return want


# ---- the known answer: a floor slab and a floating plate in one depth-6 chunk (voxels of 2 units) ---------------------------------
KNOWN_DIRECTION = (0.25, -1.0, 0.125)
FLOOR_TOP, PLATE_LO, PLATE_HI, PLATE_Y0, PLATE_Y1 = 8.0, 40.0, 88.0, 60.0, 64.0


def known_grid():
    """[z, y, x] uint16: material 1 in y < 8 (the floor), material 2 in 40 <= x, z < 88, 60 <= y < 64 (the plate)."""
    g = np.zeros((64, 64, 64), np.uint16)
    g[:, :4, :] = 1
    g[20:44, 30:32, 20:44] = 2
    return g


def known_sets(P, sel, material, margin):
    """(under, clear) among the floor hits: the point carried back along the light to the plate's two faces lies inside the plate's
    footprint by more than `margin` at both / outside it by more than `margin` at both (the two are 1.1 units apart: the whole
    segment through the slab is then inside / outside)."""
    d = np.asarray(KNOWN_DIRECTION, np.float64) / np.linalg.norm(KNOWN_DIRECTION)
    P = P.astype(np.float64)
    floor = sel & (material.reshape(-1) == 1) & (np.abs(P[:, 1] - FLOOR_TOP) < 0.01)
    out = []
    for y in (PLATE_Y0, PLATE_Y1):
        lam = (y - P[:, 1]) / -d[1]
        x, z = P[:, 0] - d[0] * lam, P[:, 2] - d[2] * lam
        out.append(np.maximum.reduce([PLATE_LO - x, x - PLATE_HI, PLATE_LO - z, z - PLATE_HI]))     # > 0: outside by that much
    under = floor & (out[0] < -margin) & (out[1] < -margin)
    clear = floor & (out[0] > margin) & (out[1] > margin)
    return under, clear
