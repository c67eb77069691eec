"""Host model of svo_trace_local_shadows (include/svo.h): the occlusion rays rebuilt in numpy float32 with the header's expressions,
marched by the unchanged CPU oracle, and the `t < dist` rule applied here.  Test infrastructure of tests/test_local_shadows.py."""
import ctypes as C

import numpy as np

HIT, SHADOWED, ERR = 1, 4, 1 << 15
LOCAL_SHADOWS, SHADOWED_POINT, SHADOWED_SPOT = 1 << 5, 1 << 6, 1 << 7
POINT, SPOT = (50.0, 8.0, 65.0), (50.0, 20.0, 70.0)         # the reference's lights (src/Main.cpp:101-131, svo_shade_defaults)
F = np.float32


def camera_rays(oracle, cam, rect=None):
    """orc_camera_ray of every pixel of the rectangle, row-major: (origins, dirs), float32 [n, 3]."""
    ocam = oracle.camera_from(cam)
    x0, y0, w, h = rect if rect is not None else (0, 0, cam.width, cam.height)
    o = np.zeros((h * w, 3), F)
    d = np.zeros((h * w, 3), F)
    vo, vd = oracle.Vec3(), oracle.Vec3()
    for k in range(h * w):
        oracle.lib.orc_camera_ray(C.byref(ocam), x0 + k % w, y0 + k // w, C.byref(vo), C.byref(vd))
        o[k] = (vo.x, vo.y, vo.z)
        d[k] = (vd.x, vd.y, vd.z)
    return o, d


def resolved_eps(semantics, eps=0.0):
    return F(eps) if eps else F(1.0 / 4096.0 if semantics == 1 else 1.0 / 8192.0)


def usable(records):
    f = records["flags"].reshape(-1)
    return ((f & HIT) != 0) & ((f & ERR) == 0)


def sample_points(o, d, records, eps):
    """P = o + d * (t - eps): numpy rounds every float32 operation on its own."""
    t = records["t"].reshape(-1).astype(F)
    return (o + d * (t - F(eps))[:, None]).astype(F)


def light_rays(P, light):
    """(valid, dirs, dist): v = L - P, q summed left to right, v * (1 / sqrt(q)), sqrt(q); valid where q is finite and not 0."""
    with np.errstate(all="ignore"):
        v = (np.asarray(light, F)[None, :] - P).astype(F)
        q = ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(F)
        dist = np.sqrt(q).astype(F)
        dirs = (v * (F(1.0) / dist)[:, None]).astype(F)
    assert v.dtype == F and q.dtype == F and dist.dtype == F and dirs.dtype == F
    return np.isfinite(q) & (q != 0), dirs, dist


def occlusion(oracle, ow, P, light, sel, semantics):
    """Per pixel: (occluded, hit terrain at t >= dist, relative distance of t from dist) of the ray towards `light`; False / inf
    outside `sel` (the usable hits) and where the light has no ray."""
    valid, dirs, dist = light_rays(P, light)
    go = sel & valid
    rec = ow.trace_rays(P[go], dirs[go], params=oracle.make_params(shadow=False, semantics=semantics), threads=8)
    hit = usable(rec)
    occ = np.zeros(P.shape[0], bool)
    behind = np.zeros(P.shape[0], bool)
    near = np.full(P.shape[0], np.inf)
    occ[go] = hit & (rec["t"] < dist[go])
    behind[go] = hit & ~(rec["t"] < dist[go])
    near[go] = np.where(hit, np.abs(rec["t"].astype(np.float64) - dist[go]) / dist[go], np.inf)
    runaway = int(np.count_nonzero(rec["flags"] & ERR))
    return occ, behind, near, runaway


def expected(oracle, ow, cam, rect, frame, point, spot, semantics, stats=None):
    """The records svo_trace_local_shadows leaves: `frame` (the oracle's svo_trace records of the rectangle) with the three bits ORed in."""
    want = np.array(frame, copy=True).reshape(-1)
    o, d = camera_rays(oracle, cam, rect)
    sel = usable(want)
    P = sample_points(o, d, want, resolved_eps(semantics))
    shadowed = (want["flags"] & SHADOWED) != 0
    bits = np.zeros(want.shape[0], np.uint16)
    for name, light, bit in (("point", point, SHADOWED_POINT), ("spot", spot, SHADOWED_SPOT)):
        if light is None:
            on = shadowed
        else:
            on, behind, near, runaway = occlusion(oracle, ow, P, light, sel, semantics)
            if stats is not None:
                stats[name] = dict(hits=int(sel.sum()), occluded=float(on[sel].mean()), lit=float((~on)[sel].mean()), behind=int(behind.sum()),
                                   differs=float((on != shadowed)[sel].mean()), nearest=float(near.min()), runaways=runaway)
        bits |= np.where(on, bit, 0).astype(np.uint16)
    want["flags"] = np.where(sel, (want["flags"] & ~np.uint16(SHADOWED_POINT | SHADOWED_SPOT)) | np.uint16(LOCAL_SHADOWS) | bits, want["flags"])
    return want
