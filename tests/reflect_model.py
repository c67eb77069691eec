"""Host model of svo_trace_reflections and svo_shade_reflections (include/svo.h): the mirror ray in numpy float32, one numpy operation
per float operation of the header's steps 1-4, on hit_voxels_model's camera_dirs / sample_points / face_normal; the march of the rays
is the CPU oracle's trace_rays; the Fresnel term and the blend in float32; and a float64 restatement of the shading stage's hit formula
over explicit (origin, direction) arrays, written from include/svo.h and shaders/World.Fragment.glsl:63-138,180-197 as shade_model.py
is (tests/test_reflect_cpu.py holds it to shade_model.terms on the camera's own rays).  Also the scenes of the tests, so that the CPU
tests can check what they see.  Test infrastructure."""
import numpy as np

import hit_voxels_model as H
import sky_model

F = np.float32
HIT_FLAG, ERR_FLAG, INSIDE = H.HIT_FLAG, H.ERR_FLAG, H.INSIDE
SHADOWED, LOCAL_SHADOWS, SHADOWED_POINT, SHADOWED_SPOT = 4, 32, 64, 128
WATER = 6
WORLD = (2, 1, 2, 128, 8)                           # World.generate(w, h, d, chunksize, depth): every generated world has a lake at y = 6
IMAGE = (128, 96)
# name -> (eye, forward) of make_camera(eye, forward, (0, 1, 0), 60, *IMAGE); None: default_camera(2, 2, 128, *IMAGE)
VIEWS = {"lakeN": ((120.3, 20.2, 150.4), (0.1, -0.15, 1.0)),
         "lakeW": ((215.3, 25.2, 60.4), (-1.0, -0.2, 0.1)),
         "default": None}


def camera(svo, name):
    if VIEWS[name] is None:
        return svo.default_camera(2, 2, 128, *IMAGE)
    eye, forward = VIEWS[name]
    return svo.make_camera(eye, forward, (0.0, 1.0, 0.0), 60.0, *IMAGE)


def resolved_eps(semantics=0, eps=0.0):
    """The launch's eps: 0 = 1/8192, or 1/4096 under SVO_SEMANTICS_GLSL."""
    return F(eps) if eps else F(1.0 / 4096.0 if semantics == 1 else 1.0 / 8192.0)


def mirror_pixels(records, voxels, material):
    g, v = np.ascontiguousarray(records).reshape(-1), np.ascontiguousarray(voxels).reshape(-1)
    return (((g["flags"] & HIT_FLAG) != 0) & ((g["flags"] & ERR_FLAG) == 0) & ((material == 0) | (g["material"] == material))
            & ((v["flags"] & INSIDE) != 0))


def mirror_rays(cam, rect, records, voxels, material, eps, origin_on_face=True):
    """-> dict(on [n] bool, O [n][3], R [n][3], axis [n], c [n]): steps 1-4 of include/svo.h for every pixel of the rectangle (rows
    that are not mirror pixels hold whatever the arithmetic gives).  origin_on_face=False leaves out rule 3: O = P."""
    g, v = np.ascontiguousarray(records).reshape(-1), np.ascontiguousarray(voxels).reshape(-1)
    n = g.shape[0]
    eps = F(eps)
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        d = H.camera_dirs(cam, rect)
        o = np.broadcast_to(np.array(list(cam.eye), F), (n, 3))
        P = H.sample_points(o, d, g["t"], eps)                                  # 1.
        lo = v["bmin"].astype(F)
        hi = (lo + v["size"].astype(F)[:, None]).astype(F)
        nrm = H.face_normal(P, lo, hi, d)                                       # 2.
        k = np.argmax(np.abs(nrm), axis=1)
        sgn = nrm[rows, k].astype(F)
        O = P.copy()
        if origin_on_face:
            O[rows, k] = (np.where(sgn > 0, hi[rows, k], lo[rows, k]) + sgn * eps).astype(F)        # 3.
        c = np.abs(d[rows, k]).astype(F)
        R = d.copy()
        R[rows, k] = (sgn * c).astype(F)                                        # 4.
    return dict(on=mirror_pixels(g, v, material), O=O, R=R, axis=k, c=c)


def reflect_records(oracle, ow, cam, rect, records, voxels, material, shadow=False, semantics=0, origin_on_face=True, **params):
    """-> (rays, want): mirror_rays and the HIT_DTYPE [n] records svo_trace_reflections writes: the oracle's for the mirror rays, all
    zero elsewhere."""
    rays = mirror_rays(cam, rect, records, voxels, material, resolved_eps(semantics, params.get("eps", 0.0)), origin_on_face)
    on = rays["on"]
    want = np.zeros(on.shape[0], H.HIT_DTYPE)
    if on.any():
        want[on] = ow.trace_rays(rays["O"][on], rays["R"][on], params=oracle.make_params(shadow=shadow, semantics=semantics, **params), threads=8)
    return rays, want


def fresnel(c, f0, schlick):
    """F per pixel in float32: f0, or Schlick's f0 + (1 - f0) * (((x*x) * (x*x)) * x) with x = 1 - c."""
    c, f0 = np.asarray(c, F), F(f0)
    if not schlick:
        return np.full(c.shape, f0, F)
    x = F(1) - c
    return (f0 + (F(1) - f0) * (((x * x) * (x * x)) * x)).astype(F)


def blend(rgba, on, Fr, C):
    """The image svo_shade_reflections leaves, float32 [n][4]: rgb * (1 - F) + C * F on mirror pixels whose F != 0, per channel."""
    out = np.array(rgba, F, copy=True).reshape(-1, 4)
    w = on & (Fr != 0)
    keep = (F(1) - Fr)[:, None]
    with np.errstate(all="ignore"):
        mixed = (out[:, :3] * keep + np.asarray(C, F) * Fr[:, None]).astype(F)
    out[w, :3] = mixed[w]
    return out


# ---- the hit formula in float64 over explicit rays ------------------------------------------------------------------------------------
def _v(x):
    return np.array(list(x), np.float64)


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _unit(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        return a / np.sqrt(_dot(a, a))[..., None]


def _max0(x):
    return np.where(x < 0.0, 0.0, x)


def _pow(x, y):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.exp2(y * np.log2(np.where(x > 0.0, x, 1.0)))
    r = np.where(x > 0.0, r, np.where(np.isnan(x), np.nan, 0.0))
    return np.where(y == 0.0, 1.0, r)


def shade_rays(P, origins, dirs, records):
    """-> (rgb [n][3], cond [n]) of svo_shade's hit formula for every record, seen from origins[k] along dirs[k]: the point is
    origin + dir * (t - eps), the view vector -dir (dirs are unit vectors; for t > eps that is normalize(origin - point)).  cond as
    shade_model's: shininess * the sum over the lights of the largest |specular term|."""
    g = np.asarray(records).reshape(-1)
    eye, beta = np.asarray(origins, np.float64), np.asarray(dirs, np.float64)
    eps = float(P.eps) or 1.0 / 8192.0
    gam = float(P.gamma) or float(F(2.2))
    t = g["t"].astype(np.float64)
    p = eye + beta * (t - eps)[:, None]
    nrm = g["normal"].astype(np.float64)
    flags = g["flags"].astype(np.int64)
    mat = g["material"].astype(np.int64)
    mi = np.where(mat < 8, mat, 0)
    shin = np.array([float(m.shininess) for m in P.materials])[mi]
    with np.errstate(invalid="ignore"):
        diffuse = np.array([list(m.diffuse) for m in P.materials], np.float64)[mi] ** gam
        specular = np.array([list(m.specular) for m in P.materials], np.float64)[mi] ** gam
    lit_dir = np.where(flags & SHADOWED, 0.0, 1.0)
    local = (flags & LOCAL_SHADOWS) != 0
    lit_point = np.where(local, np.where(flags & SHADOWED_POINT, 0.0, 1.0), lit_dir)
    lit_spot = np.where(local, np.where(flags & SHADOWED_SPOT, 0.0, 1.0), lit_dir)
    vdir = -beta

    def light(L, l, lit):
        hv = _unit(l + vdir)
        d = _max0(_dot(nrm, l))
        s = _pow(_max0(_dot(vdir, hv)), shin)
        return (_v(L.ambient) * diffuse, _v(L.diffuse) * d[:, None] * diffuse * lit[:, None],
                _v(L.specular) * s[:, None] * specular * lit[:, None])

    def att(L, dist):
        return 1.0 / (float(L.constant) + float(L.linear) * dist + float(L.quadratic) * dist * dist)

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        lv = _v(P.point.position) - p                                           # computePointLight_BlinnPhong, :80-97
        amb, dif, spe = light(P.point, _unit(lv), lit_point)
        a = att(P.point, np.sqrt(_dot(lv, lv)))[:, None]
        color, spec_point = (amb + dif + spe) * a, spe * a
        l = np.broadcast_to(_unit(-_v(P.directional.direction)), p.shape)       # computeDirectionalLight_BlinnPhong, :99-114
        amb, dif, spe = light(P.directional, l, lit_dir)
        color, spec_dir = color + (amb + dif + spe), spe
        lv = _v(P.spot.position) - p                                            # computeSpotlight_BlinnPhong, :116-138
        l = _unit(lv)
        amb, dif, spe = light(P.spot, l, lit_spot)
        a = att(P.spot, np.sqrt(_dot(lv, lv)))[:, None]
        theta = _dot(l, _unit(-_v(P.spot.direction)))
        inten = np.clip((theta - float(P.spot.cos_gamma)) / (float(P.spot.cos_phi) - float(P.spot.cos_gamma)), 0.0, 1.0)[:, None]
        color, spec_spot = color + (amb + (dif + spe) * inten) * a, spe * inten * a
        cond = shin * sum(np.nan_to_num(np.abs(s).max(axis=1), nan=0.0, posinf=0.0) for s in (spec_point, spec_dir, spec_spot))
    return color, cond


def shade_reflections(P, mirror_f0, schlick, background, rays, reflect, rgba, faces=None, sky_filter=0):
    """-> (rgba [n][4] float64, cond [n], F [n]): the image svo_shade_reflections leaves over `rgba` (a shade call's, float32) - the
    reflected colour by shade_rays in float64 from `reflect`, the sky (sky_model.lookup along R) or the background; F in float32.
    cond is shade_rays' scaled by F, 0 where nothing is shaded."""
    r = np.asarray(reflect).reshape(-1)
    on = rays["on"]
    Fr = fresnel(rays["c"], mirror_f0, schlick)
    C, cond = shade_rays(P, rays["O"], rays["R"], r)
    hit = (r["flags"] & HIT_FLAG) != 0
    away = np.broadcast_to(np.asarray(background, F).astype(np.float64), C.shape).copy()
    if faces is not None:
        sky, face = sky_model.lookup(rays["R"], faces, sky_filter)
        away[face >= 0] = sky[face >= 0]
    C = np.where(hit[:, None], C, away)
    out = np.asarray(rgba, F).reshape(-1, 4).astype(np.float64)
    w = on & (Fr != 0)
    f = Fr.astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        mixed = out[:, :3] * (1.0 - f) + C * f
    out[w, :3] = mixed[w]
    return out, np.where(w & hit, cond * Fr, 0.0), Fr
