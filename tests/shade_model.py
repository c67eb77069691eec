"""Float64 model of the shading stage and of the packed G-buffer, written from include/svo.h and
shaders/World.Fragment.glsl:63-138,180-197 (not from csrc/shade.hip): plain numpy, vectorised over records, every
operation in double precision on the float32 inputs.  Also the synthetic G-buffers of tests/test_shade_model_cpu.py and
tests/test_shading_synthetic.py, and the tolerance both files judge with.

    shade(cam, params, rect, gbuffer)                                   -> rgba[n, 4], cond[n]
    shade_translucent(cam, params, absorption, rect, surface, behind)   -> rgba[n, 4], cond[n]
    pack(records) -> uint64[n]          unpack(words) -> records[n]     (integer-exact)

cond is the conditioning of the specular power: sum over the lights of shininess * max_c |that light's specular term after
attenuation and spot intensity|.  x^y turns a relative rounding r of x into y * r of the result, which no fixed relative
tolerance covers at a shininess of 10000; `within` adds K * 2^-23 * cond for it.
"""
import ctypes as C
import math

import numpy as np

HIT, SHADOWED, FACE_NORMAL, SEE_THROUGH = 1, 4, 8, 16
LOCAL_SHADOWS, SHADOWED_POINT, SHADOWED_SPOT, ERR = 32, 64, 128, 1 << 15
HIT_DTYPE = np.dtype([("t", "<f4"), ("normal", "<f4", (3,)), ("material", "<u2"), ("flags", "<u2"),
                      ("chunk", "<u4"), ("node", "<u4"), ("cell", "<u4")])
ATOL, RTOL = 1e-6, 2e-5             # the project's figures for the shading stage (tests/test_shading.py)
INV_SQRT2, INV_SQRT3 = 0x3F3504F3, 0x3F13CD3A       # the march kernels' normalize(ivec3) constants (include/svo.h)
# K_ORACLE: the smallest K with which the C oracle - float32, correctly rounded divisions and square roots, glibc's powf - passes
# `within` against this model on every case of all_cases (measured by tests/test_shade_model_cpu.py, which fails if it grows).
# The kernel replaces three correctly rounded normalisations on the way to the power's base (beta, l, hv) by 1-ulp ones and powf by
# 1-ulp log2 / exp2: four more roundings of that size, hence K = 4 K_ORACLE, rounded up.  Never tuned to the kernel.
K_ORACLE = 1.76
K_GPU = math.ceil(4.0 * K_ORACLE)


def _v(x):
    return np.array(list(x), np.float64)


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _unit(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        return a / np.sqrt(_dot(a, a))[..., None]


def _max0(x):
    return np.where(x < 0.0, 0.0, x)                # max(x, 0.0) that keeps a NaN, as the oracle's and the kernel's do


def within(got, want, cond, K):
    """|got - want| / (ATOL + RTOL |want| + K 2^-23 cond) per component; NaN where want is NaN (checked separately)."""
    want = np.asarray(want, np.float64)
    tol = ATOL + RTOL * np.abs(want) + K * 2.0 ** -23 * np.asarray(cond, np.float64)[:, None] * np.array([1.0, 1.0, 1.0, 0.0])
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(got, np.float64) - want) / tol


def needed_K(got, want, cond):
    """The smallest K with which `got` passes `within` against the model (0 if the fixed terms suffice)."""
    want = np.asarray(want, np.float64)[:, :3]
    excess = np.abs(np.asarray(got, np.float64)[:, :3] - want) - (ATOL + RTOL * np.abs(want))
    c = np.asarray(cond, np.float64)[:, None]
    ok = np.isfinite(excess) & (excess > 0.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        k = np.where(ok, excess / (2.0 ** -23 * c), 0.0)
    return float(k.max()) if k.size else 0.0


class ShadeModel:
    """The stage as svo.h and the fragment shader state it.  The methods below are the places where the CPU tests plant their
    mutations (tests/test_shade_model_cpu.py); the model itself never overrides them."""

    def material_index(self, material):
        return np.where(material < 8, material, 0)                      # ML[8]; svo.h folds everything else to entry 0

    def shininess(self, table, mi):
        return table[mi]

    def gamma(self, g):
        return g

    def sample_distance(self, t, eps):
        return t - eps                                                  # point = alpha + beta * (sigma - EPS), :174

    def depth_distance(self, p, eye, t, eps):
        return np.sqrt(_dot(p - eye, p - eye))                          # distance(point, eye), :193

    def lit(self, flags):
        """(point, directional, spot) factors 1.0 - shadow: SVO_SHADOWED for all three (:186-190), unless the record carries
        SVO_LOCAL_SHADOWS - then the point light and the spotlight have their own bit (include/svo.h)."""
        d = np.where(flags & SHADOWED, 0.0, 1.0)
        local = (flags & LOCAL_SHADOWS) != 0
        return (np.where(local, np.where(flags & SHADOWED_POINT, 0.0, 1.0), d), d,
                np.where(local, np.where(flags & SHADOWED_SPOT, 0.0, 1.0), d))

    def spot_intensity(self, x):
        return np.clip(x, 0.0, 1.0)

    def log2(self, x):
        return np.log2(x)

    def power(self, x, y):
        """pow(x, y) for x >= 0: pow(x, 0) = 1 also for x = 0, pow(0, y > 0) = 0."""
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.exp2(y * self.log2(np.where(x > 0.0, x, 1.0)))
        r = np.where(x > 0.0, r, np.where(np.isnan(x), np.nan, 0.0))
        return np.where(y == 0.0, 1.0, r)

    # ---- the stage ----
    def terms(self, cam, P, rect, g, t=None):
        """Every intermediate of the hit formula for all records of `g` (hit or not), as a dict; t overrides g['t']."""
        x0, y0, w, h = rect
        g = np.asarray(g).reshape(-1)
        n = g.shape[0]
        assert n == w * h
        eps = float(P.eps) or 1.0 / 8192.0
        gam = self.gamma(float(P.gamma) or float(np.float32(2.2)))
        near, far = float(P.near_plane) or 0.125, float(P.far_plane) or 8192.0
        k = np.arange(n)
        px, py = x0 + k % max(w, 1), y0 + k // max(w, 1)
        u = ((px + 0.5) / cam.width * 2.0 - 1.0) * float(cam.tan_half_x)
        v = (1.0 - (py + 0.5) / cam.height * 2.0) * float(cam.tan_half_y)
        eye = _v(cam.eye)
        beta = _unit(_v(cam.forward) + _v(cam.right) * u[:, None] + _v(cam.up) * v[:, None])
        t = g["t"].astype(np.float64) if t is None else np.asarray(t, np.float64)
        p = eye + beta * self.sample_distance(t, eps)[:, None]
        nrm = g["normal"].astype(np.float64)
        flags = g["flags"].astype(np.int64)
        mi = self.material_index(g["material"].astype(np.int64))
        shin = self.shininess(np.array([float(m.shininess) for m in P.materials]), mi)
        with np.errstate(invalid="ignore"):
            diffuse = np.array([list(m.diffuse) for m in P.materials], np.float64)[mi] ** gam
            specular = np.array([list(m.specular) for m in P.materials], np.float64)[mi] ** gam
        lit_point, lit_dir, lit_spot = self.lit(flags)
        vdir = _unit(eye - p)
        out = dict(beta=beta, p=p, shininess=shin, vdir=vdir)

        def blinn_phong(light, l, lit):
            hv = _unit(l + vdir)
            d = _max0(_dot(nrm, l))
            x = _max0(_dot(vdir, hv))
            s = self.power(x, shin)
            amb = _v(light.ambient) * diffuse
            dif = _v(light.diffuse) * d[:, None] * diffuse * lit[:, None]
            spe = _v(light.specular) * s[:, None] * specular * lit[:, None]
            return amb, dif, spe, x

        def att(light, dist):
            return 1.0 / (float(light.constant) + float(light.linear) * dist + float(light.quadratic) * dist * dist)

        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            # computePointLight_BlinnPhong, :80-97
            lv = _v(P.point.position) - p
            amb, dif, spe, x = blinn_phong(P.point, _unit(lv), lit_point)
            a = att(P.point, np.sqrt(_dot(lv, lv)))[:, None]
            color = (amb + dif + spe) * a
            out["x_point"], out["spec_point"] = x, spe * a
            # computeDirectionalLight_BlinnPhong, :99-114
            l = np.broadcast_to(_unit(-_v(P.directional.direction)), p.shape)
            amb, dif, spe, x = blinn_phong(P.directional, l, lit_dir)
            color = color + (amb + dif + spe)
            out["x_directional"], out["spec_directional"] = x, spe
            # computeSpotlight_BlinnPhong, :116-138
            lv = _v(P.spot.position) - p
            l = _unit(lv)
            amb, dif, spe, x = blinn_phong(P.spot, l, lit_spot)
            a = att(P.spot, np.sqrt(_dot(lv, lv)))[:, None]
            theta = _dot(l, _unit(-_v(P.spot.direction)))
            inten = self.spot_intensity((theta - float(P.spot.cos_gamma)) / (float(P.spot.cos_phi) - float(P.spot.cos_gamma)))[:, None]
            color = color + (amb + (dif + spe) * inten) * a
            out["x_spot"], out["spec_spot"], out["theta"] = x, spe * inten * a, theta
            # gl_FragDepth, :193-197
            depth = (1.0 / self.depth_distance(p, eye, t, eps) - 1.0 / near) / (1.0 / far - 1.0 / near)
        out["rgba"] = np.concatenate([color, depth[:, None]], axis=1)
        with np.errstate(invalid="ignore"):
            out["cond"] = shin * sum(np.nan_to_num(np.abs(out[f]).max(axis=1), nan=0.0, posinf=0.0)
                                     for f in ("spec_point", "spec_directional", "spec_spot"))
        return out

    def shade(self, cam, P, rect, g, t=None):
        g = np.asarray(g).reshape(-1)
        T = self.terms(cam, P, rect, g, t)
        hit = (g["flags"] & HIT) != 0
        rgba = np.where(hit[:, None], T["rgba"], np.array([0.0, 0.0, 0.0, 1.0]))            # discard: {0, 0, 0, 1}
        return rgba, np.where(hit, T["cond"], 0.0)

    def shade_translucent(self, cam, P, absorption, rect, surface, behind):
        s, b = np.asarray(surface).reshape(-1), np.asarray(behind).reshape(-1)
        cs, conds = self.shade(cam, P, rect, s)
        t1, t2 = s["t"].astype(np.float64), b["t"].astype(np.float64)
        cb, condb = self.shade(cam, P, rect, b, t=t1 + t2)                                   # the behind record at the eye distance
        a = float(absorption) or 0.5
        with np.errstate(invalid="ignore"):
            k = np.clip(t2 * a, 0.0, 1.0)
        blend = ((s["flags"] & HIT) != 0) & ((s["flags"] & SEE_THROUGH) != 0) & ((b["flags"] & HIT) != 0)
        rgba = cs.copy()
        mixed = np.concatenate([cb[:, :3] * (1.0 - k)[:, None] + cs[:, :3] * k[:, None], cb[:, 3:]], axis=1)
        rgba[blend] = mixed[blend]
        return rgba, np.where(blend, condb * (1.0 - k) + conds * k, conds)


MODEL = ShadeModel()
shade = MODEL.shade
shade_translucent = MODEL.shade_translucent
terms = MODEL.terms


# ---- the 8-byte record { float t; uint32 w } as one little-endian uint64: t's bits low, w high (include/svo.h) ----
def pack(records):
    r = np.asarray(records).reshape(-1)
    nrm = r["normal"]
    with np.errstate(invalid="ignore"):
        axis = np.where(nrm < 0, 0, np.where(nrm > 0, 2, 1)).astype(np.uint64)               # 0: -, 1: 0 (and -0.0), 2: +
    nan = np.isnan(nrm).any(axis=1)
    code = np.where(nan, np.uint64(1 << 6), axis[:, 0] | (axis[:, 1] << np.uint64(2)) | (axis[:, 2] << np.uint64(4)))
    flags = r["flags"].astype(np.uint64)
    w = (r["material"].astype(np.uint64) | ((flags & np.uint64(0xFF)) << np.uint64(16)) | (code << np.uint64(24))
         | (((flags >> np.uint64(15)) & np.uint64(1)) << np.uint64(31)))
    return r["t"].view(np.uint32).astype(np.uint64) | (w << np.uint64(32))


def unpack(words):
    q = np.asarray(words, np.uint64).reshape(-1)
    w = (q >> np.uint64(32)).astype(np.uint32)
    r = np.zeros(q.shape[0], HIT_DTYPE)                                                      # chunk, node, cell: not carried
    r["t"] = (q & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)
    r["material"] = w & 0xFFFF
    r["flags"] = ((w >> 16) & 0xFF) | np.where(w >> 31, ERR, 0)
    iv = np.stack([((w >> s) & 3).astype(np.int64) - 1 for s in (24, 26, 28)], axis=1)
    dot = (iv * iv).sum(axis=1)
    bits = np.select([dot == 1, dot == 2, dot == 3], [np.uint32(0x3F800000), np.uint32(INV_SQRT2), np.uint32(INV_SQRT3)],
                     np.uint32(0x7FC00000)).astype(np.uint32)
    with np.errstate(invalid="ignore"):
        nrm = iv.astype(np.float32) * bits.view(np.float32)[:, None]                         # normalize(ivec3); (0,0,0) -> NaN
    nrm[((w >> 30) & 1) != 0] = np.float32(np.nan)
    nrm[(r["flags"] & HIT) == 0] = 0.0                                                       # a miss carries no normal
    r["normal"] = nrm
    return r


def cube_normals():
    """The 26 values normalize(ivec3 in {-1,0,1}^3 \\ 0) the march writes, bit for bit, in sign-code order."""
    out = []
    for z in (-1, 0, 1):
        for y in (-1, 0, 1):
            for x in (-1, 0, 1):
                d = x * x + y * y + z * z
                if d:
                    inv = np.array([0x3F800000, INV_SQRT2, INV_SQRT3][d - 1], np.uint32).view(np.float32)
                    out.append(np.array([x, y, z], np.float32) * inv)
    return np.array(out, np.float32)


def is_cube_or_nan(records):
    """Hit-or-not, does the record's normal survive the packed form bit for bit (one of the 26 vectors, or any NaN)?"""
    r = np.asarray(records).reshape(-1)
    forced = r.copy()
    forced["flags"] |= HIT
    back = unpack(pack(forced))["normal"]
    nan = np.isnan(r["normal"]).any(axis=1)
    return nan | (back.view(np.uint32) == r["normal"].view(np.uint32)).all(axis=1)


# ---- synthetic G-buffers -----------------------------------------------------------------------------------------
IMAGE = (131, 97)                                   # the camera's image
RECT = (23, 17, 67, 45)                             # x0, y0, w, h: 3015 records, 11 full blocks of 256 and one of 199
CUSTOM_SHININESS = (0.0, 0.5, 1.0, 8.0, 64.0, 100.0, 1000.0, 10000.0)
SHADOW_FLAG_SETS = [a | b | c | d for a in (0, SHADOWED) for b in (0, LOCAL_SHADOWS) for c in (0, SHADOWED_POINT) for d in (0, SHADOWED_SPOT)]


def camera(svo, eye, forward=(0.2, -0.3, 0.9), vfov=90.0):
    return svo.make_camera(eye, forward, (0.0, 1.0, 0.0), vfov, *IMAGE)


def copy_params(P):
    Q = type(P)()
    C.memmove(C.byref(Q), C.byref(P), C.sizeof(P))
    return Q


def explicit(P):
    """P with its four 0 = default fields spelled out."""
    Q = copy_params(P)
    Q.eps, Q.gamma = Q.eps or 1.0 / 8192.0, Q.gamma or 2.2
    Q.near_plane, Q.far_plane = Q.near_plane or 0.125, Q.far_plane or 8192.0
    return Q


def custom_params(svo, gamma=2.4, attenuation=((1.0, 0.02, 0.004), (0.8, 0.0, 0.0))):
    """Every field away from its default: gamma, the planes, eps, the attenuation constants (the spotlight's with
    linear = quadratic = 0), and a material table whose entries 0..7 have the shininess of CUSTOM_SHININESS and no zero colour."""
    P = svo.shade_defaults()
    P.gamma, P.near_plane, P.far_plane, P.eps = gamma, 0.5, 1000.0, 1.0 / 4096.0
    (P.point.constant, P.point.linear, P.point.quadratic), (P.spot.constant, P.spot.linear, P.spot.quadratic) = attenuation
    P.directional.specular[:] = [0.6, 0.5, 0.4]
    for i, s in enumerate(CUSTOM_SHININESS):
        m = P.materials[i]
        m.shininess = s
        m.diffuse[:] = [0.3 + 0.08 * i, 0.9 - 0.07 * i, 0.5]
        m.specular[:] = [0.9 - 0.05 * i, 0.6, 0.35 + 0.07 * i]
    return P


def _records(n):
    return np.zeros(n, HIT_DTYPE)


def _garbage(rng, g, idx):
    """Records that are not hits: every other field holds garbage (stale normals, NaN and inf among them)."""
    m = idx.size
    g["flags"][idx] = rng.integers(0, 1 << 15, m).astype(np.uint16) & ~np.uint16(HIT)
    g["t"][idx] = rng.choice(np.array([np.nan, np.inf, -1.0, 0.0, 7.5, 1e30], np.float32), m)
    g["normal"][idx] = rng.choice(np.array([np.nan, -np.inf, 0.0, 1.0, -0.57735026, 3.0], np.float32), (m, 3))
    g["material"][idx] = rng.integers(0, 1 << 16, m)
    for f in ("chunk", "node", "cell"):
        g[f][idx] = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)


def general_buffer(n=RECT[2] * RECT[3], seed=1):
    """t uniform in [1, 150]; the 26 cube normals, NaN normals and face normals; materials 0..7, 8, 255, 0xFFFF; all sixteen
    values of the four shadow bits; other flag bits at random; a tenth of the records not hit, with garbage in every field."""
    rng = np.random.default_rng(seed)
    g = _records(n)
    g["t"] = rng.uniform(1.0, 150.0, n).astype(np.float32)
    normals = np.concatenate([cube_normals(), np.full((2, 3), np.nan, np.float32),
                              np.array([[np.nan, 0.0, 1.0], [0.0, -1.0, np.nan]], np.float32)])
    g["normal"] = normals[rng.integers(0, len(normals), n)]
    face = np.arange(n) % 5 == 0                                        # SVO_NORMAL_FACE records: +-axis, flagged
    ax = rng.integers(0, 3, n)
    fn = np.zeros((n, 3), np.float32)
    fn[np.arange(n), ax] = rng.choice(np.array([-1.0, 1.0], np.float32), n)
    g["normal"][face] = fn[face]
    g["material"] = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 255, 0xFFFF], np.uint16)[rng.integers(0, 11, n)]
    g["flags"] = HIT | np.array(SHADOW_FLAG_SETS, np.uint16)[np.arange(n) % 16] | np.where(face, FACE_NORMAL, 0).astype(np.uint16) \
        | (rng.integers(0, 2, n).astype(np.uint16) * np.uint16(2)) | (rng.integers(0, 128, n).astype(np.uint16) << np.uint16(8))
    g["flags"] = rng.permutation(g["flags"])
    g["flags"] = np.where(face, g["flags"] | FACE_NORMAL, g["flags"] & ~np.uint16(FACE_NORMAL))
    for f in ("chunk", "node", "cell"):
        g[f] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    _garbage(rng, g, np.nonzero(rng.random(n) < 0.1)[0])
    return g


def general_case(svo, params="default"):
    """(cam, params, rect, buffer): the eye a few units from the origin, so that eye + beta * s is well conditioned for every t."""
    cam = camera(svo, (2.5, 3.25, -1.5), forward=(0.45, 0.1, 0.9))
    P = svo.shade_defaults() if params == "default" else custom_params(svo, **params)
    return cam, explicit(P), RECT, general_buffer()


def _rays(cam, rect):
    x0, y0, w, h = rect
    k = np.arange(w * h)
    u = ((x0 + k % w + 0.5) / cam.width * 2.0 - 1.0) * float(cam.tan_half_x)
    v = (1.0 - (y0 + k // w + 0.5) / cam.height * 2.0) * float(cam.tan_half_y)
    return _unit(_v(cam.forward) + _v(cam.right) * u[:, None] + _v(cam.up) * v[:, None])


def highlight_depths(n, seed):
    """d = 1 - dot(vdir, hv) wanted per record: 0, 2^-24, 2^-12 and both neighbours of 1/64 first, then a quarter log-uniform
    below 2^-10 (where a shininess of 1000 or 10000 leaves anything), a quarter uniform within 1/256 of the seam at 1/64, a
    quarter log-uniform up to 1/8 and a quarter uniform over [0, 1/8]."""
    rng = np.random.default_rng(seed)
    d = np.concatenate([2.0 ** rng.uniform(-26, -10, n // 4), rng.uniform(1 / 64 - 1 / 256, 1 / 64 + 1 / 256, n // 4),
                        2.0 ** rng.uniform(-10, -3, n // 4), rng.uniform(0.0, 0.125, n - 3 * (n // 4))])
    rng.shuffle(d)
    fixed = [0.0, 2.0 ** -24, 2.0 ** -12, 1 / 64 - 2.0 ** -30, 1 / 64, 1 / 64 + 2.0 ** -30, 0.125]
    d[:len(fixed)] = fixed
    return d


def _highlight_params(svo, light):
    """Custom materials; only `light`'s specular colour is on (no ambient, no diffuse: the picture IS the highlight), gentle
    attenuation, a cone wide enough for the whole rectangle."""
    P = custom_params(svo, gamma=2.2, attenuation=((1.0, 0.02, 0.001), (1.0, 0.01, 0.002)))
    for L in (P.point, P.directional, P.spot):
        for f in ("ambient", "diffuse", "specular"):
            getattr(L, f)[:] = [0.0, 0.0, 0.0]
    getattr(P, light).specular[:] = [1.0, 0.9, 0.8]
    P.spot.cos_phi, P.spot.cos_gamma = math.cos(math.radians(50.0)), math.cos(math.radians(62.0))
    return P


def _highlight_records(n, seed):
    rng = np.random.default_rng(seed)
    g = _records(n)
    g["normal"] = cube_normals()[np.arange(n) % 26]
    g["material"] = np.arange(n) % 8                                    # every shininess of the custom table
    g["flags"] = HIT | np.where(rng.random(n) < 0.05, SHADOWED, 0).astype(np.uint16)
    return g


def highlight_case(svo, light, aim=0.0):
    """The specular term of one light, swept through d = 1 - dot(vdir, hv) in [0, 1/8].  dot(vdir, hv) is the cosine of HALF the
    angle A between the direction to the light and the direction to the eye, so d needs A = 2 acos(1 - d).
    point / spot: the light sits 0.02 beside the eye (at the origin, so that eye + beta * s rounds relative to s alone); on a
      pixel's ray the point at distance s sees the light at A with tan A = b / (s - a) (a, b: the light's offset along and
      across the ray), so every record takes the s of its own d.  s runs from 0.013 (d = 1/8) to 29 (d = 2^-24); d = 0 takes s = 150.
    directional: the light shines from behind the camera along the ray of pixel (8, 6) of the rectangle, turned by the A of `aim`;
      A then depends on the pixel alone (90 degree field of view: the rectangle spans 67 degrees), so d moves in pixel steps: the
      caller runs aim = 0, 2^-24 and 2^-12, and the ring of pixels 17 from that one straddles 1/64, the far corner reaches 1/8."""
    cam = camera(svo, (0.0, 0.0, 0.0))
    P = _highlight_params(svo, light)
    n = RECT[2] * RECT[3]
    g = _highlight_records(n, 7)
    beta = _rays(cam, RECT)
    eps = 1.0 / 4096.0
    if light == "directional":
        c = beta[6 * RECT[2] + 8]
        A = 2.0 * math.acos(1.0 - aim)
        side = _unit(np.cross(c, _v(cam.up)))
        l = c * -math.cos(A) + side * -math.sin(A)                      # towards the light: -c turned by A
        P.directional.direction[:] = [float(x) for x in -l]
        g["t"] = np.random.default_rng(11).uniform(1.0, 150.0, n).astype(np.float32)
        return cam, explicit(P), RECT, g
    o = 0.02 * _unit(_v(cam.right) * 0.8 + _v(cam.up) * 0.6 - _v(cam.forward) * 0.1)
    getattr(P, light).position[:] = [float(x) for x in o]
    if light == "spot":
        P.spot.direction[:] = list(cam.forward)                         # shines where the camera looks
    o = _v(getattr(P, light).position)
    d = highlight_depths(n, 5)
    A = 2.0 * np.arccos(1.0 - d)
    a = beta @ o
    b = np.sqrt(np.maximum(_dot(o, o) - a * a, 0.0))
    with np.errstate(divide="ignore"):
        s = np.where(d > 0.0, a + b / np.tan(A), 150.0)
    g["t"] = (np.minimum(s, 150.0) + eps).astype(np.float32)
    return cam, explicit(P), RECT, g


def spot_cone_case(svo):
    """theta = dot(l, axis) below cos_gamma, between the bounds and above cos_phi, and within 1e-6 of either bound.  The spotlight
    sits beside the eye and shines where the camera looks: on a pixel's ray theta runs from its value at the eye (about 0.1) to
    dot(beta, forward) >= 0.68 far away, monotonically, so every record takes the s at which theta is the value wanted for it
    (bisection in float64)."""
    cam = camera(svo, (0.0, 0.0, 0.0))
    P = custom_params(svo, gamma=2.2, attenuation=((1.0, 0.14, 0.09), (1.0, 0.02, 0.001)))
    P.eps = 1.0 / 8192.0
    P.spot.cos_phi, P.spot.cos_gamma = 0.58, 0.41
    L = 3.0 * _v(cam.right) + 1.0 * _v(cam.up) + 0.4 * _v(cam.forward)
    P.spot.position[:] = [float(x) for x in L]
    P.spot.direction[:] = list(cam.forward)
    L, axis = _v(P.spot.position), _unit(-_v(P.spot.direction))
    n = RECT[2] * RECT[3]
    rng = np.random.default_rng(3)
    g = _highlight_records(n, 9)
    g["normal"] = cube_normals()[np.argmax(cube_normals().astype(np.float64) @ _unit(L))]     # faces the light: diffuse is on
    cg, cp = float(P.spot.cos_gamma), float(P.spot.cos_phi)
    want = np.concatenate([rng.uniform(0.2, cg, n // 5), rng.uniform(cg, cp, n // 5), rng.uniform(cp, 0.66, n // 5),
                           cg + rng.uniform(-1e-6, 1e-6, n // 5), cp + rng.uniform(-1e-6, 1e-6, n - 4 * (n // 5))])
    rng.shuffle(want)
    want[:5] = [cg, cp, 0.5 * (cg + cp), np.nextafter(np.float32(cg), np.float32(0)), np.nextafter(np.float32(cp), np.float32(1))]
    beta = _rays(cam, RECT)

    def theta(s):
        lv = L - beta * s[:, None]
        return _dot(_unit(lv), axis)
    lo, hi = np.zeros(n), np.full(n, 400.0)
    assert np.all(theta(lo) < 0.2) and np.all(theta(hi) > 0.66)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        below = theta(mid) < want
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    g["t"] = (0.5 * (lo + hi) + float(P.eps)).astype(np.float32)
    return cam, explicit(P), RECT, g


def near_eye_case(svo):
    """t - eps in (0, 2e-3]: log-uniform from 1e-6, a third within 10 % of 1e-3 (the kernel's own distance of a hit in front of
    the eye ends there), the float32 1e-3 itself and its neighbours, and a few records with t < eps (the point lies behind the
    eye).  The eye is the origin: eye + beta * s then rounds relative to s.  Two inputs are left out because the shader's formula
    is 0/0 there and nothing can be compared: t == eps exactly (normalize(eye - point) of a zero vector) and a light exactly at the
    point; both lights are 0.003 beside the eye and behind it, where no ray of the rectangle passes."""
    cam = camera(svo, (0.0, 0.0, 0.0))
    P = custom_params(svo, gamma=2.2, attenuation=((1.0, 0.14, 0.09), (1.0, 0.0, 0.0)))
    P.eps = 1.0 / 8192.0
    P.point.position[:] = [float(x) for x in 0.003 * _v(cam.right) - 0.001 * _v(cam.forward)]
    P.spot.position[:] = [float(x) for x in -0.002 * _v(cam.right) + 0.002 * _v(cam.up) - 0.001 * _v(cam.forward)]
    P.spot.direction[:] = list(cam.forward)
    P.spot.cos_phi, P.spot.cos_gamma = math.cos(math.radians(50.0)), math.cos(math.radians(62.0))
    n = RECT[2] * RECT[3]
    rng = np.random.default_rng(13)
    g = _highlight_records(n, 15)
    s = np.where(rng.random(n) < 1 / 3, rng.uniform(0.9e-3, 1.1e-3, n), 10.0 ** rng.uniform(-6.0, math.log10(2e-3), n))
    eps, edge = np.float32(P.eps), np.float32(1e-3)
    t = (s + float(eps)).astype(np.float32)
    t[:3] = [eps + np.nextafter(edge, np.float32(0)), eps + edge, eps + np.nextafter(edge, np.float32(1))]
    behind = rng.random(n) < 0.02
    t[behind] = (float(eps) - 10.0 ** rng.uniform(-7.0, -4.0, n)).astype(np.float32)[behind]
    assert not np.any(t == eps)
    g["t"] = t
    return cam, explicit(P), RECT, g


def all_cases(svo):
    """name -> (cam, params, rect, buffer) of every synthetic shading case; the parameter structs have no 0 = default field."""
    cases = {"general_default": general_case(svo),
             "general_gamma1": general_case(svo, dict(gamma=1.0)),
             "general_gamma2.4": general_case(svo, dict(gamma=2.4, attenuation=((0.7, 0.0, 0.0), (1.0, 0.03, 0.0))))}
    for light in ("point", "spot"):
        cases["highlight_" + light] = highlight_case(svo, light)
    for name, aim in (("0", 0.0), ("2^-24", 2.0 ** -24), ("2^-12", 2.0 ** -12)):
        cases["highlight_directional_" + name] = highlight_case(svo, "directional", aim)
    cases["spot_cone"] = spot_cone_case(svo)
    cases["near_eye"] = near_eye_case(svo)
    return cases


def translucent_case(svo, params="default"):
    """(cam, params, rect, surface, behind): SVO_SEE_THROUGH set and clear, the behind record hit and missed, t2 * absorption
    below, at and above 1 for absorption 0 (0.5) and 0.2 (t2 = 2 and t2 = 5 exactly among them), behind records with shadow
    bits of their own, surface misses with a behind hit (stays {0,0,0,1})."""
    cam, P, rect, s = general_case(svo, params)
    n = s.shape[0]
    rng = np.random.default_rng(21)
    s["t"] = rng.uniform(1.0, 60.0, n).astype(np.float32)
    hit = (s["flags"] & HIT) != 0
    s["flags"] = np.where(hit & (rng.random(n) < 0.6), s["flags"] | SEE_THROUGH, s["flags"] & ~np.uint16(SEE_THROUGH))
    s["material"] = np.where((s["flags"] & SEE_THROUGH) != 0, 6, s["material"])
    b = general_buffer(seed=2)
    t2 = rng.choice(np.array([0.0, 0.25, 1.0, 1.999, 2.0, 2.001, 3.5, 4.999, 5.0, 5.001, 9.0, 40.0], np.float32), n)
    t2 = np.where(rng.random(n) < 0.5, t2, rng.uniform(0.0, 8.0, n).astype(np.float32))
    b["t"] = np.where((b["flags"] & HIT) != 0, t2, b["t"])
    return cam, P, rect, s, b


def pack_records(n, seed=31):
    """Records for the pack / unpack checks: all 27 sign triples at unit and non-unit magnitudes with -0.0 for the zeros of every
    other one, NaN in one, two and three components, +-inf components, every value of the low flag byte with and without
    SVO_ERR_FLAG and with bits 8-14, materials 0, 1 and 0xFFFF, t as NaN, +-inf, -0.0 and a denormal, misses with stale normals,
    and a hit whose normal is (0,0,0) (record 13 of every 27: sign triple (0,0,0))."""
    rng = np.random.default_rng(seed)
    g = _records(n)
    k = np.arange(n)
    sign = np.stack([k % 3 - 1, (k // 3) % 3 - 1, (k // 9) % 3 - 1], axis=1).astype(np.float32)
    inv = np.array([0x7FC00000, 0x3F800000, INV_SQRT2, INV_SQRT3], np.uint32).view(np.float32)[(sign * sign).sum(axis=1).astype(int)]
    mag = np.where(((k // 27) % 2 == 0)[:, None], np.where(sign == 0, np.float32(1.0), inv[:, None]), rng.choice(np.array([1e-30, 0.57735026, 0.70710677, 2.5, 1e30], np.float32), (n, 3)))
    nrm = (sign * mag).astype(np.float32)
    nrm[(sign == 0) & ((k // 27) % 2 == 1)[:, None]] = np.float32(-0.0)
    special = np.array([[np.nan, 1, 0], [0, np.nan, -1], [1, 1, np.nan], [np.nan, np.nan, 0], [np.nan, -1, np.nan], [0, np.nan, np.nan],
                        [np.nan, np.nan, np.nan], [np.inf, 0, 0], [0, -np.inf, 1], [-np.inf, np.inf, -np.inf], [np.inf, np.nan, 0]], np.float32)
    sp = (k % 7 == 3) & (k >= 27)
    nrm[sp] = special[(k // 7) % len(special)][sp]
    g["normal"] = nrm
    g["flags"] = (k % 256).astype(np.uint16) | np.where((k // 256) % 2 == 1, ERR, 0).astype(np.uint16) \
        | (rng.integers(0, 128, n).astype(np.uint16) << np.uint16(8))
    if n < 512:                                     # short buffers: the low byte and the error bit at random instead of in sequence
        g["flags"] = rng.integers(0, 1 << 16, n).astype(np.uint16)
    g["material"] = np.array([0, 1, 0xFFFF, 6], np.uint16)[rng.integers(0, 4, n)]
    tbits = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x41200000], np.uint32)
    g["t"] = np.where(k % 3 == 0, tbits[(k // 3) % 8], rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)).astype(np.uint32).view(np.float32)
    for f in ("chunk", "node", "cell"):
        g[f] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return g
