"""Host model of svo_shade_sky and svo_frame_rgba8 (include/svo.h): the cube-map lookup in numpy float32, one float32 operation per
operation of the header's statement, so that the device kernel is held to it bit for bit; a second, plain float64 lookup written from
the OpenGL cube-map rules without that ordering (weights instead of nested lerps), which the float32 one is checked against; the
RGBA8 conversion; and the cameras of the GPU tests, so that the CPU tests can check what they see.  Test infrastructure."""
import numpy as np

from hit_voxels_model import F, HIT_FLAG, IMAGE, WORLDS, camera_dirs, cameras as mixed_cameras  # noqa: F401  (camera_dirs: the pixel directions)

LINEAR, NEAREST = 0, 1
FACE_NAMES = ("+X", "-X", "+Y", "-Y", "+Z", "-Z")
WORLD = "grid_2x1x2_d6"


# ---- the float32 statement ---------------------------------------------------------------------------------------------------------
def face_coords(d):
    """-> (face [n] int, -1 where !(ma > 0); s [n], t [n] float32) for directions d [n][3] float32."""
    d = np.asarray(d, F)
    ax, ay, az = np.abs(d[:, 0]), np.abs(d[:, 1]), np.abs(d[:, 2])
    x_major = (ax >= ay) & (ax >= az)
    y_major = ~x_major & (ay >= az)
    axis = np.where(x_major, 0, np.where(y_major, 1, 2))
    rows = np.arange(d.shape[0])
    ma = np.abs(d[rows, axis])
    neg = d[rows, axis] < 0
    face = axis * 2 + neg
    sc = np.select([face == 0, face == 1, face == 5], [-d[:, 2], d[:, 2], -d[:, 0]], d[:, 0])
    tc = np.select([face == 2, face == 3], [d[:, 2], -d[:, 2]], -d[:, 1])
    with np.errstate(all="ignore"):
        s = ((sc / ma + F(1)) * F(0.5)).astype(F)
        t = ((tc / ma + F(1)) * F(0.5)).astype(F)
    return np.where(ma > 0, face, -1), s, t


def _int(v):
    """(int)v of a floor()ed coordinate; NaN reads texel 0."""
    return np.where(np.isnan(v), 0, v).astype(np.int64)


def nearest_index(s, t, size):
    with np.errstate(all="ignore"):
        x = np.clip(_int(np.floor(s * F(size))), 0, size - 1)
        y = np.clip(_int(np.floor(t * F(size))), 0, size - 1)
    return x, y


def lookup(d, faces, filter=LINEAR):
    """-> (rgb [n][3] float32, face [n]): what svo_shade_sky writes into r, g, b of a sky pixel of direction d; rows with face == -1 are
    pixels it leaves alone (rgb 0 there).  faces: uint8 [6][size][size][3], face order +X, -X, +Y, -Y, +Z, -Z, row 0 at t = 0."""
    faces = np.asarray(faces, np.uint8)
    size = faces.shape[1]
    face, s, t = face_coords(d)
    on = face >= 0
    f = np.where(on, face, 0)

    def T(x, y):
        return faces[f, y, x].astype(F) / F(255)

    with np.errstate(all="ignore"):
        if filter == NEAREST:
            x, y = nearest_index(s, t, size)
            c = T(x, y)
        else:
            u, v = s * F(size) - F(0.5), t * F(size) - F(0.5)
            i, j = np.floor(u), np.floor(v)
            a, b = (u - i)[:, None], (v - j)[:, None]
            xl, xr = np.clip(_int(i), 0, size - 1), np.clip(_int(i) + 1, 0, size - 1)
            yl, yr = np.clip(_int(j), 0, size - 1), np.clip(_int(j) + 1, 0, size - 1)
            top = T(xl, yl) + (T(xr, yl) - T(xl, yl)) * a
            bot = T(xl, yr) + (T(xr, yr) - T(xl, yr)) * a
            c = top + (bot - top) * b
    c = c.astype(F)
    c[~on] = 0
    return c, face


def shade_sky(rgba, records, dirs, faces, filter=LINEAR):
    """The image svo_shade_sky leaves: rgba [n][4] float32 as a shade call wrote it, records the HIT_DTYPE (or any array with "flags")."""
    out = np.array(rgba, F, copy=True).reshape(-1, 4)
    c, face = lookup(dirs, faces, filter)
    sky = ((np.asarray(records).reshape(-1)["flags"] & HIT_FLAG) == 0) & (face >= 0)
    out[sky, :3] = c[sky]
    return out


def frame_rgba8(rgba):
    """uint8 [n][4]: svo_frame_rgba8 of float32 [n][4] pixels."""
    c = np.asarray(rgba, F).reshape(-1, 4)[:, :3]
    with np.errstate(all="ignore"):
        mid = (np.where((c > 0) & (c < 1), c, F(0)) * F(255) + F(0.5)).astype(F).astype(np.int64)
    rgb = np.where(c >= 1, 255, np.where(c > 0, mid, 0))      # NaN fails both compares: 0
    return np.concatenate([rgb, np.full((rgb.shape[0], 1), 255)], axis=1).astype(np.uint8)


def ulp(x, k):
    return (np.array([x], F).view(np.uint32) + np.uint32(k)).view(F)[0] if k >= 0 else (np.array([x], F).view(np.uint32) - np.uint32(-k)).view(F)[0]


def rgba8_inputs():
    """NaN, +-inf, -0.0, 1 +- 1 ulp, and k / 255 and (k + 0.5) / 255 +- 1 ulp for every k: float32 [n][4], depth 0.25."""
    v = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, ulp(1.0, 1), ulp(1.0, -1), -1.0, 2.0, 1e-30, 0.5]
    for k in range(256):
        for base in (F(k) / F(255), (F(k) + F(0.5)) / F(255)):
            v += [base, ulp(base, 1)] + ([ulp(base, -1)] if base > 0 else [])
    v = np.array(v, F)
    v = np.concatenate([v, np.zeros(-v.size % 3, F)])
    return np.concatenate([v.reshape(-1, 3), np.full((v.size // 3, 1), 0.25, F)], axis=1)


# ---- the float64 lookup: OpenGL 4.6 core 8.13 (cube map face selection) and 8.14.2 (linear filtering as a weighted sum) ----------------
def lookup64(d, faces, filter=LINEAR):
    faces = np.asarray(faces, np.uint8)
    size = faces.shape[1]
    d = np.asarray(d, F).astype(np.float64)
    out = np.zeros((d.shape[0], 3))
    for k, (x, y, z) in enumerate(d):
        mags = [abs(x), abs(y), abs(z)]
        axis = 0 if mags[0] >= mags[1] and mags[0] >= mags[2] else (1 if mags[1] >= mags[2] else 2)
        ma = mags[axis]
        if not ma > 0:
            continue
        face = 2 * axis + (1 if (x, y, z)[axis] < 0 else 0)
        sc = {0: -z, 1: z, 2: x, 3: x, 4: x, 5: -x}[face]
        tc = {0: -y, 1: -y, 2: z, 3: -z, 4: -y, 5: -y}[face]
        s, t = 0.5 * (sc / ma + 1.0), 0.5 * (tc / ma + 1.0)
        img = faces[face].astype(np.float64) / 255.0
        if filter == NEAREST:
            out[k] = img[min(max(int(np.floor(t * size)), 0), size - 1), min(max(int(np.floor(s * size)), 0), size - 1)]
            continue
        u, v = s * size - 0.5, t * size - 0.5
        i0, j0 = int(np.floor(u)), int(np.floor(v))
        a, b = u - i0, v - j0
        cl = lambda q: min(max(q, 0), size - 1)
        out[k] = ((1 - a) * (1 - b) * img[cl(j0), cl(i0)] + a * (1 - b) * img[cl(j0), cl(i0 + 1)]
                  + (1 - a) * b * img[cl(j0 + 1), cl(i0)] + a * b * img[cl(j0 + 1), cl(i0 + 1)])
    return out


# ---- faces and cameras of the tests -------------------------------------------------------------------------------------------------
def identity_faces(size=256):
    """Texel (x, y) of face f holds the bytes (x, y, f)."""
    y, x = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    return np.stack([np.stack([x, y, np.full_like(x, f)], axis=2) for f in range(6)]).astype(np.uint8)


def random_faces(size, seed):
    return np.random.default_rng(seed).integers(0, 256, (6, size, size, 3), np.uint8)


def flat_faces(size, byte):
    return np.full((6, size, size, 3), byte, np.uint8)


def world_box(name=WORLD):
    w, h, d, cs, ccm, _, _ = WORLDS[name]
    lo = np.array(ccm, np.float64) * cs
    return lo, lo + np.array([w, h, d], np.float64) * cs


def sky_cameras(svo, name=WORLD):
    """All-sky views, 64 x 48: the eye 10 units outside one face of the world box looking straight away from it with a 100 degree
    vertical fov (every ray moves away from the box: none can enter it; the view covers one cube face and the rims of its four neighbours), one per
    +-axis; and one along (1, 1, 1) from beyond the max corner, whose centre pixels sit where |d.x|, |d.y|, |d.z| meet."""
    lo, hi = world_box(name)
    mid = 0.5 * (lo + hi)
    out = {}
    for axis in range(3):
        for sign, corner in ((1.0, hi), (-1.0, lo)):
            eye, fwd = mid.copy(), np.zeros(3)
            eye[axis] = corner[axis] + sign * 10.0
            fwd[axis] = sign
            up = (0.0, 0.0, 1.0) if axis == 1 else (0.0, 1.0, 0.0)
            out[FACE_NAMES[2 * axis + (sign < 0)]] = svo.make_camera(tuple(eye), tuple(fwd), up, 100.0, *IMAGE)
    out["corner"] = svo.make_camera(tuple(hi + 10.0), (1.0, 1.0, 1.0), (0.0, 1.0, 0.0), 100.0, *IMAGE)
    return out


def all_cameras(svo, name=WORLD):
    """name -> (camera, all_sky, semantics): the seven all-sky views and the two mixed views of hit_voxels_model.cameras.  The all-sky
    views are traced under SVO_SEMANTICS_GLSL, the march the reference renders with: src/Traverse.cpp's chunkmarch also enters a box
    that lies BEHIND the eye (a negative entry distance), so under SVO_SEMANTICS_CPU half of their pixels are hits at t < 0."""
    out = {k: (c, True, 1) for k, c in sky_cameras(svo, name).items()}
    out.update({k: (c, False, 0) for k, c in mixed_cameras(svo, name).items()})
    return out
