"""Host model of svo_shade_boxes, svo_cursor_place and the corner rule of svo_world_edit_cube (include/svo.h), in numpy float32: one
float32 operation per operation of the header's statement, so that the device kernel is held to it bit for bit.  Also the box lists
and cameras of the GPU tests, so that the CPU tests can check what they see.  Test infrastructure."""
import numpy as np

from hit_voxels_model import F, HIT_DTYPE, HIT_FLAG, ERR_FLAG, IMAGE, WORLDS, camera_dirs, cameras as mixed_cameras  # noqa: F401

SOLID, CURSOR, HIDDEN = 0, 1, 1 << 8
MAX_BOXES = 64
WORLD = "grid_2x1x2_d6"
BOX_DTYPE = np.dtype([("bmin", "<f4", (3,)), ("size", "<f4"), ("color", "<f4", (3,)), ("alpha", "<f4"), ("style", "<u4"), ("_pad", "<u4", (3,))])
FACE_NAMES = ("-Z", "-X", "+Z", "+X", "-Y", "+Y")            # the draw order of CUBE_INDICES (src/Parallax.cpp:25-38)
ORDER = {(2, 0): 0, (0, 0): 1, (2, 1): 2, (0, 1): 3, (1, 0): 4, (1, 1): 5}      # (axis, max side) -> place in the draw order
IN_FACE = {0: (0, 1), 2: (0, 1), 1: (1, 2), 3: (1, 2), 4: (0, 2), 5: (0, 2)}     # face -> its two in-face axes
EDGE_LO, EDGE_HI = F(1) / F(64), F(1) - F(1) / F(64)
INF = F(np.inf)


def box(bmin, size, color=(0.8, 0.8, 0.8), alpha=0.2, style=SOLID):
    b = np.zeros(1, BOX_DTYPE)
    b["bmin"], b["size"], b["color"], b["alpha"], b["style"] = np.asarray(bmin, F), F(size), np.asarray(color, F), F(alpha), style
    return b


def box_list(*boxes):
    return np.concatenate(boxes) if boxes else np.zeros(0, BOX_DTYPE)


# ---- svo_shade_boxes ---------------------------------------------------------------------------------------------------------------
def slabs(o, d, bmin, size):
    """-> (hit, tnear, tfar, fnear, ffar) per ray: the slab intersection of the header, faces as places in the draw order."""
    o, d = np.broadcast_to(np.asarray(o, F), np.asarray(d, F).shape), np.asarray(d, F)
    n = d.shape[0]
    tnear, tfar = np.full(n, -INF, F), np.full(n, INF, F)
    fnear, ffar = np.full(n, -1), np.full(n, -1)
    missed = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            lo = F(bmin[a])
            hi = F(lo + F(size))
            oa, da = o[:, a], d[:, a]
            on = da != 0
            t0, t1 = (lo - oa) / da, (hi - oa) / da
            min_first = t0 <= t1
            near, far = np.where(min_first, t0, t1), np.where(min_first, t1, t0)
            take = on & (near > tnear)
            tnear = np.where(take, near, tnear)
            fnear = np.where(take, np.where(min_first, ORDER[a, 0], ORDER[a, 1]), fnear)
            take = on & (far < tfar)
            tfar = np.where(take, far, tfar)
            ffar = np.where(take, np.where(min_first, ORDER[a, 1], ORDER[a, 0]), ffar)
            missed |= ~on & ((oa < lo) | (oa > hi))
        hit = ~missed & (fnear >= 0) & (ffar >= 0) & (tnear <= tfar)
    return hit, tnear.astype(F), tfar.astype(F), fnear, ffar


def fragment_depth(t, near=0.0, far=0.0):
    near, far = F(near if near else 0.125), F(far if far else 8192.0)
    inv_near = F(1) / near
    with np.errstate(all="ignore"):
        return ((F(1) / np.asarray(t, F) - inv_near) / (F(1) / far - inv_near)).astype(F)


def is_edge(c):
    return (c <= EDGE_LO) | (c >= EDGE_HI)


def shade_boxes(rgba, o, d, boxes, near=0.0, far=0.0):
    """-> (image [n][4] float32, stats): what svo_shade_boxes leaves of rgba [n][4] for the rays (o, d [n][3]) and the BOX_DTYPE list.
    stats: per pixel `passed` (fragments that passed the depth test), `failed` (fragments that did not) and `edge` (a cursor fragment
    that passed was an edge)."""
    out = np.array(rgba, F, copy=True).reshape(-1, 4)
    d = np.asarray(d, F).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(o, F), d.shape)
    n = d.shape[0]
    stats = {k: np.zeros(n, np.int64) for k in ("passed", "failed", "edge")}
    with np.errstate(all="ignore"):
        for b in np.asarray(boxes).reshape(-1):
            size = F(b["size"])
            if (int(b["style"]) & HIDDEN) or not size > 0:
                continue
            bmin = b["bmin"].astype(F)
            hit, tnear, tfar, fnear, ffar = slabs(o, d, bmin, size)
            entry_first = fnear < ffar
            for first in (True, False):
                is_entry = entry_first == first
                t = np.where(is_entry, tnear, tfar).astype(F)
                face = np.where(is_entry, fnear, ffar)
                frag = hit & (t > 0)
                f = fragment_depth(t, near, far)
                ok = frag & (f < out[:, 3])
                src = np.repeat(np.concatenate([b["color"], [b["alpha"]]]).astype(F)[None], n, axis=0)
                if (int(b["style"]) & 0xFF) == CURSOR:
                    p = (o + d * t[:, None]).astype(F)
                    c = ((p - bmin[None]) / size).astype(F)
                    u = np.select([np.isin(face, (0, 2)), np.isin(face, (1, 3))], [c[:, 0], c[:, 1]], c[:, 0])
                    v = np.select([np.isin(face, (0, 2)), np.isin(face, (1, 3))], [c[:, 1], c[:, 2]], c[:, 2])
                    edge = is_edge(u) | is_edge(v)
                    src[edge] = np.array([0, 0, 0, 1], F)
                    stats["edge"] += ok & edge
                a = src[:, 3:4]
                rgb = (src[:, :3] * a + out[:, :3] * (F(1) - a)).astype(F)
                out[ok, :3] = rgb[ok]
                out[ok, 3] = f[ok]
                stats["passed"] += ok
                stats["failed"] += frag & ~ok
    return out, stats


# ---- svo_cursor_place --------------------------------------------------------------------------------------------------------------
def cursor_place(origin, direction, record, size, box_in):
    """The svo_box that svo_cursor_place leaves of box_in (BOX_DTYPE[1]) for the ray's record (a HIT_DTYPE scalar)."""
    out = np.array(box_in, copy=True).reshape(1)
    flags = int(record["flags"])
    if (flags & HIT_FLAG) and not (flags & ERR_FLAG):
        sigma = (np.asarray(origin, F) + np.asarray(direction, F) * F(record["t"])).astype(F)
        out["bmin"][0] = (sigma - F(size) * F(0.5)).astype(F)
        out["size"][0] = F(size)
        out["style"][0] &= ~np.uint32(HIDDEN)
    else:
        out["style"][0] |= np.uint32(HIDDEN)
    return out


# ---- the corner rule of svo_world_edit_cube (modify(), src/Main.cpp:321-338) ----------------------------------------------------------
def pmod(n, m):
    return (m + int(np.fmod(n, m))) % m                     # src/World.cpp:276-279 (C's %, truncating)


def world_index(q, dims):
    w, h, d = dims
    return pmod(q[1], h) * w * d + pmod(q[2], d) * w + pmod(q[0], w)        # src/World.cpp:288-293


def index_float(p, chunksize):
    f = np.asarray(p, F) / F(chunksize)                     # src/World.cpp:323-332
    f = np.where(f < 0, f - F(1), f).astype(F)
    return [int(x) for x in np.trunc(f)]


def chunk_positions(dims, chunksize, ccm):
    """Chunk (X, Y, Z) = ccm + (x, y, z) sits at (X, Y, Z) * chunksize and lives at World::index(X, Y, Z)."""
    w, h, d = dims
    pos = np.zeros((w * h * d, 3), F)
    for y in range(h):
        for z in range(d):
            for x in range(w):
                q = (ccm[0] + x, ccm[1] + y, ccm[2] + z)
                pos[world_index(q, dims)] = np.array(q, F) * F(chunksize)
    return pos


def cube_corners(bmin, size):
    bmin, size = np.asarray(bmin, F), F(size)
    return [(bmin + np.array([bool(i & 4), bool(i & 2), bool(i & 1)], F) * size).astype(F) for i in range(8)]


def corner_chunks(bmin, size, dims, chunksize, ccm, positions=None):
    """-> (the chunk of each corner that passes the test, in corner order (the reference's calls); the distinct ones in order of first
    appearance (svo_world_edit_cube's chunks_out))."""
    pos = chunk_positions(dims, chunksize, ccm) if positions is None else np.asarray(positions, F)
    calls = []
    for p in cube_corners(bmin, size):
        j = world_index(index_float(p, chunksize), dims)
        lo = pos[j]
        hi = (lo + F(chunksize)).astype(F)
        if np.all(p >= lo) and np.all(hi >= p):             # isInsideCube, src/Traverse.cpp:18-23
            calls.append(j)
    return calls, list(dict.fromkeys(calls))


# ---- the scene of the GPU tests -------------------------------------------------------------------------------------------------------
def world_spec(name=WORLD):
    w, h, d, cs, ccm, _, _ = WORLDS[name]
    return (w, h, d), cs, ccm


def eye_of(cam):
    return np.array(cam.eye, F)


def forward_point(cam, dist, right=0.0, up=0.0):
    """A point `dist` ahead of the eye, moved sideways; float64, for placing boxes."""
    e, f, r, u = (np.array(a, np.float64) for a in (cam.eye, cam.forward, cam.right, cam.up))
    return e + f * dist + r * right + u * up


def scene_boxes(cam, records):
    """The eight boxes of the GPU test for one mixed view, placed from the view's own records (HIT_DTYPE [h*w], by the oracle or the
    device: they are equal): a solid marker in the air in front of terrain, one half buried, one entirely behind terrain, one over sky
    pixels, a translucent cursor overlapping the marker, one containing the eye, one behind the eye, one hidden."""
    g = np.asarray(records).reshape(-1)
    W, H = IMAGE
    d = camera_dirs(cam).astype(np.float64)
    e = np.array(cam.eye, np.float64)
    hit = ((g["flags"] & HIT_FLAG) != 0) & ((g["flags"] & ERR_FLAG) == 0)
    assert hit.sum() >= 300 and (~hit).sum() >= 300

    def pixel(want, frac_x):
        """A pixel of the wanted kind near column frac_x * W, as far from the other kind as the view allows (the middle row of its run)."""
        col = int(frac_x * W)
        rows = np.nonzero(want.reshape(H, W)[:, col])[0]
        assert rows.size >= 4, (col, rows.size)
        return rows[rows.size // 2] * W + col

    k_air = pixel(hit, 0.30)
    k_bury = pixel(hit, 0.70)
    k_behind = pixel(hit, 0.50)
    k_sky = pixel(~hit, 0.50)
    t = g["t"].astype(np.float64)
    s_air = 0.1 * t[k_air]
    marker = e + d[k_air] * (0.4 * t[k_air])                 # in the air, in front of the terrain
    s_bury = 0.15 * t[k_bury]
    buried = e + d[k_bury] * t[k_bury]                      # centred on the surface: half of it inside the terrain
    s_behind = 0.1 * t[k_behind]
    behind = e + d[k_behind] * (1.25 * t[k_behind])         # beyond the surface
    sky = e + d[k_sky] * 120.0
    s_cursor = 0.35 * t[k_air]                              # a face of it spans tens of pixels: its 1/64 edges are about a pixel wide
    boxes = box_list(
        box(marker - 0.5 * s_air, s_air, (1.0, 0.9, 0.2), 1.0, SOLID),
        box(buried - 0.5 * s_bury, s_bury, (0.2, 0.9, 1.0), 1.0, SOLID),
        box(behind - 0.5 * s_behind, s_behind, (1.0, 0.0, 1.0), 1.0, SOLID),
        box(sky - 15.0, 30.0, (0.9, 0.3, 0.1), 1.0, SOLID),
        box(marker - 0.5 * s_cursor, s_cursor, (0.8, 0.8, 0.8), 0.2, CURSOR),        # holds the marker, translucent, with edges
        box(e - 3.0, 6.0, (0.1, 0.1, 0.9), 0.25, SOLID),                           # contains the eye: its exit faces only, on every pixel
        box(forward_point(cam, -30.0) - 5.0, 10.0, (0.0, 1.0, 0.0), 1.0, SOLID),    # behind the eye
        box(marker - 20.0, 40.0, (1.0, 1.0, 1.0), 1.0, SOLID | HIDDEN),             # hidden
    )
    return boxes


EYE_BOX = 5                                                 # scene_boxes()[EYE_BOX] covers every pixel


def without_eye_box(boxes):
    """The list without the box that holds the eye: the one under which pixels stay unwritten."""
    return np.delete(boxes, EYE_BOX)


def translucent_pair(boxes):
    """Two overlapping translucent solids at the scene's marker: the pair whose order shows."""
    m = boxes[0]
    return box_list(box(m["bmin"], m["size"] * F(1.5), (1.0, 0.0, 0.0), 0.5, SOLID),
                    box(m["bmin"] - m["size"] * F(0.5), m["size"] * F(1.5), (0.0, 0.0, 1.0), 0.3, SOLID))


def counts(hit, stats):
    """What the placement must provide (pixels): a fragment passing over a hit, one failing against nearer terrain, one passing over
    sky, two blended layers, a cursor edge."""
    return {"over_hit": int((hit & (stats["passed"] > 0)).sum()), "behind_terrain": int((hit & (stats["failed"] > 0)).sum()),
            "over_sky": int((~hit & (stats["passed"] > 0)).sum()), "two_layers": int((stats["passed"] >= 2).sum()),
            "cursor_edge": int((stats["edge"] > 0).sum())}


NEEDED = {"over_hit": 50, "behind_terrain": 50, "over_sky": 50, "two_layers": 20, "cursor_edge": 20}
