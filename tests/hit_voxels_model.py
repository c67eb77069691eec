"""Host model of svo_hit_voxels, svo_hit_uv and the texel lookup of svo_shade_textured (include/svo.h), in numpy float32 on the pools
that World.chunk(i) returns: a top-down parent map per chunk (reachable blocks only), the box by traverse()'s arithmetic
(src/Traverse.cpp:34-48,66), cubeUV / leafUV restated from shaders/Chunkmarch.glsl:138-149 and shaders/World.Fragment.glsl:5-15 with one
float32 operation per GLSL operation, and GL_NEAREST / repeat.  Test infrastructure: the yardstick the device kernels are held against;
also the worlds, cameras and ray lists of the GPU tests, so that the CPU tests can check them for hits of every kind."""
import os

import numpy as np

F = np.float32
EMPTY, LEAF, BRANCH, TWIG = 0, 1, 2, 3
HIT_FLAG, ERR_FLAG, FACE_NORMAL = 1, 1 << 15, 8
INSIDE, SOLID = 1, 2
CELL_NONE = 0xFF
NONE = 0xFFFFFFFF
HIT_DTYPE = np.dtype([("t", "<f4"), ("normal", "<f4", (3,)), ("material", "<u2"), ("flags", "<u2"),
                      ("chunk", "<u4"), ("node", "<u4"), ("cell", "<u4")])
VOXEL_DTYPE = np.dtype([("bmin", "<f4", (3,)), ("size", "<f4"), ("material", "<u2"), ("flags", "<u2"),
                        ("chunk", "<u4"), ("node", "<u4"), ("cell", "<u4")])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the parent map ----------------------------------------------------------------------------------------------------------------
def parent_map(chunk):
    """-> (parent, level) per 8-block k (nodes 1 + 8k .. 8 + 8k): the index of the BRANCH that owns it and its level, (NONE, 0) for a
    block no BRANCH reachable from the root points at.  Top-down, level by level: an orphan block's words are never looked at."""
    tree = np.asarray(chunk["tree"], np.uint32)
    n = tree.size
    parent = np.full((n - 1) // 8, NONE, np.uint32)
    level = np.zeros((n - 1) // 8, np.uint8)
    front = np.zeros(1, np.int64)
    lv = 0
    while front.size and lv < 28:
        branch = front[(tree[front] >> 30) == BRANCH]
        off = (tree[branch] & 0x3FFFFFFF).astype(np.int64)
        ok = (off > branch) & ((off - 1) % 8 == 0) & (off + 8 <= n)
        branch, off = branch[ok], off[ok]
        parent[(off - 1) // 8] = branch
        level[(off - 1) // 8] = lv + 1
        front = (off[:, None] + np.arange(8)[None]).reshape(-1)
        lv += 1
    return parent, level


def hit_voxels(chunks, records):
    """VOXEL_DTYPE[n]: the records svo_hit_voxels writes for `records` (HIT_DTYPE[n]) on a world of `chunks` (World::index() order)."""
    g = np.ascontiguousarray(records).reshape(-1)
    out = np.zeros(g.shape[0], VOXEL_DTYPE)
    usable = ((g["flags"] & HIT_FLAG) != 0) & ((g["flags"] & ERR_FLAG) == 0)
    for c, chunk in enumerate(chunks):
        tree = np.asarray(chunk["tree"], np.uint32)
        sel = np.nonzero(usable & (g["chunk"] == c) & (g["node"] < tree.size))[0]
        if not sel.size:
            continue
        parent, level = parent_map(chunk)
        node, cell = g["node"][sel].astype(np.int64), g["cell"][sel]
        kind = tree[node] >> 30
        lv = np.where(node == 0, 0, level[np.maximum(node - 1, 0) // 8] if level.size else 0).astype(np.int64)
        ok = (((kind == LEAF) & (cell == CELL_NONE)) | ((kind == TWIG) & (cell < 64))) & ((node == 0) | (lv > 0))
        sel, node, cell, kind, lv = sel[ok], node[ok], cell[ok], kind[ok], lv[ok]
        if not sel.size:
            continue
        deepest = int(lv.max())
        slots = np.zeros((sel.size, max(deepest, 1)), np.int64)
        cur = node.copy()
        for i in range(deepest):                                 # the walk up
            on = i < lv
            slots[on, lv[on] - 1 - i] = (cur[on] - 1) & 7
            cur[on] = parent[(cur[on] - 1) // 8]
        assert not cur.any()
        bmin = np.repeat(np.array(chunk["position"], F)[None], sel.size, axis=0)
        size = np.full(sel.size, F(chunk["size"]), F)
        for i in range(deepest):                                 # the replay: halfsize = size * 0.5f, bmin += vec3(ge) * halfsize
            on = i < lv
            half = size * F(0.5)
            ge = np.stack([slots[:, i] & 1, (slots[:, i] >> 1) & 1, (slots[:, i] >> 2) & 1], axis=1).astype(F)
            step = bmin + ge * half[:, None]
            bmin[on] = step[on]
            size[on] = half[on]
        brick = kind == TWIG                                     # leafsize = size / 4, bmin += vec3(off) * leafsize
        leafsize = size / F(4)
        off = np.stack([cell & 3, (cell >> 2) & 3, cell >> 4], axis=1).astype(F)
        step = bmin + off * leafsize[:, None]
        bmin[brick] = step[brick]
        size[brick] = leafsize[brick]
        out["bmin"][sel], out["size"][sel] = bmin, size
        out["material"][sel], out["flags"][sel] = g["material"][sel], INSIDE | SOLID
        out["chunk"][sel], out["node"][sel], out["cell"][sel] = c, node, cell
    return out


# ---- the camera, the shaded point, cubeNormal, cubeUV / leafUV, the texel ----------------------------------------------------------
def camera_dirs(cam, rect=None):
    """The pinhole camera of include/svo.h, one float32 operation per operation of the kernels' ray generation; [h*w][3], row-major."""
    x0, y0, w, h = rect if rect is not None else (0, 0, cam.width, cam.height)
    px, py = np.meshgrid(np.arange(x0, x0 + w).astype(F), np.arange(y0, y0 + h).astype(F))
    px, py = px.reshape(-1), py.reshape(-1)
    u = (((px + F(0.5)) / F(cam.width)) * F(2) - F(1)) * F(cam.tan_half_x)
    v = (F(1) - ((py + F(0.5)) / F(cam.height)) * F(2)) * F(cam.tan_half_y)
    f, r, up = (np.array(a, F)[None] for a in (cam.forward, cam.right, cam.up))
    d = (f + r * u[:, None]) + up * v[:, None]
    dot = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return (d * (F(1) / np.sqrt(dot))[:, None]).astype(F)


def sample_points(origins, dirs, t, eps):
    """point = alpha + beta * (sigma - EPS), shaders/World.Fragment.glsl:174."""
    return (np.asarray(origins, F) + np.asarray(dirs, F) * (np.asarray(t, F) - F(eps))[:, None]).astype(F)


def cube_normal(s, cmin, cmax, eps):
    """cubeNormal, shaders/Chunkmarch.glsl:128-136, on arrays; NaN where the integer vector is (0, 0, 0)."""
    with np.errstate(all="ignore"):
        c = (cmin + cmax) * F(0.5)
        p = s - c
        d = np.abs(cmin - cmax) * F(0.5)
        n = (p / d) * (F(1) + F(eps))
        i = (np.where(np.isfinite(n), np.trunc(n), F(0)) + F(0)).astype(F)      # vec3(ivec3(n)): no negative zero
        dot = (i[:, 0] * i[:, 0] + i[:, 1] * i[:, 1]) + i[:, 2] * i[:, 2]
        return (i * (F(1) / np.sqrt(dot))[:, None]).astype(F)


def face_normal(s, cmin, cmax, beta):
    """The build's SVO_NORMAL_FACE (include/svo.h svo_trace_params.normal_mode) on arrays."""
    c = (cmin + cmax) * F(0.5)
    p = s - c
    a = np.abs(p)
    k = np.zeros(p.shape[0], np.int64)
    k[a[:, 1] > a[np.arange(p.shape[0]), k]] = 1
    k[a[:, 2] > a[np.arange(p.shape[0]), k]] = 2
    rows = np.arange(p.shape[0])
    pk, bk = p[rows, k], beta[rows, k]
    sgn = np.where(pk > 0, 1.0, np.where(pk < 0, -1.0, np.where(bk > 0, -1.0, 1.0))).astype(F)
    out = np.zeros_like(p)
    out[rows, k] = sgn
    return out


def cube_uv(p, cmin, cmax, eps):
    """cubeUV, shaders/Chunkmarch.glsl:138-149: the six tests in the shader's order, a later one that holds winning."""
    eps = F(eps)
    size = cmax[:, 0] - cmin[:, 0]
    uv = np.zeros((p.shape[0], 2), F)
    for axis, (a, b) in ((0, (1, 2)), (1, (0, 2)), (2, (0, 1))):
        for corner in (cmin, cmax):
            on = np.abs(p[:, axis] - corner[:, axis]) <= eps
            cand = np.stack([p[:, a] - corner[:, a], p[:, b] - corner[:, b]], axis=1)
            uv[on] = cand[on]
    return (np.abs(uv) / size[:, None]).astype(F)


def leaf_uv(p, bmin, size, material, eps):
    """leafUV, shaders/World.Fragment.glsl:5-15."""
    eps = F(eps)
    iuv = cube_uv(p, bmin, bmin + size[:, None], eps)
    nudge = (iuv < F(0.125)).astype(F) - (iuv > F(0.125)).astype(F)
    iuv = iuv + (nudge * eps) * F(2)
    m = np.asarray(material, np.uint32)
    tile = np.stack([m & 0xFF, (m >> 8) & 0xFF], axis=1).astype(F)
    return ((tile + iuv) / F(256)).astype(F)


def hit_uv(origins, dirs, records, voxels, eps):
    """[n][2] float32: what svo_hit_uv writes - leafUV where the record is a usable hit with a box, (0, 0) elsewhere."""
    g, v = np.ascontiguousarray(records).reshape(-1), np.ascontiguousarray(voxels).reshape(-1)
    on = ((g["flags"] & HIT_FLAG) != 0) & ((g["flags"] & ERR_FLAG) == 0) & ((v["flags"] & INSIDE) != 0)
    out = np.zeros((g.shape[0], 2), F)
    p = sample_points(np.broadcast_to(np.asarray(origins, F), (g.shape[0], 3))[on], np.asarray(dirs, F)[on], g["t"][on], eps)
    out[on] = leaf_uv(p, v["bmin"][on], v["size"][on], g["material"][on], eps)
    return out


def texel_index(uv, width, height):
    """GL_NEAREST with repeat wrap: x = min(int(floor((u - floor(u)) * width)), width - 1), y likewise."""
    uv = np.asarray(uv, F)
    fx = (uv[:, 0] - np.floor(uv[:, 0])) * F(width)
    fy = (uv[:, 1] - np.floor(uv[:, 1])) * F(height)
    return np.minimum(np.floor(fx).astype(np.int64), width - 1), np.minimum(np.floor(fy).astype(np.int64), height - 1)


# ---- the worlds, cameras and ray lists of the GPU tests ----------------------------------------------------------------------------
# name -> (w, h, d, chunksize, chunkcoordmin, depth of every chunk in World::index() order, golden ray list or None)
WORLDS = {
    "grid_2x1x2_d6": (2, 1, 2, 128, (0, 0, 0), [6] * 4, "grid_2x1x2_depth6.npz"),
    "grid_neg_2x2x2_d5": (2, 2, 2, 128, (-1, -1, -1), [5] * 8, "grid_neg_2x2x2_depth5.npz"),
    "mixed_6_2_4_5": (2, 1, 2, 128, (0, 0, 0), [6, 2, 4, 5], None),
    "inexact_100_d5": (2, 1, 1, 100, (0, 0, 0), [5, 5], None),           # chunk size 100: voxel corners round, the literal kernel only
}
IMAGE = (64, 48)


def make_chunks(svo, name):
    """The chunk dicts of WORLDS[name], generated on the host by the library."""
    w, h, d, cs, ccm, depths, _ = WORLDS[name]
    gen = {}
    for depth in sorted(set(depths)):
        W = svo.World.generate(w, h, d, cs, depth, chunkcoordmin=ccm)
        gen[depth] = [W.chunk(i) for i in range(w * h * d)]
        W.destroy()
    return [gen[depth][i] for i, depth in enumerate(depths)]


def cameras(svo, name):
    """Two 64 x 48 views per world: from above and in front (brick cells of the surface), and level with the ground from outside
    the front face (the cut through the terrain: LEAF nodes)."""
    w, h, d, cs, ccm, _, _ = WORLDS[name]
    lo = np.array(ccm, np.float64) * cs
    hi = lo + np.array([w, h, d], np.float64) * cs
    cx = 0.5 * (lo[0] + hi[0])
    return {"above": svo.make_camera((cx, hi[1] + 22.0, lo[2] - 40.0), (0.0, -0.5, 0.866), (0.0, 1.0, 0.0), 60.0, *IMAGE),
            "front": svo.make_camera((cx + 3.3, hi[1] - cs + 9.7, lo[2] - 30.0), (0.1, -0.05, 1.0), (0.0, 1.0, 0.0), 75.0, *IMAGE)}


def ray_list(name, n=2000):
    """(origins, dirs): the golden ray list of the world where it has one, else rays from a shell around the world towards points
    inside it (float64 directions normalised, then cast)."""
    w, h, d, cs, ccm, _, golden = WORLDS[name]
    if golden:
        z = np.load(os.path.join(GOLDEN, golden), allow_pickle=False)
        return z["origins"], z["dirs"]
    rng = np.random.default_rng(sum(name.encode()) + 4049)
    lo = np.array(ccm, np.float64) * cs
    ext = np.array([w, h, d], np.float64) * cs
    o = lo - 0.25 * ext + rng.random((n, 3)) * 1.5 * ext
    target = lo + rng.random((n, 3)) * ext * np.array([1.0, 0.3, 1.0])
    dirs = target - o
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return o.astype(F), dirs.astype(F)


L_, B_, T_ = 1 << 30, 2 << 30, 3 << 30


def handmade_chunk():
    """depth 4, 128 units.  Root -> block 9 (level 1): slot 1 (node 10) -> block 17 (level 2), slot 5 (node 14) a LEAF 3; block 17:
    slot 6 (node 23) a TWIG, slot 0 (node 17) a LEAF 2.  Block 1 is an ORPHAN that lies before both live blocks: its node 3 is a
    BRANCH word naming the live block 17, its node 4 a LEAF."""
    tree = np.zeros(25, np.uint32)
    tree[0] = B_ | 9
    tree[3], tree[4] = B_ | 17, L_ | 5
    tree[10], tree[14] = B_ | 17, L_ | 3
    tree[17], tree[23] = L_ | 2, T_ | 0
    twig = np.arange(1, 65, dtype=np.uint16)
    return dict(position=(0.0, 0.0, 0.0), size=128.0, depth=4, tree=tree, twig=twig)


def kinds(records):
    """(LEAF hits, brick-cell hits) among usable hit records."""
    g = np.ascontiguousarray(records).reshape(-1)
    on = ((g["flags"] & HIT_FLAG) != 0) & ((g["flags"] & ERR_FLAG) == 0)
    return int((on & (g["cell"] == CELL_NONE)).sum()), int((on & (g["cell"] != CELL_NONE)).sum())
