"""The model of svo_grid_add_mesh / svo_grid_fill_enclosed, written from include/svo.h in numpy: every triangle's clamped cell box is
visited, every operation is a separately rounded float32 operation in the header's order (dtype=np.float64 evaluates the same rule in
double, for the property check), the fill is a breadth-first flood.  Also the meshes the tests share.

The meshes keep their coordinates at magnitudes (1e-3 .. 1e3, no two vertices closer than 1e-6) at which no intermediate of the rule
is subnormal: products of two differences stay above 1e-12, far from 1.2e-38."""
import numpy as np


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def add_mesh(grid, vertices, indices, origin=(0.0, 0.0, 0.0), cell=1.0, material=1, materials=None, dtype=np.float32):
    """grid ([z, y, x] uint16) raised in place by the rule; returns it."""
    T = dtype
    N = grid.shape[0]
    V = np.asarray(vertices, np.float32).reshape(-1, 3).astype(T)
    I = np.asarray(indices, np.uint32).reshape(-1, 3)
    org = np.asarray(origin, np.float32).astype(T)
    inv = T(1.0) / T(np.float32(cell))
    one, zero = T(1.0), T(0.0)
    with np.errstate(all="ignore"):
        for t in range(I.shape[0]):
            m = int(material if materials is None else materials[t])
            if (I[t] >= V.shape[0]).any():
                continue
            v = [(V[int(i)] - org) * inv for i in I[t]]
            if not all(np.isfinite(p).all() for p in v):
                continue
            e = [v[1] - v[0], v[2] - v[1], v[0] - v[2]]
            a, b = e[0], e[1]
            n = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], T)
            if (n == 0).all() or m == 0:
                continue
            lo = np.minimum(np.minimum(v[0], v[1]), v[2])
            hi = np.maximum(np.maximum(v[0], v[1]), v[2])
            # the clamped cell box: p <= hi and p + 1 >= lo, in exact integers
            c0 = [max(0, int(np.floor(float(lo[k]))) - 1) for k in range(3)]
            c1 = [min(N - 1, int(np.floor(float(hi[k])))) for k in range(3)]
            if any(c0[k] > c1[k] for k in range(3)):
                continue
            P = [np.arange(c0[0], c1[0] + 1).astype(T)[None, None, :], np.arange(c0[1], c1[1] + 1).astype(T)[None, :, None],
                 np.arange(c0[2], c1[2] + 1).astype(T)[:, None, None]]
            ok = np.ones((P[2].size, P[1].size, P[0].size), bool)
            for k in range(3):
                ok &= (P[k] <= hi[k]) & (P[k] + one >= lo[k])
            c = np.where(n > 0, one, zero).astype(T)
            d1 = _dot(c - v[0], n)
            d2 = _dot((one - c) - v[0], n)
            q = _dot(P, n)
            ok &= (q + d1) * (q + d2) <= 0
            for i, j, w in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
                s = one if n[w] >= 0 else -one
                for k in range(3):
                    ea = -e[k][j] * s
                    eb = e[k][i] * s
                    de = ((-(ea * v[k][i] + eb * v[k][j])) + (ea if ea > 0 else zero)) + (eb if eb > 0 else zero)
                    ok &= (ea * P[i] + eb * P[j]) + de >= 0
            sub = grid[c0[2]:c1[2] + 1, c0[1]:c1[1] + 1, c0[0]:c1[0] + 1]
            sub[ok & (sub < m)] = m
    return grid


def outside_of(grid):
    """The empty cells a path of 6-neighbour steps through empty cells connects to an empty cell on one of the grid's faces."""
    empty = grid == 0
    face = np.zeros_like(empty)
    face[0], face[-1], face[:, 0], face[:, -1], face[:, :, 0], face[:, :, -1] = (True,) * 6
    outside = empty & face
    front = outside
    while front.any():
        nxt = np.zeros_like(front)
        nxt[1:] |= front[:-1]; nxt[:-1] |= front[1:]
        nxt[:, 1:] |= front[:, :-1]; nxt[:, :-1] |= front[:, 1:]
        nxt[:, :, 1:] |= front[:, :, :-1]; nxt[:, :, :-1] |= front[:, :, 1:]
        front = nxt & empty & ~outside
        outside = outside | front
    return outside


def fill_enclosed(grid, material):
    """grid filled in place; returns how many cells."""
    inside = (grid == 0) & ~outside_of(grid)
    grid[inside] = material
    return int(inside.sum())


def reaches_face(grid, start):
    """Does a flood through the empty cells from the [z, y, x] cell `start` reach one of the grid's faces?"""
    assert grid[start] == 0
    return bool(outside_of(grid)[start])


# ---- meshes: (vertices [nv, 3] float32, indices [nt, 3] uint32) ----------------------------------------------------------------
def uv_sphere(centre, radius, nu=12, nv=8):
    """nu meridians, nv parallels' bands: 2 * nu * (nv - 1) triangles (12 x 8: 168), watertight."""
    verts = [(0.0, 0.0, 1.0)]
    for r in range(1, nv):
        th = np.pi * r / nv
        for k in range(nu):
            ph = 2 * np.pi * k / nu
            verts.append((np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)))
    verts.append((0.0, 0.0, -1.0))
    ring = lambda r, k: 1 + (r - 1) * nu + k % nu
    tris = [(0, ring(1, k), ring(1, k + 1)) for k in range(nu)]
    for r in range(1, nv - 1):
        for k in range(nu):
            tris += [(ring(r, k), ring(r + 1, k), ring(r + 1, k + 1)), (ring(r, k), ring(r + 1, k + 1), ring(r, k + 1))]
    tris += [(len(verts) - 1, ring(nv - 1, k + 1), ring(nv - 1, k)) for k in range(nu)]
    v = (np.asarray(centre, np.float64) + radius * np.asarray(verts, np.float64)).astype(np.float32)
    return v, np.asarray(tris, np.uint32)


def torus(centre, major, minor, nu=16, nv=8):
    verts = []
    for a in range(nu):
        for b in range(nv):
            u, w = 2 * np.pi * a / nu, 2 * np.pi * b / nv
            verts.append(((major + minor * np.cos(w)) * np.cos(u), minor * np.sin(w), (major + minor * np.cos(w)) * np.sin(u)))
    at = lambda a, b: (a % nu) * nv + b % nv
    tris = []
    for a in range(nu):
        for b in range(nv):
            tris += [(at(a, b), at(a + 1, b), at(a + 1, b + 1)), (at(a, b), at(a + 1, b + 1), at(a, b + 1))]
    return (np.asarray(centre, np.float64) + np.asarray(verts, np.float64)).astype(np.float32), np.asarray(tris, np.uint32)


def box_mesh(lo, hi):
    """The 12 triangles of the axis-aligned box [lo, hi]."""
    lo, hi = np.broadcast_to(np.asarray(lo, np.float32), 3), np.broadcast_to(np.asarray(hi, np.float32), 3)
    v = np.array([[(lo, hi)[(c >> k) & 1][k] for k in range(3)] for c in range(8)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return v, np.asarray(tris, np.uint32)


def lattice_cube():
    """Corners at cells 4 and 8: every face lies in a lattice plane."""
    return box_mesh(4.0, 8.0)


def soup(seed, count, n, small=0.0):
    """`count` seeded random triangles around a grid of n cells per axis (cell 1, origin 0): centres from -0.2 n to 1.2 n, some of
    them outside; extents up to n / 3, or below `small` cells when that is given.  Returns vertices, indices and materials (1 .. 999)."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-0.2 * n, 1.2 * n, (count, 1, 3))
    ext = small if small else rng.uniform(0.05, n / 3, (count, 1, 1))
    v = (centre + rng.uniform(-0.5, 0.5, (count, 3, 3)) * ext).astype(np.float32).reshape(-1, 3)
    return v, np.arange(3 * count, dtype=np.uint32).reshape(-1, 3), rng.integers(1, 1000, count).astype(np.uint16)


def concat(*meshes):
    """Meshes (vertices, indices[, materials]) as one, in order."""
    vs, ix, base = [], [], 0
    for m in meshes:
        vs.append(m[0]); ix.append(m[1] + np.uint32(base)); base += m[0].shape[0]
    return np.concatenate(vs), np.concatenate(ix)


def sphere_case(depth, origin=(0.0, 0.0, 0.0), cell=1.0):
    """The sphere that fills most of a grid of that depth, frame (origin, cell): (vertices, indices)."""
    n = 1 << depth
    o = np.asarray(origin, np.float64)
    return uv_sphere(o + 0.5 * n * cell + np.array([0.13, -0.21, 0.07]) * cell, 0.39 * n * cell)


_CASES, _MODEL = {}, {}


def cases():
    """The voxelisation cases the CPU and the GPU tests share: name -> (depth, vertices, indices, keyword arguments of add_mesh)."""
    if not _CASES:
        off, fine = (99.9, 0.1, -9.9), 0.2
        _CASES["sphere5"] = (5, *sphere_case(5), {})
        _CASES["sphere5_off"] = (5, *sphere_case(5, off, fine), dict(origin=off, cell=fine))
        _CASES["sphere4"] = (4, *sphere_case(4), {})
        _CASES["torus5"] = (5, *torus((16.2, 15.7, 16.4), 9.3, 3.1), dict(material=7))
        for d in (2, 5):
            v, ix, m = soup(7, 60, 1 << d)
            _CASES[f"soup{d}"] = (d, v, ix, dict(materials=m))
        _CASES["lattice_cube"] = (4, *lattice_cube(), dict(material=2))
    return _CASES


def model_grid(name):
    """The model's grid of a case (computed once; callers copy before they write)."""
    if name not in _MODEL:
        depth, v, ix, kw = cases()[name]
        n = 1 << depth
        _MODEL[name] = add_mesh(np.zeros((n, n, n), np.uint16), v, ix, **kw)
        _MODEL[name].setflags(write=False)
    return _MODEL[name]


def nested_shells():
    """Two nested spherical shells at depth 5, materials 4 (outer) and 6 (inner): the gap between them and the core are enclosed."""
    g = np.zeros((32, 32, 32), np.uint16)
    add_mesh(g, *uv_sphere((16.1, 15.9, 16.2), 13.0), material=4)
    add_mesh(g, *uv_sphere((16.1, 15.9, 16.2), 6.0), material=6)
    return g


def fill_cases():
    """The fill cases the CPU and the GPU tests share: name -> grid (callers copy)."""
    shell = model_grid("sphere5").copy()
    holed = shell.copy()
    outside = outside_of(shell)

    def beside(mask):
        out = np.zeros_like(mask)
        out[1:] |= mask[:-1]; out[:-1] |= mask[1:]
        out[:, 1:] |= mask[:, :-1]; out[:, :-1] |= mask[:, 1:]
        out[:, :, 1:] |= mask[:, :, :-1]; out[:, :, :-1] |= mask[:, :, 1:]
        return out

    thin = (shell != 0) & beside(outside) & beside((shell == 0) & ~outside)      # shell cells between the outside and the inside
    holed[tuple(np.argwhere(thin)[0])] = 0                  # one of them removed opens the shell
    full = np.full((8, 8, 8), 5, np.uint16)
    d2 = np.full((4, 4, 4), 9, np.uint16)
    d2[1:3, 1:3, 1:3] = 0                                   # depth 2: the 8 inner cells, enclosed
    d2[2, 2, 2] = 1
    return {"shell": shell, "holed": holed, "nested": nested_shells(), "full": full, "empty": np.zeros((8, 8, 8), np.uint16), "depth2": d2}


def serpentine(depth=5, block=16, at=4, sealed=False, along=0):
    """A grid with a block^3 cube of material 3 at cell `at` per axis and a corridor one cell wide winding through it: rows of
    block - 2 cells along axis `along` (0 = x, 1 = y, 2 = z), every other row of every other layer, joined at alternating ends through
    the wall between them.  No two cells of the corridor touch except along it.  Its mouth is in the cube's face at the low end of
    `along`: open to the grid's empty space, or - `sealed` - behind a plug.  Returns (grid, the corridor's cells in order as [z, y, x]
    index tuples)."""
    n = 1 << depth
    g = np.zeros((n, n, n), np.uint16)
    g[at:at + block, at:at + block, at:at + block] = 3
    rows = list(range(1, block - 1, 2))
    cells, a = [(0, rows[0], rows[0])], 1                    # (a, b, c): along the row, across the rows, across the layers; the mouth
    for li, c in enumerate(rows):
        order = rows if li % 2 == 0 else rows[::-1]
        for ri, b in enumerate(order):
            end = block - 2 if a == 1 else 1
            cells += [(k, b, c) for k in range(a, end + (1 if end > a else -1), 1 if end > a else -1)]
            a = end
            if ri + 1 < len(order):
                cells.append((a, (b + order[ri + 1]) // 2, c))
        if li + 1 < len(rows):
            cells.append((a, order[-1], c + 1))
    perm = {0: (0, 1, 2), 1: (1, 2, 0), 2: (2, 0, 1)}[along]  # where a, b, c go in (x, y, z)
    path = []
    for cell in cells:
        xyz = [0, 0, 0]
        for k in range(3):
            xyz[perm[k]] = at + cell[k]
        path.append((xyz[2], xyz[1], xyz[0]))
    for zyx in path:
        g[zyx] = 0
    if sealed:
        plug = list(path[0]); plug[2 - perm[0]] -= 1
        g[tuple(plug)] = 3
    return g, path
