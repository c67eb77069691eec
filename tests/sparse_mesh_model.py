"""What the sparse voxeliser's tests share (svo_chunk_from_mesh / svo_world_chunk_from_mesh, include/svo.h): the cases, the model's
pools of the cases a dense grid reaches - grid_model.grid_to_pools(mesh_model.add_mesh(zeros)) - and, for the depths it does not
reach, a windowed restatement of svo_grid_add_mesh's rule: the same arithmetic as mesh_model.add_mesh, written into sub-arrays
("windows") of the conceptual N^3 grid, every triangle's clamped cell box asserted to lie in one of them.  Test infrastructure."""
import numpy as np

import grid_model as G
import mesh_model as M


def zeros(depth):
    n = 1 << depth
    return np.zeros((n, n, n), np.uint16)


def mesh(v, ix, **kw):
    """One entry of a mesh list: the keyword arguments of mesh_model.add_mesh (origin, cell, material, materials)."""
    return dict(vertices=v, indices=ix, **kw)


def add_kw(m):
    return {k: m[k] for k in ("origin", "cell", "material", "materials") if k in m}


def model_pools(depth, meshes):
    """The definition at a depth the dense model reaches: every mesh added to one cleared grid, then the tree of that grid."""
    g = zeros(depth)
    for m in meshes:
        M.add_mesh(g, m["vertices"], m["indices"], **add_kw(m))
    c = G.chunk_of(g)
    return c, g


# ---- the windowed rule ---------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def add_mesh_windows(windows, n, vertices, indices, origin=(0.0, 0.0, 0.0), cell=1.0, material=1, materials=None):
    """mesh_model.add_mesh in float32 on the conceptual grid of n cells per axis, of which only `windows` exist: a list of
    ((x0, y0, z0), [z, y, x] uint16 array) - the array holds the cells from that corner on.  Raised in place.  Asserts that the clamped
    cell box of every triangle that is not dropped lies inside one window: no cell outside the windows can be marked."""
    T = np.float32
    V = np.asarray(vertices, np.float32).reshape(-1, 3)
    I = np.asarray(indices, np.uint32).reshape(-1, 3)
    org = np.asarray(origin, np.float32)
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
            nrm = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], T)
            if (nrm == 0).all() or m == 0:
                continue
            lo = np.minimum(np.minimum(v[0], v[1]), v[2])
            hi = np.maximum(np.maximum(v[0], v[1]), v[2])
            c0 = [max(0, int(np.floor(float(lo[k]))) - 1) for k in range(3)]
            c1 = [min(n - 1, int(np.floor(float(hi[k])))) for k in range(3)]
            if any(c0[k] > c1[k] for k in range(3)):
                continue
            home = [(w0, arr) for w0, arr in windows
                    if all(w0[k] <= c0[k] and c1[k] < w0[k] + arr.shape[2 - k] for k in range(3))]
            assert home, f"triangle {t}: its cell box {c0} .. {c1} lies in no window"
            w0, arr = home[0]
            P = [np.arange(c0[0], c1[0] + 1).astype(T)[None, None, :], np.arange(c0[1], c1[1] + 1).astype(T)[None, :, None],
                 np.arange(c0[2], c1[2] + 1).astype(T)[:, None, None]]
            ok = np.ones((P[2].size, P[1].size, P[0].size), bool)
            for k in range(3):
                ok &= (P[k] <= hi[k]) & (P[k] + one >= lo[k])
            c = np.where(nrm > 0, one, zero).astype(T)
            d1 = _dot(c - v[0], nrm)
            d2 = _dot((one - c) - v[0], nrm)
            q = _dot(P, nrm)
            ok &= (q + d1) * (q + d2) <= 0
            for i, j, w in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
                s = one if nrm[w] >= 0 else -one
                for k in range(3):
                    ea = -e[k][j] * s
                    eb = e[k][i] * s
                    de = ((-(ea * v[k][i] + eb * v[k][j])) + (ea if ea > 0 else zero)) + (eb if eb > 0 else zero)
                    ok &= (ea * P[i] + eb * P[j]) + de >= 0
            sub = arr[c0[2] - w0[2]:c1[2] + 1 - w0[2], c0[1] - w0[1]:c1[1] + 1 - w0[1], c0[0] - w0[0]:c1[0] + 1 - w0[0]]
            sub[ok & (sub < m)] = m
    return windows


def occupied_cells(chunk) -> int:
    """How many finest voxels of the chunk are not empty: LEAF volumes and the non-zero cells of the bricks, from the root."""
    tree, twig = chunk["tree"], chunk["twig"]
    total, stack = 0, [(0, 1 << int(chunk["depth"]))]
    while stack:
        i, e = stack.pop()
        w = int(tree[i])
        kind, off = w >> 30, w & 0x3FFFFFFF
        if kind == G.LEAF:
            total += e ** 3
        elif kind == G.TWIG:
            total += int(np.count_nonzero(twig[off * 64:off * 64 + 64])) * (e // 4) ** 3
        elif kind == G.BRANCH:
            stack.extend((off + c, e // 2) for c in range(8))
    return total


def check_against_windows(chunk, windows):
    """Every cell of every window read back from the pools with grid_model.voxel_material, and nothing occupied outside them."""
    for w0, arr in windows:
        got = np.zeros_like(arr)
        for z in range(arr.shape[0]):
            for y in range(arr.shape[1]):
                for x in range(arr.shape[2]):
                    got[z, y, x] = G.voxel_material(chunk, w0[0] + x, w0[1] + y, w0[2] + z)
        bad = np.argwhere(got != arr)
        assert bad.size == 0, f"window at {w0}: {bad.shape[0]} cells differ, first [z, y, x] {bad[:4].tolist()}"
    assert occupied_cells(chunk) == sum(int(np.count_nonzero(arr)) for _, arr in windows), "cells outside the windows are occupied"


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def slab_fill(lo, hi, material):
    """Axis-aligned quads in the lattice planes z = lo + 1, lo + 3, .. of the box [lo, hi) (cells, per axis; an even number of layers):
    the closed rule marks both neighbouring layers of every quad, and the quads end a quarter cell inside the box in x and y, so exactly
    the cells of the box are marked.  One mesh entry."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    assert (z1 - z0) % 2 == 0
    vs, ix = [], []
    for z in range(z0 + 1, z1, 2):
        b = len(vs)
        vs += [(x0 + 0.25, y0 + 0.25, z), (x1 - 0.25, y0 + 0.25, z), (x1 - 0.25, y1 - 0.25, z), (x0 + 0.25, y1 - 0.25, z)]
        ix += [(b, b + 1, b + 2), (b, b + 2, b + 3)]
    return mesh(np.array(vs, np.float32), np.array(ix, np.uint32), material=material)


def tiny_triangle(cell, material):
    """A triangle well inside the cell (x, y, z): it marks that cell alone."""
    c = np.asarray(cell, np.float64)
    v = (c + np.array([[0.3, 0.3, 0.3], [0.6, 0.4, 0.35], [0.4, 0.7, 0.5]])).astype(np.float32)
    return mesh(v, np.array([(0, 1, 2)], np.uint32), material=material)


def collapse_cases():
    """name -> (depth, meshes, check(tree, twig)): check asserts, on the model's pools, that the node the case is about is there."""
    kind = lambda w: int(w) >> 30
    off = lambda w: int(w) & 0x3FFFFFFF

    def root_leaf(m):
        def check(tree, twig):
            assert tree.tolist() == [G.node(G.LEAF, m)] and twig.size == 0
        return check

    def leaf_above_bricks(tree, twig):                      # depth 4: the 8^3 node (x 8, y 0, z 8) is child 1 + 4 of the root
        assert kind(tree[0]) == G.BRANCH and off(tree[0]) == 1 and int(tree[1 + 5]) == G.node(G.LEAF, 300)
        assert [kind(w) for w in tree[1:9]].count(G.EMPTY) == 7 and tree.size == 9 and twig.size == 0

    def twig_with(values):
        def check(tree, twig):                              # depth 3: the block (4, 4, 4) is child 7 of the root
            assert kind(tree[0]) == G.BRANCH and kind(tree[8]) == G.TWIG and off(tree[8]) == 0 and twig.size == 64
            assert sorted(np.unique(twig, return_counts=True)[1].tolist()) == sorted(values.values())
            assert {int(k) for k in np.unique(twig)} == set(values)
        return check

    return {
        "depth2_full": (2, [slab_fill((0, 0, 0), (4, 4, 4), 7)], root_leaf(7)),
        "depth3_full": (3, [slab_fill((0, 0, 0), (8, 8, 8), 0xFFFF)], root_leaf(0xFFFF)),
        "leaf_above_bricks": (4, [slab_fill((8, 0, 8), (16, 8, 16), 300)], leaf_above_bricks),
        "full_block_one_other_cell": (3, [slab_fill((4, 4, 4), (8, 8, 8), 3), tiny_triangle((5, 6, 5), 9)], twig_with({3: 63, 9: 1})),
        "full_block_two_materials": (3, [slab_fill((4, 4, 4), (8, 8, 6), 3), slab_fill((4, 4, 6), (8, 8, 8), 5)], twig_with({3: 32, 5: 32})),
    }


def deep_cases():
    """name -> (depth, meshes, windows as (corner, shape)) beyond the dense grid's reach: per depth a sphere of about 24 cells radius
    far from the origin, and two tiny triangles in the grid's first and last cell."""
    out = {}
    for depth, origin, cell in ((12, (0.0, 0.0, 0.0), 1.0), (16, (10.0, -20.0, 30.0), 0.25)):
        n = 1 << depth
        centre = np.array([0.73 * n + 0.3, 0.71 * n + 0.7, 0.76 * n + 0.1])
        v, ix = M.uv_sphere(np.asarray(origin) + centre * cell, 24.0 * cell)
        corner = tuple(int(c) - 28 for c in centre)
        out[f"sphere{depth}"] = (depth, [mesh(v, ix, origin=origin, cell=cell, material=6)], [(corner, (56, 56, 56))])
        ends = [tiny_triangle((n - 1, n - 1, n - 1), 0xFFFF), tiny_triangle((0, 0, 0), 2)]
        out[f"ends{depth}"] = (depth, ends, [((0, 0, 0), (4, 4, 4)), ((n - 4, n - 4, n - 4), (4, 4, 4))])
    return out


_deep = {}


def deep_windows(name):
    """The windowed model of a deep case, computed once: [(corner, array)]; callers leave them unchanged."""
    if name not in _deep:
        depth, meshes, wins = deep_cases()[name]
        windows = [(c, np.zeros(shape, np.uint16)) for c, shape in wins]
        for m in meshes:
            add_mesh_windows(windows, 1 << depth, m["vertices"], m["indices"], **add_kw(m))
        for _, arr in windows:
            arr.setflags(write=False)
        _deep[name] = windows
    return _deep[name]


def shared_cases():
    """name -> (depth, meshes) of every case a dense grid reaches, which the CPU and the GPU tests share."""
    out = {name: (depth, [mesh(v, ix, **kw)]) for name, (depth, v, ix, kw) in M.cases().items()}
    s, t = M.cases()["sphere5"], M.cases()["torus5"]
    out["two_meshes"] = (5, [mesh(s[1], s[2], material=3), mesh(t[1], t[2], material=9, origin=(0.5, -0.25, 1.0), cell=1.25)])
    tri = np.array([[3.3, 2.2, 3.1], [10.6, 4.4, 9.7], [6.9, 12.8, 5.2]], np.float32)
    mats = np.random.default_rng(4).permutation(64).astype(np.uint16) + 1
    out["coincident"] = (4, [mesh(np.tile(tri, (64, 1)), np.arange(192, dtype=np.uint32).reshape(64, 3), materials=mats)])
    for name, (depth, meshes, _) in collapse_cases().items():
        out[name] = (depth, meshes)
    return out


_pools = {}


def case_pools(name):
    """The model's chunk of a shared case (computed once, left unchanged)."""
    if name not in _pools:
        depth, meshes = shared_cases()[name]
        c, _ = model_pools(depth, meshes)
        c["tree"].setflags(write=False)
        c["twig"].setflags(write=False)
        _pools[name] = c
    return _pools[name]


def dropped_mesh():
    """A mesh whose every triangle is dropped or writes nothing: a bad index, a NaN vertex, a zero normal, material 0."""
    v = np.array([[2, 2, 2], [9, 3, 4], [4, 10, 6], [float("nan"), 5, 5], [3, 3, 3], [4, 4, 4], [5, 5, 5]], np.float32)
    ix = np.array([(0, 1, 7), (0, 1, 3), (4, 5, 6), (0, 1, 2)], np.uint32)
    return mesh(v, ix, materials=np.array([5, 5, 5, 0], np.uint16))
