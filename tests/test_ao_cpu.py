"""svo_hit_ao / svo_shade_ao without a device: the C ABI surface, the argument checks that are settled before any device work, the host
model (tests/ao_model.py) on hand-made worlds with every expected float written out, and - with the CPU oracle - the input
conditions the GPU tests of tests/test_ao.py rest on.  CPU only."""
import os
import re
import subprocess

import numpy as np
import pytest

import ao_model as M
import hit_voxels_model as H
import locate_model as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_new_symbols_are_declared_and_exported(svo):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svo.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+svo_hit_ao\s*\(\s*svo_world\s*\*\s*,\s*const svo_camera\s*\*\s*cam\s*,\s*const svo_trace_params\s*\*\s*params\s*,\s*float cell\s*,"
                     r"\s*int x0\s*,\s*int y0\s*,\s*int w\s*,\s*int h\s*,\s*const svo_hit\s*\*\s*gbuffer_dev\s*,\s*const svo_voxel\s*\*\s*voxels_dev\s*,"
                     r"\s*float\s*\*\s*ao_dev\s*,\s*void\s*\*\s*stream\s*\)", header)
    assert re.search(r"\bint\s+svo_shade_ao\s*\(\s*const float\s*\*\s*ao_dev\s*,\s*float strength\s*,\s*int64_t n\s*,\s*float\s*\*\s*rgba_dev\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", header)
    out = subprocess.run(["nm", "-D", "--defined-only", svo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("svo_hit_ao", "svo_shade_ao"):
        assert name in svo.ABI_SYMBOLS and hasattr(svo.lib, name)
        assert re.search(rf" T {name}$", out, flags=re.M)
    assert "#define SVO_ABI_VERSION 4" in header and svo.lib.svo_abi_version() == 4     # functions added, nothing changed


def test_argument_checks_precede_any_device_work(svo):
    W = svo.World.create([dict(position=(0, 0, 0), size=128.0, depth=4, tree=np.array([(1 << 30) | 6], np.uint32), twig=np.zeros(0, np.uint16))], 1, 1, 1, 128)
    fake = 256                                                  # never dereferenced: every call below fails before device work
    cam = svo.default_camera(1, 1, 128, 16, 16)
    rect = (0, 0, 16, 16)

    def code(fn, *args, **kw):
        with pytest.raises(svo.SvoError) as e:
            fn(*args, **kw)
        return e.value.code

    prm = svo.trace_params()
    # bad arguments first (the world is not resident: -5 would show a check out of order)
    assert svo.lib.svo_hit_ao(None, cam, prm, 0.0, 0, 0, 16, 16, fake, fake, fake, None) == -1
    assert code(W.hit_ao, None, prm, rect, fake, fake, fake) == -1
    assert code(W.hit_ao, cam, prm, rect, None, fake, fake) == -1
    assert code(W.hit_ao, cam, prm, rect, fake, None, fake) == -1
    assert code(W.hit_ao, cam, prm, rect, fake, fake, None) == -1
    for bad in ((-1, 0, 16, 16), (0, -1, 16, 16), (0, 0, -1, 16), (0, 0, 16, -1)):
        assert code(W.hit_ao, cam, prm, bad, fake, fake, fake) == -1
    for cell in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert code(W.hit_ao, cam, prm, rect, fake, fake, fake, cell=cell) == -1
    assert code(W.hit_ao, cam, svo.trace_params(see_through=0x10000), rect, fake, fake, fake) == -1
    assert code(W.hit_ao, cam, svo.trace_params(semantics=2), rect, fake, fake, fake) == -1
    assert code(W.hit_ao, cam, svo.trace_params(kernel=3), rect, fake, fake, fake) == -1
    # then the residency - also for an empty rectangle and for params == NULL
    assert code(W.hit_ao, cam, prm, rect, fake, fake, fake) == -5
    assert code(W.hit_ao, cam, None, rect, fake, fake, fake, cell=2.0) == -5
    assert code(W.hit_ao, cam, prm, (0, 0, 0, 16), None, None, None) == -5
    W.destroy()
    # svo_shade_ao takes no world
    for strength in (-0.25, 1.5, float("nan"), float("inf")):
        assert code(svo.shade_ao, fake, strength, 8, fake) == -1
    assert code(svo.shade_ao, fake, 0.5, -1, fake) == -1
    assert code(svo.shade_ao, None, 0.5, 8, fake) == -1
    assert code(svo.shade_ao, fake, 0.5, 8, None) == -1
    svo.shade_ao(None, 0.5, 0, None)                            # n == 0 launches nothing
    assert code(svo.shade_ao, fake, 0.5, 1 << 40, fake) == -6   # a grid that does not fit one launch, behind the argument check


# ---- (a) hand-made worlds, every expected float written out --------------------------------------------------------------------------
# One 128-unit chunk of depth 5 (voxels of 4): a floor of 8 voxel layers, y in [0, 32) - folded by the builder into LEAF nodes of 32 -
# and solid cells of material 2 on it, given as (x, y, z) cell ranges.
def floor_world(svo, blocks=()):
    g = np.zeros((32, 32, 32), np.uint16)                       # [z, y, x]
    g[:, :8, :] = 1
    for (x0, x1), (y0, y1), (z0, z1) in blocks:
        g[z0:z1, y0:y1, x0:x1] = 2
    c = svo.chunk_from_grid(g, (0.0, 0.0, 0.0), 128.0)
    assert c["depth"] == 5
    return [c], L.world_of([c], 1, 1, 1, 128)


def one_pixel(svo, chunks, twin, eye, forward, up, t, inside, cell=0.0, occupancy=None):
    """The model on ONE pixel: a 1 x 1 image whose ray is exactly `forward` (an axis), the record a hit at distance t, the voxel record
    what locate_one finds at `inside`, a point of the voxel that was hit.  -> (ao, detail)."""
    cam = svo.make_camera(eye, forward, up, 60.0, 1, 1)
    assert np.array_equal(H.camera_dirs(cam)[0], np.array(forward, F))
    g = np.zeros(1, H.HIT_DTYPE)
    g[0] = (t, (0, 0, 0), 1, H.HIT_FLAG, 0, 0, H.CELL_NONE)
    v = np.zeros(1, H.VOXEL_DTYPE)
    r = L.locate_one(twin, inside)
    v[0] = (np.array(r[0], F), r[1], r[2], r[3], r[4], r[5], r[6])
    detail = {}
    ao = M.hit_ao(chunks, 128, cam, None, g, v, occupancy or M.TwinOccupancy(twin), cell=cell, detail=detail)
    detail["voxel"] = v[0]
    return ao[0], detail


def down(svo, chunks, twin, x, z, top=32.0, **kw):
    """Straight down from y = 100 onto the face y = top: P = (x, top + eps, z) exactly."""
    return one_pixel(svo, chunks, twin, (x, 100.0, z), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), 100.0 - top, (x, top - 0.25, z), **kw)


def test_a_flat_floor_is_open(svo):
    chunks, twin = floor_world(svo)
    for x, z in ((50.3, 61.7), (40.0, 48.0), (2.0, 2.0), (127.5, 0.25)):
        ao, d = down(svo, chunks, twin, x, z)
        assert d["on"][0] and not d["occ"].any() and ao == F(1.0) and d["voxel"]["size"] == 32.0


def test_one_wall_beside_the_hit(svo):
    """A block of 2 x 2 x 1 cells on the floor, x in [32, 40), y in [32, 40), z in [48, 52); the floor beside it, on its +x side, is a LEAF
    node of 32 shaded on the lattice of 4: the open cell's neighbour (-1, 0) is the wall, s1 = 1 for the two corners towards it."""
    chunks, twin = floor_world(svo, [((8, 10), (8, 10), (12, 13))])
    two_thirds = F(2) / F(3)
    # at the corner on the wall's side, f_u = 0: 2/3
    ao, d = down(svo, chunks, twin, 40.0, 50.0)
    assert d["voxel"]["size"] == 32.0 and d["voxel"]["cell"] == H.CELL_NONE        # a LEAF face of a large node ...
    assert np.array_equal(d["N"][0, 3], np.array([38.0, 34.0, 50.0], F))           # ... on the finest lattice: the cell of 4 beside the hit
    assert list(d["occ"][0]) == [False, False, False, True, False, False, False, False]
    assert d["fu"][0] == 0.0 and d["fv"][0] == 0.5 and ao == two_thirds
    # at f_u = 0.25 (x = 41): 2/3 + (1 - 2/3) * 0.25 on both rows
    ao, d = down(svo, chunks, twin, 41.0, 50.0)
    assert d["fu"][0] == 0.25 and ao == two_thirds + (F(1) - two_thirds) * F(0.25)
    # the far corner, f_u -> 1: the wall's share fades
    ao, d = down(svo, chunks, twin, 43.5, 50.0)
    assert d["fu"][0] == 0.875 and ao == two_thirds + (F(1) - two_thirds) * F(0.875)
    # one cell further out nothing is near
    assert down(svo, chunks, twin, 45.0, 50.0)[0] == F(1.0)
    # diagonal to the block only the corner cell is solid: level 2 at that corner alone, f = (0.25, 0.75) from it
    ao, d = down(svo, chunks, twin, 41.0, 55.0)
    assert list(np.nonzero(d["occ"][0])[0]) == [0] and d["fu"][0] == 0.25 and d["fv"][0] == 0.75
    l0 = two_thirds + (F(1) - two_thirds) * F(0.25)
    assert ao == l0 + (F(1) - l0) * F(0.75)
    # cell = 8 beside a block of 2 x 2 x 2 cells, z in [48, 56): the lattice of 8 - Q = (44, 36, 52), the block is its neighbour (-1, 0),
    # f_u = 41 / 8 - 5 = 0.125; on the lattice of 4 the block fills the cells (-1, 0) and (-1, 1): levels 2 and 1 towards it
    chunks, twin = floor_world(svo, [((8, 10), (8, 10), (12, 14))])
    ao, d = down(svo, chunks, twin, 41.0, 50.0)
    assert list(np.nonzero(d["occ"][0])[0]) == [3, 5] and d["fu"][0] == 0.25 and d["fv"][0] == 0.5
    l0, l1 = two_thirds + (F(1) - two_thirds) * F(0.25), F(1) / F(3) + (F(1) - F(1) / F(3)) * F(0.25)
    assert ao == l0 + (l1 - l0) * F(0.5)
    ao, d = down(svo, chunks, twin, 41.0, 50.0, cell=8.0)
    assert np.array_equal(d["N"][0, 3], np.array([36.0, 36.0, 52.0], F)) and list(np.nonzero(d["occ"][0])[0]) == [3]
    assert d["fu"][0] == 0.125 and d["fv"][0] == 0.25 and ao == two_thirds + (F(1) - two_thirds) * F(0.125)
    # cell = 64: every neighbour is far from the block, or outside the world
    assert down(svo, chunks, twin, 41.0, 50.0, cell=64.0)[0] == F(1.0)


def test_two_sides_close_the_corner_whatever_it_holds(svo):
    """Walls at (-1, 0) and (0, -1) of the open cell x in [40, 44), z in [56, 60): corner (-1, -1) has level 0 with the corner cell
    solid and with it empty."""
    third, two_thirds = F(1) / F(3), F(2) / F(3)
    assert third == F(0.33333334) and two_thirds == F(0.6666667)
    for corner_cell in (True, False):
        blocks = [((9, 10), (8, 9), (14, 15)), ((10, 11), (8, 9), (13, 14))] + ([((9, 10), (8, 9), (13, 14))] if corner_cell else [])
        chunks, twin = floor_world(svo, blocks)
        ao, d = down(svo, chunks, twin, 40.0, 56.0)
        assert list(np.nonzero(d["occ"][0])[0]) == ([0, 1, 3] if corner_cell else [1, 3])
        assert d["fu"][0] == 0.0 and d["fv"][0] == 0.0 and ao == F(0.0)
        lv = M.corner_levels(d["occ"])
        assert [int(lv[c][0]) for c in ((-1, -1), (1, -1), (-1, 1), (1, 1))] == [0, 2, 2, 3]
        # the middle of the cell: l0 = 0 + (2/3 - 0) / 2, l1 = 2/3 + (1 - 2/3) / 2, ao = l0 + (l1 - l0) / 2
        ao, d = down(svo, chunks, twin, 42.0, 58.0)
        l0, l1 = two_thirds * F(0.5), two_thirds + (F(1) - two_thirds) * F(0.5)
        assert ao == l0 + (l1 - l0) * F(0.5) and abs(float(ao) - 7.0 / 12.0) < 1e-6
    # a pit one cell wide and deep: all four corners closed, exactly 0 wherever the point lies
    chunks, twin = floor_world(svo, [((9, 12), (8, 9), (13, 14)), ((9, 12), (8, 9), (15, 16)), ((9, 10), (8, 9), (14, 15)), ((11, 12), (8, 9), (14, 15))])
    ao, d = down(svo, chunks, twin, 41.3, 57.9)
    assert d["occ"].all() and ao == F(0.0)


def test_a_face_on_the_worlds_boundary_is_open(svo):
    """Along +x onto the floor's side at x = 0: P and the open cell lie outside the world, so do all eight neighbours."""
    chunks, twin = floor_world(svo, [((0, 1), (8, 10), (0, 32))])
    occ = M.TwinOccupancy(twin)
    ao, d = one_pixel(svo, chunks, twin, (-50.0, 10.0, 50.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 50.0, (0.25, 10.0, 50.0), occupancy=occ)
    assert d["on"][0] and np.all(d["N"][0, :, 0] == -2.0) and np.all(occ.chunks == -1) and ao == F(1.0)
    # the same ray one step inside (the wall on the floor's edge, x in [0, 4), seen from above) is not open
    ao, d = down(svo, chunks, twin, 4.0, 50.0)
    assert list(np.nonzero(d["occ"][0])[0]) == [0, 3, 5] and d["fu"][0] == 0.0 and ao == F(1) / F(3)       # s1 and the corner cell: level 1


def test_pixels_that_get_no_rule_and_shade_ao(svo):
    chunks, twin = floor_world(svo, [((8, 10), (8, 10), (12, 14))])
    r = L.locate_one(twin, (41.0, 31.75, 50.0))
    g, v = np.zeros(7, H.HIT_DTYPE), np.zeros(7, H.VOXEL_DTYPE)
    g[:] = (68.0, (0, 0, 0), 1, H.HIT_FLAG, 0, 0, H.CELL_NONE)
    v[:] = (np.array(r[0], F), r[1], r[2], r[3], r[4], r[5], r[6])
    g["flags"][1] = 0                                           # a miss
    g["flags"][2] = H.HIT_FLAG | H.ERR_FLAG                     # an error record
    v[3] = np.zeros(1, H.VOXEL_DTYPE)[0]                        # no box
    v["chunk"][4] = 1                                           # the chunk count
    g["t"][5] = np.inf                                          # r_u, r_v not finite (P = eye + d * inf has NaN in x and z)
    g["t"][6] = np.nan
    wide = svo.make_camera((41.0, 100.0, 50.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), 1e-3, 7, 1)      # seven rays that all but coincide
    ao = M.hit_ao(chunks, 128, wide, None, g, v, M.TwinOccupancy(twin))
    assert ao[0] < 1.0 and np.all(ao[1:] == F(1.0))
    # svo_shade_ao: f = 1 - strength * (1 - ao) on r, g, b; depth, ao == 1 and NaN pixels keep their bits
    rgba = np.array([[0.5, 0.25, 1.0, 0.75], [0.5, 0.25, 1.0, 0.75], [0.3, 0.6, 0.9, 0.1], [np.nan, -0.0, 0.2, 0.3]], F)
    got = M.shade_ao(np.array([0.5, 1.0, np.nan, 0.0], F), 0.5, rgba)
    want = np.array([[0.375, 0.1875, 0.75, 0.75], [0.5, 0.25, 1.0, 0.75], [0.3, 0.6, 0.9, 0.1], [np.nan, -0.0, 0.1, 0.3]], F)
    assert np.array_equal(got.view(np.uint32)[:3], want.view(np.uint32)[:3]) and np.array_equal(got[3, 1:], want[3, 1:]) and np.signbit(got[3, 1])
    assert np.array_equal(M.shade_ao(np.array([0.5, 1.0, np.nan, 0.0], F), 0.0, rgba).view(np.uint32), rgba.view(np.uint32))
    assert np.array_equal(M.shade_ao(np.array([0.25], F), 1.0, rgba[:1])[0], np.array([0.125, 0.0625, 0.25, 0.75], F))


# ---- (b) the GPU scenes are not vacuous --------------------------------------------------------------------------------------------
def scene_detail(svo, oracle, name, view):
    w, h, d, ccm, _ = M.WORLDS[name]
    chunks = M.make_chunks(svo, name)
    O = oracle.OracleWorld.from_chunks(chunks, w, h, d, 128, ccm)
    cam = M.camera(svo, name, view)
    g = O.trace_image(cam, params=oracle.make_params())
    g = (g[0] if isinstance(g, tuple) else g).reshape(-1)
    O.close()
    v = H.hit_voxels(chunks, g)
    occ = M.TwinOccupancy(L.world_of(chunks, w, h, d, 128, ccm))
    detail = {}
    ao = M.hit_ao(chunks, 128, cam, None, g, v, occ, detail=detail)
    detail.update(ao=ao, g=g, v=v, neighbour_chunks=occ.chunks.reshape(-1, 8))
    return detail


def test_inputs_keep_the_gpu_comparisons_from_passing_vacuously(svo, oracle):
    """The rule on the CPU oracle's G-buffers of the GPU tests' scenes, 64 x 48: occlusion on a good share of the hits, every corner
    level, LEAF hits under the low camera, neighbour points in another chunk than the hit's on the mixed-depth world."""
    d = scene_detail(svo, oracle, "grid_2x1x2_d8", "default")
    hits, dark = int(d["on"].sum()), int((d["ao"] < 1).sum())
    levels = np.concatenate(list(M.corner_levels(d["occ"]).values()))
    counts = [int((levels == i).sum()) for i in range(4)]
    print(f"depth 8, default camera: {hits} hits, ao < 1 on {dark}, corner levels {counts}")
    assert hits >= 1000 and dark * 4 >= hits and min(counts) >= 100
    assert d["ao"].min() >= 0.0 and d["ao"].max() == 1.0 and np.all(d["ao"][~d["on"]] == 1.0)
    d = scene_detail(svo, oracle, "grid_2x1x2_d8", "low")
    leaf, cell = H.kinds(d["g"])
    print(f"depth 8, low camera: {int(d['on'].sum())} hits, ao < 1 on {int((d['ao'] < 1).sum())}, {leaf} LEAF hits, {cell} cell hits")
    assert leaf >= 500 and cell >= 500 and int((d["ao"] < 1).sum()) * 4 >= int(d["on"].sum())
    d = scene_detail(svo, oracle, "mixed_7_2_4_5", "default")
    own = d["v"]["chunk"][d["on"]].astype(np.int64)[:, None]
    outside, crossing = d["neighbour_chunks"] < 0, (d["neighbour_chunks"] >= 0) & (d["neighbour_chunks"] != own)
    print(f"depths 7/2/4/5: {int(d['on'].sum())} hits, ao < 1 on {int((d['ao'] < 1).sum())}, of {outside.size} neighbour points "
          f"{int(crossing.sum())} land in another chunk than the hit's, {int(outside.sum())} are outside the world")
    assert int(crossing.sum()) >= 300 and int((d["ao"] < 1).sum()) * 4 >= int(d["on"].sum())
