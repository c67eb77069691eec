"""svo_hit_voxels / svo_hit_uv / svo_shade_textured without a device: the C ABI surface, the argument checks that are settled before
any device work, the host model (tests/hit_voxels_model.py) on a hand-made chunk with every expected record written out, and - with
the CPU oracle - the input conditions the GPU tests of tests/test_hit_voxels.py and tests/test_shade_textured.py rest on.  CPU only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hit_voxels_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, B, T = 1 << 30, 2 << 30, 3 << 30
NONE = 0xFF
NEW = ("svo_hit_voxels", "svo_hit_uv", "svo_shade_textured")


def test_new_symbols_are_declared_exported_and_sized(svo, tmp_path):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svo.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+svo_hit_voxels\s*\(\s*svo_world\s*\*\s*,\s*const svo_hit\s*\*\s*gbuffer_dev\s*,\s*int64_t n\s*,\s*svo_voxel\s*\*\s*out_dev\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", header)
    assert re.search(r"\bint\s+svo_hit_uv\s*\(\s*const svo_camera\s*\*\s*cam\s*,\s*float eps\s*,\s*int x0\s*,\s*int y0\s*,\s*int w\s*,\s*int h\s*,\s*"
                     r"const svo_hit\s*\*\s*gbuffer_dev\s*,\s*const svo_voxel\s*\*\s*voxels_dev\s*,\s*float\s*\*\s*uv_dev\s*,\s*void\s*\*\s*stream\s*\)", header)
    assert re.search(r"\bint\s+svo_shade_textured\s*\(\s*const svo_camera\s*\*\s*cam\s*,\s*const svo_shade_params\s*\*\s*p\s*,\s*const svo_atlas\s*\*\s*atlas\s*,"
                     r"\s*int x0\s*,\s*int y0\s*,\s*int w\s*,\s*int h\s*,\s*const svo_hit\s*\*\s*gbuffer_dev\s*,\s*const svo_voxel\s*\*\s*voxels_dev\s*,"
                     r"\s*float\s*\*\s*rgba_dev\s*,\s*void\s*\*\s*stream\s*\)", header)
    out = subprocess.run(["nm", "-D", "--defined-only", svo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in svo.ABI_SYMBOLS and hasattr(svo.lib, name)
        assert re.search(rf" T {name}$", out, flags=re.M)
    # functions added, nothing changed
    assert "#define SVO_ABI_VERSION 4" in header and svo.lib.svo_abi_version() == 4
    src = r'''#include "svo.h"
#include <stdio.h>
#include <stddef.h>
int main(void){printf("%zu %zu %zu %zu %zu %zu %zu\n",sizeof(svo_atlas),offsetof(svo_atlas,diffuse_dev),offsetof(svo_atlas,specular_dev),
offsetof(svo_atlas,width),offsetof(svo_atlas,height),sizeof(svo_hit),sizeof(svo_trace_params));return 0;}'''
    exe = str(tmp_path / "svo_atlas_size")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe], input=src, text=True, check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [24, 0, 8, 16, 20, 32, 80]
    assert C.sizeof(svo.Atlas) == 24 and svo.Atlas.width.offset == 16 and svo.Atlas.height.offset == 20
    assert svo.VOXEL_DTYPE == M.VOXEL_DTYPE and svo.HIT_DTYPE == M.HIT_DTYPE


def test_argument_checks_precede_any_device_work(svo):
    W = svo.World.create([dict(position=(0, 0, 0), size=128.0, depth=4, tree=np.array([L | 6], np.uint32), twig=np.zeros(0, np.uint16))], 1, 1, 1, 128)
    fake = 256                                                  # never dereferenced: every call below fails before device work

    def code(fn, *args):
        with pytest.raises(svo.SvoError) as e:
            fn(*args)
        return e.value.code

    # svo_hit_voxels on a world that is not resident: bad arguments first, then the residency, then n == 0
    assert code(W.hit_voxels, fake, -1, fake) == -1
    assert code(W.hit_voxels, None, 8, fake) == -1
    assert code(W.hit_voxels, fake, 8, None) == -1
    assert svo.lib.svo_hit_voxels(None, fake, 8, fake, None) == -1
    assert svo.lib.svo_hit_voxels(None, None, 0, None, None) == -1
    assert code(W.hit_voxels, fake, 8, fake) == -5
    assert code(W.hit_voxels, None, 0, None) == -5
    assert code(W.hit_voxels, fake, 0, fake) == -5
    W.destroy()
    # svo_hit_uv and svo_shade_textured take no world: their bad arguments are refused before HIP is touched
    cam = svo.default_camera(1, 1, 128, 16, 16)
    rect = (0, 0, 16, 16)
    assert code(svo.hit_uv, None, 0.0, rect, fake, fake, fake) == -1
    assert code(svo.hit_uv, cam, 0.0, rect, None, fake, fake) == -1
    assert code(svo.hit_uv, cam, 0.0, rect, fake, None, fake) == -1
    assert code(svo.hit_uv, cam, 0.0, rect, fake, fake, None) == -1
    assert code(svo.hit_uv, cam, -1.0, rect, fake, fake, fake) == -1
    assert code(svo.hit_uv, cam, float("nan"), rect, fake, fake, fake) == -1
    assert code(svo.hit_uv, cam, 0.0, (0, 0, -1, 16), fake, fake, fake) == -1
    svo.hit_uv(cam, 0.0, (0, 0, 0, 16), fake, fake, fake)       # an empty rectangle launches nothing
    P = svo.shade_defaults()
    atlas = svo.Atlas(fake, None, 256, 256)
    assert code(svo.shade_textured, cam, P, None, rect, fake, fake, fake) == -1
    assert code(svo.shade_textured, cam, P, svo.Atlas(None, fake, 256, 256), rect, fake, fake, fake) == -1
    assert code(svo.shade_textured, cam, P, svo.Atlas(fake, fake, 0, 256), rect, fake, fake, fake) == -1
    assert code(svo.shade_textured, cam, P, svo.Atlas(fake, fake, 256, -4), rect, fake, fake, fake) == -1
    assert code(svo.shade_textured, cam, P, atlas, rect, fake, None, fake) == -1
    assert code(svo.shade_textured, cam, P, atlas, rect, None, fake, fake) == -1
    assert code(svo.shade_textured, cam, P, atlas, rect, fake, fake, None) == -1
    assert code(svo.shade_textured, None, P, atlas, rect, fake, fake, fake) == -1
    assert code(svo.shade_textured, cam, None, atlas, rect, fake, fake, fake) == -1
    svo.shade_textured(cam, P, atlas, (0, 0, 16, 0), fake, fake, fake)


def hit(chunk, node, cell, material=3, flags=1, t=10.0):
    r = np.zeros(1, M.HIT_DTYPE)
    r[0] = (t, (0, 1, 0), material, flags, chunk, node, cell)
    return r


def expect(chunks, record, want):
    got = M.hit_voxels(chunks, record)
    w = np.zeros(1, M.VOXEL_DTYPE)
    if want is not None:
        w[0] = (np.array(want[0], np.float32), want[1], want[2], want[3], want[4], want[5], want[6])
    assert np.array_equal(got.view(np.uint8), w.view(np.uint8)), f"{record[0]}: got {got[0]}, want {w[0]}"


def test_model_known_answers_on_a_handmade_chunk(svo):
    c = M.handmade_chunk()
    svo.World.create([c], 1, 1, 1, 128).destroy()               # the library accepts it: the orphan is tolerated
    parent, level = M.parent_map(c)
    assert list(parent) == [M.NONE, 0, 10] and list(level) == [0, 1, 2]      # block 17 belongs to node 10, not to the orphan's node 3
    # a LEAF directly under the root: slot 5 = (x 1, y 0, z 1)
    expect([c], hit(0, 14, NONE), ((64, 0, 64), 64.0, 3, 3, 0, 14, NONE))
    # a LEAF at level 2 under slot 1, slot 0
    expect([c], hit(0, 17, NONE, material=2), ((64, 0, 0), 32.0, 2, 3, 0, 17, NONE))
    # a TWIG at level depth - 2: slot 1 then slot 6 = (0, 1, 1): its cell 27 = (3, 2, 1), 8 units a cell; the record's material is copied
    expect([c], hit(0, 23, 27, material=28), ((64 + 24, 32 + 16, 32 + 8), 8.0, 28, 3, 0, 23, 27))
    expect([c], hit(0, 23, 0, material=0x4321), ((64, 32, 32), 8.0, 0x4321, 3, 0, 23, 0))
    expect([c], hit(0, 23, 63), ((88, 56, 56), 8.0, 3, 3, 0, 23, 63))
    # what names nothing: a miss, an error record, a chunk / node / cell out of range, a LEAF with a cell, a TWIG without one, an
    # EMPTY node, a BRANCH, and the orphan block's nodes
    for rec in (hit(0, 14, NONE, flags=0), hit(0, 14, NONE, flags=1 | M.ERR_FLAG), hit(0, 14, NONE, flags=M.ERR_FLAG), hit(1, 14, NONE),
                hit(0, 25, NONE), hit(0, 0xFFFFFFFF, NONE), hit(0, 23, 64), hit(0, 23, NONE), hit(0, 14, 5), hit(0, 9, NONE), hit(0, 10, NONE),
                hit(0, 0, NONE), hit(0, 4, NONE), hit(0, 3, NONE)):
        expect([c], rec, None)
    # a root that is itself the voxel
    expect([dict(c, tree=np.array([L | 7], np.uint32), twig=np.zeros(0, np.uint16))], hit(0, 0, NONE, material=7), ((0, 0, 0), 128.0, 7, 3, 0, 0, NONE))
    expect([dict(c, depth=2, tree=np.array([T | 0], np.uint32))], hit(0, 0, 22), ((64, 32, 32), 32.0, 3, 3, 0, 0, 22))
    # an inexact frame: every step is a float32 operation of its own
    odd = dict(c, position=(0.1, 0.2, 0.3), size=100.0)
    f = np.float32
    h1, h2 = f(100.0) * f(0.5), f(100.0) * f(0.5) * f(0.5)
    lo = [f(0.1) + f(1) * h1 + f(0) * h2, f(0.2) + f(0) * h1 + f(1) * h2, f(0.3) + f(0) * h1 + f(1) * h2]
    leaf = h2 / f(4)
    expect([odd], hit(0, 23, 27), ([lo[0] + f(3) * leaf, lo[1] + f(2) * leaf, lo[2] + f(1) * leaf], leaf, 3, 3, 0, 23, 27))


def test_model_uv_and_texel_known_answers():
    f = np.float32
    eps = f(1 / 8192)
    bmin, size = np.array([[8, 16, 24]], f), np.array([8], f)
    # on the box's lower x face: uv = p.yz - cmin.yz = (2, 6) -> iuv (0.25, 0.75), nudged down by 2 eps; material 0x0203 -> tile (3, 2)
    uv = M.leaf_uv(np.array([[8, 18, 30]], f), bmin, size, [0x0203], eps)
    want = (np.array([3, 2], f) + (np.array([0.25, 0.75], f) - eps * f(2))) / f(256)
    assert np.array_equal(uv[0], want)
    # on the upper y face, measured from cmax: uv = p.xz - cmax.xz = (9 - 16, 24 - 32) -> (0.875, 1.0)
    uv = M.leaf_uv(np.array([[9, 24, 24]], f), bmin, size, [0], eps)
    # ... but p.z == cmin.z also holds and comes later: uv = p.xy - cmin.xy = (1, 8) -> (0.125 exactly: no nudge, 1.0 - 2 eps)
    assert np.array_equal(uv[0], np.array([f(0.125), f(1) - eps * f(2)], f) / f(256))
    # no face within eps: uv = 0 -> nudged up by 2 eps
    uv = M.leaf_uv(np.array([[12, 20, 28]], f), bmin, size, [0xFFFF], eps)
    assert np.array_equal(uv[0], (np.array([255, 255], f) + eps * f(2)) / f(256))
    x, y = M.texel_index(np.array([[0.0, 0.999999], [1.0, 1.5], [-0.25, 2.75], [0.5, 0.25]], f), 512, 256)
    assert list(x) == [0, 0, 384, 256] and list(y) == [255, 128, 192, 64]


def test_inputs_keep_the_gpu_comparisons_from_passing_vacuously(svo, oracle):
    """Every world of the GPU tests, traced by the CPU oracle from the same cameras and ray lists: each input set holds a few hundred
    LEAF hits and a few hundred brick-cell hits, so that no comparison of boxes or UVs passes on an empty set; and every such record
    gets a box from the model."""
    for name, (w, h, d, cs, ccm, depths, _) in M.WORLDS.items():
        chunks = M.make_chunks(svo, name)
        O = oracle.OracleWorld.from_chunks(chunks, w, h, d, cs, ccm)
        sets = {}
        for semantics in (0, 1):
            for view, cam in M.cameras(svo, name).items():
                sets[f"{view}/semantics {semantics}"] = O.trace_image(cam, params=oracle.make_params(semantics=semantics))
        o, dd = M.ray_list(name)
        sets["rays"] = O.trace_rays(o, dd)
        per_world = [0, 0]
        for what, g in sets.items():
            g = g[0] if isinstance(g, tuple) else g
            leaf, cell = M.kinds(g)
            print(f"{name} {what}: {leaf} LEAF hits, {cell} cell hits of {g.size}")
            per_world[0] += leaf
            per_world[1] += cell
            v = M.hit_voxels(chunks, g)
            usable = ((g.reshape(-1)["flags"] & 1) != 0) & ((g.reshape(-1)["flags"] & M.ERR_FLAG) == 0)
            assert np.array_equal((v["flags"] & M.INSIDE) != 0, usable), f"{name} {what}: a hit without a box"
            assert leaf + cell >= 300, f"{name} {what}: {leaf + cell} hits"
        assert per_world[0] >= 300 and per_world[1] >= 300, f"{name}: {per_world}"
        for view in ("above", "front"):
            leaf, cell = M.kinds(sets[f"{view}/semantics 0"])
            assert (cell if view == "above" else leaf) >= 200, f"{name} {view}: {leaf} LEAF, {cell} cell hits"
        O.close()
