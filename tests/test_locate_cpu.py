"""svo_world_locate (point queries): the C ABI surface, the argument checks that run before any device work, the host model
(tests/locate_model.py) on hand-made chunks with every expected record written out, and - on the model alone - the input
conditions the GPU tests of tests/test_locate.py rest on.  CPU only."""
import os
import re
import subprocess

import numpy as np
import pytest

import locate_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, B, T = 1 << 30, 2 << 30, 3 << 30
NONE = 0xFF


def test_new_symbol_is_declared_exported_and_sized(svo, tmp_path):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svo.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+svo_world_locate\s*\(\s*svo_world\s*\*\s*,\s*const float\s*\*\s*points_dev\s*,\s*int64_t n\s*,\s*"
                     r"const svo_trace_params\s*\*\s*params\s*,\s*svo_voxel\s*\*\s*out_dev\s*,\s*void\s*\*\s*stream\s*\)", header)
    assert "svo_world_locate" in svo.ABI_SYMBOLS and hasattr(svo.lib, "svo_world_locate")
    out = subprocess.run(["nm", "-D", "--defined-only", svo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T svo_world_locate$", out, flags=re.M)
    assert "#define SVO_ABI_VERSION 4" in header and svo.lib.svo_abi_version() == 4
    src = r'''#include "svo.h"
#include <stdio.h>
#include <stddef.h>
int main(void){printf("%zu %zu %zu %zu %zu %d %d\n",sizeof(svo_voxel),offsetof(svo_voxel,size),offsetof(svo_voxel,material),offsetof(svo_voxel,flags),
offsetof(svo_voxel,cell),(int)SVO_LOCATE_INSIDE,(int)SVO_LOCATE_SOLID);return 0;}'''
    exe = str(tmp_path / "svo_voxel_size")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe], input=src, text=True, check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [32, 12, 16, 18, 28, svo.LOCATE_INSIDE, svo.LOCATE_SOLID] == [32, 12, 16, 18, 28, 1, 2]
    assert svo.VOXEL_DTYPE == M.VOXEL_DTYPE and svo.VOXEL_DTYPE.itemsize == 32 and svo.VOXEL_DTYPE.fields["cell"][1] == 28


def test_argument_validation_precedes_any_device_work(svo):
    W = svo.World.create([dict(position=(0, 0, 0), size=128.0, depth=4, tree=np.array([L | 6], np.uint32), twig=np.zeros(0, np.uint16))], 1, 1, 1, 128)
    fake = 256                                                  # never dereferenced: every call below fails before device work
    prm = svo.trace_params()

    def code(*args):
        with pytest.raises(svo.SvoError) as e:
            W.locate(*args)
        return e.value.code

    # the world is not resident, and still every bad argument is named first
    assert code(fake, -1, prm, fake) == -1
    assert code(None, 8, prm, fake) == -1
    assert code(fake, 8, prm, None) == -1
    assert code(fake, 8, svo.trace_params(see_through=0x10000), fake) == -1
    assert code(fake, 8, svo.trace_params(semantics=2), fake) == -1
    assert code(fake, 8, svo.trace_params(semantics=-1), fake) == -1
    assert code(fake, 8, svo.trace_params(kernel=3), fake) == -1
    assert svo.lib.svo_world_locate(None, fake, 8, prm, fake, None) == -1
    # good arguments: the world is not resident (with and without params; n == 0 launches nothing but asks the same of the world)
    assert code(fake, 8, prm, fake) == -5
    assert code(fake, 8, None, fake) == -5
    assert code(fake, 8, svo.trace_params(see_through=0xFFFF, semantics=1, kernel=svo.KERNEL_STACK), fake) == -5
    assert code(None, 0, prm, None) == -5
    W.destroy()


def rec(bmin, size, material, flags, chunk, node, cell):
    r = np.zeros(1, M.VOXEL_DTYPE)
    r[0] = (np.array(bmin, np.float32), size, material, flags, chunk, node, cell)
    return r


def expect(world, p, want, **kw):
    got = M.locate(world, [p], **kw)
    want = np.zeros(1, M.VOXEL_DTYPE) if want is None else rec(*want)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"{p} {kw}: got {got[0]}, want {want[0]}"


def chunk(tree, twig=(), depth=4, pos=(0, 0, 0), size=128.0):
    return dict(position=pos, size=size, depth=depth, tree=np.array(tree, np.uint32), twig=np.array(twig, np.uint16))


def test_model_on_a_leaf_chunk_and_the_world_faces():
    w1 = M.world_of([chunk([L | 6])], 1, 1, 1, 128)
    expect(w1, (5, 5, 5), ((0, 0, 0), 128.0, 6, 3, 0, 0, NONE))
    expect(w1, (0, 0, 0), ((0, 0, 0), 128.0, 6, 3, 0, 0, NONE))                  # closed box: both corners
    expect(w1, (128, 128, 128), ((0, 0, 0), 128.0, 6, 3, 0, 0, NONE))            # (one chunk per axis: the index wraps onto the chunk that holds p)
    expect(w1, (128.00002, 5, 5), None)
    expect(w1, (5, -1e-30, 5), None)
    expect(w1, (5, 5, 5), ((0, 0, 0), 128.0, 0, 1, 0, 0, NONE), see_through=6)    # the LEAF reported as material 0, not solid; node and box unchanged
    expect(w1, (5, 5, 5), ((0, 0, 0), 128.0, 6, 3, 0, 0, NONE), see_through=5)
    for p in M.SPECIAL[:8]:                                                     # NaN and +-inf in any component
        expect(w1, p, None)
    expect(w1, (-0.0, -0.0, -0.0), ((0, 0, 0), 128.0, 6, 3, 0, 0, NONE))
    # two chunks on x: the max face of the world wraps to chunk 0, which does not hold p (step 2) - the seam belongs to chunk 1
    w2 = M.world_of([chunk([L | 6]), chunk([L | 2], pos=(128, 0, 0))], 2, 1, 1, 128)
    expect(w2, (256, 5, 5), None)
    expect(w2, (128, 5, 5), ((128, 0, 0), 128.0, 2, 3, 1, 0, NONE))
    expect(w2, (127.99999, 5, 5), ((0, 0, 0), 128.0, 6, 3, 0, 0, NONE))
    expect(w2, (255.99998, 128, 128), ((128, 0, 0), 128.0, 2, 3, 1, 0, NONE))    # y, z have one chunk: their max faces stay inside
    # a LEAF of material 0 is still a LEAF: solid (the march hits it)
    expect(M.world_of([chunk([L | 0x30000])], 1, 1, 1, 128), (1, 1, 1), ((0, 0, 0), 128.0, 0, 3, 0, 0, NONE))


def test_model_on_a_twig_root():
    """depth 2: the chunk is one brick of 32-unit cells; every third cell holds 1 + cell % 5."""
    cells = np.array([(1 + c % 5) if c % 3 == 0 else 0 for c in range(64)], np.uint16)
    w = M.world_of([chunk([T | 0], cells, depth=2)], 1, 1, 1, 128)
    expect(w, (70, 40, 100), ((64, 32, 96), 32.0, 5, 3, 0, 0, 54))               # off (2,1,3): cell 54, material 1 + 54 % 5
    expect(w, (40, 10, 10), ((32, 0, 0), 32.0, 0, 1, 0, 0, 1))                   # an empty cell: its own box, cell 1
    expect(w, (0, 0, 0), ((0, 0, 0), 32.0, 1, 3, 0, 0, 0))
    expect(w, (96, 96, 96), ((96, 96, 96), 32.0, 4, 3, 0, 0, 63))                # a cell's lower corner belongs to it (1 + 63 % 5)
    # the chunk's max face: off == 4 - the TWIG node's own box, no cell, not solid (twigmarch returns "no hit", src/Traverse.cpp:59)
    expect(w, (128, 10, 10), ((0, 0, 0), 128.0, 0, 1, 0, 0, NONE))
    expect(w, (10, 128, 127), ((0, 0, 0), 128.0, 0, 1, 0, 0, NONE))
    expect(w, (70, 40, 100), ((64, 32, 96), 32.0, 0, 1, 0, 0, 54), see_through=5)  # the cell reported empty; cell and box unchanged
    expect(w, (70, 40, 100), ((64, 32, 96), 32.0, 5, 3, 0, 0, 54), see_through=1)
    for sem in (0, 1):
        expect(w, (70, 40, 100), ((64, 32, 96), 32.0, 5, 3, 0, 0, 54), semantics=sem)


def test_model_on_a_branch_over_every_node_kind():
    """depth 3: the root's children are EMPTY, LEAF 3, TWIG 0, TWIG 1, LEAF 6, EMPTY, LEAF 2 (offset 0x10002), EMPTY (slot = x + 2y + 4z);
    brick 0 holds 6 in its odd cells, brick 1 holds 2 in its lower half (z < 2)."""
    b0 = [6 if c % 2 else 0 for c in range(64)]
    b1 = [2 if (c >> 4) < 2 else 0 for c in range(64)]
    w = M.world_of([chunk([B | 1, 0, L | 3, T | 0, T | 1, L | 6, 0, L | 0x10002, 0], b0 + b1, depth=3)], 1, 1, 1, 128)
    expect(w, (10, 10, 10), ((0, 0, 0), 64.0, 0, 1, 0, 1, NONE))                 # EMPTY
    expect(w, (100, 10, 10), ((64, 0, 0), 64.0, 3, 3, 0, 2, NONE))               # LEAF
    expect(w, (10, 100, 10), ((0, 96, 0), 16.0, 0, 1, 0, 3, 8))                  # TWIG 0, off (0,2,0): an even cell
    expect(w, (30, 100, 10), ((16, 96, 0), 16.0, 6, 3, 0, 3, 9))                 # ... and an odd one
    expect(w, (100, 100, 40), ((96, 96, 32), 16.0, 0, 1, 0, 4, 42))              # TWIG 1, off (2,2,2): upper half, empty
    expect(w, (100, 100, 20), ((96, 96, 16), 16.0, 2, 3, 0, 4, 26))
    expect(w, (10, 100, 100), ((0, 64, 64), 64.0, 2, 3, 0, 7, NONE))             # material = offset & 0xFFFF
    # exactly on a midpoint: the upper child, per axis
    expect(w, (64, 64, 64), ((64, 64, 64), 64.0, 0, 1, 0, 8, NONE))
    expect(w, (64, 10, 10), ((64, 0, 0), 64.0, 3, 3, 0, 2, NONE))
    expect(w, (63.999996, 10, 64), ((0, 0, 64), 64.0, 6, 3, 0, 5, NONE))
    # the max face of a TWIG that does not touch the chunk's: the neighbour's lower face (no off == 4 inside a chunk)
    expect(w, (64, 100, 10), ((64, 96, 0), 16.0, 2, 3, 0, 4, 8))
    # ... but on the chunk's max face it does happen
    expect(w, (100, 128, 10), ((64, 64, 0), 64.0, 0, 1, 0, 4, NONE))
    expect(w, (10, 10, 100), ((0, 0, 64), 64.0, 0, 1, 0, 5, NONE), see_through=6)
    expect(w, (30, 100, 10), ((16, 96, 0), 16.0, 0, 1, 0, 3, 9), see_through=6)
    expect(w, (100, 100, 20), ((96, 96, 16), 16.0, 2, 3, 0, 4, 26), see_through=6)


def test_the_glsl_and_cpu_cell_formulas():
    """(p - bmin) / leafsize against (p - bmin) * (1 / leafsize).  With a power-of-two chunk size - every world the stack kernel
    accepts - 1 / leafsize is exact and the two agree on every float; a search over 2 M random offsets per level and the 64 floats
    below every cell boundary found no difference at chunk size 100 or 10 either.  Chunk size 7 has one: leafsize 1.75, and the float
    below it is cell 0 by division, cell 1 by the reciprocal (1 / 1.75 rounds up)."""
    cells = np.arange(1, 65, dtype=np.uint16)
    w = M.world_of([chunk([T | 0], cells, depth=2, size=7.0)], 1, 1, 1, 7)
    x = float(np.nextafter(np.float32(1.75), np.float32(0)))
    expect(w, (x, 0.5, 0.5), ((0, 0, 0), 1.75, 1, 3, 0, 0, 0), semantics=0)
    expect(w, (x, 0.5, 0.5), ((1.75, 0, 0), 1.75, 2, 3, 0, 0, 1), semantics=1)
    expect(w, (1.75, 0.5, 0.5), ((1.75, 0, 0), 1.75, 2, 3, 0, 0, 1), semantics=0)
    w128 = M.world_of([chunk([T | 0], cells, depth=2)], 1, 1, 1, 128)
    pts = M.lattice_points(np.random.default_rng(5), 2000, np.zeros(3), np.full(3, 128.0), 0.5)
    pts = np.concatenate([pts, np.nextafter(pts, np.float32(-1e9)), np.nextafter(pts, np.float32(1e9))])
    assert np.array_equal(M.locate(w128, pts, 0).view(np.uint8), M.locate(w128, pts, 1).view(np.uint8))


def test_inputs_keep_the_gpu_comparisons_from_passing_vacuously(svo):
    """The model alone, on the worlds and point sets of tests/test_locate.py: every class of point - outside, EMPTY, LEAF, solid cell,
    empty cell - is there, none holds more than 90 % of a world's points; the lattice sets reach the wrap of step 2 and every node kind."""
    worlds = {name: (M.make_chunks(svo, name),) + spec[:4] for name, spec in M.WORLDS.items()}
    worlds["handmade"] = (M.handmade_chunks(),) + M.HANDMADE
    for name, (chunks, w, h, d, ccm) in worlds.items():
        world = M.world_of(chunks, w, h, d, 128, ccm)
        lo, hi = M.box_of(w, h, d, 128, ccm)
        sets = M.point_sets(name, lo, hi)
        pts = np.concatenate(list(sets.values()))
        assert pts.shape[0] <= 20000
        R = M.locate(world, pts)
        share = M.classes(R)
        print(name, pts.shape[0], "points:", share)
        assert sum(share.values()) == pts.shape[0]
        for cls in M.CLASSES:
            assert 0 < share[cls] <= 0.9 * pts.shape[0], f"{name}: class {cls} holds {share[cls]} of {pts.shape[0]} points"
        # the wrap: a lattice point inside the closed world box whose record is all zero
        for which in ("lattice", "half_lattice"):
            p = sets[which].astype(np.float64)
            in_box = np.all((p >= lo) & (p <= hi), axis=1)
            r = M.locate(world, sets[which])
            wraps = int((in_box & (r["flags"] == 0)).sum())
            print(f"  {which}: {wraps} wrap cases, {M.classes(r)}")
            if w > 1 or h > 1 or d > 1:
                assert wraps > 0
            assert all(M.classes(r)[cls] > 0 for cls in M.CLASSES)
        assert not M.locate(world, M.SPECIAL[:8]).view(np.uint8).any()
