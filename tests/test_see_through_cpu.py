"""See-through materials (svo_trace_params.see_through, svo_trace_translucent, svo_shade_translucent): the C ABI surface, argument
checks that run before any device work, and the numpy rewrite the GPU tests check the kernels against.  CPU only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, L = 2 << 30, 3 << 30, 1 << 30


def test_new_symbols_are_exported_and_declared(svo):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svo.h")).read(), flags=re.S)
    for name in ("svo_trace_translucent", "svo_shade_translucent"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in svo.ABI_SYMBOLS
        assert hasattr(svo.lib, name)
    out = subprocess.run(["nm", "-D", "--defined-only", svo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T svo_trace_translucent$", out, flags=re.M) and re.search(r" T svo_shade_translucent$", out, flags=re.M)
    assert svo.SEE_THROUGH == 16 and "SVO_SEE_THROUGH   = 1u << 4" in header


def test_trace_params_keeps_its_size(svo, tmp_path):
    assert C.sizeof(svo.TraceParams) == 80 and svo.TraceParams.see_through.offset == 76
    src = r'''#include "svo.h"
#include <stddef.h>
#include <stdio.h>
int main(void){printf("%zu %zu %d\n",sizeof(svo_trace_params),offsetof(svo_trace_params,see_through),SVO_ABI_VERSION);return 0;}'''
    exe = str(tmp_path / "svo_see_through_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe], input=src, text=True, check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["80", "76", "4"]
    assert svo.trace_params().see_through == 0 and svo.trace_params(see_through=6).see_through == 6


def _tiny_world(svo):
    return svo.World.create([dict(position=(0, 0, 0), size=128.0, depth=4, tree=np.array([L | 6], np.uint32),
                                  twig=np.zeros(0, np.uint16))], 1, 1, 1, 128)


def test_argument_checks(svo):
    W = _tiny_world(svo)
    cam = svo.default_camera(1, 1, 128, 8, 8)
    fake = 256                                                  # never dereferenced: every call below fails before device work
    with pytest.raises(svo.SvoError) as e:
        W.trace(cam, svo.trace_params(see_through=0x10000), (0, 0, 8, 8), fake)
    assert e.value.code == -1
    with pytest.raises(svo.SvoError) as e:
        W.trace_rays(fake, fake, 1, svo.trace_params(see_through=0xFFFFFFFF), fake)
    assert e.value.code == -1
    with pytest.raises(svo.SvoError) as e:
        W.trace_translucent(cam, svo.trace_params(see_through=0), (0, 0, 8, 8), fake, fake)
    assert e.value.code == -1
    with pytest.raises(svo.SvoError) as e:
        W.trace_translucent(cam, svo.trace_params(see_through=0x10000), (0, 0, 8, 8), fake, fake)
    assert e.value.code == -1
    with pytest.raises(svo.SvoError) as e:
        W.trace_translucent(cam, svo.trace_params(see_through=6), (0, 0, 8, 8), fake, fake)
    assert e.value.code == -5                                   # SVO_ERR_NOT_UPLOADED
    with pytest.raises(svo.SvoError) as e:
        W.trace(cam, svo.trace_params(see_through=6), (0, 0, 8, 8), fake)
    assert e.value.code == -5
    with pytest.raises(svo.SvoError) as e:
        svo.shade_translucent(cam, svo.shade_defaults(), (0, 0, 8, 8), fake, 0, fake)
    assert e.value.code == -1
    with pytest.raises(svo.SvoError) as e:
        svo.shade_translucent(cam, svo.shade_defaults(), (0, 0, 8, 8), fake, fake, fake, absorption=-1.0)
    assert e.value.code == -1
    W.destroy()


def test_rewrite_helper_on_a_hand_built_chunk(svo):
    # root BRANCH -> block of 8: LEAF(6), LEAF(4), EMPTY, TWIG(0), LEAF(0x10006) (material 6 in its low 16 bits), BRANCH -> block, LEAF(6), TWIG(1)
    tree = np.array([B | 1, L | 6, L | 4, 0, T | 0, L | 0x10006, B | 9, L | 6, T | 1] + [L | 6, 0, L | 3, 0, 0, 0, 0, L | 6], np.uint32)
    twig = np.zeros(128, np.uint16)
    twig[[0, 5, 63]] = 6
    twig[[1, 64]] = 4
    twig[[65, 66]] = 6
    chunk = dict(position=(0.0, 0.0, 0.0), size=128.0, depth=5, tree=tree, twig=twig)
    out = svo.see_through_chunk(chunk, 6)
    want_tree = tree.copy()
    want_tree[[1, 5, 7, 9, 16]] = 0
    want_twig = twig.copy()
    want_twig[[0, 5, 63, 65, 66]] = 0
    assert out["tree"].dtype == np.uint32 and np.array_equal(out["tree"], want_tree)
    assert out["twig"].dtype == np.uint16 and np.array_equal(out["twig"], want_twig)
    assert np.array_equal(chunk["tree"], tree) and np.array_equal(chunk["twig"], twig)       # the input is not touched
    assert out["depth"] == 5 and out["position"] == (0.0, 0.0, 0.0)
    # the shape of the tree stays: BRANCH and TWIG words are never rewritten, whatever their offsets
    assert np.array_equal(svo.see_through_chunk(chunk, 1)["tree"], tree) and np.array_equal(svo.see_through_chunk(chunk, 9)["twig"], twig)
    # the rewritten chunk is still a valid world
    svo.World.create([out], 1, 1, 1, 128).destroy()
