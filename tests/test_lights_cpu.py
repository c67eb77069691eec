"""svo_trace_lights and svo_shade_lights: the C ABI surface, the argument checks that run before any device work, the model's
statistics on the GPU tests' scene, and planted mutations of the model that each change the scene's words.  CPU only (oracle only)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lights_model as LM
import local_shadows_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF = 1 << 30
W_, H_ = 128, 96
N_ = W_ * H_
INVALID, NOT_UPLOADED, UNSUPPORTED = -1, -5, -6


def test_struct_and_symbols(svo, tmp_path):
    assert C.sizeof(svo.Light) == 64 and svo.MAX_LIGHTS == 32 == LM.MAX_LIGHTS
    src = r'''#include "svo.h"
#include <stdio.h>
#include <stddef.h>
int main(void){printf("%zu %d %zu %zu %zu %zu %zu %zu %zu %zu\n",sizeof(svo_light),SVO_MAX_LIGHTS,offsetof(svo_light,position),offsetof(svo_light,reach),offsetof(svo_light,ambient),
offsetof(svo_light,constant),offsetof(svo_light,diffuse),offsetof(svo_light,linear),offsetof(svo_light,specular),offsetof(svo_light,quadratic));return 0;}'''
    exe = str(tmp_path / "svo_light_size")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe], input=src, text=True, check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [64, 32] + [getattr(svo.Light, f).offset for f in ("position", "reach", "ambient", "constant", "diffuse", "linear", "specular", "quadratic")]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svo.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", svo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("svo_trace_lights", "svo_shade_lights"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in svo.ABI_SYMBOLS and re.search(r" T %s$" % name, out, flags=re.M)
    assert "#define SVO_ABI_VERSION 4" in header and svo.lib.svo_abi_version() == 4


def _lights(svo, **change):
    kw = dict(position=(50.0, 8.0, 65.0), reach=64.0)
    kw.update(change)
    return [svo.Light(kw["position"], kw["reach"], (0.1, 0.1, 0.1), (0.5, 0.5, 0.5), (1.0, 1.0, 1.0), (1.0, 0.14, 0.09))]


def test_trace_lights_refuses_before_any_device_work(svo):
    """Every refused argument returns its status on a world that is not uploaded - so SVO_ERR_INVALID_ARG comes before
    SVO_ERR_NOT_UPLOADED - and without a device; the dummy pointers are never dereferenced."""
    W = svo.World.create([dict(position=(0, 0, 0), size=128.0, depth=4, tree=np.array([LEAF | 6], np.uint32), twig=np.zeros(0, np.uint16))], 1, 1, 1, 128)
    cam = svo.default_camera(1, 1, 128, 8, 8)
    fake = 256
    nan, inf = float("nan"), float("inf")
    good = dict(cam=cam, params=svo.trace_params(), rect=(0, 0, 8, 8), gbuffer_ptr=fake, lights=_lights(svo), visible_ptr=fake, max_rays=0)
    bad = [dict(cam=None), dict(params=None), dict(gbuffer_ptr=None), dict(visible_ptr=None), dict(lights=None), dict(lights=[]),
           dict(lights=_lights(svo) * 33), dict(max_rays=-1), dict(max_rays=-2 ** 63), dict(rect=(0, 0, -1, 8)), dict(rect=(0, 0, 8, -1)), dict(rect=(-1, 0, 8, 8)),
           dict(rect=(0, -1, 8, 8)), dict(lights=_lights(svo, position=(nan, 0.0, 0.0))), dict(lights=_lights(svo, position=(0.0, inf, 0.0))),
           dict(lights=_lights(svo, position=(0.0, 0.0, -inf))), dict(lights=_lights(svo, reach=0.0)), dict(lights=_lights(svo, reach=-1.0)),
           dict(lights=_lights(svo, reach=inf)), dict(lights=_lights(svo, reach=nan)), dict(lights=_lights(svo) + _lights(svo, reach=nan)),
           dict(params=svo.trace_params(see_through=0x10000)), dict(rect=(0, 0, 0, 0), lights=None), dict(rect=(0, 0, 1 << 20, 1 << 20), max_rays=-1)]
    for change in bad:
        kw = dict(good, **change)
        with pytest.raises(svo.SvoError) as e:
            W.trace_lights(kw["cam"], kw["params"], kw["rect"], kw["gbuffer_ptr"], kw["lights"], kw["visible_ptr"], max_rays=kw["max_rays"])
        assert e.value.code == INVALID, change
        assert svo.lib.svo_last_error(), change
    arr, n = svo.light_array(_lights(svo))
    assert svo.lib.svo_trace_lights(None, C.byref(cam), C.byref(good["params"]), arr, n, 0, 0, 0, 8, 8, fake, fake, None, None) == INVALID       # a null world
    for change in (dict(), dict(rect=(0, 0, 0, 0)), dict(rect=(0, 0, 1 << 20, 1 << 20)), dict(max_rays=1 << 40), dict(lights=_lights(svo, reach=1e30)),
                   dict(params=svo.trace_params(semantics=7))):
        kw = dict(good, **change)
        with pytest.raises(svo.SvoError) as e:
            W.trace_lights(kw["cam"], kw["params"], kw["rect"], kw["gbuffer_ptr"], kw["lights"], kw["visible_ptr"], max_rays=kw["max_rays"])
        assert e.value.code == NOT_UPLOADED, change             # generated or created, not resident: nothing was traced on the CPU
    W.destroy()


def test_shade_lights_refuses_before_hip_is_touched(svo):
    cam = svo.default_camera(1, 1, 128, 16, 16)
    P = svo.shade_defaults()
    ptr, rect = 0x1000, (0, 0, 16, 16)
    good = dict(cam=cam, P=P, rect=rect, g=ptr, lights=_lights(svo), out=ptr, vis=ptr)
    for change in (dict(cam=None), dict(P=None), dict(g=None), dict(out=None), dict(lights=None), dict(lights=[]), dict(lights=_lights(svo) * 33),
                   dict(rect=(0, 0, -1, 16)), dict(rect=(0, 0, 16, -1)), dict(rect=(-1, 0, 16, 16)), dict(rect=(0, -1, 16, 16)),
                   dict(rect=(0, 0, 1 << 20, 1 << 20), lights=None), dict(rect=(0, 0, 0, 0), out=None)):
        kw = dict(good, **change)
        with pytest.raises(svo.SvoError) as e:
            svo.shade_lights(kw["cam"], kw["P"], kw["rect"], kw["g"], kw["lights"], kw["out"], visible_ptr=kw["vis"])
        assert e.value.code == INVALID, change
    for vis in (ptr, None):
        with pytest.raises(svo.SvoError) as e:
            svo.shade_lights(cam, P, (0, 0, 1 << 20, 1 << 20), ptr, _lights(svo), ptr, visible_ptr=vis)      # too large for one launch, behind the argument check
        assert e.value.code == UNSUPPORTED
        for empty in ((0, 0, 0, 16), (0, 0, 16, 0), (3, 5, 0, 0)):
            svo.shade_lights(cam, P, empty, ptr, _lights(svo) * 32, ptr, visible_ptr=vis)                    # an empty rectangle is SVO_OK


@pytest.fixture(scope="module")
def scene(svo, oracle):
    W = svo.World.generate(2, 1, 2, 128, 8)
    ow = oracle.OracleWorld.from_chunks([W.chunk(i) for i in range(4)], 2, 1, 2, 128)
    cam = svo.default_camera(2, 2, 128, W_, H_)
    frame = ow.trace_image(cam, params=oracle.make_params(shadow=True), threads=8)
    frame.setflags(write=False)
    yield ow, cam, frame
    W.destroy()


def test_model_statistics_of_the_scene(oracle, scene):
    """The oracle alone, on the GPU tests' scene: the figures the conditions of tests/test_lights.py rest on."""
    ow, cam, frame = scene
    rect = (0, 0, W_, H_)
    m = LM.trace(oracle, ow, cam, rect, frame, LM.LIGHTS, max_rays=10 * N_)
    s = m["stats"]
    assert m["usable"] == 7087 and m["counts"] == (19123, 19123) and m["cap"] == 10 * N_
    assert [x["pairs"] for x in s] == [1177, 1614, 5976, 684, 2843, 33, 287, 6371, 0, 138]
    assert [(s[j]["occluded"], s[j]["visible"]) for j in (0, 1, 2, 3, 4, 7)] == [(344, 833), (482, 1132), (2603, 3373), (139, 545), (1490, 1353), (4086, 2285)]
    for j in (0, 1, 2, 3, 4, 7):
        assert s[j]["occluded"] >= 100 and s[j]["visible"] >= 500
    assert all(s[j]["visible"] == 0 and s[j]["occluded"] == s[j]["pairs"] for j in (5, 6, 9))           # under water, inside rock, under a slope
    assert s[8]["pairs"] == 0 and s[8]["backfacing"] == 2                                               # the empty segment
    assert all(292 <= s[j]["backfacing"] <= 1439 for j in range(8)) and all(x["backfacing"] >= 200 for x in s[:8])
    assert all(x["runaways"] == 0 for x in s) and min(x["nearest"] for x in s) > 0.03
    assert np.all(m["words"][~M.usable(frame)] == 0) and np.all(m["words"] < 1 << 10)
    # the ranks are a light-major numbering without gaps
    slot = m["slot"][m["pair"]]
    assert np.array_equal(slot, np.arange(19123))
    # the default cap: one slot per pixel
    d = LM.trace(oracle, ow, cam, rect, frame, LM.LIGHTS)
    assert d["counts"] == (19123, 12288) and d["cap"] == N_
    assert [x["dropped"] for x in d["stats"]] == [0, 0, 0, 0, 6, 33, 287, 6371, 0, 138]
    lit = d["pair"] & (d["slot"] < 0)
    for j in range(10):
        assert np.all((d["words"][lit[j]] >> np.uint32(j)) & 1 == 1)                                    # dropped pairs count as not occluded


class ReachStrict(LM.TraceModel):
    def in_reach(self, q, R2):
        with np.errstate(invalid="ignore"):
            return q < R2


class FacingStrict(LM.TraceModel):
    def facing(self, s):
        with np.errstate(invalid="ignore"):
            return ~(s < 0)


class PixelMajor(LM.TraceModel):
    def ranks(self, pair):
        flat = pair.T.reshape(-1)
        return (np.cumsum(flat) - flat).reshape(pair.T.shape).T


class DroppedDark(LM.TraceModel):
    def dropped_visible(self):
        return False


def _special_lights(oracle, scene):
    """Two lights for the mutations: one whose reach squared equals one visible pixel's q exactly, and one in the plane of a visible
    pixel's face (s == 0 exactly), each with a reach so small that it has few other pairs."""
    ow, cam, frame = scene
    rect = (0, 0, W_, H_)
    rec = frame.reshape(-1)
    o, d = M.camera_rays(oracle, cam, rect)
    sel = M.usable(rec)
    P = M.sample_points(o, d, rec, M.resolved_eps(0))
    up = np.nonzero(sel & (rec["normal"][:, 0] == 0) & (rec["normal"][:, 1] == 1) & (rec["normal"][:, 2] == 0))[0]
    assert up.size >= 100
    exact = plane = None
    for k in up[::7]:
        if exact is None:
            position = tuple(float(c) for c in (P[k] + np.array([1.0, 3.0, 0.5], np.float32)).astype(np.float32))
            _, q = LM.light_vectors(P[k:k + 1], position)
            R = np.sqrt(q[0]).astype(np.float32)
            if R * R == q[0]:
                m = LM.trace(oracle, ow, cam, rect, frame, [(position, float(R))], max_rays=N_)
                if m["words"][k] == 1:
                    exact = (k, (position, float(R)))
        if plane is None:
            position = (float(np.float32(P[k][0] + np.float32(0.25))), float(P[k][1]), float(P[k][2]))
            m = LM.trace(oracle, ow, cam, rect, frame, [(position, 1.0)], max_rays=N_)
            if not m["pair"][0][k] and FacingStrict().trace(oracle, ow, cam, rect, frame, [(position, 1.0)], max_rays=N_)["words"][k] == 1:
                plane = (k, (position, 1.0))
        if exact and plane:
            break
    assert exact and plane
    return exact, plane


def test_planted_mutations_change_the_words(oracle, scene):
    """No rule of the definition goes untested: each mutation of the model changes the words the GPU is compared with."""
    ow, cam, frame = scene
    rect = (0, 0, W_, H_)
    (k_exact, exact), (k_plane, plane) = _special_lights(oracle, scene)
    lights = LM.LIGHTS + [exact, plane]
    want = LM.trace(oracle, ow, cam, rect, frame, lights, max_rays=12 * N_)
    assert want["words"][k_exact] & (1 << 10) and not want["words"][k_plane] & (1 << 11)
    capped = LM.trace(oracle, ow, cam, rect, frame, lights)
    assert capped["counts"][0] > capped["counts"][1]

    got = ReachStrict().trace(oracle, ow, cam, rect, frame, lights, max_rays=12 * N_)
    assert got["words"][k_exact] != want["words"][k_exact] and got["counts"][0] < want["counts"][0]
    got = FacingStrict().trace(oracle, ow, cam, rect, frame, lights, max_rays=12 * N_)
    assert got["words"][k_plane] != want["words"][k_plane] and got["counts"][0] > want["counts"][0]
    for mutant in (PixelMajor(), DroppedDark()):
        assert np.array_equal(mutant.trace(oracle, ow, cam, rect, frame, lights, max_rays=12 * N_)["words"], want["words"])       # (no overflow: no difference)
        got = mutant.trace(oracle, ow, cam, rect, frame, lights)
        assert np.count_nonzero(got["words"] != capped["words"]) >= 500, type(mutant).__name__
