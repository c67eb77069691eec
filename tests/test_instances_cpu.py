"""svo_trace_instances and svo_trace_instance_shadows: the C ABI surface, the argument rules that run before any device work, and
the numpy model of tests/instances_model.py against the unchanged oracle - anchored where the transform is exact, with planted
mutations for the rules the anchor does not reach.  CPU only (oracle only)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import instances_model as IM
import local_shadows_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF = 1 << 30
INVALID, NOT_UPLOADED, UNSUPPORTED = -1, -5, -6
W_, H_ = 96, 64
N_ = W_ * H_


def test_struct_and_symbols(svo, tmp_path):
    assert C.sizeof(svo.Instance) == 64 and svo.MAX_INSTANCES == 32 == IM.MAX_INSTANCES
    src = r'''#include "svo.h"
#include <stdio.h>
#include <stddef.h>
int main(void){printf("%zu %d %zu %zu %zu %zu\n",sizeof(svo_instance),SVO_MAX_INSTANCES,offsetof(svo_instance,rot),offsetof(svo_instance,pos),
offsetof(svo_instance,scale),offsetof(svo_instance,_pad));return 0;}'''
    exe = str(tmp_path / "svo_instance_size")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe], input=src, text=True, check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [64, 32] + [getattr(svo.Instance, f).offset for f in ("rot", "pos", "scale", "_pad")]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svo.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", svo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("svo_trace_instances", "svo_trace_instance_shadows"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in svo.ABI_SYMBOLS and re.search(r" T %s$" % name, out, flags=re.M)
    assert "#define SVO_ABI_VERSION 4" in header and svo.lib.svo_abi_version() == 4


# ---- the argument rules ------------------------------------------------------------------------------------------------
def _inst(svo, **change):
    kw = dict(rot=np.eye(3), pos=(1.0, 2.0, 3.0), scale=1.0)
    kw.update(change)
    return [svo.Instance(kw["rot"], kw["pos"], kw["scale"])]


def _rot_with(k, value):
    r = np.eye(3).reshape(-1)
    r[k] = value
    return r


def _one_leaf_world(svo):
    return svo.World.create([dict(position=(0, 0, 0), size=128.0, depth=4, tree=np.array([LEAF | 6], np.uint32), twig=np.zeros(0, np.uint16))], 1, 1, 1, 128)


def test_refuses_before_any_device_work(svo):
    """Every refused argument returns SVO_ERR_INVALID_ARG on worlds that are not uploaded - so it comes before SVO_ERR_NOT_UPLOADED - and
    without a device; the dummy pointers are never dereferenced."""
    S, Mw = _one_leaf_world(svo), _one_leaf_world(svo)
    cam = svo.default_camera(1, 1, 128, 8, 8)
    fake = 256
    nan, inf = float("nan"), float("inf")
    good = dict(scene=S, model=Mw, cam=cam, params=svo.trace_params(), rect=(0, 0, 8, 8), g=fake, inst=_inst(svo), merged=fake, owner=fake, max_rays=0, bias=0.0)

    def stage1(kw):
        kw["scene"].trace_instances(kw["model"], kw["cam"], kw["params"], kw["rect"], kw["g"], kw["inst"], kw["merged"], kw["owner"], max_rays=kw["max_rays"])

    def stage2(kw):
        kw["scene"].trace_instance_shadows(kw["model"], kw["cam"], kw["params"], kw["rect"], kw["inst"], kw["merged"], kw["owner"], max_rays=kw["max_rays"],
                                           bias=kw["bias"])

    bad = [dict(model=None), dict(cam=None), dict(params=None), dict(inst=None), dict(inst=[]), dict(inst=_inst(svo) * 33), dict(merged=None), dict(owner=None),
           dict(max_rays=-1), dict(max_rays=-2 ** 63), dict(rect=(0, 0, -1, 8)), dict(rect=(0, 0, 8, -1)), dict(rect=(-1, 0, 8, 8)), dict(rect=(0, -1, 8, 8)),
           dict(inst=_inst(svo, pos=(nan, 0.0, 0.0))), dict(inst=_inst(svo, pos=(0.0, inf, 0.0))), dict(inst=_inst(svo, pos=(0.0, 0.0, -inf))),
           dict(inst=_inst(svo, scale=0.0)), dict(inst=_inst(svo, scale=-1.0)), dict(inst=_inst(svo, scale=inf)), dict(inst=_inst(svo, scale=nan)),
           dict(inst=_inst(svo) + _inst(svo, scale=nan)), dict(params=svo.trace_params(see_through=0x10000)), dict(rect=(0, 0, 0, 0), inst=None),
           dict(rect=(0, 0, 1 << 20, 1 << 20), max_rays=-1)]
    bad += [dict(inst=_inst(svo, rot=_rot_with(k, v))) for k in range(9) for v in (nan, inf)]
    for call, extra in ((stage1, [dict(g=None)]), (stage2, [dict(bias=-1.0), dict(bias=nan), dict(bias=-1e-30)])):
        for change in bad + extra:
            with pytest.raises(svo.SvoError) as e:
                call(dict(good, **change))
            assert e.value.code == INVALID, (call.__name__, change)
            assert svo.lib.svo_last_error(), change
    arr, n = svo.instance_array(_inst(svo))
    prm = good["params"]
    assert svo.lib.svo_trace_instances(None, Mw._h, C.byref(cam), C.byref(prm), arr, n, 0, 0, 0, 8, 8, fake, fake, fake, None, None) == INVALID      # a null scene
    assert svo.lib.svo_trace_instance_shadows(None, Mw._h, C.byref(cam), C.byref(prm), arr, n, 0, 0.0, 0, 0, 8, 8, fake, fake, None, None) == INVALID
    # what is no fault of the arguments comes to the worlds' residency: an empty or a huge rectangle, any cap, any bias >= 0, the
    # scene as its own model, an unknown semantics (svo_trace's order: residency before it)
    for call in (stage1, stage2):
        for change in (dict(), dict(rect=(0, 0, 0, 0)), dict(rect=(0, 0, 1 << 20, 1 << 20)), dict(max_rays=1 << 40), dict(bias=inf), dict(bias=0.5), dict(model=S),
                       dict(inst=_inst(svo, scale=1e-30)), dict(params=svo.trace_params(semantics=7)), dict(inst=_inst(svo) * 32)):
            with pytest.raises(svo.SvoError) as e:
                call(dict(good, **change))
            assert e.value.code == NOT_UPLOADED, (call.__name__, change)
    S.destroy()
    Mw.destroy()


# ---- the model against the oracle --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_world(svo, oracle):
    chunk = svo.chunk_from_grid(IM.model_grid(), (0.0, 0.0, 0.0), float(IM.MODEL_SIZE))
    assert chunk["depth"] == IM.MODEL_DEPTH
    ow = oracle.OracleWorld.from_chunks([chunk], 1, 1, 1, IM.MODEL_SIZE)
    return ow, IM.world_box((0, 0, 0), (1, 1, 1), IM.MODEL_SIZE)


def _misses(svo, n):
    return np.zeros(n, svo.HIT_DTYPE)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("semantics", [0, 1])
@pytest.mark.parametrize("normal_mode", [0, 1])
def test_anchor_identity_is_the_direct_trace(svo, oracle, model_world, semantics, normal_mode):
    """R = I, pos = 0, scale = 1 in front of an all-miss G-buffer: om = o and dm = d exactly, so merged is the oracle's own image of the
    model world, every field of every pixel.  The camera is chosen so that the box rule culls no pixel the direct trace hits (0 of
    2572 hits: a condition on the input, not a tolerance)."""
    ow, box = model_world
    cam = svo.make_camera((50.0, 44.0, -25.0), (-34.0, -28.0, 41.0), (0.0, 1.0, 0.0), 32.0, W_, H_)
    rect = (0, 0, W_, H_)
    want = ow.trace_image(cam, params=oracle.make_params(shadow=False, semantics=semantics, normal_mode=normal_mode), threads=8).reshape(-1)
    m = IM.trace(oracle, ow, box, cam, rect, _misses(svo, N_), [IM.instance((0.0, 0.0, 0.0))], semantics=semantics, normal_mode=normal_mode)
    hit = M.usable(want)
    assert hit.sum() >= 1500 and (~hit).sum() >= 1500
    assert np.count_nonzero(hit & ~m["pair"][0]) == 0, "the box rule culls a pixel the direct trace hits"
    assert m["pair"][0].sum() > hit.sum() + 500 and m["stats"][0]["runaways"] == 0      # pairs that pass through the shell's holes or beside it
    got = m["merged"]
    for f in ("flags", "material", "chunk", "node", "cell"):
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(_bits(got["t"]), _bits(want["t"]))
    gn, wn = got["normal"], want["normal"]
    assert np.all((np.isnan(gn) & np.isnan(wn)) | (_bits(gn) == _bits(wn)))
    assert np.array_equal(m["owner"], hit.astype(np.uint32))
    if normal_mode == 1:
        assert np.all((got["flags"][hit] & IM.FACE) != 0)


def test_translation_is_the_trace_of_the_moved_world(svo, oracle, model_world):
    """The model at an integer position against the oracle's trace of a world created with that chunk AT that position: hit / miss and
    the integer fields are equal on all pixels.  t is compared where o - pos is exact - the eye has integer coordinates, so that is
    every pixel, 6144 - and NOT bit for bit: the march accumulates t through points o + d * t that it rounds at the magnitude of the
    world's coordinates (up to 128 here, up to 32 in the model's own space), so the two marches round differently whatever the
    transform does - 1826 of the 2572 hits differ, by up to 9 ulp.  The bound is the contract's for t across such differences,
    helpers.T_RTOL (1e-4, relative; 9 ulp is 1.1e-6), no number of this test's."""
    from helpers import T_RTOL
    ow, box = model_world
    pos = (64.0, -32.0, 96.0)
    chunk = svo.chunk_from_grid(IM.model_grid(), pos, float(IM.MODEL_SIZE))
    moved = oracle.OracleWorld.from_chunks([chunk], 1, 1, 1, IM.MODEL_SIZE, (2, -1, 3))
    cam = svo.make_camera((114.0, 12.0, 71.0), (-34.0, -28.0, 41.0), (0.0, 1.0, 0.0), 32.0, W_, H_)
    rect = (0, 0, W_, H_)
    want = moved.trace_image(cam, params=oracle.make_params(shadow=False), threads=8).reshape(-1)
    m = IM.trace(oracle, ow, box, cam, rect, _misses(svo, N_), [IM.instance(pos)])
    got = m["merged"]
    hit = M.usable(want)
    assert hit.sum() >= 1500
    for f in ("flags", "material", "chunk", "node", "cell"):
        assert np.array_equal(got[f], want[f]), f
    o, _ = M.camera_rays(oracle, cam, rect)
    exact = np.all((o.astype(np.float64) - np.asarray(pos)) == (o - np.asarray(pos, np.float32)).astype(np.float64), axis=1)
    assert exact.sum() == N_
    sel = exact & hit
    assert np.all(np.abs(got["t"][sel].astype(np.float64) - want["t"][sel]) <= T_RTOL * np.maximum(1.0, np.abs(want["t"][sel])))
    assert np.array_equal(_bits(got["t"][~hit]), _bits(want["t"][~hit]))
    assert np.all((np.isnan(got["normal"]) & np.isnan(want["normal"])) | (_bits(got["normal"]) == _bits(want["normal"])))


@pytest.fixture(scope="module")
def view(svo, oracle, model_world):
    """A rotated, scaled instance under the anchor's camera, in front of misses: (cam, rect, instance, its model result)."""
    ow, box = model_world
    cam = svo.make_camera((50.0, 44.0, -25.0), (-34.0, -28.0, 41.0), (0.0, 1.0, 0.0), 32.0, W_, H_)
    inst = IM.centred((16.0, 16.0, 16.0), 1.25, IM.rotation((1, 2, 3), 40.0))
    return cam, (0, 0, W_, H_), inst, IM.trace(oracle, ow, box, cam, (0, 0, W_, H_), _misses(svo, N_), [inst])


class TiesToTheLast(IM.Model):
    def nearer(self, tw, best):
        return tw <= best


class PixelMajor(IM.Model):
    def ranks(self, pair):
        flat = pair.T.reshape(-1)
        return (np.cumsum(flat) - flat).reshape(pair.T.shape).T


class EntersAtOrBefore(IM.Model):
    def before(self, tn, far):
        with np.errstate(invalid="ignore"):
            return tn <= far


def test_tie_goes_to_the_lowest_instance(svo, oracle, model_world, view):
    ow, box = model_world
    cam, rect, inst, one = view
    two = IM.trace(oracle, ow, box, cam, rect, _misses(svo, N_), [inst, inst], max_rays=2 * N_)
    owned = one["owner"] != 0
    assert owned.sum() >= 1500 and two["contested"] == owned.sum()
    assert np.array_equal(two["owner"], one["owner"]) and np.array_equal(two["merged"].view(np.uint8), one["merged"].view(np.uint8))
    assert two["counts"] == (2 * one["counts"][0],) * 2
    mutant = TiesToTheLast().trace(oracle, ow, box, cam, rect, _misses(svo, N_), [inst, inst], max_rays=2 * N_)
    assert np.all(mutant["owner"][owned] == 2)


def test_a_capped_run_drops_the_pairs_from_the_cap_on(svo, oracle, model_world, view):
    ow, box = model_world
    cam, rect, inst, one = view
    far = IM.centred((16.0, 16.0, 60.0), 1.25, IM.rotation((1, 2, 3), 40.0))           # behind the first, partly beside it
    full = IM.trace(oracle, ow, box, cam, rect, _misses(svo, N_), [inst, far], max_rays=2 * N_)
    total = full["counts"][0]
    assert np.array_equal(full["slot"][full["pair"]], np.arange(total)) and full["stats"][1]["owned"] >= 200
    cap = one["counts"][0] + full["stats"][1]["pairs"] // 2
    capped = IM.trace(oracle, ow, box, cam, rect, _misses(svo, N_), [inst, far], max_rays=cap)
    assert capped["counts"] == (total, cap) and capped["cap"] == cap
    assert np.array_equal(capped["pair"], full["pair"])
    assert np.array_equal(capped["slot"] >= 0, full["pair"] & (full["slot"] < cap)) and np.array_equal(capped["slot"][capped["slot"] >= 0], np.arange(cap))
    assert [s["dropped"] for s in capped["stats"]] == [0, total - cap]
    # a dropped pair is no hit: the pixels instance 1 owned through a pair past the cap fall back to the G-buffer, the rest is unchanged
    lost = (full["owner"] == 2) & (full["slot"][1] >= cap)
    assert lost.sum() >= 100 and (full["owner"] == 2).sum() - lost.sum() >= 100
    assert np.all(capped["owner"][lost] == 0) and np.array_equal(capped["owner"][~lost], full["owner"][~lost])
    assert np.array_equal(capped["merged"][~lost].view(np.uint8), full["merged"][~lost].view(np.uint8))
    # the default cap is one slot per pixel, and the order of the ranks decides who is dropped
    assert IM.trace(oracle, ow, box, cam, rect, _misses(svo, N_), [inst, far])["cap"] == N_
    mutant = PixelMajor().trace(oracle, ow, box, cam, rect, _misses(svo, N_), [inst, far], max_rays=cap)
    assert np.count_nonzero(mutant["owner"] != capped["owner"]) >= 100


def test_an_occluded_instance_owns_nothing(svo, oracle, model_world, view):
    """A G-buffer of usable hits nearer than the box: no pairs.  One of hits inside the box but in front of every voxel: pairs, and
    the bounded march ends them all.  And the strict tn < far: a hit exactly where the ray enters the box is no pair."""
    ow, box = model_world
    cam, rect, inst, one = view
    o, d = M.camera_rays(oracle, cam, rect)
    om, dm = IM.to_model(o, d, inst)
    missed, tn = IM.MODEL.box_rule(om, dm, box)
    assert np.array_equal(~missed, one["pair"][0])
    g = _misses(svo, N_)
    g["flags"] = IM.HIT
    g["material"] = 1
    with np.errstate(invalid="ignore"):
        g["t"] = np.where(missed, 10.0, tn * inst[2] * np.float32(0.5))
    m = IM.trace(oracle, ow, box, cam, rect, g, [inst])
    assert m["counts"] == (0, 0) and not m["owner"].any() and np.array_equal(m["merged"].view(np.uint8), g.view(np.uint8))
    hitting = one["owner"] != 0
    g["t"] = np.where(hitting, one["merged"]["t"] * np.float32(0.999), 10.0)
    m = IM.trace(oracle, ow, box, cam, rect, g, [inst])
    assert m["counts"][0] >= 1500 and m["stats"][0]["lost_to_scene"] == hitting.sum() and not m["owner"].any()
    assert np.array_equal(m["merged"].view(np.uint8), g.view(np.uint8))
    # far == tn exactly on the pairs (scale 1, so far = t): strict, so none is a pair; `<=` would take them all
    unit = IM.centred((16.0, 16.0, 16.0), 1.0, IM.rotation((1, 2, 3), 40.0))
    om, dm = IM.to_model(o, d, unit)
    missed, tn = IM.MODEL.box_rule(om, dm, box)
    g["t"] = np.where(missed, 10.0, tn)
    assert IM.trace(oracle, ow, box, cam, rect, g, [unit])["counts"][0] == 0
    assert EntersAtOrBefore().trace(oracle, ow, box, cam, rect, g, [unit])["counts"][0] == (~missed).sum() >= 1500


def test_a_runaway_or_unusable_record_bounds_nothing(svo, oracle, model_world, view):
    ow, box = model_world
    cam, rect, inst, one = view
    g = _misses(svo, N_)
    g["t"] = 1.0
    g["flags"] = IM.HIT | IM.ERR                            # not usable: far = +inf whatever t says
    m = IM.trace(oracle, ow, box, cam, rect, g, [inst])
    assert np.array_equal(m["owner"], one["owner"]) and m["counts"] == one["counts"]
    keep = m["owner"] == 0
    assert np.array_equal(m["merged"][keep].view(np.uint8), g[keep].view(np.uint8))


def test_shadow_model_on_one_instance(svo, oracle, model_world, view):
    """Stage 2 without a scene hit in sight: the instance shadows itself through its shell and is lit through its holes; a pixel is
    written only where it is considered, and only in its flag word."""
    ow, box = model_world
    cam, rect, inst, one = view
    empty = oracle.OracleWorld.from_chunks([dict(position=(0.0, 0.0, 0.0), size=128.0, depth=4, tree=np.zeros(1, np.uint32), twig=np.zeros(0, np.uint16))],
                                           1, 1, 1, 128, (8, 8, 8))
    s = IM.shadows(oracle, empty, ow, box, cam, rect, one["merged"], one["owner"], [inst], bias=IM.BIAS)
    owned = one["owner"] != 0
    assert np.array_equal(s["considered"], owned) and not s["by_scene"].any() and s["runaways"] == 0
    assert (owned & s["by_model"]).sum() >= 300 and (owned & ~s["by_model"]).sum() >= 300
    want = one["merged"].copy()
    want["flags"][owned] |= IM.TRACED
    want["flags"][owned & s["by_model"]] |= IM.SHADOWED
    assert np.array_equal(s["merged"].view(np.uint8), want.view(np.uint8))
    again = IM.shadows(oracle, empty, ow, box, cam, rect, s["merged"], one["owner"], [inst], bias=IM.BIAS)
    assert np.array_equal(again["considered"], owned & ~s["by_model"])           # a shadowed record is settled
    assert np.array_equal(again["merged"].view(np.uint8), s["merged"].view(np.uint8))
