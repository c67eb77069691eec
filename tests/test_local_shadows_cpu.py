"""svo_trace_local_shadows (one shadow flag per local light): the C ABI surface, the argument checks that run before any device
work, and the host model the GPU tests compare with, on hand-made rays.  CPU only."""
import os
import re
import subprocess

import numpy as np
import pytest

import local_shadows_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 1 << 30


def test_new_symbol_and_flags_are_declared_and_exported(svo):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svo.h")).read(), flags=re.S)
    assert re.search(r"\bsvo_trace_local_shadows\s*\(", header)
    assert "svo_trace_local_shadows" in svo.ABI_SYMBOLS and hasattr(svo.lib, "svo_trace_local_shadows")
    out = subprocess.run(["nm", "-D", "--defined-only", svo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T svo_trace_local_shadows$", out, flags=re.M)
    for name, shift, value in (("SVO_LOCAL_SHADOWS", 5, svo.LOCAL_SHADOWS), ("SVO_SHADOWED_POINT", 6, svo.SHADOWED_POINT), ("SVO_SHADOWED_SPOT", 7, svo.SHADOWED_SPOT)):
        assert re.search(name + r"\s*=\s*1u << %d\b" % shift, header), name
        assert value == 1 << shift
    assert (M.LOCAL_SHADOWS, M.SHADOWED_POINT, M.SHADOWED_SPOT) == (svo.LOCAL_SHADOWS, svo.SHADOWED_POINT, svo.SHADOWED_SPOT)
    assert "#define SVO_ABI_VERSION 4" in header and svo.lib.svo_abi_version() == 4


def test_flag_bits_fit_the_packed_record(svo):
    """The packed record carries flags & 0xFF (include/svo.h): the three bits lie inside it and collide with no other flag."""
    new = svo.LOCAL_SHADOWS | svo.SHADOWED_POINT | svo.SHADOWED_SPOT
    old = svo.HIT_FLAG | svo.SHADOW_TRACED | svo.SHADOWED | svo.FACE_NORMAL | svo.SEE_THROUGH | svo.ERR_FLAG
    assert new & 0xFF == new and new & old == 0


def test_argument_validation_precedes_any_device_work(svo):
    W = svo.World.create([dict(position=(0, 0, 0), size=128.0, depth=4, tree=np.array([L | 6], np.uint32), twig=np.zeros(0, np.uint16))], 1, 1, 1, 128)
    cam = svo.default_camera(1, 1, 128, 8, 8)
    fake = 256                                                  # never dereferenced: every call below fails before device work
    prm = svo.trace_params()
    rect = (0, 0, 8, 8)
    bad = [dict(cam=None), dict(params=None), dict(gbuffer_ptr=None), dict(point=None, spot=None), dict(rect=(0, 0, -1, 8)), dict(rect=(0, 0, 8, -1)),
           dict(rect=(-1, 0, 8, 8)), dict(params=svo.trace_params(see_through=0x10000))]
    for change in bad:
        kw = dict(cam=cam, params=prm, rect=rect, gbuffer_ptr=fake, point=M.POINT, spot=M.SPOT)
        kw.update(change)
        with pytest.raises(svo.SvoError) as e:
            W.trace_local_shadows(kw["cam"], kw["params"], kw["rect"], kw["gbuffer_ptr"], point=kw["point"], spot=kw["spot"])
        assert e.value.code == -1, change
    assert svo.lib.svo_trace_local_shadows(None, cam, prm, None, None, 0, 0, 8, 8, fake, None) == -1       # a null world
    for point, spot in ((M.POINT, M.SPOT), (M.POINT, None), (None, M.SPOT)):
        with pytest.raises(svo.SvoError) as e:
            W.trace_local_shadows(cam, prm, rect, fake, point=point, spot=spot)
        assert e.value.code == -5                               # SVO_ERR_NOT_UPLOADED: generated, not resident
    W.destroy()
    G = svo.World.generate(1, 1, 1, 128, 4)
    with pytest.raises(svo.SvoError) as e:
        G.trace_local_shadows(cam, prm, rect, fake, point=M.POINT)
    assert e.value.code == -5
    G.destroy()


def test_model_on_hand_made_rays():
    """light_rays: float32 throughout, the left-to-right sum, no ray where the light sits on the point or q overflows."""
    P = np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [4.0, 6.0, 3.0], [3e38, 0.0, 0.0]], np.float32)
    valid, dirs, dist = M.light_rays(P, (1.0, 2.0, 3.0))
    assert list(valid) == [False, True, True, False]
    assert dist[1] == np.sqrt(np.float32(14.0)) and dist[2] == np.float32(5.0)
    assert np.array_equal(dirs[2], np.array([-3.0, -4.0, 0.0], np.float32) * (np.float32(1.0) / np.float32(5.0)))
    # the sum is (x*x + y*y) + z*z in float32: 2^24 + 1 is lost from the left, kept from the right
    v = np.array([[4096.0, 1.0, 1.0]], np.float32)
    _, _, d1 = M.light_rays(-v, (0.0, 0.0, 0.0))
    assert d1[0] == np.sqrt(np.float32(np.float32(16777216.0 + 1.0) + np.float32(1.0)))
    assert M.resolved_eps(0) == np.float32(1 / 8192) and M.resolved_eps(1) == np.float32(1 / 4096) and M.resolved_eps(1, 0.5) == np.float32(0.5)


def test_model_reproduces_the_measured_shares(svo, oracle):
    """The oracle alone, on the GPU tests' scene: the shares the conditions of tests/test_local_shadows.py rest on."""
    W = svo.World.generate(2, 1, 2, 128, 8)
    ow = oracle.OracleWorld.from_chunks([W.chunk(i) for i in range(4)], 2, 1, 2, 128)
    cam = svo.default_camera(2, 2, 128, 128, 96)
    for semantics, want in ((0, dict(point=(0.843, 0.471, 1093), spot=(0.801, 0.484, 970))), (1, dict(point=(0.834, 0.468, 1150), spot=(0.794, 0.481, 1019)))):
        frame = ow.trace_image(cam, params=oracle.make_params(shadow=True, semantics=semantics), threads=8)
        stats = {}
        out = M.expected(oracle, ow, cam, None, frame, M.POINT, M.SPOT, semantics, stats)
        for light, (occluded, differs, behind) in want.items():
            s = stats[light]
            assert s["hits"] == 7087 and s["behind"] == behind and s["runaways"] == 0 and s["nearest"] > 1e-3
            assert abs(s["occluded"] - occluded) < 1e-3 and abs(s["differs"] - differs) < 1e-3
        sel = M.usable(frame.reshape(-1))
        assert np.array_equal(out[~sel].view(np.uint8), frame.reshape(-1)[~sel].view(np.uint8))
    W.destroy()
