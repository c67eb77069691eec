"""svo_trace_segments (bounded rays): the C ABI surface, the argument checks that run before any device work, the host model
(tests/segments_model.py) on hand-made records, and - on the oracle alone - the input conditions the GPU tests of
tests/test_segments.py rest on.  CPU only."""
import os
import re
import subprocess

import numpy as np
import pytest

import local_shadows_model as LM
import segments_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 1 << 30


def test_new_symbol_is_declared_and_exported(svo):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svo.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+svo_trace_segments\s*\(\s*svo_world\s*\*\s*,\s*const float\s*\*\s*origins_dev\s*,\s*const float\s*\*\s*dirs_dev\s*,\s*"
                     r"const float\s*\*\s*tmax_dev\s*,\s*int64_t n\s*,\s*const svo_trace_params\s*\*\s*params\s*,\s*svo_hit\s*\*\s*out_dev\s*,\s*void\s*\*\s*stream\s*\)", header)
    assert "svo_trace_segments" in svo.ABI_SYMBOLS and hasattr(svo.lib, "svo_trace_segments")
    out = subprocess.run(["nm", "-D", "--defined-only", svo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T svo_trace_segments$", out, flags=re.M)
    assert "#define SVO_ABI_VERSION 4" in header and svo.lib.svo_abi_version() == 4


def test_argument_validation_precedes_any_device_work(svo):
    W = svo.World.create([dict(position=(0, 0, 0), size=128.0, depth=4, tree=np.array([L | 6], np.uint32), twig=np.zeros(0, np.uint16))], 1, 1, 1, 128)
    fake = 256                                                  # never dereferenced: every call below fails before device work
    prm = svo.trace_params()
    with pytest.raises(svo.SvoError) as e:                      # no far ends
        W.trace_segments(fake, fake, None, 8, prm, fake)
    assert e.value.code == -1 and "tmax" in str(e.value)
    for o, d, out, n in ((None, fake, fake, 8), (fake, None, fake, 8), (fake, fake, None, 8), (fake, fake, fake, -1)):
        with pytest.raises(svo.SvoError) as e:
            W.trace_segments(o, d, fake, n, prm, out)
        assert e.value.code in (-1, -5)
    with pytest.raises(svo.SvoError) as e:
        W.trace_segments(fake, fake, fake, 8, svo.trace_params(see_through=0x10000), fake)
    assert e.value.code == -1
    with pytest.raises(svo.SvoError) as e:                      # a world that is not resident
        W.trace_segments(fake, fake, fake, 8, prm, fake)
    assert e.value.code == -5
    assert svo.lib.svo_trace_segments(None, fake, fake, fake, 8, prm, fake, None) == -1
    W.destroy()


def records(svo, rows):
    r = np.zeros(len(rows), svo.HIT_DTYPE)
    for k, (t, flags) in enumerate(rows):
        r[k]["t"], r[k]["flags"], r[k]["material"], r[k]["node"] = t, flags, 3, 7 + k
    return r


def test_model_on_hand_made_records(svo):
    r = records(svo, [(10.0, 1), (10.0, 1), (10.0, 1), (10.0, 1 | M.ERR), (0.0, 0), (10.0, 1 | 2 | 4), (10.0, 1), (10.0, 1), (10.0, 1)])
    tmax = np.array([10.5, 10.0, np.nextafter(np.float32(10.0), np.float32(11.0)), 99.0, 99.0, np.inf, 0.0, -1.0, np.nan], np.float32)
    assert list(M.kept(r, tmax)) == [True, False, True, False, False, True, False, False, False]      # strict; ERR and misses never; NaN false
    out = M.expected(r, tmax)
    keep = M.kept(r, tmax)
    assert np.array_equal(out[keep].view(np.uint8), r[keep].view(np.uint8))                     # kept records byte for byte, shadow bits included
    assert not out[~keep].view(np.uint8).any()                                                  # the others all zero
    assert np.array_equal(M.expected(r, np.inf)[M.usable(r)].view(np.uint8), r[M.usable(r)].view(np.uint8))
    assert M.shares(r, tmax) == (7, 3, 4, 1)
    # the far-end inputs
    assert list(M.near_ties(r)) == [200.0, 10.0, 10.0, 10.0, 200.0, 200.0, 10.0, 10.0, 10.0]
    h = M.half_way(r)
    assert h[0] == 5.0 and np.isinf(h[3]) and np.isinf(h[4]) and not M.kept(r, h).any()
    assert M.uniform(r).dtype == np.float32 and np.all(M.uniform(r) == 200.0)


def test_inputs_keep_the_gpu_comparisons_from_passing_vacuously(svo, oracle):
    """The oracle alone, on the GPU tests' scene: the shares of kept and dropped hits and the exact ties of every far-end input."""
    W = svo.World.generate(2, 1, 2, 128, 8)
    ow = oracle.OracleWorld.from_chunks([W.chunk(i) for i in range(4)], 2, 1, 2, 128)
    cam = svo.default_camera(2, 2, 128, 128, 96)
    o, d = LM.camera_rays(oracle, cam)
    for semantics in (0, 1):
        R = ow.trace_rays(o, d, params=oracle.make_params(shadow=True, semantics=semantics), threads=8)
        assert R.shape[0] == 12288 and not np.any(R["flags"] & M.ERR)
        hits, keep, drop, _ = M.shares(R, M.uniform(R))
        print(f"semantics {semantics} uniform 200: {hits} hits, {keep} kept, {drop} dropped")
        assert hits == 7087 and keep >= 0.20 * hits and drop >= 0.20 * hits
        assert abs(keep / hits - 0.481) < 2e-3
        for value, share in ((150.0, 0.228), (250.0, 0.824)):
            assert abs(M.shares(R, M.uniform(R, value))[1] / hits - share) < 2e-3
        hits, keep, drop, ties = M.shares(R, M.near_ties(R))
        print(f"semantics {semantics} near ties: {keep} kept, {drop} dropped, {ties} exact ties")
        assert keep >= 1000 and drop >= 1000 and ties >= 1
        hits, keep, drop, _ = M.shares(R, M.half_way(R))
        assert keep == 0 and drop == 7087
        # shadow bits do not move t: the far ends made from either launch are the same
        R0 = ow.trace_rays(o, d, params=oracle.make_params(shadow=False, semantics=semantics), threads=8)
        assert np.array_equal(R0["t"].view(np.uint32), R["t"].view(np.uint32))
    W.destroy()
