"""The chunk step of the stack kernel (chunk_step_asm.hip.h: one hand-scheduled statement; the C++ twin of chunk_step_cxx.hip.h in the
`cxxstep` build) on the cases the grids of tests/test_gpu_blocks.py do not reach - tests/chunk_step_cases.py lists them: rays that end on
cap_chunk 1, 2, 3 in each chunk of their path, origins outside the world (beside it, in front of it, grazing, corners and edges), origins on chunk faces
and on negative exact multiples of the chunk edge (the containment test ends them), zero direction components from a lattice plane, a
shifted world, chunks of mixed depth side by side, a chunk table outside LDS, shadow rays on and off, the shader twin's step past a
box that does not contain its point, and bounded rays whose far end lies one float before, on and behind a chunk face.

Worlds of depth 3 - 5, lists of 4,096 rays, one small camera per world.  Every field is compared with the oracle's as tests/helpers.py
does - integer fields equal, t bit-identical - through the shipped library and, each in its own process, through the `cxxstep`, `wide64`
and `timing` builds that build() makes.  The oracle's records are computed once per session; the first test checks on them,
without a GPU, that every list reaches what it is for."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chunk_step_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "octree-raymarcher_amd", "build")
RUNNER = os.path.join(ROOT, "tests", "chunk_step_cases.py")


@pytest.fixture(scope="module")
def reference(svo, oracle, tmp_path_factory):
    ref = cases.reference(svo, oracle)
    path = str(tmp_path_factory.mktemp("chunk_step") / "reference.npz")
    np.savez(path, **ref)
    return ref, path


def test_cases_reach_what_they_are_for(svo, reference):
    ref, _ = reference
    HIT = svo.HIT_FLAG
    lists = cases.case_lists()
    hit = lambda r: (r["flags"] & HIT) != 0
    # caps: with cap_chunk k a ray visits k chunks at the most - rays that hit uncapped are cut off at every k, fewer at each, and what
    # is left hits in every chunk of the world
    for key in ("caps/random", "caps/flat"):
        free = ref[key + "/free"]
        lost = [int((hit(free) & ~hit(ref[f"{key}/{cap}"])).sum()) for cap in cases.CAPS]
        assert lost[0] > lost[1] > lost[2] > 0, (key, lost)             # rays end on the cap in their 1st, 2nd and 3rd chunk
        for cap in cases.CAPS:
            r = ref[f"{key}/{cap}"]
            assert not (hit(r) & ~hit(free)).any(), (key, cap)
            assert hit(r).sum() > 100, (key, cap)
        assert set(free["chunk"][hit(free)].tolist()) == set(range(6)), key
    # outside: misses of the box, hits, and rays in a face plane / at a corner that go either way
    q = cases.RAYS // 4
    r = ref["outside/1"]
    assert not hit(r[:q:2]).any() and 0 < hit(r[1:q:2]).sum()          # beside the box; the box behind the origin
    assert 0 < hit(r[q:2 * q]).sum() < q and 0 < hit(r[2 * q:3 * q]).sum() < q and 0 < hit(r[3 * q:4 * q]).sum() < q
    # faces: origins the chunk found for them does not contain - they end there (CPU march), hits in every chunk otherwise
    for name in ("3x1x2neg", "2x2x2neg"):
        dims = cases.GRIDS[name][0]
        out = ref[f"faces/{name}/uncontained"]
        r = ref[f"faces/{name}/1"]
        assert out.sum() > 50 and not hit(r[out]).any(), (name, int(out.sum()))
        assert len(set(r["chunk"][hit(r)].tolist())) >= 6 and max(r["chunk"][hit(r)]) < dims[0] * dims[1] * dims[2], name
        _, o, d = lists[f"faces/{name}"]
        on_plane = (np.mod(o, cases.CHUNK) == 0)
        assert ((d == 0) & on_plane).any(axis=1).sum() > 500, name            # 0 * inf in the escape distance
        assert ((o < 0) & on_plane).any(axis=1).sum() > 200, name             # negative exact multiples
        assert (ref[f"faces/{name}/0"]["flags"] & svo.SHADOWED).sum() == 0 and (r["flags"] & svo.SHADOWED).sum() > 0, name
    # the shader twin steps on where the CPU march ends the ray: some of those origins hit
    out = ref["faces/2x2x2neg/uncontained"]
    assert hit(ref["glsl/faces"][out]).sum() > 10
    assert hit(ref["glsl/image"]).sum() > 100
    # table outside LDS, shift, mixed depths: hits all over the grid, shadowed ones among them
    r = ref["table/1"]
    assert len(set(r["chunk"][hit(r)].tolist())) > 40 and max(r["chunk"][hit(r)]) < 72
    g = ref["table/glsl"]
    assert len(set(g["chunk"][hit(g)].tolist())) > 40 and (g["flags"] & svo.SHADOWED).sum() > 0
    for sem, key in ((0, "table/1"), (1, "table/glsl")):
        hits, kept, dropped, _ = cases.seg.shares(ref[key], cases.seg.near_ties(ref[key]))
        assert kept > 100 and dropped > 100, (key, hits, kept, dropped)
    for name in ("3x1x2", "9x1x8"):
        assert hit(ref[f"image/{name}"]).sum() > 100, name
    assert tuple(ref["shift/ccm"]) == (1, 0, 0)
    for what in ("shift/random", "shift/faces", "shift/image"):
        r = ref[what].reshape(-1)
        assert hit(r).sum() > 100 and (r["flags"] & svo.SHADOWED).sum() > 0, what
    assert set(ref["shift/random"]["chunk"][hit(ref["shift/random"])].tolist()) == set(range(6))
    for what in ("mixed/random", "mixed/faces", "mixed/image"):
        r = ref[what].reshape(-1)
        assert hit(r).sum() > 100, what
    assert set(ref["mixed/random"]["chunk"][hit(ref["mixed/random"])].tolist()) == {0, 1, 2, 3}
    # segments: far ends on every side of the first face, kept and dropped hits, a far end in front of hits in the NEXT chunk
    o, d, tmax = cases.segment_list()
    for sem in (0, 1):
        r = ref[f"segments/{sem}"]
        hits, kept, dropped, _ = cases.seg.shares(r, tmax)
        assert hits > 500 and kept > 100 and dropped > 100, (sem, hits, kept, dropped)
        kind = np.arange(len(tmax)) % 5
        for k in (0, 1, 2):                 # one float before / on / one float behind the face: hits beyond the face are dropped
            sel = (kind == k) & cases.seg.usable(r)
            assert (sel & ~cases.seg.kept(r, tmax)).sum() > 20, (sem, k)


@pytest.mark.gpu
def test_every_case_equals_the_oracle(svo, reference):
    cases.march_all(svo, reference[0])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["cxxstep", "wide64", "timing"])
def test_variant_build_equals_the_oracle(variant, reference):
    lib = os.path.join(BUILD, f"libsvo_{variant}.so")
    assert os.path.exists(lib), f"{lib} missing: __graft_entry__.build() makes it (make -C octree-raymarcher_amd variants)"
    r = subprocess.run([sys.executable, RUNNER, lib, reference[1]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
