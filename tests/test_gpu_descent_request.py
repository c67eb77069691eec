"""The stack kernel's descent through BRANCH entries on the smallest trees that have them ("the next wide level
requested a step early"): a lane at a BRANCH entry pushes the child wide node onto its LDS column and either sits the step out or takes
the level inside the step (step_asm_body.inc, "3:").  Anything that moves a load or a wait there - the experiment of that section did -
can go wrong in two ways only, a bad address or a mis-ordered wait, and either shows as a wrong record.  So: single chunks of depth
3 - 7 (levels 1 - 5: odd and even, one to three wide levels) and a 2x1x2 world of mixed depths; a seeded random list and a list of
axis-parallel rays on the pitch of the deepest wide nodes +- one voxel; shadow ray on; both semantics; integer fields equal and t
bit-identical to the oracle's (tests/helpers.py).  The same lists go through the large-pool addressing (`wide64`) and the timing build
where build() has made them, each in its own process; the timing build's counters must show that the lists reach BRANCH entries.

The oracle's records are computed once per session and shared by every test here."""
import os
import subprocess
import sys

import numpy as np
import pytest

import descent_request_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "octree-raymarcher_amd", "build")
RUNNER = os.path.join(ROOT, "tests", "descent_request_cases.py")


@pytest.fixture(scope="module")
def reference(svo, oracle, tmp_path_factory):
    """{f"{world}/{list}/{semantics}": the oracle's records}, also as an .npz for the processes that march a variant build."""
    ref = {}
    for name, dims, depths in cases.WORLDS:
        chunks = cases.chunks_of(svo, dims, depths)
        O = oracle.OracleWorld.from_chunks(chunks, *dims, cases.CHUNK)
        for lname, (o, d) in cases.ray_lists(name, dims, depths).items():
            for sem in cases.SEMANTICS:
                ref[f"{name}/{lname}/{sem}"] = O.trace_rays(o, d, params=oracle.make_params(shadow=True, semantics=sem), threads=8)
    path = str(tmp_path_factory.mktemp("descent") / "reference.npz")
    np.savez(path, **ref)
    return ref, path


@pytest.mark.gpu
def test_lists_reach_the_terrain(reference):
    """The lists are worth marching: in every world both of them hit voxels and cast shadow rays."""
    ref, _ = reference
    for key, want in ref.items():
        assert int((want["flags"] & 1).sum()) > 100, key


@pytest.mark.gpu
def test_stack_kernel_equals_the_oracle(svo, reference):
    ref, _ = reference
    cases.march_all(svo, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["wide64", "timing"])
def test_variant_build_equals_the_oracle(variant, reference):
    lib = os.path.join(BUILD, f"libsvo_{variant}.so")
    if not os.path.exists(lib):
        pytest.skip(f"{lib} is absent: __graft_entry__.build() makes it (make -C octree-raymarcher_amd variants)")
    _, path = reference
    r = subprocess.run([sys.executable, RUNNER, lib, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
