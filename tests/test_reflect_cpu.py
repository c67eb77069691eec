"""Mirror reflections without a GPU: what the scenes of tests/test_reflect.py hold (asserted on the CPU oracle's own result, so that no
GPU comparison passes vacuously), the float64 ray-shading restatement of tests/reflect_model.py against shade_model.terms, why the
mirror ray starts on the face plane and not at the sample point, and the statuses both entry points settle before any device work."""
import numpy as np
import pytest

import hit_voxels_model as H
import reflect_model as M
import shade_model as S

INVALID, NOT_UPLOADED = -1, -5
MATERIAL = {"lakeN": M.WATER, "lakeW": M.WATER, "default": 0}


@pytest.fixture(scope="module")
def scene(svo, oracle):
    W = svo.World.generate(*M.WORLD)
    chunks = [W.chunk(i) for i in range(4)]
    ow = oracle.OracleWorld.from_chunks(chunks, 2, 1, 2, 128)
    made = {}

    def frame(view, semantics=0):
        if (view, semantics) not in made:
            cam = M.camera(svo, view)
            g = ow.trace_image(cam, params=oracle.make_params(shadow=True, semantics=semantics), threads=8).reshape(-1)
            v = H.hit_voxels(chunks, g)
            rays, want = M.reflect_records(oracle, ow, cam, (0, 0, *M.IMAGE), g, v, MATERIAL[view], shadow=True, semantics=semantics)
            made[(view, semantics)] = (cam, g, v, rays, want)
        return made[(view, semantics)]

    yield W, ow, frame
    W.destroy()


@pytest.mark.parametrize("semantics", [0, 1])
@pytest.mark.parametrize("view", sorted(M.VIEWS))
def test_the_scenes_hold_what_the_gpu_tests_compare(scene, view, semantics):
    _, _, frame = scene
    cam, g, v, rays, want = frame(view, semantics)
    on = rays["on"]
    n, mirrors = on.size, int(on.sum())
    hits = int(((want["flags"] & M.HIT_FLAG) != 0)[on].sum())
    misses = mirrors - hits
    axes = np.bincount(rays["axis"][on], minlength=3)
    print(f"{view} semantics {semantics}: {mirrors} mirror pixels of {n}, axes x/y/z {axes.tolist()}, {hits} reflected hits, {misses} misses")
    assert n == 12288
    assert not (g["flags"] & M.ERR_FLAG).any() and not (want["flags"] & M.ERR_FLAG).any()
    assert not want[~on].view(np.uint8).any()
    if view == "lakeN":
        assert mirrors >= 0.40 * n and hits >= 0.20 * mirrors and misses >= 0.20 * mirrors
    elif view == "lakeW":
        assert hits >= 0.80 * mirrors and misses >= 150
    else:
        assert axes.min() >= 500 and hits >= 0.30 * mirrors and misses >= 0.30 * mirrors
    if MATERIAL[view]:
        assert np.all(g["material"][on] == MATERIAL[view])
        assert (rays["axis"][on] == 1).sum() >= 0.99 * mirrors and np.all(rays["R"][on & (rays["axis"] == 1), 1] > 0), "the lake is seen from above"


def test_ray_shading_restatement_equals_the_shade_model(svo, scene):
    """shade_rays fed the camera's own rays is shade_model.terms: on a traced frame and on the synthetic general case."""
    _, _, frame = scene
    cam, g, _, _, _ = frame("default")
    cases = [(cam, svo.shade_defaults(), (0, 0, *M.IMAGE), g), S.general_case(svo), S.general_case(svo, dict(gamma=2.4))]
    for cam, P, rect, records in cases:
        T = S.terms(cam, P, rect, records)
        eye = np.broadcast_to(np.array(list(cam.eye), np.float64), T["beta"].shape)
        rgb, cond = M.shade_rays(P, eye, S._rays(cam, rect), records)
        hit = (np.asarray(records).reshape(-1)["flags"] & 1) != 0
        assert hit.sum() > 1000
        assert np.array_equal(np.isnan(rgb[hit]), np.isnan(T["rgba"][hit, :3]))
        assert np.allclose(rgb[hit], T["rgba"][hit, :3], rtol=0.0, atol=1e-12, equal_nan=True)
        assert np.allclose(cond[hit], T["cond"][hit], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("view,least", [("default", 150), ("lakeN", 900)])
def test_a_ray_from_the_sample_point_hits_its_own_voxel(svo, oracle, scene, view, least):
    """Rule 3 left out (O = P), the water of both views: the sample point lies on or inside the closed box of its voxel, and the march
    reports that voxel again at t = 0.  With the origin on the face plane that is gone.  So a kernel that starts at P cannot pass the
    GPU tests."""
    _, ow, frame = scene
    cam, g, v, _, _ = frame(view)
    rect = (0, 0, *M.IMAGE)
    rays, want = M.reflect_records(oracle, ow, cam, rect, g, v, M.WATER, shadow=True)
    _, naive = M.reflect_records(oracle, ow, cam, rect, g, v, M.WATER, shadow=True, origin_on_face=False)
    on = rays["on"]

    def own(r):                                                 # the reflected ray hit the voxel it left
        return on & ((r["flags"] & 1) != 0) & (r["chunk"] == g["chunk"]) & (r["node"] == g["node"]) & (r["cell"] == g["cell"])

    differ = on & ((naive["flags"] != want["flags"]) | (naive["chunk"] != want["chunk"]) | (naive["node"] != want["node"]) | (naive["cell"] != want["cell"]))
    near = int((on & ((want["flags"] & 1) != 0) & (want["t"] < 0.01)).sum())
    print(f"{view}: {int(on.sum())} mirror pixels, {int(((naive['flags'] & 1) != 0)[on].sum())} reflected hits from P, {int(own(naive).sum())} of them "
          f"their own voxel; {int(differ.sum())} records differ from the model, which has {int(own(want).sum())} self-hits and {near} hits with t < 0.01")
    self_hits = own(naive) & differ
    assert self_hits.sum() >= least
    assert np.all(naive["t"][self_hits] < 0.01)
    assert own(want).sum() == 0 and near <= 1


def _code(svo, call, *args, **kw):
    with pytest.raises(svo.SvoError) as e:
        call(*args, **kw)
    return e.value.code


def test_trace_reflections_settles_its_arguments_before_the_residency(svo, scene):
    """On a world that is not uploaded: every SVO_ERR_INVALID_ARG case comes before SVO_ERR_NOT_UPLOADED (the dummy pointers are never
    dereferenced)."""
    W, _, _ = scene
    cam, prm, rect, ptr = M.camera(svo, "lakeN"), svo.trace_params(shadow=True), (0, 0, *M.IMAGE), 0x1000
    cold = svo.World(None)
    assert _code(svo, cold.trace_reflections, cam, prm, rect, ptr, ptr, ptr) == INVALID
    assert _code(svo, W.trace_reflections, None, prm, rect, ptr, ptr, ptr) == INVALID
    assert _code(svo, W.trace_reflections, cam, None, rect, ptr, ptr, ptr) == INVALID
    for bufs in ((None, ptr, ptr), (ptr, None, ptr), (ptr, ptr, None)):
        assert _code(svo, W.trace_reflections, cam, prm, rect, *bufs) == INVALID
    for bad in ((0, 0, -1, 4), (0, 0, 4, -1), (-2, 0, 4, 4), (0, -2, 4, 4)):
        assert _code(svo, W.trace_reflections, cam, prm, bad, ptr, ptr, ptr) == INVALID
    assert _code(svo, W.trace_reflections, cam, prm, rect, ptr, ptr, ptr, material=0x10000) == INVALID
    assert _code(svo, W.trace_reflections, cam, svo.trace_params(see_through=0x10000), rect, ptr, ptr, ptr) == INVALID
    # then the residency: also for an empty rectangle, for a rectangle too large, and before the semantics and the kernel id are looked at
    assert _code(svo, W.trace_reflections, cam, prm, rect, ptr, ptr, ptr) == NOT_UPLOADED
    assert _code(svo, W.trace_reflections, cam, prm, rect, ptr, ptr, ptr, material=M.WATER) == NOT_UPLOADED
    assert _code(svo, W.trace_reflections, cam, prm, (0, 0, 0, 7), None, None, None) == NOT_UPLOADED
    assert _code(svo, W.trace_reflections, cam, prm, (0, 0, 1 << 16, 1 << 16), ptr, ptr, ptr) == NOT_UPLOADED
    assert _code(svo, W.trace_reflections, cam, svo.trace_params(semantics=7), rect, ptr, ptr, ptr) == NOT_UPLOADED
    assert _code(svo, W.trace_reflections, cam, svo.trace_params(kernel=9), rect, ptr, ptr, ptr) == NOT_UPLOADED


def test_shade_reflections_refusals(svo):
    cam, P, rect, ptr = M.camera(svo, "lakeW"), svo.shade_defaults(), (0, 0, *M.IMAGE), 0x1000
    good = svo.Mirror(M.WATER, 0.02, True, (0.1, 0.2, 0.3))

    def code(cam=cam, P=P, mirror=good, rect=rect, bufs=(ptr, ptr, ptr, ptr)):
        return _code(svo, svo.shade_reflections, cam, P, mirror, rect, *bufs)

    assert code(cam=None) == INVALID and code(P=None) == INVALID and code(mirror=None) == INVALID
    for k in range(4):
        assert code(bufs=tuple(None if j == k else ptr for j in range(4))) == INVALID
    for f0 in (-0.01, 1.01, float("nan"), float("inf")):
        assert code(mirror=svo.Mirror(M.WATER, f0)) == INVALID
    assert code(mirror=svo.Mirror(0x10000, 0.5)) == INVALID
    for bg in ((float("nan"), 0, 0), (0, float("inf"), 0), (0, 0, -float("inf"))):
        assert code(mirror=svo.Mirror(M.WATER, 0.5, background=bg)) == INVALID
    skies = [svo.Sky((ptr,) * 5 + (None,), 4), svo.Sky((ptr,) * 6, 0), svo.Sky((ptr,) * 6, 4, filter=2), svo.Sky((None,) + (ptr,) * 5, 4)]
    for sky in skies:
        assert code(mirror=svo.Mirror(M.WATER, 0.5, sky=sky)) == INVALID
    for bad in ((0, 0, -1, 4), (0, 0, 4, -1), (-2, 0, 4, 4), (0, -2, 4, 4)):
        assert code(rect=bad) == INVALID
    nocam = svo.make_camera((0, 0, 0), (0, 0, 1), (0, 1, 0), 60.0, 8, 8)
    nocam.width = 0
    assert code(cam=nocam) == INVALID
    # an empty rectangle is SVO_OK with no buffers at all, but not with a bad mirror; f0 = 0 and f0 = 1 are in range
    for f0 in (0.0, 1.0):
        svo.shade_reflections(cam, P, svo.Mirror(0, f0, False), (3, 4, 0, 9), None, None, None, None)
    svo.shade_reflections(cam, P, svo.Mirror(M.WATER, 0.5, sky=svo.Sky((ptr,) * 6, 4)), (3, 4, 9, 0), None, None, None, None)
    assert code(mirror=svo.Mirror(M.WATER, 2.0), rect=(0, 0, 0, 0), bufs=(None,) * 4) == INVALID
    # a rectangle whose grid does not fit one launch: behind the argument check, before any launch
    assert code(rect=(0, 0, 1 << 20, 1 << 20)) == -6


def test_the_struct_matches_the_header(svo, tmp_path):
    import ctypes as C
    import os
    import subprocess
    src = '#include "svo.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n",sizeof(svo_mirror),' \
          'offsetof(svo_mirror,material),offsetof(svo_mirror,f0),offsetof(svo_mirror,fresnel),offsetof(svo_mirror,background),offsetof(svo_mirror,sky));return 0;}'
    exe = str(tmp_path / "svo_mirror_layout")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-x", "c", "-", "-o", exe], input=src, text=True, check=True)
    sizes = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    T = svo.Mirror
    assert sizes == [C.sizeof(T), T.material.offset, T.f0.offset, T.fresnel.offset, T.background.offset, T.sky.offset]
