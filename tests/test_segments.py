"""svo_trace_segments on the GPU: rays that end at their own far end, checked record for record against the unchanged CPU oracle
(the call is defined as a filter over what svo_trace_rays writes: tests/segments_model.py), and - against the same library's
unbounded launch - that the march really ends at the far end instead of being filtered afterwards.

Run as a script - python tests/test_segments.py <libsvo_*.so> - it puts one variant build of the library through the uniform and the
near-ties case on the stack kernel (one library per process, as tests/variant_check.py)."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import local_shadows_model as LM
import segments_model as M
from helpers import assert_gbuffer_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"stack": 2, "literal": 1}
WATER = 6
W_, H_ = 128, 96
N = W_ * H_


class Scene:
    def __init__(self, svo, oracle):
        self.svo, self.oracle = svo, oracle
        self.W = svo.World.generate(2, 1, 2, 128, 8)
        self.chunks = [self.W.chunk(i) for i in range(4)]
        self.W.upload(0)
        self.ow = oracle.OracleWorld.from_chunks(self.chunks, 2, 1, 2, 128)
        self.cam = svo.default_camera(2, 2, 128, W_, H_)
        self.o, self.d = LM.camera_rays(oracle, self.cam)       # the camera's primary rays as an explicit list
        self.od, self.dd = svo.DeviceBuffer.from_numpy(self.o), svo.DeviceBuffer.from_numpy(self.d)
        self._unbounded = {}

    def unbounded(self, semantics, shadow, ow=None, world=""):
        """R: the oracle's svo_trace_rays records of the list (on `ow`, cached under the name `world`, instead of the scene's own)."""
        key = (semantics, shadow, world)
        if key not in self._unbounded:
            R = (ow or self.ow).trace_rays(self.o, self.d, params=self.oracle.make_params(shadow=shadow, semantics=semantics), threads=8)
            assert not np.any(R["flags"] & M.ERR)                # (such records are outside the equality)
            self._unbounded[key] = R
        return self._unbounded[key]

    def segments(self, tmax, counters=False, tile_cost=False, **params):
        """One svo_trace_segments launch over the list (tmax None: svo_trace_rays): (records, ray count[, counters][, tile cost])."""
        svo = self.svo
        out = svo.DeviceBuffer(N * 32)
        cnt = svo.DeviceBuffer(N * 16) if counters else None
        cost = svo.DeviceBuffer((N // 64) * 8) if tile_cost else None
        prm = svo.trace_params(counters_dev=cnt.ptr if cnt else None, tile_cost_dev=cost.ptr if cost else None, **params)
        td = None if tmax is None else svo.DeviceBuffer.from_numpy(np.ascontiguousarray(tmax, np.float32))
        if td is None:
            self.W.trace_rays(self.od.ptr, self.dd.ptr, N, prm, out.ptr)
        else:
            self.W.trace_segments(self.od.ptr, self.dd.ptr, td.ptr, N, prm, out.ptr)
        rays = self.W.last_ray_count()
        res = [out.to_numpy(svo.HIT_DTYPE, N), rays]
        if counters:
            res.append(cnt.to_numpy(np.uint32, N * 4).reshape(N, 4).astype(np.int64))
        if tile_cost:
            res.append(cost.to_numpy(np.uint32, (N // 64) * 2).reshape(N // 64, 2).astype(np.int64))
        for b in (out, cnt, cost, td):
            if b is not None:
                b.free()
        return res

    def close(self):
        self.od.free()
        self.dd.free()
        self.W.destroy()


@pytest.fixture(scope="module")
def scene(svo, oracle):
    if svo.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    s = Scene(svo, oracle)
    yield s
    s.close()


def uniform_case(s, kernel, semantics, shadow):
    R = s.unbounded(semantics, shadow)
    tmax = M.uniform(R)
    hits, keep, drop, _ = M.shares(R, tmax)
    print(f"uniform {M.UNIFORM}: kernel {kernel} semantics {semantics} shadow {shadow}: {hits} hits, {keep} kept, {drop} dropped")
    assert keep >= 0.20 * hits and drop >= 0.20 * hits          # the oracle's own records: neither side of the filter is empty
    got, rays = s.segments(tmax, kernel=kernel, semantics=semantics, shadow=shadow)
    assert_gbuffer_equal(got, M.expected(R, tmax), f"uniform far end: kernel {kernel} semantics {semantics} shadow {shadow}")
    assert rays == N + (keep if shadow else 0)


def near_ties_case(s, kernel, semantics, shadow):
    R = s.unbounded(semantics, shadow)
    tmax = M.near_ties(R)
    hits, keep, drop, ties = M.shares(R, tmax)
    print(f"near ties: kernel {kernel} semantics {semantics} shadow {shadow}: {keep} kept, {drop} dropped, {ties} exact ties")
    assert keep >= 1000 and drop >= 1000 and ties >= 1
    got, rays = s.segments(tmax, kernel=kernel, semantics=semantics, shadow=shadow)
    assert_gbuffer_equal(got, M.expected(R, tmax), f"near ties: kernel {kernel} semantics {semantics} shadow {shadow}")
    assert rays == N + (keep if shadow else 0)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("semantics", [0, 1])
def test_uniform_far_end(scene, kernel, shadow, semantics):
    uniform_case(scene, KERNELS[kernel], semantics, shadow)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("semantics", [0, 1])
def test_near_ties(scene, kernel, shadow, semantics):
    near_ties_case(scene, KERNELS[kernel], semantics, shadow)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_edge_values(svo, scene, kernel):
    s, k = scene, KERNELS[kernel]
    for shadow in (False, True):
        # +inf is svo_trace_rays, byte for byte: the oracle's records and the library's own
        R = s.unbounded(0, shadow)
        got, rays = s.segments(np.full(N, np.inf, np.float32), kernel=k, shadow=shadow)
        own, own_rays = s.segments(None, kernel=k, shadow=shadow)
        assert_gbuffer_equal(got, R, f"+inf {kernel}")
        assert np.array_equal(got.view(np.uint8), own.view(np.uint8)) and rays == own_rays
        for value in (0.0, -1.0, np.nan, -np.inf):
            got, rays = s.segments(np.full(N, value, np.float32), kernel=k, shadow=shadow)
            assert not got.view(np.uint8).any(), f"tmax {value}: not an all-miss buffer"
            assert rays == N
        mixed = np.resize(np.array([np.inf, 0.0, -1.0, np.nan, 200.0, 1e30, 1e-30], np.float32), N)
        got, _ = s.segments(mixed, kernel=k, shadow=shadow)
        assert_gbuffer_equal(got, M.expected(R, mixed), f"mixed far ends {kernel}")
        assert M.shares(R, mixed)[1] > 1000 and M.shares(R, mixed)[2] > 1000
    prm = svo.trace_params(kernel=k)
    s.W.trace_segments(s.od.ptr, s.dd.ptr, s.od.ptr, 0, prm, s.od.ptr)         # n = 0: SVO_OK, nothing is touched
    s.W.trace_segments(None, None, None, 0, prm, None)
    assert s.W.last_ray_count() == 0
    with pytest.raises(svo.SvoError) as e:
        s.W.trace_segments(s.od.ptr, s.dd.ptr, None, N, prm, s.od.ptr)
    assert e.value.code == -1


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_see_through(svo, oracle, scene, kernel):
    s = scene
    ow6 = oracle.OracleWorld.from_chunks([svo.see_through_chunk(c, WATER) for c in s.chunks], 2, 1, 2, 128)
    for shadow in (False, True):
        R6, R = s.unbounded(0, shadow, ow6, "water"), s.unbounded(0, shadow)
        assert np.count_nonzero(R6["t"].view(np.uint32) != R["t"].view(np.uint32)) > 300      # the water is in view: see_through moves hits
        tmax = M.uniform(R6)
        hits, keep, drop, _ = M.shares(R6, tmax)
        assert keep >= 0.20 * hits and drop >= 0.20 * hits
        got, rays = s.segments(tmax, kernel=KERNELS[kernel], shadow=shadow, see_through=WATER)
        assert_gbuffer_equal(got, M.expected(R6, tmax), f"see_through {kernel} shadow {shadow}")
        assert rays == N + (keep if shadow else 0)
    ow6.close()


def test_the_literal_march_ends(scene):
    """counters_dev of the bounded launch: never more than the unbounded launch read, in any word of any ray, and fewer tree steps in all."""
    s = scene
    for semantics in (0, 1):
        R = s.unbounded(semantics, False)
        tmax = M.half_way(R)
        got, _, bounded = s.segments(tmax, counters=True, kernel=1, semantics=semantics)
        _, _, free = s.segments(None, counters=True, kernel=1, semantics=semantics)
        assert_gbuffer_equal(got, M.expected(R, tmax), "half way")
        assert not (got["flags"] & 1).any()
        print(f"literal semantics {semantics}: tree steps {bounded[:, 3].sum()} bounded, {free[:, 3].sum()} unbounded; "
              f"node words {bounded[:, 0].sum()} / {free[:, 0].sum()}")
        assert np.all(bounded <= free)
        assert bounded[:, 3].sum() < free[:, 3].sum()
        miss = ~M.usable(R)                                     # tmax = +inf: the same march
        assert np.array_equal(bounded[miss], free[miss])


def test_the_stack_march_ends(scene):
    """tile_cost_dev (the kernel's own step counts, largest per tile): the bounded launch's sum is smaller than the unbounded launch's."""
    s = scene
    for semantics in (0, 1):
        R = s.unbounded(semantics, False)
        tmax = M.half_way(R)
        got, _, bounded = s.segments(tmax, tile_cost=True, kernel=2, semantics=semantics)
        _, _, free = s.segments(None, tile_cost=True, kernel=2, semantics=semantics)
        assert_gbuffer_equal(got, M.expected(R, tmax), "half way")
        print(f"stack semantics {semantics}: summed tile cost {bounded[:, 0].sum()} bounded, {free[:, 0].sum()} unbounded")
        assert free[:, 0].sum() > 0 and not bounded[:, 1].any()
        assert bounded[:, 0].sum() < free[:, 0].sum()


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_ray_count(scene, kernel):
    s = scene
    R = s.unbounded(0, True)
    hits = int(M.usable(R).sum())
    for tmax, keep in ((M.uniform(R), M.shares(R, M.uniform(R))[1]), (np.full(N, np.inf, np.float32), hits), (np.zeros(N, np.float32), 0)):
        assert s.segments(tmax, kernel=KERNELS[kernel], shadow=False)[1] == N
        assert s.segments(tmax, kernel=KERNELS[kernel], shadow=True)[1] == N + keep
    assert 0 < M.shares(R, M.uniform(R))[1] < hits


def test_chunkmarch_takes_a_far_end(scene):
    s = scene
    R = s.unbounded(0, True)
    got = s.W.chunkmarch(s.o, s.d, shadow=True, tmax=M.UNIFORM)
    assert_gbuffer_equal(got, M.expected(R, M.uniform(R)), "World.chunkmarch(tmax=)")
    assert_gbuffer_equal(s.W.chunkmarch(s.o, s.d, shadow=True), R, "World.chunkmarch()")


def variant_libraries():
    return sorted(glob.glob(os.path.join(ROOT, "octree-raymarcher_amd", "build", "libsvo_*.so")))


def test_variants():
    """The uniform and the near-ties case, stack kernel, through every library under build/ (SVO_AMD_LIB; one library per process)."""
    from test_variants import VARIANTS, lib_of
    libs = variant_libraries()
    for name in sorted({n for n, _ in VARIANTS}):
        assert lib_of(name) in libs, f"{lib_of(name)} missing: __graft_entry__.build() makes it"
    for lib in libs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), lib], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, lib + "\n" + r.stdout[-3000:] + r.stderr[-3000:]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from variant_check import load
    svo_, ob_ = load(os.path.abspath(sys.argv[1]))
    if svo_.device_count() < 1:
        print("no HIP device")
        sys.exit(3)
    s0 = Scene(svo_, ob_)
    for semantics_ in (0, 1):
        for shadow_ in (False, True):
            uniform_case(s0, 2, semantics_, shadow_)
            near_ties_case(s0, 2, semantics_, shadow_)
    s0.close()
    print("segments: records equal to the filtered oracle's")
