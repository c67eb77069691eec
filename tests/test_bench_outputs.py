"""bench.py --dump-outputs: the last timed step's G-buffer as <field>.npy in float32 / float64, finite, under 64 MB, the
same pixels in every file; and a plain run's result line (no --full) carries the headline fields and nothing of --full's legs."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HIT = np.dtype([("t", "<f4"), ("normal", "<f4", (3,)), ("material", "<u2"), ("flags", "<u2"),
                ("chunk", "<u4"), ("node", "<u4"), ("cell", "<u4")])


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _records(n, seed):
    """Records as the kernels write them: random ids and flags, finite t, normals that are a normalised vector of
    {-1,0,1}^3, the reference's all-NaN normal, or a miss's zero vector."""
    rng = np.random.default_rng(seed)
    recs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8).view(HIT).reshape(n)
    recs["t"] = rng.uniform(0.0, 2000.0, n).astype(np.float32)
    v = rng.integers(-1, 2, size=(n, 3)).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        recs["normal"] = v / np.sqrt((v * v).sum(axis=1, keepdims=True))       # (0,0,0) -> NaN, as cubeNormal
    recs["normal"][rng.random(n) < 0.1] = 0.0                                  # misses
    return recs


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_frame_is_written_whole(tmp_path):
    b = _bench()
    recs = _records(64 * 48, 1)
    b.dump_outputs(str(tmp_path), recs, b.DUMP_FIELDS)
    assert sorted(os.listdir(tmp_path)) == sorted(f + ".npy" for f, _ in b.DUMP_FIELDS)
    for f, dt in b.DUMP_FIELDS:
        a = np.load(tmp_path / (f + ".npy"))
        assert a.dtype == np.dtype(dt) and a.shape == recs[f].shape and np.isfinite(a).all()
        if f == "normal":
            nan = np.isnan(recs["normal"]).all(axis=1)
            assert nan.any() and not np.isnan(recs["normal"][~nan]).any()
            assert np.array_equal(a[nan], np.zeros((nan.sum(), 3), np.float32))          # the NaN normal is written as (0, 0, 0)
            assert np.array_equal(a[~nan].view(np.uint32), recs["normal"][~nan].view(np.uint32))
        elif f == "t":
            assert np.array_equal(a.view(np.uint32), recs[f].view(np.uint32))
        else:
            assert np.array_equal(a, recs[f])


def test_non_finite_values_are_refused(tmp_path):
    b = _bench()
    recs = _records(64, 3)
    recs["t"][5] = np.inf
    with pytest.raises(SystemExit, match="non-finite"):
        b.dump_outputs(str(tmp_path), recs, b.DUMP_FIELDS)


def test_1080p_frame_is_sampled_under_the_budget(tmp_path):
    b = _bench()
    recs = _records(1920 * 1080, 2)
    b.dump_outputs(str(tmp_path / "a"), recs, b.DUMP_FIELDS)
    b.dump_outputs(str(tmp_path / "b"), recs, b.DUMP_FIELDS)
    assert _dir_bytes(tmp_path / "a") <= 64_000_000
    assert all(np.isfinite(np.load(tmp_path / "a" / f)).all() for f in os.listdir(tmp_path / "a"))
    pix = np.load(tmp_path / "a" / "pixel.npy")
    assert pix.dtype == np.float64 and np.array_equal(pix, np.load(tmp_path / "b" / "pixel.npy"))     # fixed, seeded sample
    idx = pix.astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[-1] < recs.shape[0] and idx.shape[0] > recs.shape[0] // 2
    assert np.array_equal(np.load(tmp_path / "a" / "node.npy"), recs["node"][idx].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "a" / "flags.npy"), recs["flags"][idx].astype(np.float32))


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "5", "--warmup", "2", "--workload", "c3small_1080p_depth10_4x1x4_shadow",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 5 and out["ms_per_step"] > 0 and out["value"] > 0 and out["unit"] == "Mrays/s" and out["dtype"] == "f32"
    assert not {"roofline", "cpu_baseline", "diagnostics", "single_frame_ms"} & set(out)
    assert _dir_bytes(tmp_path) <= 64_000_000
    flags = np.load(tmp_path / "flags.npy")
    assert flags.dtype == np.float32 and (flags.astype(np.int64) & 1).sum() > 1000      # the frame sees terrain
    n = np.load(tmp_path / "pixel.npy").shape[0]
    assert all(np.load(tmp_path / (f + ".npy")).shape[0] == n for f in ("t", "normal", "material", "chunk", "node", "cell"))
    assert all(np.isfinite(np.load(tmp_path / f)).all() for f in os.listdir(tmp_path))
    hit_normal = np.load(tmp_path / "normal.npy")[(flags.astype(np.int64) & 1) == 1]
    assert (np.abs(hit_normal).sum(axis=1) == 0).any()                  # depth 10: some hits carry the reference's NaN normal
