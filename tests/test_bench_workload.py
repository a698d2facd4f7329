"""bench.py's own pieces: the workload it times (made on a pool of host threads, it must be exactly synth.drive_pairs, so
that the benchmark's inputs are the same from run to run), what --dump-outputs writes, and a plain run end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_build_workload_equals_drive_pairs():
    import bench
    from staticmapping_amd import synth
    ref = synth.drive_pairs(5, n_points=3000, seed=5)
    for threads in (1, 4):
        got = bench.build_workload(5, 3000, None, threads=threads)
        assert len(got) == len(ref)
        for a, b in zip(got, ref):
            assert a.keys() == b.keys()
            for k in a:
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


@pytest.mark.gpu
def test_build_workload_equals_drive_pairs_on_the_device():
    """The same with the ray casts on the GPU (how bench.py makes its scans): many host threads share the device."""
    import torch
    import bench
    from staticmapping_amd import synth
    dev = torch.device("cuda", 0)
    ref = synth.drive_pairs(12, n_points=120_000, device=dev, seed=5)
    got = bench.build_workload(12, 120_000, dev, threads=12)
    assert len(got) == len(ref) == 12
    for a, b in zip(got, ref):
        for k in a:
            assert np.array_equal(a[k], b[k]), k


def test_dump_outputs_writes_float_arrays_within_the_cap(tmp_path):
    import bench
    rng = np.random.default_rng(1)
    n = 40
    T = rng.normal(size=(n, 4, 4))
    sc = rng.uniform(size=n)
    it = np.full(n, 20, dtype=np.int64)
    bench.dump_outputs(str(tmp_path / "all"), T, sc, it)
    got = {f[:-4]: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    assert set(got) == {"poses", "fitness_scores", "iterations", "pair_index"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["poses"], T) and np.array_equal(got["fitness_scores"], sc) and np.array_equal(got["iterations"], it)
    assert np.array_equal(got["pair_index"], np.arange(n))
    # beyond the cap: a fixed sample, the same every time
    cap = 10 * 8 * 19
    bench.dump_outputs(str(tmp_path / "a"), T, sc, it, max_bytes=cap)
    bench.dump_outputs(str(tmp_path / "b"), T, sc, it, max_bytes=cap)
    idx = np.load(tmp_path / "a" / "pair_index.npy").astype(np.int64)
    assert len(idx) == 10 and np.array_equal(idx, np.load(tmp_path / "b" / "pair_index.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "poses.npy"), T[idx])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) < cap + 4 * 256


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_and_dumps_its_outputs(tmp_path):
    """A plain run (no --full): one JSON line with the headline fields and nothing of the --full legs; --steps is what it
    timed; --dump-outputs holds every pair's pose of the last timed step, each within the truth's reach."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--pairs", "16", "--distinct", "8", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-500:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "alignments/s" and d["higher_is_better"]
    assert abs(d["ms_per_step"] - 1e3 * 16 / d["value"]) < 0.01 * d["ms_per_step"] + 0.002
    assert not {"roofline", "figures", "cpu_baseline", "other_workloads", "end_to_end", "single_pair"} & set(d)
    T = np.load(out / "poses.npy")
    it = np.load(out / "iterations.npy")
    assert T.shape == (16, 4, 4) and T.dtype == np.float64 and np.all(it == 20)
    assert np.load(out / "fitness_scores.npy").shape == (16,)
    import torch
    import bench
    import staticmapping_amd as sm
    work = bench.build_workload(8, bench.N_POINTS, torch.device("cuda", 0))
    for g in range(16):                                       # slot g holds distinct pair g mod 8
        assert sm.se3_error(T[g], work[g % 8]["T"])[1] < 0.05, g


@pytest.mark.gpu
def test_plain_bench_runs_its_multi_rank_sequence_to_the_end(tmp_path):
    """The plain line under torch.distributed.run with two ranks, in the shared-GPU dry-run mode of
    tests/test_shard_driver_gpu.py: both ranks time, reduce and leave together; rank 0 alone prints and dumps."""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, SMHIP_BENCH_SHARED_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--pairs", "8", "--distinct", "8", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-500:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["value"] > 0 and d["config"]["rccl_ranks"] == 2
    assert np.load(out / "poses.npy").shape == (16, 4, 4) and np.all(np.load(out / "iterations.npy") == 20)
