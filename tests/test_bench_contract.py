"""Driver bench contract: the exact torchrun launch the driver uses at
round end must produce one JSON line with the agreed schema (weak-scaling
whole-job value, per-rank max step time). Runs on CPU with shrunk sizes."""

import json
import os
import subprocess
import sys

import pytest

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED_FIELDS = [
    "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
]


def run_bench(cmd, env):
    out = subprocess.run(
        cmd, cwd=REPO_ROOT, env=env, capture_output=True, text=True,
        timeout=420,
    )
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert lines, out.stdout[-2000:]
    return json.loads(lines[-1])


def test_bench_single_rank():
    env = {**os.environ, "FAABRIC_BENCH_BASE_OFFSET": "12000",
           "LOG_LEVEL": "error"}
    parsed = run_bench(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "2",
         "--warmup", "1", "--batch", "8"],
        env,
    )
    for f in REQUIRED_FIELDS:
        assert f in parsed, f
    assert parsed["n_gpus"] == 1
    assert parsed["steps"] == 2
    assert parsed["value"] > 0
    assert parsed["scaling"] == "weak"
    assert parsed["config"]["global_batch"] == 8


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last timed step's outputs as float32
    .npy files, identical from run to run; --full is accepted and keeps
    the result line's schema."""
    import numpy as np

    env = {**os.environ, "FAABRIC_BENCH_BASE_OFFSET": "12300",
           "LOG_LEVEL": "error"}
    base = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3",
            "--warmup", "1", "--batch", "8", "--bytes", str(1 << 20)]
    first = run_bench(base + ["--dump-outputs", str(tmp_path / "a")], env)
    second = run_bench(
        base + ["--full", "--dump-outputs", str(tmp_path / "b")], env)
    for parsed in (first, second):
        for f in REQUIRED_FIELDS:
            assert f in parsed, f
        assert parsed["steps"] == 3
        assert parsed["ms_per_step"] > 0
    assert first["config"]["full"] is False
    assert second["config"]["full"] is True

    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["allreduce.npy", "alltoall.npy",
                     "batch_return_values.npy"]
    total = 0
    for name in names:
        a = np.load(tmp_path / "a" / name)
        b = np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32
        assert a.size > 0
        assert np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 * 1024 * 1024
    # 1-rank world: both collectives hand back the fill pattern sent
    fill = np.frombuffer(b"\x3f" * 4, dtype=np.float32)[0]
    ar = np.load(tmp_path / "a" / "allreduce.npy")
    assert ar.size == (1 << 20) // 4
    assert np.all(ar == fill)
    assert np.all(np.load(tmp_path / "a" / "alltoall.npy") == 0x11)
    rvs = np.load(tmp_path / "a" / "batch_return_values.npy")
    assert rvs.size == 8
    assert np.all(rvs == 0)


def test_bench_torchrun_two_ranks():
    """The N>1 launch shape the driver uses (one rank per GPU; gloo/host
    plane on CPU here)."""
    env = {**os.environ, "FAABRIC_BENCH_BASE_OFFSET": "12600",
           "LOG_LEVEL": "error"}
    parsed = run_bench(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29731", "bench.py", "--gpus", "2",
         "--steps", "2", "--warmup", "1", "--batch", "8"],
        env,
    )
    assert parsed["n_gpus"] == 2
    assert parsed["value"] > 0
    # Whole-job aggregate: batch is per host x N
    assert parsed["config"]["global_batch"] == 16
    assert parsed["config"]["pingpong_bytes"] > 0
