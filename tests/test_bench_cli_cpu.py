"""CPU: bench.py's own argument path.  `python bench.py --gpus 2` with no launcher in the environment must start two ranks
itself (before any GPU call), run the index broadcast between them and print ONE JSON line with n_gpus == 2 -- rehearsed here
with gloo and the test double tests/bench_double.py in place of the HIP library (LNR_BENCH_DOUBLE=1)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*argv):
    env = dict(os.environ, LNR_BENCH_DOUBLE="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [1, 2])
def test_bench_gpus_flag_starts_that_many_ranks(n):
    out = run_bench("--gpus", str(n), "--steps", "3", "--warmup", "1", "--workload", "small", "--reads", "64", "--full")
    assert out["n_gpus"] == n and out["steps"] == 3 and out["warmup"] == 1
    assert out["config"]["ranks_reported_by_backend"] == n
    assert out["scaling"] == "weak" and out["value"] > 0
    assert out["config"]["distinct_batches"] == 4
    if n > 1:
        assert out["config"]["index_broadcast_s"] is not None and out["config"]["index_bytes"] > 8000
    for k in ("metric", "unit", "ms_per_step", "higher_is_better", "vs_baseline", "dtype", "data", "roofline"):
        assert k in out


def test_bench_plain_run_times_only_the_headline_and_dumps_outputs(tmp_path):
    """Without --full the line carries the headline and none of the extra measurements; --dump-outputs writes the last timed step's cords
    (per-read counts of the whole batch, cord words of a seeded read sample) as float64 .npy files."""
    d = tmp_path / "out"
    out = run_bench("--steps", "3", "--warmup", "1", "--workload", "small", "--reads", "64", "--dump-outputs", str(d))
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["unit"] == "reads/s" and out["higher_is_better"] is True and out["dtype"] == "u64"
    assert "roofline" not in out and "cpu_baseline" not in out and "device_resident_reads_per_s" not in out["config"]
    assert sorted(os.listdir(d)) == ["cords_end.npy", "cords_per_read.npy", "cords_str.npy", "sample_reads.npy"]
    arrays = {f: np.load(d / f) for f in os.listdir(d)}
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert arrays["cords_per_read.npy"].shape == (64,) and arrays["sample_reads.npy"].shape == (64,)
    assert arrays["cords_str.npy"].shape == arrays["cords_end.npy"].shape == (int(arrays["cords_per_read.npy"].sum()), 7)
