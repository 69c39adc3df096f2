"""bench.py's plain run on the GPU: the lean line (contract fields and the roofline of the timed epochs, none of --full's
blocks) and --dump-outputs, which must hold what the timed path computed -- the codebook and BMU ids of its last epoch, as
the same epochs through HipEngine in this process give them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import som_oracle as O
from tests.conftest import REPO

pytestmark = pytest.mark.gpu


def test_plain_bench_line_and_its_dumped_outputs(tmp_path):
    from xpysom_dask_amd import distributed as D
    from xpysom_dask_amd.decays import exponential_decay
    from xpysom_dask_amd.engine import HipEngine
    import bench
    X = Y = 256; F = 128; N = 65536; W, K = 1, 2
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W),
           "--rows", str(N), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    out = json.loads(lines[0])
    assert out["metric"] == out["unit"] == "samples/sec/epoch" and out["higher_is_better"] is True and out["dtype"] == "f16"
    assert out["steps"] == K and out["warmup"] == W and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(N / (out["ms_per_step"] * 1e-3), rel=1e-9)
    assert 0 < out["roofline"]["frac"] < 1
    for k in ("throughput_mode", "cpu_baseline", "ms_per_step_by_kernel", "whole_schedule", "data_variants", "queries",
              "without_block_skipping", "precision_modes_at_batch65536"):
        assert k not in out, k
    assert "batch65536" not in out["roofline"]

    cb = np.load(tmp_path / "out" / "codebook.npy")
    ids = np.load(tmp_path / "out" / "bmu.npy")
    assert cb.dtype == np.float32 and cb.shape == (X * Y, F)
    assert ids.dtype == np.float64 and ids.shape == (N,)
    e = HipEngine(X, Y, F, precision="exact")
    e.set_weights(O.default_codebook(X, Y, F, 1234).astype(np.float32))
    e.set_data(bench.workload_rows("c3", N, 1234))
    for t in range(W + K):
        D.epoch(e, exponential_decay(X / 2, 1, t, W + K), exponential_decay(0.5, 0.01, t, W + K), True)
    assert np.array_equal(cb, e.get_weights())
    assert np.array_equal(ids, e.epoch_fetch()[2].astype(np.float64))
    e.close()


def test_full_bench_replays_at_most_the_default_schedule_whatever_the_steps():
    """--full's whole-schedule blocks (float32 runs among them, ~50x the headline's epoch) must not grow with --steps: past the
    default flags they run on FULL_WARMUP + FULL_STEPS epochs, and the line says so; the headline still times every step."""
    import bench
    W, K = bench.FULL_WARMUP + 1, 3 * bench.FULL_STEPS
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W),
           "--rows", "65536", "--full", "--no-cpu-baseline"]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["steps"] == K and out["warmup"] == W and out["roofline"]["launches"] >= K
    side = out["other_blocks_schedule"]
    n = bench.FULL_WARMUP + bench.FULL_STEPS
    assert side["epochs"] == n and side["is_the_headline_schedule"] is False
    assert out["whole_schedule"]["epochs"] == n and len(out["per_epoch_ms"]) == n
    assert all(len(v["per_epoch_ms"]) == n for k, v in out["data_variants"].items() if k != "what")
    assert out["codebook_equal_to_f32_run"] is True and out["codebook_equal_to_headline_run"] is True
    assert out["without_block_skipping"]["codebook_equal_to_headline_run"] is True
