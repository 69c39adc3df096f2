"""XPySom.linear_weights_init under a process group: two ranks of the real engine, rows cut contiguously and strided, host rows and
device rows, with and without sample weights.  Every rank returns the same bits, and the result is the single-process result within
the derived tolerance (tests/moments_ref.py, linear_tolerance).  The ranks are started as tests/test_gpu_distributed.py starts its
own: gloo with both ranks on GPU 0; nccl needs two GPUs and is skipped otherwise."""
import os

import numpy as np
import pytest

from tests import moments_ref as M
from tests.conftest import REPO
from tests.init_dist_worker import case
from tests.test_gpu_distributed import _run_ranks
from xpysom_dask_amd.xpysom import _linear_codebook

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _launch(backend, out_dir, shard, world=2):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    r = _run_ranks([os.path.join(REPO, "tests", "init_dist_worker.py"), backend, str(out_dir), shard], env, world, 600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]


def _check(out_dir, shard, world=2):
    from xpysom_dask_amd import XPySom
    x, w = case()
    for name, weights in (("host", None), ("dev", None), ("hostw", w), ("devw", w)):
        got = [np.load(os.path.join(out_dir, "%s_%s_%d.npy" % (name, shard, r))) for r in range(world)]
        for g in got[1:]:
            assert np.array_equal(got[0].view(np.uint32), g.view(np.uint32)), name        # every rank: the same bits
        # the pivot is float32(mean) to an ulp whichever way the rows were cut; the bound moves by parts in 10^6 with it
        tol = M.linear_tolerance(x, weights, M.moments64(x, weights)[1].astype(F32)) * (1 + 1e-5)
        want = _linear_codebook(*M.moments64(x, weights), 9, 6)
        assert np.linalg.norm(got[0].astype(F64) - want, axis=-1).max() <= tol, name
        single = XPySom(9, 6, x.shape[1], random_seed=1)
        single.linear_weights_init(x, sample_weight=weights)
        # (2 tol: the triangle inequality -- the two-rank result, just above, and the single-process one are EACH within tol of the
        #  float64 model; neither is the other's reference)
        assert np.linalg.norm(got[0].astype(F64) - single._weights, axis=-1).max() <= 2 * tol, name
    few = [np.load(os.path.join(out_dir, "few_%s_%d.npy" % (shard, r))) for r in range(world)]
    for f in few:                                           # one row, two ranks, an empty shard: the map is that row
        assert np.array_equal(f, np.broadcast_to(x[0], f.shape))


@pytest.mark.parametrize("shard", ["contiguous", "strided"])
def test_two_ranks_under_gloo(tmp_path, shard):
    _launch("gloo", tmp_path, shard)
    _check(tmp_path, shard)


def test_two_ranks_under_rccl(tmp_path):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (the driver's multi-GPU node)")
    for shard in ("contiguous", "strided"):
        _launch("nccl", tmp_path, shard)
        _check(tmp_path, shard)
