"""'tanimoto' (csrc/bmu_tanimoto.hpp): the float64 model's bound, integer rows bit for bit under every part count, one epoch."""
import numpy as np
import pytest

from tests import tanimoto_ref as R
from tests import update_ref as U
from xpysom_dask_amd.engine import HipEngine
from xpysom_dask_amd.xpysom import XPySom

pytestmark = pytest.mark.gpu

# one partial tile everywhere | one feature past a chunk, scalar loads | unit tiles, a partial row tile | the cap, several parts
CASES = [(6, 5, 3, 50), (16, 16, 129, 300), (24, 24, 1024, 700), (64, 64, 4096, 300)]


def case(c):
    """Count-like rows near units of a count-like codebook: the float64 model decides them.  Units 2j and 2j + 1 differ in ONE feature
    (the last, the first of the last chunk, one with f % 8 >= 4) and row j equals unit 2j: a search that loses it answers 2j + 1."""
    (X, Y, D, N), rs = c, np.random.RandomState(c[2])
    w = (rs.randint(1, 4, (X * Y, D)) * (rs.rand(X * Y, D) < (1.0 if D < 64 else 0.15)) * rs.uniform(0.5, 1.0, (X * Y, D))).astype(R.F32)
    x = (w[rs.randint(0, X * Y, N)] * (rs.rand(N, D) > 0.05) * rs.uniform(0.9, 1.1, (N, D))).astype(R.F32)
    for j, f in enumerate(sorted({D - 1, (D - 1) // 32 * 32, min(5, D - 1)})):
        w[2 * j, f] = 0
        w[2 * j + 1] = w[2 * j]
        w[2 * j, f] = 0.25 * np.sqrt((w[2 * j] ** 2).sum())
        x[j] = w[2 * j]
    return x, w


def ids_of(X, Y, x, w):
    e = HipEngine(X, Y, x.shape[1], distance="tanimoto", precision="f32")
    try:
        e.set_weights(w)
        return e.bmu(x)
    finally:
        e.close()


@pytest.mark.parametrize("c", CASES, ids=lambda c: "%dx%dx%d_n%d" % c)
def test_search_against_float64(c):
    x, w = case(c)
    print("%s: %.2f %% of the rows undecided" % (c, 100 * R.check(ids_of(c[0], c[1], x, w), x, w)))


@pytest.mark.parametrize("parts", [None, 1, 1 << 20], ids=["parts_auto", "parts_1", "parts_max"])
@pytest.mark.parametrize("c", [(24, 24, 200, 300), (16, 16, 129, 300), (64, 64, 4096, 300)], ids=lambda c: "%dx%dx%d_n%d" % c)
def test_integer_rows_exactly_under_every_part_count(c, parts, monkeypatch):
    """Random 0/1 rows (input_len 200; counts 0..3 elsewhere) against a codebook of the same kind: every row competes between many
    units, and p, a, b are exact in float32, so the scores are NumPy's float32 quotient and difference bit for bit -- at 0/1 the
    Jaccard distance in the integer quotients' order.  Unit 2 again at ids 5 and K - 1 (a tie in a block and across parts), a zero
    unit 7; row 0 = unit 2, row 1 zero, rows 2, 3, N - 1 hold NaN, +inf, -inf.  The ids equal that argmin under every part count."""
    (X, Y, D, N), rs = c, np.random.RandomState(7)
    w, x = ((rs.randint(1, 2 if D == 200 else 4, (n, D)) * (rs.rand(n, D) < 0.3)).astype(R.F32) for n in (X * Y, N))
    w[5] = w[-1] = x[0] = w[2]
    w[7] = x[1] = 0
    x[2, D // 2], x[3, 0], x[N - 1, D - 1] = np.nan, np.inf, -np.inf
    if parts is not None:
        monkeypatch.setenv("SOM_TANIMOTO_PARTS", str(parts))
    got = ids_of(X, Y, x, w)
    xi, wi = np.where(np.isfinite(x), x, 0).astype(R.F64), w.astype(R.F64)      # (integers: every float64 sum below is exact)
    p = xi @ wi.T
    q = (xi * xi).sum(1)[:, None] + (wi * wi).sum(1)[None, :] - p
    s = np.where(q > 0, R.F32(1) - p.astype(R.F32) / np.maximum(q, 1).astype(R.F32), R.F32(0))
    assert s.dtype == R.F32 and (D != 200 or np.array_equal(s.argmin(1), np.where(q > 0, 1 - p / np.maximum(q, 1), 0.0).argmin(1)))
    ref = np.where(np.isfinite(x).all(axis=1), s.argmin(axis=1), 0)
    assert np.array_equal(got, ref) and tuple(ref[:4]) == (2, 7, 0, 0) and ref[-1] == 0 and len(np.unique(ref)) > N // 4, np.flatnonzero(got != ref)[:10]


def test_one_epoch_and_device_rows():
    """Accumulators and merged codebook against the update reference fed the kernel's own ids; train on device rows = host rows."""
    import torch
    X, Y, D, N = 12, 10, 64, 500
    rs = np.random.RandomState(11)
    x = (rs.randint(1, 4, (N, D)) * (rs.rand(N, D) < 0.4)).astype(R.F32)
    soms = [XPySom(X, Y, D, sigma=3.0, activation_distance='tanimoto', random_seed=3) for _ in range(2)]
    start = soms[0].get_weights().copy()
    w0 = np.abs(start.reshape(-1, D)).astype(R.F32)
    e = HipEngine(X, Y, D, distance="tanimoto")
    try:
        e.set_weights(w0)
        e.set_data(x)
        e.epoch_accumulate(3.0, 0.5, True)
        num, den, bmu = e.epoch_fetch()
        e.epoch_merge()
        ref = U.reference_update(x, bmu, X, Y, 0.5, 3.0, wide=True)
        U.check_accumulators(num, den, ref, "tanimoto")
        U.check_merge(w0, e.get_weights(), num, den, ref, False, "tanimoto")
    finally:
        e.close()
    soms[0].train(x, 2)
    soms[1].train(torch.from_numpy(x).cuda(), 2)
    assert np.array_equal(soms[0].get_weights(), soms[1].get_weights()) and not np.array_equal(soms[0].get_weights(), start)
