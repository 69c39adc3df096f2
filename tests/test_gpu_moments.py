"""The row moments on the device -- som_row_moments / som_row_moments_device / som_gather_rows_device (include/somhip.h,
csrc/moments.hpp) -- against the float64 model and the derived bound of tests/moments_ref.py.  GPU only (`-m gpu`).

Every case runs through the host and the device entry point, unweighted and weighted, and checks
  (a) moments_ref.check_moments passes
  (b) the device entry point returns the host entry point's bits
  (c) a second call returns the same bits
  (d) gram is symmetric in bits.
The shapes are the smallest that cross each boundary of the kernels: one, two, three rows (half an MFMA step, one, one and a half);
feature counts around the 32-feature operand block, the 64-lane column group of the sums kernel and the four-tile workgroup; the
cap; one chunk of the float32 chain less one, exact, plus one; one row more than a whole round of the row split; and 70 000 rows."""
import numpy as np
import pytest

from tests import moments_ref as M

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
R = M.chunk_rows()


def engine(D, X=4, Y=4, **kw):
    from xpysom_dask_amd.engine import HipEngine
    kw.setdefault("precision", "f32")
    return HipEngine(X, Y, D, **kw)


def _dev(a, dtype=F32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, F64), np.ascontiguousarray(b, F64)
    assert a.shape == b.shape, what
    bad = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
    assert len(bad) == 0, "%s: %d entries differ, first at %r: %r against %r" % (what, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


def _same_moments(a, b, what):
    _same_bits(np.array([a[0]]), np.array([b[0]]), what + " wsum")
    _same_bits(a[1], b[1], what + " s1")
    if a[2] is not None or b[2] is not None:
        _same_bits(a[2], b[2], what + " gram")


def rows(n, D, seed, mean=2.0):
    rs = np.random.RandomState(seed)
    return (mean + rs.normal(0, 1, (n, D)) * rs.uniform(0.5, 2.0, D)).astype(F32)


def both_entries(e, x, w=None, p=None, gram=True, what=""):
    """The moments of (x, w, p) through the host and the device entry point, checks (a) - (d) applied; returns the host's."""
    xd = _dev(x)
    wd = _dev(w) if w is not None else None
    host = e.row_moments(x, w, p, gram)
    dev = e.row_moments_device(xd.data_ptr(), len(x), wd.data_ptr() if wd is not None else None, p, gram)
    M.check_moments(host, x, w, p, what + " host")                                   # (a)
    _same_moments(dev, host, what + " device against host")                          # (b)
    _same_moments(e.row_moments(x, w, p, gram), host, what + " host, second call")   # (c)
    _same_moments(e.row_moments_device(xd.data_ptr(), len(x), wd.data_ptr() if wd is not None else None, p, gram), host,
                  what + " device, second call")
    if gram:
        _same_bits(host[2], host[2].T, what + " symmetry")                           # (d)
    return host


ROUND_D3 = M.plan(1, 3)["round"]
SHAPES = ([(n, 3) for n in (1, 2, 3)]
          + [(300, D) for D in (1, 3, 31, 32, 33, 64, 65, 128, 130, 800)]
          + [(70, 2048)]
          + [(n, 33) for n in (R - 1, R, R + 1)]
          + [(ROUND_D3 * R + 1, 3)]                           # one row more than a whole round of the row split
          + [(70000, 3)])


@pytest.mark.parametrize("n, D", SHAPES, ids=["n%d-D%d" % s for s in SHAPES])
def test_moments_against_the_model(n, D):
    x = rows(n, D, 100 + n + D)
    rs = np.random.RandomState(n + 7 * D)
    w = rs.uniform(0, 3, n).astype(F32)
    w[rs.rand(n) < 0.2] = 0
    p = (x.astype(F64).mean(axis=0) + rs.normal(0, 0.1, D)).astype(F32)
    e = engine(D)
    try:
        if n == ROUND_D3 * R + 1:
            pl = M.plan(n, D)
            assert pl["splits"] == pl["round"] == ROUND_D3 and (n + R - 1) // R == pl["round"] + 1
        both_entries(e, x, None, None, what="unweighted, pivot 0")
        both_entries(e, x, w, p, what="weighted, pivot near the mean")
    finally:
        e.close()


def test_large_mean_small_spread():
    """Rows with mean 1000 and spread 1, about 0 and about the mean: each inside its own bound, and the covariance the shifted-data
    formula takes from the pivot at the mean is the float64 covariance to the bound's few parts in 10^5."""
    n, D = 3000, 5
    x = rows(n, D, 3, mean=1000.0)
    e = engine(D)
    try:
        _, s1, _ = both_entries(e, x, None, None, gram=False, what="sums")
        mean = (s1 / n).astype(F32)
        both_entries(e, x, None, None, what="pivot 0")
        got = both_entries(e, x, None, mean, what="pivot at the mean")
    finally:
        e.close()
    exact = M.central(*M.model(x, None, mean)[0])
    err = np.abs(M.central(*got) - exact)
    assert (err <= M.central_bound(x, None, mean)).all()
    assert err.max() < 1e-4 * np.abs(exact).max()


def test_unit_weights_are_no_weights():
    x = rows(2 * R + 50, 33, 4)
    p = x.mean(axis=0).astype(F32)
    e = engine(33)
    try:
        _same_moments(both_entries(e, x, np.ones(len(x), F32), p), both_entries(e, x, None, p), "weights of 1.0")
    finally:
        e.close()


def test_integer_weights_are_repeated_rows():
    x = rows(700, 9, 5)
    w = np.random.RandomState(6).randint(0, 4, 700)
    rep = np.repeat(x, w, axis=0)
    e = engine(9)
    try:
        a = both_entries(e, x, w.astype(F32), None, what="weighted")
        b = both_entries(e, rep, None, None, what="repeated")
    finally:
        e.close()
    # both are within their bounds of ONE model (the model of the repeated rows is the weighted model): so of each other
    ba, bb = M.bounds(x, w.astype(F32), None), M.bounds(rep, None, None)
    assert abs(a[0] - b[0]) <= ba[0] + bb[0] and a[0] == w.sum()
    assert (np.abs(a[1] - b[1]) <= ba[1] + bb[1]).all() and (np.abs(a[2] - b[2]) <= ba[2] + bb[2]).all()


def test_weight_zero_rows_are_selected_out():
    """A row of weight 0 full of NaN and Inf reaches no sum: every output is finite; the bits are those of the same call with
    ordinary numbers in that row, and -- the row being the last -- of the call without the row."""
    n, D = R + 40, 33
    x = rows(n, D, 8)
    w = np.random.RandomState(9).uniform(0.5, 2, n).astype(F32)
    w[[17, n - 1]] = 0
    bad = x.copy()
    bad[17, ::2], bad[17, 1::2] = np.nan, np.inf
    bad[n - 1, ::3], bad[n - 1, 1::3], bad[n - 1, 2::3] = -np.inf, np.nan, np.inf
    p = x.mean(axis=0).astype(F32)
    e = engine(D)
    try:
        got = both_entries(e, bad, w, p, what="NaN rows of weight 0")
        assert np.isfinite(got[0]) and np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
        _same_moments(got, e.row_moments(x, w, p), "against ordinary numbers in the rows of weight 0")
        # without the last row: the same chunks, the same grids (moments_plan), so the same bits
        assert M.plan(n, D) == M.plan(n - 1, D)
        bad[17] = 1.0
        _same_moments(got, e.row_moments(bad[:-1], w[:-1], p), "against the call without the last row")
    finally:
        e.close()


def test_sums_only_call_returns_the_full_call_s1():
    x = rows(2 * R + 3, 65, 10)
    w = np.random.RandomState(1).uniform(0, 2, len(x)).astype(F32)
    p = x.mean(axis=0).astype(F32)
    e = engine(65)
    try:
        full = both_entries(e, x, w, p)
        sums = both_entries(e, x, w, p, gram=False)
    finally:
        e.close()
    assert sums[2] is None
    _same_moments((full[0], full[1], None), sums, "gram == NULL")


def test_refusals():
    from xpysom_dask_amd.engine import SomHipError
    e = engine(2049)
    try:
        with pytest.raises(SomHipError, match="input_len 2049 exceeds SOM_MOMENTS_MAX_FEATURES"):
            e.row_moments(np.zeros((4, 2049), F32))
        xd = _dev(np.zeros((4, 2049), F32))
        with pytest.raises(SomHipError, match="input_len 2049 exceeds SOM_MOMENTS_MAX_FEATURES"):
            e.row_moments_device(xd.data_ptr(), 4)
    finally:
        e.close()
    e = engine(3)
    try:
        x = rows(10, 3, 1)
        for w in (np.r_[np.ones(9), -1.0], np.r_[np.ones(9), np.nan], np.r_[np.ones(9), np.inf]):
            with pytest.raises(SomHipError, match="weights must be finite and >= 0"):
                e.row_moments(x, w.astype(F32))
        xd = _dev(x)
        got = e.gather_rows_device(xd.data_ptr(), 10, [9, 0, 0, 3])
        assert np.array_equal(got, x[[9, 0, 0, 3]])
        for idx in ([0, 10], [-1]):
            with pytest.raises(SomHipError, match="outside the block of 10 rows"):
                e.gather_rows_device(xd.data_ptr(), 10, idx)
        assert e.row_moments(np.zeros((0, 3), F32))[0] == 0.0
    finally:
        e.close()


def test_a_moments_call_leaves_the_training_state_alone():
    """Two epochs on a resident 'exact' 64 x 64 x 32 map with a moments call on OTHER rows between them: the codebook bits, the
    BMUs and the resident row count of two epochs without it."""
    from oracle import som_oracle as O
    x = O.gaussian_blobs(5000, 32, seed=4)
    other = rows(3000, 32, 12)
    w0 = O.default_codebook(64, 64, 32, 3).astype(F32)
    out = []
    for between in (False, True):
        e = engine(32, 64, 64, precision="exact")
        try:
            e.set_weights(w0)
            e.set_data(x)
            for t in range(2):
                e.epoch_accumulate(O.exponential_decay(32.0, 1.0, t, 2), O.exponential_decay(0.5, 0.01, t, 2), True)
                e.epoch_merge()
                if between and t == 0:
                    M.check_moments(e.row_moments(other, None, other.mean(axis=0).astype(F32)), other, None, other.mean(axis=0).astype(F32))
                    od = _dev(other)
                    e.row_moments_device(od.data_ptr(), len(other))
            out.append((e.get_weights(), e.epoch_fetch()[2], e.n_rows))
        finally:
            e.close()
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2] == 5000
