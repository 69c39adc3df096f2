"""The row moments' bound (tests/moments_ref.py) without a GPU: a NumPy float32 emulation of the Gram kernel's order stays inside it,
a one-pass float32 textbook formula does not, and the shifted-data formula gives one covariance whatever the pivot."""
import numpy as np
import pytest

from tests import moments_ref as M

F32, F64 = np.float32, np.float64


def _rows(n, D, mean, seed):
    rs = np.random.RandomState(seed)
    return (mean + rs.normal(0, 1, (n, D)) * rs.uniform(0.5, 2.0, D)).astype(F32)


def test_the_library_exports_the_chunk_length():
    p = M.plan(1000, 128)
    assert p["R"] == M.chunk_rows() and p["R"] >= 2 and p["R"] % 2 == 0
    assert p["tiles"] == 10 and p["max_features"] == 2048
    assert 1 <= p["splits"] <= p["round"] <= 1024


@pytest.mark.parametrize("n, D, weighted", [(1, 3, False), (7, 2, True), (M.chunk_rows() + 1, 5, False), (2 * M.chunk_rows() + 37, 4, True)])
def test_emulation_of_the_kernel_order_is_inside_the_bound(n, D, weighted):
    x = _rows(n, D, 3.0, 11 + n)
    w = np.random.RandomState(n).uniform(0, 3, n).astype(F32) if weighted else None
    if weighted:
        w[::5] = 0
    for p in (None, x.mean(axis=0).astype(F32)):
        worst = M.check_moments(M.emulate(x, w, p), x, w, p, "emulation")
        assert worst <= 1.0


def test_the_bound_is_not_vacuous():
    """Rows with mean 1000 and spread 1: sum x x^T - (sum x)(sum x)^T / n in one float32 pass loses the covariance to cancellation;
    offered as the moments about the mean it is caught."""
    n, D = 2000, 3
    x = _rows(n, D, 1000.0, 5)
    s = np.zeros(D, F32)
    g = np.zeros((D, D), F32)
    for r in range(n):
        s = (s + x[r]).astype(F32)
        g = (g + np.outer(x[r], x[r]).astype(F32)).astype(F32)
    onepass = (g - np.outer(s, s).astype(F32) / F32(n)).astype(F64)
    p = x.astype(F64).mean(axis=0).astype(F32)
    (wsum, s1, gram), _ = M.model(x, None, p)
    M.check_moments((wsum, s1, gram), x, None, p)          # the model itself passes
    with pytest.raises(AssertionError, match="gram"):
        M.check_moments((wsum, s1, onepass), x, None, p)


def test_shifted_data_formula_is_pivot_free():
    """cov from the moments about 0 and about float32(mean): the same matrix within the two bounds."""
    n, D = 2 * M.chunk_rows() + 100, 4
    x = _rows(n, D, 5.0, 9)
    w = np.random.RandomState(2).randint(0, 4, n).astype(F32)
    exact = M.central(*M.model(x, w, None)[0])
    mean = (M.model(x, w, None)[0][1] / w.sum()).astype(F32)
    got = {}
    for name, p in (("zero", None), ("mean", mean)):
        got[name] = M.central(*M.emulate(x, w, p))
        err = np.abs(got[name] - exact)
        assert (err <= M.central_bound(x, w, p)).all(), (name, err.max())
    assert (np.abs(got["zero"] - got["mean"]) <= M.central_bound(x, w, None) + M.central_bound(x, w, mean)).all()
    # ... and the pivot at the mean is the tighter of the two, by the ratio of the second moments
    assert M.central_bound(x, w, mean).max() < 0.2 * M.central_bound(x, w, None).max()
