"""The float64 model of activation_distance='tanimoto' (csrc/bmu_tanimoto.hpp): score64 = 1 - p / (a + b - p) from the float32
inputs, 0 where a + b - p <= 0 (both vectors zero); a row holding a NaN or an infinity gets unit 0.
The bound.  The kernel forms p by one chain of D float32 fused multiply-adds, so |p^ - p| <= g |x||w| with g = gamma_D =
D u / (1 - D u), u = 2^-24; a and b are float32 sums of D rounded squares, |a^ - a| <= g a, |b^ - b| <= g b.  With q = a + b - p:
ds/dp = -(a + b) / q^2 and ds/da = ds/db = p / q^2, so |s^ - s| <= g (a + b)(|x||w| + |p|) / q^2 + 9 u =: e(n, k); the 9 u
cover the two roundings of q, the division and the subtraction from 1 (q >= (a + b) / 2 >= |p|, |s| <= 2).  A returned unit and the
true minimum each carry their own e, so tol(n) = 2 max_k e(n, k) <= 8 g + 18 u."""
import numpy as np

F32, F64, U = np.float32, np.float64, 2.0 ** -24


def scores64(x, w):
    """(score64 (n, K), tol (n,)) of finite float32 rows x against the codebook w"""
    x, w = np.asarray(x, F32).astype(F64), np.asarray(w, F32).astype(F64)
    g = x.shape[1] * U / (1 - x.shape[1] * U)
    p, a, b = x @ w.T, (x * x).sum(1)[:, None], (w * w).sum(1)[None, :]
    q = np.where(a + b - p > 0, a + b - p, np.inf)
    e = g * (a + b) * (np.sqrt(a * b) + np.abs(p)) / q ** 2 + 9 * U
    return np.where(np.isfinite(q), 1.0 - p / q, 0.0), 2.0 * e.max(axis=1)


def check(ids, x, w):
    """Every returned unit scores within tol of the float64 row minimum; where best and second best lie more than 2 tol apart the id
    IS the float64 argmin; a non-finite row has unit 0; the case leaves at most 1 % of the rows undecided.  Returns that share."""
    ids, fin = np.asarray(ids), np.isfinite(x).all(axis=1)
    assert (ids[~fin] == 0).all(), "a row holding a NaN or an infinity must get unit 0"
    s, tol = scores64(x[fin], w)
    got, rows = ids[fin], np.arange(int(fin.sum()))
    two = np.partition(s, 1, axis=1)[:, :2]
    decided = two[:, 1] - two[:, 0] > 2 * tol
    assert decided.mean() >= 0.99, "the case leaves %.2f %% of its rows within 2 tol" % (100 - 100 * decided.mean())
    over = (s[rows, got] - two[:, 0]) / tol
    assert (over <= 1.0).all(), "a returned unit scores %.3g tol above the row minimum" % over.max()
    assert (got == s.argmin(axis=1))[decided].all(), "a decided row has another unit than the float64 argmin"
    return 1.0 - decided.mean()
