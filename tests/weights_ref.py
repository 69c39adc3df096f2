"""A float64 model of the update with per-row sample weights.

Shared by tests/test_weights_cpu.py and tests/test_gpu_weights.py (not a conftest).

    num[k] = sum_n w_n h(bmu_n -> k) x_n        den[k] = sum_n w_n h(bmu_n -> k)

`weighted_segment_sums` forms, per distinct BMU, S = sum w x, A = sum w |x| and c = sum w (a stable sort, then
np.add.reduceat over the runs), and `reference_update_weighted` hands them to tests/update_ref.py's `accumulate`
unchanged, with the neighbourhood rows `reference_update` builds.  A row of weight 0 is absent, as in the library: it is
dropped before anything is multiplied, so a NaN in it reaches neither model nor device sums.

The library forms fmaf(w, x, acc) where the unweighted run sum forms acc + x: one rounding per row either way, so
update_ref.TOL and its magnitude-relative form (update_ref.check_accumulators) apply as they stand.
"""
import numpy as np

from oracle import som_oracle as O
from tests import update_ref as U

F32, F64 = np.float32, np.float64


def weighted_segment_sums(data, bmu, w):
    """(units, S, A, c): the distinct BMUs of the rows of nonzero weight in ascending order, and per unit the float64
    sums of w x, of w |x| and of w."""
    x = np.asarray(data, F64)
    bmu = np.asarray(bmu, np.int64)
    w = np.asarray(w, F64)
    keep = w != 0
    x, bmu, w = x[keep], bmu[keep], w[keep]
    if len(bmu) == 0:
        return np.zeros(0, np.int64), np.zeros((0, x.shape[1])), np.zeros((0, x.shape[1])), np.zeros(0)
    order = np.argsort(bmu, kind="stable")
    sb = bmu[order]
    starts = np.flatnonzero(np.r_[True, sb[1:] != sb[:-1]])
    xs, ws = x[order], w[order]
    S = np.add.reduceat(xs * ws[:, None], starts, axis=0)
    A = np.add.reduceat(np.abs(xs) * ws[:, None], starts, axis=0)
    c = np.add.reduceat(ws, starts)
    return sb[starts], S, A, c


def reference_update_weighted(data, bmu, w, X, Y, eta, sigma, *, wide, neighbourhood="gaussian", topology="rectangular",
                              compact=False, std_coeff=0.5):
    """(num (K, D), den (K,), mag_num (K, D), mag_den (K,)), float64: update_ref.reference_update with weighted
    segment sums (the neighbourhoods that need their own magnitude rows -- the mexican hat -- are not asked for here)."""
    assert neighbourhood != "mexican_hat"
    units, S, A, c = weighted_segment_sums(data, bmu, w)
    fn = O.NEIGHBOURHOODS[U.oracle_key(neighbourhood, topology)]
    eta_t = F64(eta) if wide else float(eta)

    def h_of(u):
        return fn(X, Y, std_coeff, compact, u // Y, u % Y, sigma, wide) * eta_t

    return U.accumulate(S, A, c, units, X * Y, h_of)


def brute_force_update(data, bmu, w, X, Y, eta, sigma, *, wide, neighbourhood="gaussian", topology="rectangular",
                       compact=False, std_coeff=0.5):
    """(num, den) as the definition reads: one neighbourhood row per data row, a Python loop, float64."""
    fn = O.NEIGHBOURHOODS[U.oracle_key(neighbourhood, topology)]
    eta_t = F64(eta) if wide else float(eta)
    x = np.asarray(data, F64)
    K = X * Y
    num, den = np.zeros((K, x.shape[1])), np.zeros(K)
    for n in range(len(x)):
        if w[n] == 0:
            continue
        b = np.array([bmu[n]], np.int64)
        h = np.asarray(fn(X, Y, std_coeff, compact, b // Y, b % Y, sigma, wide) * eta_t, F64).reshape(K)
        num += float(w[n]) * h[:, None] * x[n][None, :]
        den += float(w[n]) * h
    return num, den


def make_weights(N, seed, zero_share=0.1):
    """float32 weights in [0, 2), about `zero_share` of them (at least one) exactly 0."""
    rs = np.random.RandomState(seed)
    w = (rs.rand(N) * 2).astype(F32)
    z = rs.rand(N) < zero_share
    z[rs.randint(0, N)] = True
    w[z] = 0
    return w
