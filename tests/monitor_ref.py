"""The training monitor's float64 model (include/somhip.h, "Training monitor"): what one epoch's record must be, from the rows,
the ids the epoch's own search found, the codebook it ran with and its final accumulator.

  row_metrics    sum_n w_n d_n, sum_n w_n, the rows measured and the rows whose id changed, d_n = the float64 Euclidean distance of
                 row n to W[ids_n] (masked: over the observed features; a row with nothing observed has d_n = 0 and counts).  Rows of
                 weight 0 are left out of everything but `changed`.
  merged         the float32 codebook the merge writes: num / den where den != 0 (one IEEE float32 division), else the old value
  shift          sum of (W' - W)^2 over all elements -- every difference of two float32 is formed in float64, its square summed with
                 math.fsum, i.e. the correctly rounded sum of the squares as float64 holds them -- and float32's max |W' - W|

The bounds (the checks assert them; nothing here is fitted to what the kernels return):
  QE             |qe - ref| <= gamma(D + 10) ref, query_ref.check_qe's bound for these per-row float32 distances: D fma steps, six
                 butterfly adds, a square root, and the widening; the double sums over n rows add n 2^-53, far inside it
  rows, changed  exact
  shift_max      exact: a maximum of float32 values rounds nothing
  shift_sumsq    relative K D 2^-52: n = K D terms, each square rounded once (2^-53) and at most n - 1 roundings of the running
                 sum of non-negative terms, whatever the tree ((n - 1) 2^-53 to first order; twice that covers the higher orders)
"""
import math

import numpy as np

from tests import query_ref as Q

F32, F64 = np.float32, np.float64


def row_distances(x, w, ids, masked=False):
    """float64 |x_n - w[ids_n]| per row; masked: over the non-NaN features."""
    x64 = np.asarray(x, F32).astype(F64)
    w64 = np.asarray(w, F32).astype(F64)
    d = x64 - w64[np.asarray(ids, np.int64)]
    sq = d * d
    if masked:
        sq = np.where(np.isnan(x64), 0.0, sq)
    return np.sqrt(sq.sum(axis=1))


def row_metrics(x, w, ids, weights=None, prev=None, masked=False):
    """dict(sum_wd, sum_w, rows, changed) of one epoch; changed is -1 without `prev`."""
    ids = np.asarray(ids, np.int64)
    n = len(ids)
    wt = np.ones(n, F64) if weights is None else np.asarray(weights, F32).astype(F64)
    keep = wt > 0
    d = row_distances(np.asarray(x, F32)[keep], w, ids[keep], masked) if keep.any() else np.zeros(0, F64)
    return {"sum_wd": math.fsum(wt[keep] * d), "sum_w": math.fsum(wt[keep]), "rows": int(keep.sum()),
            "changed": -1 if prev is None else int((np.asarray(prev, np.int64) != ids).sum())}


def qe_of(m):
    return m["sum_wd"] / m["sum_w"] if m["sum_w"] != 0 else float("nan")


def merged(w_old, num, den):
    """The merge: float32 num / den where den != 0, else the old value.  den: (K,) or, masked, (K, D)."""
    w_old, num, den = np.asarray(w_old, F32), np.asarray(num, F32), np.asarray(den, F32)
    if den.ndim == 1:
        den = den[:, None]
    with np.errstate(all="ignore"):
        return np.where(den != 0, num / den, w_old).astype(F32)


def shift(w_old, w_new):
    """(sumsq float64, max float32) of the move from w_old to w_new, both float32."""
    w_old, w_new = np.asarray(w_old, F32), np.asarray(w_new, F32)
    d = w_new.astype(F64) - w_old.astype(F64)
    return math.fsum((d * d).ravel()), F32(np.abs(w_new - w_old).max()) if w_old.size else F32(0)


def check_rows(m, x, w, ids, weights=None, prev=None, masked=False, what=""):
    """The four row fields of a device record against the model; returns QE's err / bound."""
    ref = row_metrics(x, w, ids, weights, prev, masked)
    assert m["rows"] == ref["rows"], "%s: rows %r, model %r" % (what, m["rows"], ref["rows"])
    assert m["changed"] == ref["changed"], "%s: changed %r, model %r" % (what, m["changed"], ref["changed"])
    if ref["rows"] == 0:
        assert m["sum_w"] == 0 and m["sum_wd"] == 0, what
        return 0.0
    assert abs(m["sum_w"] - ref["sum_w"]) <= ref["rows"] * Q.U64 * ref["sum_w"], "%s: weight %r, model %r" % (what, m["sum_w"], ref["sum_w"])
    qe, qref = qe_of(m), qe_of(ref)
    D = np.asarray(w).shape[1]
    bound = Q.gamma(D + 10) * qref
    err = abs(qe - qref)
    ratio = 0.0 if err == 0 else (err / bound if bound > 0 else math.inf)
    assert ratio <= 1.0, "%s: QE %r, float64 model %r (bound %r)" % (what, qe, qref, bound)
    return ratio


def check_shift(m, w_old, w_new, what=""):
    """shift_max exactly, shift_sumsq within K D 2^-52 relative; returns the latter's err / bound."""
    sumsq, mx = shift(w_old, w_new)
    got = F32(m["shift_max"])
    assert got == mx, "%s: shift_max %r, float32 max |W' - W| %r" % (what, got, mx)
    bound = np.asarray(w_old).size * 2.0 ** -52 * sumsq
    err = abs(m["shift_sumsq"] - sumsq)
    ratio = 0.0 if err == 0 else (err / bound if bound > 0 else math.inf)
    assert ratio <= 1.0, "%s: shift_sumsq %r, model %r (bound %r)" % (what, m["shift_sumsq"], sumsq, bound)
    return ratio
