"""A float64 model of the label and value maps -- som_unit_label_counts / som_unit_value_sums, XPySom.label_counts / unit_means /
classify -- and the bound on the device's sums.

Shared by tests/test_project_cpu.py and tests/test_gpu_project.py (not a conftest).

The contract (include/somhip.h): a_n is the unit som_bmu(ACTIVATION) names for row n, and per unit k over the rows with a_n = k
  counts[k][c]            the rows whose label is c, 0 <= c < C; a label outside [0, C) is counted nowhere
  count / sum / sumsq     per column c of the values: the rows whose value is not NaN, the sum of those values and of their squares
                          in double; +-Inf is a value.

The bound on a sum.  A float32 and its square are exact in double, so the device adds m exact terms in double in SOME order; for
any order the result differs from the exact sum by at most gamma(m - 1) * sum |v|, gamma(m) = m u / (1 - m u), u = 2^-53 (Higham,
Accuracy and Stability of Numerical Algorithms, eq. 4.4).  The model is math.fsum, the correctly rounded exact sum: at most
u * sum |v| from it.  Together: |device - model| <= gamma(m) * sum |v|, m the column's count in the unit -- and for sumsq the
same with sum v^2 (every term is >= 0).  Where the column of a unit holds an infinity the sums are not finite and must equal
IEEE's answer: +Inf, -Inf, or NaN for both signs at once (sumsq: +Inf).
"""
import math
from fractions import Fraction

import numpy as np

F32, F64 = np.float32, np.float64
U64 = 2.0 ** -53


def gamma(m):
    m = np.asarray(m, F64)
    return m * U64 / (1 - m * U64)


# ------------------------------------------------------------------------------------------------------ the model
def label_counts_model(ids, labels, K, C):
    """int64 (K, C): one bincount over unit * C + label of the rows whose label lies in [0, C)."""
    ids, labels = np.asarray(ids, np.int64), np.asarray(labels, np.int64)
    ok = (labels >= 0) & (labels < C)
    return np.bincount(ids[ok] * C + labels[ok], minlength=K * C).astype(np.int64).reshape(K, C)


def brute_force_label_counts(ids, labels, K, C):
    """The same array straight from the definition, a Python loop over the rows."""
    out = [[0] * C for _ in range(K)]
    for b, c in zip(np.asarray(ids).tolist(), np.asarray(labels).tolist()):
        if 0 <= c < C:
            out[b][c] += 1
    return np.array(out, np.int64).reshape(K, C)


def _values(values):
    v = np.asarray(values, F32)
    return v[:, None] if v.ndim == 1 else v


def _ieee_sum(seg):
    """Correctly rounded sum of finite float64 terms; with an infinity among them IEEE's answer."""
    return math.fsum(seg) if np.isfinite(seg).all() else float(np.sum(seg))


def value_sums_model(ids, values, K):
    """(count int64, sum float64, sumsq float64), (K, C) each, from ids and float32 values (n, C): per unit and column the
    values that are not NaN -- their number, math.fsum of them widened and of their exact squares; an empty cell has zeros."""
    ids = np.asarray(ids, np.int64)
    v = _values(values).astype(F64)
    C = v.shape[1]
    seen = ~np.isnan(v)
    count = np.zeros((K, C), np.int64)
    np.add.at(count, ids, seen.astype(np.int64))
    tot, sq = np.zeros((K, C), F64), np.zeros((K, C), F64)
    order = np.argsort(ids, kind="stable")
    cuts = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=K))])
    for k in np.flatnonzero(np.diff(cuts)):
        rows = order[cuts[k]:cuts[k + 1]]
        for c in range(C):
            seg = v[rows, c][seen[rows, c]]
            if len(seg):
                with np.errstate(invalid="ignore"):
                    tot[k, c] = _ieee_sum(seg)
                    sq[k, c] = _ieee_sum(seg * seg)
    return count, tot, sq


def brute_force_value_sums(ids, values, K):
    """The same three arrays straight from the definition, a Python loop over the rows (exact rational sums; an infinity is
    remembered by its sign)."""
    v = _values(values)
    C = v.shape[1]
    count = [[0] * C for _ in range(K)]
    tot = [[Fraction(0)] * C for _ in range(K)]
    sq = [[Fraction(0)] * C for _ in range(K)]
    inf = [[set() for _ in range(C)] for _ in range(K)]
    for b, row in zip(np.asarray(ids).tolist(), v.tolist()):
        for c, x in enumerate(row):
            if x != x:
                continue
            count[b][c] += 1
            if math.isinf(x):
                inf[b][c].add(x)
                continue
            tot[b][c] += Fraction(x)
            sq[b][c] += Fraction(x) * Fraction(x)

    def close(t, signs, square):
        if not signs:
            return float(t)
        if square:
            return math.inf
        return math.nan if len(signs) == 2 else next(iter(signs))
    return (np.array(count, np.int64).reshape(K, C),
            np.array([[close(tot[k][c], inf[k][c], False) for c in range(C)] for k in range(K)], F64).reshape(K, C),
            np.array([[close(sq[k][c], inf[k][c], True) for c in range(C)] for k in range(K)], F64).reshape(K, C))


def abs_sums(ids, values, K):
    """(sum |v|, sum v^2) per (unit, column) over the values that are not NaN, in float64: what the bound multiplies."""
    ids = np.asarray(ids, np.int64)
    v = _values(values).astype(F64)
    a = np.where(np.isnan(v), 0.0, np.abs(v))
    sa, sq = np.zeros((K, v.shape[1]), F64), np.zeros((K, v.shape[1]), F64)
    with np.errstate(over="ignore"):
        np.add.at(sa, ids, a)
        np.add.at(sq, ids, a * a)
    return sa, sq


def check_value_sums(got, ids, values, K, what=""):
    """The three (K, C) arrays against the model on the given ids and values: counts exactly, |sum - model| <= gamma(m) sum |v|
    and |sumsq - model| <= gamma(m) sum v^2 per (unit, column), m the cell's count; a cell whose sums are not finite must
    hold the model's value (the same infinity, or NaN).  Returns the worst err / bound."""
    count, tot, sq = (np.asarray(a) for a in got)
    C = _values(values).shape[1]
    assert count.dtype == np.int64 and tot.dtype == F64 and sq.dtype == F64, "%s: dtypes %s %s %s" % (what, count.dtype, tot.dtype, sq.dtype)
    assert count.shape == tot.shape == sq.shape == (K, C), "%s: shapes %r %r %r, expected %r" % (what, count.shape, tot.shape, sq.shape, (K, C))
    rc, rt, rq = value_sums_model(ids, values, K)
    assert np.array_equal(count, rc), "%s: counts differ from the model at (unit, column) %r" % (what, np.argwhere(count != rc)[:5].tolist())
    sa, sqa = abs_sums(ids, values, K)
    g = gamma(rc)
    worst = 0.0
    for name, a, r, scale in (("sum", tot, rt, sa), ("sumsq", sq, rq, sqa)):
        wild = ~np.isfinite(r)
        same = (a == r) | (np.isnan(a) & np.isnan(r))
        assert same[wild].all(), "%s: %s where the model is not finite: %r against %r" % (what, name, a[wild & ~same][:5], r[wild & ~same][:5])
        ok = ~wild
        assert np.isfinite(a[ok]).all(), "%s: %s is not finite at %r, the model is" % (what, name, np.argwhere(ok & ~np.isfinite(a))[:5].tolist())
        err = np.abs(a[ok] - r[ok])
        bound = g[ok] * scale[ok]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        if ratio.size:
            i = int(np.argmax(ratio))
            at = np.argwhere(ok)[i]
            assert ratio[i] <= 1.0, "%s: %s of unit %d column %d (%d values): %r, fsum %r, bound %r" % (
                what, name, at[0], at[1], rc[ok][i], a[ok][i], r[ok][i], bound[i])
            worst = max(worst, float(ratio[i]))
    return worst


def classify_model(ids, counts, default=None):
    """The classification rule row by row: the first maximum of the BMU's counts; a unit without a labelled row gives
    `default` (None: the first maximum of the map's totals)."""
    counts = np.asarray(counts)
    flat = counts.reshape(-1, counts.shape[-1]).tolist()
    if default is None:
        totals = [sum(col) for col in zip(*flat)]
        default = totals.index(max(totals))
    out = []
    for b in np.asarray(ids).tolist():
        row = flat[b]
        out.append(row.index(max(row)) if sum(row) > 0 else default)
    return np.array(out, np.int64)
