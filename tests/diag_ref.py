"""A float64 model of the map diagnostics -- som_bmu_distances / som_unit_stats, XPySom.quantization_distances /
unit_statistics -- and the bounds on the device's arithmetic.

Shared by tests/test_diag_cpu.py and tests/test_gpu_diag.py (not a conftest).

The contract (include/somhip.h): b_n is the unit som_bmu(QUANTIZATION) names for row n, d_n the float32 distance
quantization_error forms for the row before it widens and adds it (missing='nan': over the observed features, a row with
nothing observed has b_n = 0 and d_n = 0), and per unit k over the rows with b_n = k: count, sum d_n and sum d_n^2 in double,
max d_n in float32; a unit without rows has four zeros.

The bounds, with u = 2^-24 and query_ref.gamma(n) = n u / (1 - n u):

  d_n        against the float64 |x_n - W[b_n]| over the observed features: relative error <= gamma(D + 10), query_ref's own
             per-row bound of the QE kernel (rounded differences, a fma chain of squares, a wave reduction, one float32
             sqrt).  Where the reference is 0 -- the row equals its unit bit for bit -- the bound is 0: d_n == 0 exactly.
  count      equals numpy.bincount(ids, minlength=K).
  max        equals the maximum of the returned d over the unit's rows bit for bit (NaN ignored, as fmaxf does); 0 if none.
  sum, sumsq against math.fsum over float64(d), and over float64(d)^2 (each square of a float32 is exact in double): the
             terms are non-negative and the device adds them in double in some fixed order, so the relative error is at
             most (count - 1) 2^-53 <= count 2^-53; with count <= 1 nothing is added and the values are equal.  A unit
             holding a NaN distance has NaN sums.
  QE         sum_k sum_k / n against quantization_error on the same rows: 1e-12 relative, the room
             tests/test_gpu_query_ref.py gives the order of QE's own double atomics.  It holds only if the d_n are the
             values qe_kernel adds.
"""
import math

import numpy as np

from tests import query_ref as Q
from tests import update_ref as U

F32, F64 = np.float32, np.float64
U64 = 2.0 ** -53
QE_RTOL = 1e-12


# ------------------------------------------------------------------------------------------------------ the model
def row_distances(x, w, ids, masked=False):
    """|x_n - w[ids_n]| in float64 from the float32 operands; masked: over the features of the row that are not NaN
    (none: 0).  Unmasked rows holding a NaN give NaN."""
    with np.errstate(invalid="ignore"):
        x = np.asarray(x, F32).astype(F64)
    w = np.asarray(w, F32).astype(F64)
    d = x - w[np.asarray(ids, np.int64)]
    sq = d * d
    if masked:
        sq = np.where(np.isnan(sq), 0.0, sq)
    return np.sqrt(sq.sum(axis=1))


def dist_bound(D):
    return Q.gamma(D + 10)


def check_distances(d, x, w, ids, masked=False, what=""):
    """Every returned distance within gamma(D + 10), relative, of the float64 one (0 where that is 0; NaN where that is NaN).
    Returns the worst err / bound."""
    d = np.asarray(d)
    assert d.dtype == F32 and d.shape == (len(x),), "%s: distances must be float32 (n,), got %s %r" % (what, d.dtype, d.shape)
    ref = row_distances(x, w, ids, masked)
    nan = np.isnan(ref)
    assert (np.isnan(d) == nan).all(), "%s: NaN distances at rows %r, the reference's at %r" % (
        what, np.flatnonzero(np.isnan(d))[:5], np.flatnonzero(nan)[:5])
    ok = ~nan
    err = np.abs(d[ok].astype(F64) - ref[ok])
    bound = dist_bound(np.asarray(w).shape[1]) * ref[ok]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    if not r.size:
        return 0.0
    i = int(np.argmax(r))
    assert r[i] <= 1.0, "%s: row %d: distance %r, float64 %r, bound %r" % (what, np.flatnonzero(ok)[i], d[ok][i], ref[ok][i], bound[i])
    return float(r[i])


def unit_stats_model(ids, d, K):
    """(count int64, sum float64, sumsq float64, max float32) per unit from ids and float32 distances: correctly rounded sums
    (math.fsum) of the widened distances and of their exact squares; the maximum ignores NaN; an empty unit has zeros."""
    ids = np.asarray(ids, np.int64)
    d = np.asarray(d, F32)
    count = np.bincount(ids, minlength=K).astype(np.int64)
    tot, sq, mx = np.zeros(K, F64), np.zeros(K, F64), np.zeros(K, F32)
    order = np.argsort(ids, kind="stable")
    cuts = np.concatenate([[0], np.cumsum(count)])
    d64 = d.astype(F64)
    for k in np.flatnonzero(count):
        seg = d64[order[cuts[k]:cuts[k + 1]]]
        if np.isnan(seg).any():
            tot[k] = sq[k] = np.nan
        else:
            tot[k] = math.fsum(seg)
            sq[k] = math.fsum(seg * seg)
        seen = seg[~np.isnan(seg)]
        mx[k] = F32(seen.max()) if len(seen) else F32(0)
    return count, tot, sq, mx


def brute_force_unit_stats(ids, d, K):
    """The same four arrays straight from the definition, a Python loop over the rows (exact rational sums)."""
    from fractions import Fraction
    count = [0] * K
    tot, sq = [Fraction(0)] * K, [Fraction(0)] * K
    mx = [0.0] * K
    bad = [False] * K
    for b, v in zip(np.asarray(ids).tolist(), np.asarray(d, F32).tolist()):
        count[b] += 1
        if v != v:
            bad[b] = True
            continue
        tot[b] += Fraction(v)
        sq[b] += Fraction(v) * Fraction(v)
        mx[b] = max(mx[b], v)
    return (np.array(count, np.int64), np.array([np.nan if z else float(t) for t, z in zip(tot, bad)]),
            np.array([np.nan if z else float(t) for t, z in zip(sq, bad)]), np.array(mx, F32))


def sum_bound(count):
    """Relative bound on a double sum of `count` non-negative terms in any fixed order (0 for count <= 1: nothing is added)."""
    count = np.asarray(count, F64)
    return np.where(count <= 1, 0.0, count * U64)


def check_unit_stats(got, ids, d, K, what="", counts_for_bound=None):
    """The four per-unit arrays against the model on the returned ids and distances.  counts_for_bound: the counts the sums'
    bound is taken from (default: the unit's own).  Returns the worst err / bound over sum and sumsq."""
    count, tot, sq, mx = (np.asarray(a) for a in got)
    assert count.dtype == np.int64 and tot.dtype == F64 and sq.dtype == F64 and mx.dtype == F32, "%s: dtypes %s %s %s %s" % (
        what, count.dtype, tot.dtype, sq.dtype, mx.dtype)
    assert count.shape == tot.shape == sq.shape == mx.shape == (K,), "%s: shapes" % what
    rc, rt, rq, rm = unit_stats_model(ids, d, K)
    assert np.array_equal(count, rc), "%s: counts differ from bincount at units %r" % (what, np.flatnonzero(count != rc)[:5])
    assert np.array_equal(mx.view(np.uint32), rm.view(np.uint32)), "%s: max differs at units %r" % (
        what, np.flatnonzero(mx.view(np.uint32) != rm.view(np.uint32))[:5])
    rel = sum_bound(rc if counts_for_bound is None else counts_for_bound)
    worst = 0.0
    for name, g, r in (("sum", tot, rt), ("sumsq", sq, rq)):
        nan = np.isnan(r)
        assert (np.isnan(g) == nan).all(), "%s: %s is NaN at units %r, the model at %r" % (
            what, name, np.flatnonzero(np.isnan(g))[:5], np.flatnonzero(nan)[:5])
        ok = ~nan
        err = np.abs(g[ok] - r[ok])
        bound = rel[ok] * r[ok]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        if ratio.size:
            i = int(np.argmax(ratio))
            assert ratio[i] <= 1.0, "%s: %s of unit %d (%d rows): %r, fsum %r, bound %r" % (
                what, name, np.flatnonzero(ok)[i], rc[ok][i], g[ok][i], r[ok][i], bound[i])
            worst = max(worst, float(ratio[i]))
    return worst


def check_qe_agreement(tot, n, qe, what=""):
    """sum_k sum_k / n against quantization_error of the same rows, 1e-12 relative."""
    mine = math.fsum(np.asarray(tot, F64).tolist()) / n
    assert abs(mine - qe) <= QE_RTOL * abs(qe), "%s: sum of the unit sums / n = %r, quantization_error %r" % (what, mine, qe)


def combine(parts, K):
    """The host's combination of per-chunk results, in chunk order: counts and sums added (float64), max by np.maximum."""
    count, tot = np.zeros(K, np.int64), np.zeros(K, F64)
    sq, mx = np.zeros(K, F64), np.zeros(K, F32)
    for c, s, s2, m in parts:
        count += c
        tot += s
        sq += s2
        mx = np.maximum(mx, m)
    return count, tot, sq, mx


def mean_std(count, tot, sq):
    """(mean, std) per unit as UnitStatistics defines them: sum / hits and sqrt(max(sumsq / hits - mean^2, 0)); NaN for a
    unit without rows.  The same IEEE operations in the same order, one unit at a time: the arrays must be equal bit for bit."""
    count = np.asarray(count)
    mean, std = np.full(count.shape, np.nan), np.full(count.shape, np.nan)
    for i in np.ndindex(count.shape):
        if count[i]:
            mean[i] = tot[i] / count[i]
            std[i] = math.sqrt(max(sq[i] / count[i] - mean[i] * mean[i], 0.0))
    return mean, std


# ------------------------------------------------------------------------------------------------------ the cases
def _case(X, Y, D, n, prec="f32", data="blobs", env=None, dup=0, missing=None):
    c = dict(X=X, Y=Y, D=D, n=n, prec=prec, data=data, env=dict(env or {}), dup=dup, missing=missing)
    c["id"] = "%dx%dx%d-n%d-%s-%s%s%s" % (X, Y, D, n, prec, data, "-nan" if missing else "",
                                       "".join("-%s%s" % kv for kv in sorted(c["env"].items())))
    return c


SKIP2 = {"SOM_EXACT_SKIP": "2"}
CASES = (
    [_case(5, 7, 1, 1),                                    # one lane, one row, 34 empty units
     _case(5, 7, 3, 127),                                  # odd D; N not a multiple of 4
     _case(5, 7, 64, 129),                                 # exactly one feature per lane
     _case(12, 11, 65, 300),                               # a second fma step on lane 0 only
     _case(12, 11, 130, 1031, data="int", dup=5),          # D beyond 128; exact arithmetic
     _case(16, 16, 260, 257, prec="bf16"),                 # ids through the 16-bit search, distances still float32
     _case(16, 16, 260, 257, prec="f16")]
    # screen + window path; >= 4096 units; rows that are units
    + [_case(64, 64, 32, 5000, prec="exact", data=kind, env=env)
       for env in (None, SKIP2) for kind in ("blobs", "offset30", "offset300", "weights")]
    + [_case(64, 64, 32, 5000, data="three")]              # three segments of > 1000 rows, 4093 empty units
    + [_case(X, Y, D, n, prec=prec, missing="nan")         # 30 % NaN, one all-NaN row, one feature nobody observes
       for (X, Y, D, n) in ((12, 11, 33, 300), (5, 7, 3, 127)) for prec in ("f32", "exact")]
    # past one turn of bmu_dist_kernel's persistent loop (16 384 waves), and the per-unit kernels behind both sorts at scale
    + [_case(5, 7, 3, 40003)]                              # three turns, the last partial
    + [_case(12, 11, 130, 16389, prec=prec, missing="nan") for prec in ("f32", "exact")]   # just past the grid cap; the mask on
    #                                                        the second and third fma steps of a lane
    + [_case(12, 11, 65, 300, missing="nan")]              # the mask on lane 0's second step alone
    + [_case(128, 64, 4, 5000)]                            # K = 8 192 = CS_MAX_K: the counting sort at its ceiling
    + [_case(129, 64, 4, 5000)]                            # K = 8 256: the radix sort, 14 key bits, > 3 000 empty units
)
DIST_WAVES = 4 * 4096                                      # bmu_dist_kernel's grid cap: a wave takes rows r, r + 16 384, ...


def sort_path(c):
    """The sort sort_rows_by_unit takes for a case's query, the first of its handle: update_ref.sort_path, the rule's one restatement."""
    return U.sort_path(c["X"] * c["Y"], c["n"])


def case_seed(c):
    return (c["X"] * 7919 + c["Y"] * 131 + c["D"] * 17 + c["n"]) % 100003


def case_data(c):
    """(rows, codebook) of a case, float32.  Kinds beyond query_ref.make_rows': `weights` -- every row a copy of a unit --,
    `three` -- every row a copy of one of three rows; missing: 30 % of the entries NaN, row 0 all NaN, the last feature
    NaN in every row."""
    X, Y, D, n = c["X"], c["Y"], c["D"], c["n"]
    K, seed = X * Y, case_seed(c)
    rs = np.random.RandomState(seed + 2)
    kind = c["data"]
    base = kind if kind in ("blobs", "offset30", "offset300", "int") else "blobs"
    x = Q.make_rows(base, n, D, seed)
    w = Q.make_units(base, x, K, D, seed, c["dup"])
    if kind == "weights":
        x = np.ascontiguousarray(w[rs.randint(0, K, n)])
    elif kind == "three":
        x = np.ascontiguousarray(x[:3][np.arange(n) % 3])
    if c["missing"]:
        x = x.copy()
        x[rs.random_sample(x.shape) < 0.3] = np.nan
        x[0] = np.nan
        x[:, D - 1] = np.nan
    return x, w
