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
  sum_wd, tight  against the float32 distances d_n that bmu_distances returned for the same rows, units and codebook
                 (check_rows_tight): csrc/monitor.hpp promises that its d_n is bmu_dist_kernel's float32 bit for bit, so the exact
                 value of sum_wd is sum_n w_n d_n over those float32 -- every product float32 x float32 is exact in double -- and
                 the only roundings are the device's double additions of `rows` non-negative terms in some fixed order: at most
                 rows - 1 of them on the way to any term, (rows - 1) 2^-53 relative to first order, doubled for the higher
                 orders: |sum_wd - fsum| <= 2 rows 2^-53 fsum.  No summation tree is pinned.  One wrong, dropped or doubled
                 row among 80 000 moves the sum by about 1 / 80 000 of itself, 10^7 times that bound.

The launch geometry (rows_paths, shift_paths) restates csrc/monitor.hpp's: monitor_rows_grid, MON_ROWS_UNROLL = 4 rows per wave
and turn at row0 + j waves, monitor_shift_grid and the (k, d) walk under its stride, monitor_reduce_chunk.  BIG_CASES is the
list of cases built to reach what those helpers name; tests/test_monitor_cpu.py holds it to that, tests/test_gpu_monitor.py runs it.
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


def check_rows_tight(m, d32, weights=None, what=""):
    """sum_wd of a device record against math.fsum(float64(w_n) float64(d32_n)) over the rows of non-zero weight, d32 the
    float32 distances bmu_distances returned for the same rows and units: within 2 rows 2^-53 relative (the module docstring
    derives it).  Returns err / bound."""
    d64 = np.asarray(d32, F32).astype(F64)
    wt = np.ones(len(d64), F64) if weights is None else np.asarray(weights, F32).astype(F64)
    assert wt.shape == d64.shape, "%s: %d weights for %d distances" % (what, len(wt), len(d64))
    keep = wt != 0
    rows = int(keep.sum())
    ref = math.fsum((wt[keep] * d64[keep]).tolist())       # (float32 x float32: exact in double)
    bound = 2 * rows * Q.U64 * ref
    err = abs(m["sum_wd"] - ref)
    ratio = 0.0 if err == 0 else (err / bound if bound > 0 else math.inf)
    assert ratio <= 1.0, "%s: sum_wd %r, the sum of the float32 distances %r (err %r, bound %r)" % (what, m["sum_wd"], ref, err, bound)
    return ratio


# ------------------------------------------------------------------------------------------ the launch geometry
MON_ROWS_UNROLL, MON_REDUCE_THREADS = 4, 256


def _cdiv(a, b):
    return -(-a // b)


def rows_grid(N):
    return min(_cdiv(N, 4), 4096)


def shift_grid(elems):
    return min(_cdiv(elems, 1024), 2048)


def reduce_chunk(n_parts):
    return _cdiv(n_parts, MON_REDUCE_THREADS)


def _reduce_paths(g):
    out = set()
    if g > 0:
        c = reduce_chunk(g)
        out.add("reduce.c=%d" % c)
        if g % c:                                           # the last non-empty thread holds g mod c < c partials
            out.add("reduce.ragged")
    return out


def rows_paths(N, weights=None):
    """What monitor_rows_kernel and its reduction reach on N rows (weights: the rows' sample weights or None):
      turn.all          a wave's turn with four live rows: monitor_row_chains<., true>
      turn.tail         a turn with fewer than four rows below N
      turn.zero_weight  four rows below N, at least one of weight 0 and at least one live: <., false> with live rows around a hole
      second_turn       some wave's outer loop runs twice
      reduce.c=<c>      the run of partials a reduction thread adds; reduce.ragged: the last non-empty thread holds fewer
    A row is live when it lies below N and its weight is not 0."""
    out = set()
    g = rows_grid(N)
    if g == 0:
        return out
    waves = 4 * g
    wt = None if weights is None else np.asarray(weights, F32)
    row0 = np.arange(N, dtype=np.int64)
    row0 = row0[(row0 // waves) % MON_ROWS_UNROLL == 0]     # wave w's turns start at w + t * 4 * waves
    rows = row0[:, None] + np.arange(MON_ROWS_UNROLL, dtype=np.int64)[None, :] * waves
    below = rows < N
    live = below.copy()
    if wt is not None:
        live[below] = wt[rows[below]] != 0
    full = below.all(axis=1)
    nlive = live.sum(axis=1)
    if (nlive == MON_ROWS_UNROLL).any():
        out.add("turn.all")
    if (~full).any():
        out.add("turn.tail")
    if (full & (nlive < MON_ROWS_UNROLL) & (nlive > 0)).any():
        out.add("turn.zero_weight")
    if N > waves * MON_ROWS_UNROLL:
        out.add("second_turn")
    return out | _reduce_paths(g)


def shift_paths(K, D):
    """What monitor_shift_kernel and its reduction reach on a K x D codebook:
      grid.capped   cdiv(K D, 1024) exceeds the 2 048 workgroups; grid.multi: two workgroups or more
      sk.zero       the stride is shorter than a codebook row (sk = stride / D == 0)
      sd.nonzero    the stride is no multiple of D, so d moves
      carry         some thread's d + sd reaches D on an element it reads
      reduce.c=<c>  (and reduce.ragged) as in rows_paths
    The walk itself is replayed: (k, d) must be (i / D, i mod D) at every element, or the helper fails."""
    out = set()
    total = K * D
    g = shift_grid(total)
    if g == 0:
        return out
    if _cdiv(total, 1024) > 2048:
        out.add("grid.capped")
    if g >= 2:
        out.add("grid.multi")
    stride = g * 256
    sk = stride // D
    sd = stride - sk * D
    if sk == 0:
        out.add("sk.zero")
    if sd != 0:
        out.add("sd.nonzero")
    i = np.arange(min(stride, total), dtype=np.int64)
    k, d = i // D, i % D
    while True:
        i, k, d = i + stride, k + sk, d + sd
        on = i < total
        if not on.any():
            break
        i, k, d = i[on], k[on], d[on]
        over = d >= D
        if over.any():
            out.add("carry")
        k, d = k + over, d - over * D
        assert np.array_equal(k, i // D) and np.array_equal(d, i % D), "the (k, d) walk leaves the element at K=%d D=%d" % (K, D)
    return out | _reduce_paths(g)


# ------------------------------------------------------------------------------------------ the cases past one turn
def _big(X, Y, D, n, prec="f32", epochs=2, weights=None, masked=False, env=None, data="blobs"):
    kw = dict(precision=prec)
    if masked:
        kw["missing"] = "nan"
    return dict(X=X, Y=Y, D=D, n=n, kw=kw, env=dict(env or {}), epochs=epochs, weights=weights, masked=masked, data=data)


# name: the shapes of the issue's table; what each reaches is pinned by tests/test_monitor_cpu.py
BIG_CASES = {
    "f32-n81925": _big(12, 10, 3, 81925),
    "f32-n65536-d130": _big(12, 10, 130, 65536),
    "weighted-n81925": _big(12, 10, 7, 81925, weights="tenth_zero"),
    "masked-weighted-n70001-d65": _big(16, 16, 65, 70001, weights="012", masked=True),
    # four epochs: the assertions on the plan's counters are those of the 20 000-row case, which need three planned epochs
    "exact-skip-n81925": _big(64, 64, 32, 81925, prec="exact", epochs=4, env={"SOM_EXACT_SKIP": "2"}, data="gaussian_blobs"),
    "f32-n1025": _big(12, 10, 7, 1025),
    "shift-128x128x129": _big(128, 128, 129, 300),
    "shift-masked-24x24x65": _big(24, 24, 65, 500, weights="012", masked=True),
}


def masked_rows(n, D, seed=5):
    """Rows with 30 % of the values missing and row 7 entirely, and weights 0, 1, 2 (row 7: 1)."""
    from tests import missing_ref as M
    x = M.punch(Q.make_rows("blobs", n, D, 11), "random30", seed)
    x[7] = np.nan                                            # one row with nothing observed
    w = np.random.RandomState(2).randint(0, 3, n).astype(F32)
    w[7] = 1.0
    return x, w


def big_case_weights(name):
    c = BIG_CASES[name]
    if c["weights"] is None:
        return None
    if c["weights"] == "tenth_zero":
        from tests import weights_ref
        return weights_ref.make_weights(c["n"], 5 + c["D"])
    return masked_rows(c["n"], c["D"])[1]


def big_case_data(name):
    """(rows float32 (n, D), weights float32 (n,) or None) of a case of BIG_CASES."""
    c = BIG_CASES[name]
    n, D = c["n"], c["D"]
    if c["masked"]:
        return masked_rows(n, D)
    if c["data"] == "gaussian_blobs":
        from oracle import som_oracle as O
        return O.gaussian_blobs(n, D, seed=11), big_case_weights(name)
    return Q.make_rows("blobs", n, D, 11 + D), big_case_weights(name)


def check_near_ties(x, w, ids_a, ids_b, rows, masked=False, what=""):
    """Rows on which two float32 searches name different units: both must be minima at float32's resolution.  The training
    search scores |w|^2 - 2 x.w and the quantization search the differences themselves, each sum of D float32 terms: either
    score is within gamma(D + 2) (|x| + |w|)^2 of the exact squared distance (up to the |x|^2 both drop or keep), so two
    units each search may prefer differ in it by at most gamma(D + 10) ((|x| + |w_a|)^2 + (|x| + |w_b|)^2)."""
    x64 = np.nan_to_num(np.asarray(x, F32)[rows].astype(F64)) if masked else np.asarray(x, F32)[rows].astype(F64)
    seen = ~np.isnan(np.asarray(x, F32)[rows]) if masked else np.ones(x64.shape, bool)
    w64 = np.asarray(w, F32).astype(F64)
    wa, wb = w64[np.asarray(ids_a, np.int64)[rows]] * seen, w64[np.asarray(ids_b, np.int64)[rows]] * seen
    sa, sb = ((x64 - wa) ** 2).sum(axis=1), ((x64 - wb) ** 2).sum(axis=1)
    nx, na, nb = (np.sqrt((v * v).sum(axis=1)) for v in (x64, wa, wb))
    room = Q.gamma(w64.shape[1] + 10) * ((nx + na) ** 2 + (nx + nb) ** 2)
    bad = np.flatnonzero(np.abs(sa - sb) > room)
    assert len(bad) == 0, "%s: row %d: units %d and %d at squared distances %r and %r are no tie (room %r)" % (
        what, rows[bad[0]], ids_a[rows[bad[0]]], ids_b[rows[bad[0]]], sa[bad[0]], sb[bad[0]], room[bad[0]])
