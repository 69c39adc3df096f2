"""A float64 reference of the query kernels, rigorous bounds on their float32 arithmetic, the checks built on the two, and a
pure-Python mirror of the host's query dispatch.

Shared by tests/test_query_ref_cpu.py, tests/test_gpu_query_ref.py and tests/fuzz/fuzz_query.py (not a conftest).

`scores(x, w, mode)` computes every score matrix in float64 from the float32 operands, sharing nothing with the kernels'
order of operations, and a per-element bound E on what the kernel's float32 evaluation of the same element may be off by.
With u = 2^-24 and gamma(n) = n u / (1 - n u), S = |x| . |w|^T, Xq = |x|^2, Wq = |w|^2 (the float64 values):

  part    |w|^2 - 2 x.w                   the cross term is a k-ordered fma chain of D terms (gamma(D) S), |w|^2 a NumPy
                                          pairwise sum of rounded squares (gamma(D + 1) Wq), one fma joins them:
                                          E = gamma(D + 2) (2 S + Wq)
  sq      part + |x|^2                    one more addition, |x|^2 like |w|^2: E = gamma(D + 3) (2 S + Wq + Xq)
  sqrt    nan_to_num(sqrt(sq))            |sqrt a - sqrt b| <= sqrt |a - b| for a, b >= 0 (a negative radicand: 0), plus
                                          the sqrt's own rounding: E = sqrt(E_sq) + 2u sqrt(sq + E_sq)
  cosine  1 - nan_to_num(x.w / sqrt(Xq Wq))   E = (gamma(D) S + |x.w| gamma(D + 4)) / sqrt(Xq Wq) + 2u; a zero row or
                                          unit gives 1 exactly (0 / 0 -> NaN -> 0), E = 0 there
  even p  sum_e (-1)^e C(p,e) x^(p-e).w^e  each power rounded once, each dot a fma chain, each coefficient product
                                          rounded once, the sum in float64: the term e is off by at most
                                          gamma(D + 3) C(p,e) sum_d |x_d|^(p-e) |w_d|^e, and those terms add up to
                                          E = gamma(D + 3) sum_d (|x_d| + |w_d|)^p
  generic sum_d |x_d - w_d|^p             the difference rounded once (u), the power once more (u), p of the first
                                          inside the power, then a pairwise sum: E = gamma(D + ceil(p) + 1) sum_d
                                          |x_d - w_d|^p  (+ (D + 1) 2^-125: float32 powers of tiny differences underflow)
  f64     fl64(-2 x.w + |w|^2_f32)        a float64 fma chain against the float32 |w|^2:
                                          E = 2 gamma64(D + 2) (2 S + Wq) + gamma(D + 1) Wq (the float32 |w|^2 itself)

The checks:
  admissible pick   the float32 argmin k of scores s~ has s~_k <= s~_j for every j, so s_k <= min_j (s_j + E_j) + E_k
  exact ties        on small integer data every euclidean / manhattan score is exact: the pick IS the lowest-index argmin
  top-2             both ids differ; their scores are the row's two smallest within the same bound, in order
  distance matrix   |got - s| <= E elementwise
  QE                qe_kernel sums fma'd squares of rounded differences and takes a float32 sqrt per row: relative error
                    <= gamma(D + 10) per row, so |qe - mean |x - w[ids]|| <= gamma(D + 10) mean |x - w[ids]|

`query_paths` returns labels for the kernel instances a query call reaches (csrc/somhip.hip, lines cited below), so that
tests/test_query_ref_cpu.py can show that the GPU module's case list reaches every one of them.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
U64 = 2.0 ** -53
MODES = ("part", "sq", "sqrt", "cosine")


def gamma(n, u=U):
    return n * u / (1.0 - n * u)


def _chunks(n, K, D, budget=1 << 24):
    step = max(1, budget // max(1, K * D))
    return range(0, n, step), step


def _pow_sum(x, w, fn):
    """sum_d fn(x_d, w_d) as an (n, K) float64 matrix, in row chunks (an (n, K, D) tensor at once is too large)."""
    n, K, D = len(x), len(w), x.shape[1]
    out = np.zeros((n, K))
    starts, step = _chunks(n, K, D)
    for s in starts:
        out[s:s + step] = fn(x[s:s + step, None, :], w[None, :, :]).sum(axis=2)
    return out


def scores(x, w, mode, p=2, p_real=0.0):
    """(s, E): the float64 score matrix (n, K) of `mode` and the bound on the kernel's float32 evaluation of it.

    mode: part / sq / sqrt / cosine (the GEMM forms), even (norm_p with even integer p), generic (sum |x - w|^p with an
    integer p, manhattan is p = 1; with p_real != 0 the real exponent p_real), f64 (x taken as float64 rows)."""
    x = np.asarray(x, F64) if mode == "f64" else np.asarray(x, F32).astype(F64)
    w = np.asarray(w, F32).astype(F64)
    D = w.shape[1]
    if mode in ("even", "generic"):
        if mode == "even":
            s = _pow_sum(x, w, lambda a, b: (a - b) ** p)
            E = gamma(D + 3) * _pow_sum(x, w, lambda a, b: (np.abs(a) + np.abs(b)) ** p)
        else:
            q = p_real if p_real else p
            s = _pow_sum(x, w, lambda a, b: np.abs(a - b) ** q)
            E = gamma(D + math.ceil(q) + 1) * s + (D + 1) * 2.0 ** -125
        return s, E
    c = x @ w.T
    S = np.abs(x) @ np.abs(w).T
    Xq = (x * x).sum(1)[:, None]
    Wq = (w * w).sum(1)[None, :]
    if mode == "f64":
        return Wq - 2 * c, 2 * gamma(D + 2, U64) * (2 * S + Wq) + gamma(D + 1) * Wq
    if mode == "cosine":
        den = np.sqrt(Xq * Wq)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = 1 - np.nan_to_num(c / den)
            E = np.where(den > 0, (gamma(D) * S + np.abs(c) * gamma(D + 4)) / den + 2 * U, 0.0)
        return s, E
    part = Wq - 2 * c
    if mode == "part":
        return part, gamma(D + 2) * (2 * S + Wq)
    sq = part + Xq
    Esq = gamma(D + 3) * (2 * S + Wq + Xq)
    if mode == "sq":
        return sq, Esq
    sq = np.maximum(sq, 0.0)                               # (exact arithmetic: |x - w|^2 >= 0)
    return np.sqrt(sq), np.sqrt(Esq) + 2 * U * np.sqrt(sq + Esq)


# ------------------------------------------------------------------------------------------------------ the checks
def pick_ratio(ids, s, E):
    """Per row: how far the pick's score sits above min_j (s_j + E_j), in units of its own bound E_k (<= 1: admissible;
    an excess with E_k = 0 is infinitely wrong)."""
    ids = np.asarray(ids, np.int64)
    r = np.arange(len(ids))
    if len(ids) and (ids.min() < 0 or ids.max() >= s.shape[1]):
        return np.full(len(ids), np.inf)
    cap = (s + E).min(axis=1)
    over = s[r, ids] - cap
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(over <= 0, 0.0, over / E[r, ids])


def check_picks(ids, s, E, what=""):
    """Assert every pick admissible; returns the worst ratio."""
    rat = pick_ratio(ids, s, E)
    if not len(rat):
        return 0.0
    i = int(np.argmax(rat))
    assert rat[i] <= 1.0, "%s: row %d picks unit %d (score %r), the row's best is unit %d (%r), err/bound %.3g" % (
        what, i, int(ids[i]), float(s[i, int(ids[i])]) if 0 <= ids[i] < s.shape[1] else None, int(np.argmin(s[i])),
        float(s[i].min()), rat[i])
    return float(rat[i])


def check_ties(ids, s, what=""):
    """Exact data: the picks are the lowest-index argmin, bit for bit."""
    want = np.argmin(s, axis=1)
    bad = np.flatnonzero(np.asarray(ids) != want)
    assert len(bad) == 0, "%s: %d rows differ from the lowest-index argmin, first row %d: %d vs %d" % (
        what, len(bad), bad[0], int(ids[bad[0]]), int(want[bad[0]]))


def check_top2(i1, i2, s, E, what="", exact=False):
    """(best, second) per row: the ids differ, the pair's scores are the row's two smallest within the bound and in order;
    exact data: the two smallest values, and equal values go to the lower id first.  Returns the worst ratio."""
    i1, i2 = np.asarray(i1, np.int64), np.asarray(i2, np.int64)
    n, K = s.shape
    if K == 1:
        assert (i1 == 0).all() and (i2 == 0).all(), "%s: a one-unit map names unit 0 twice" % what
        return 0.0
    r = np.arange(n)
    assert ((i1 >= 0) & (i1 < K) & (i2 >= 0) & (i2 < K)).all(), "%s: an id out of range" % what
    same = np.flatnonzero(i1 == i2)
    assert len(same) == 0, "%s: row %d names unit %d twice" % (what, same[0], i1[same[0]])
    srt = np.sort(s, axis=1)
    s1, s2 = s[r, i1], s[r, i2]
    if exact:
        bad = np.flatnonzero((s1 != srt[:, 0]) | (s2 != srt[:, 1]) | ((s1 == s2) & (i1 > i2)))
        assert len(bad) == 0, "%s: row %d: pair (%d, %d) scores (%r, %r), the two smallest (%r, %r)" % (
            what, bad[0], i1[bad[0]], i2[bad[0]], s1[bad[0]], s2[bad[0]], srt[bad[0], 0], srt[bad[0], 1])
        return 0.0
    worst = pick_ratio(i1, s, E)
    # the second: the smallest of the row without the best, within the bound
    s_wo = s + E
    s_wo[r, i1] = np.inf
    cap2 = s_wo.min(axis=1)
    e1, e2 = E[r, i1], E[r, i2]
    with np.errstate(divide="ignore", invalid="ignore"):
        r2 = np.where(s2 - cap2 <= 0, 0.0, (s2 - cap2) / e2)
        r3 = np.where(s1 - s2 <= 0, 0.0, (s1 - s2) / (e1 + e2))        # in order: s~1 <= s~2
    worst = np.maximum(worst, np.maximum(r2, r3))
    i = int(np.argmax(worst)) if n else 0
    assert n == 0 or worst[i] <= 1.0, "%s: row %d pair (%d, %d) scores (%r, %r), the two smallest (%r, %r): err/bound %.3g" % (
        what, i, i1[i], i2[i], s1[i], s2[i], srt[i, 0], srt[i, 1], worst[i])
    return float(worst[i]) if n else 0.0


def check_matrix(got, s, E, what=""):
    """Every element within its bound; returns the worst ratio."""
    got = np.asarray(got, F64).reshape(s.shape)
    err = np.abs(got - s)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / E)
    r[~np.isfinite(got)] = np.inf
    if not r.size:
        return 0.0
    i = int(np.argmax(r))
    assert r.flat[i] <= 1.0, "%s: element (%d, %d) = %r, reference %r, bound %r" % (
        what, i // s.shape[1], i % s.shape[1], float(got.flat[i]), s.flat[i], E.flat[i])
    return float(r.flat[i])


def qe_reference(x, w, ids):
    """mean_n |x_n - w[ids_n]| in float64 (xpysom.py:700-705 with the reference's own ids)."""
    x = np.asarray(x, F32).astype(F64)
    w = np.asarray(w, F32).astype(F64)
    return float(np.linalg.norm(x - w[np.asarray(ids, np.int64)], axis=1).mean())


def check_qe(qe, x, w, ids, what=""):
    """quantization_error against the float64 mean distance to the units `ids`; returns err / bound."""
    ref = qe_reference(x, w, ids)
    bound = gamma(np.asarray(w).shape[1] + 10) * ref
    err = abs(float(qe) - ref)
    ratio = 0.0 if err == 0 else (err / bound if bound > 0 else math.inf)
    assert ratio <= 1.0, "%s: QE %r, float64 mean distance to the ids %r (bound %r)" % (what, qe, ref, bound)
    return ratio


# ------------------------------------------------------------------------------------------ the host's dispatch
PW_SAMPLES, PW_UNITS = 128, 16              # bmu_pairwise.hpp:22-23
FR_STAGE_UNITS = 64                         # bmu_f32_res.hpp:25
F32_SB = F32_UB = 128                       # bmu_f32.hpp:26-27
TL_BK = 32                                  # bmu_bf16_tiled.hpp:24
QE_ROWS_ONE_PASS = 4096 * 4                 # qe_kernel's grid: min(cdiv(n, 4), 4096) workgroups of 4 waves


def _cdiv(a, b):
    return -(-a // b)


def is_exact(X, Y, D, precision, distance, env=None):
    """Whether an 'exact' handle runs the screen (som_create, somhip.hip:1357-1392); else it runs the float32 kernels."""
    env = env or {}
    if precision != "exact":
        return False
    K = X * Y
    wide = D > 128 and K >= 4096 and _cdiv(D, TL_BK) <= 25 and env.get("SOM_BF16_WIDE", "1") != "0"
    if D <= 128:
        return distance == "euclidean"
    return distance in ("euclidean", "cosine") and wide


def query_paths(X, Y, D, n, precision, distance, call, env=None, p=2, p_real=0.0):
    """The kernel instances one query call of n rows reaches on an X x Y x D map, as labels:

      f32.res.kg{1,2,4,8,16}[.single|.multi]   the float32 resident kernel (launch_bmu_f32_res_kg, somhip.hip:584-613) with
                        its k-group (8 .. 128 features per row image); one part or several merged through the 64-bit
                        atomicMin -- named only where the count is known beforehand: one 64-unit stage, or SOM_F32_PARTS
                        set (the occupancy otherwise decides, choose_parts)
      f32.res.kgN.top2 / f32.tiled / f32.tiled.top2   its top-2 variant (always one part); the tiled kernel beyond 128 features
      pairwise.{even,generic,real}.{lds,global}   bmu_pairwise_kernel (launch_bmu_pairwise, somhip.hip:905-924): the binomial
                        form, |x - w|^p, a real p; the rows in LDS or read from global memory (150 KiB rule: D >= 266)
      dist.{part,sq,sqrt,cosine}, dist.rowtiles2+, dist.unittiles2+   dist_matrix_f32_kernel's modes, and grids of more
                        than one 128-row / 128-unit tile
      f64               bmu_f64_kernel
      qe.one_pass / qe.stride   qe_kernel with every row in its first pass, or striding (n > 16 384)
      qe.exact_screen   the value-only quantization search of an 'exact' handle: screen, tie-window test, SQRT kernel
      screen            any other 16-bit / exact screen (not a query kernel of this module)

    call: bmu, quant (som_bmu QUANTIZATION), top2, dist, dist_q (QUANTIZATION mode), f64, qe, qe_dev."""
    env = env or {}
    K = X * Y
    exact = is_exact(X, Y, D, precision, distance, env)
    prec = precision if (precision != "exact" or exact) else "f32"
    out = set()

    def f32(top2=False):
        if D > 128:
            out.add("f32.tiled.top2" if top2 else "f32.tiled")
            return
        kg = 1
        while kg * 8 < D:
            kg *= 2
        if top2:
            out.add("f32.res.kg%d.top2" % kg)
            return
        out.add("f32.res.kg%d" % kg)
        stages = _cdiv(K, FR_STAGE_UNITS)
        forced = int(env.get("SOM_F32_PARTS", "0") or 0)
        if forced > 0:
            out.add("f32.res.kg%d.%s" % (kg, "single" if min(forced, stages) == 1 else "multi"))
        elif stages == 1:
            out.add("f32.res.kg%d.single" % kg)

    def pairwise():
        lds = PW_UNITS * D * 4 + PW_SAMPLES * (D + 1) * 4 <= 150 * 1024
        if p_real:
            kind = "real"
        elif distance == "norm_p" and p % 2 == 0:
            kind = "even"
        else:
            kind = "generic"
        out.add("pairwise.%s.%s" % (kind, "lds" if lds else "global"))

    def quantization(value_only):
        if prec != "f32" and distance == "euclidean" and (not exact or value_only):
            out.add("qe.exact_screen" if exact else "screen")
        else:
            f32()

    if call == "bmu":
        if exact or prec != "f32":
            out.add("screen")
        elif distance in ("euclidean", "euclidean_no_opt", "cosine"):
            f32()
        else:
            pairwise()
    elif call == "quant":
        quantization(False)
    elif call == "top2":
        f32(top2=True)
    elif call in ("dist", "dist_q"):
        mode = "sqrt" if call == "dist_q" else {"euclidean": "part", "euclidean_no_opt": "sq", "cosine": "cosine"}[distance]
        out.add("dist." + mode)
        if n > F32_SB:
            out.add("dist.rowtiles2+")
        if K > F32_UB:
            out.add("dist.unittiles2+")
    elif call == "f64":
        out.add("f64")
    elif call in ("qe", "qe_dev"):
        quantization(True)
        out.add("qe.one_pass" if n <= QE_ROWS_ONE_PASS else "qe.stride")
    else:
        raise ValueError(call)
    return out


ALL_LABELS = ({"f32.res.kg%d.%s" % (kg, v) for kg in (1, 2, 4, 8, 16) for v in ("single", "multi", "top2")}
              | {"f32.res.kg%d" % kg for kg in (1, 2, 4, 8, 16)}
              | {"f32.tiled", "f32.tiled.top2"}
              | {"pairwise.%s.%s" % (k, m) for k in ("even", "generic", "real") for m in ("lds", "global")}
              | {"dist.part", "dist.sq", "dist.sqrt", "dist.cosine", "dist.rowtiles2+", "dist.unittiles2+"}
              | {"f64", "qe.one_pass", "qe.stride", "qe.exact_screen", "screen"})


# ------------------------------------------------------------------------------------------ data
def make_rows(kind, n, D, seed):
    """float32 rows: blobs (centred Gaussian blobs), offset30 / offset300 (blobs of spread 1e-3 / 1e-1 around a common
    offset of 30 / 300 -- float32's cancellation regime), int (small integers: every score exact)."""
    rs = np.random.RandomState(seed)
    if kind == "blobs":
        c = rs.normal(0.0, 3.0, (8, D))
        return (c[rs.randint(0, 8, n)] + rs.normal(0.0, 1.0, (n, D))).astype(F32)
    if kind in ("offset30", "offset300"):
        off, spread = (30.0, 1e-3) if kind == "offset30" else (300.0, 1e-1)
        c = off + rs.normal(0.0, spread * 10, (8, D))
        return (c[rs.randint(0, 8, n)] + rs.normal(0.0, spread, (n, D))).astype(F32)
    if kind == "int":
        return rs.randint(-3, 4, (n, D)).astype(F32)
    raise ValueError(kind)


def make_units(kind, rows, K, D, seed, dup=0):
    """A codebook (K, D) near the rows: units drawn from the rows plus noise of the rows' own scale (int: small integers);
    `dup` > 0 repeats the first dup units at the end (duplicate units: the lowest id must win)."""
    rs = np.random.RandomState(seed + 1)
    if kind == "int":
        w = rs.randint(-3, 4, (K, D)).astype(F32)
    else:
        base = rows[rs.randint(0, len(rows), K)].astype(F64)
        spread = {"blobs": 1.0, "offset30": 1e-3, "offset300": 1e-1}[kind]
        w = (base + rs.normal(0.0, spread, (K, D))).astype(F32)
    if dup:
        w[K - dup:] = w[:dup]
    return w
