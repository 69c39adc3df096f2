"""A float64 model of the engine with missing values (`XPySom(..., missing='nan')`, SOM_MISSING_NAN).

Shared by tests/test_missing_cpu.py, tests/test_gpu_missing.py and tests/test_gpu_missing_large.py (not a conftest); the
last one's forced-update grid, LARGE_FORCED, lives here so that the CPU coverage test reads the same table.

A NaN in a row means "not observed".  With m_nd = 1 where x_nd is observed and 0 otherwise, x~_nd = x_nd where observed and
0 otherwise:

    BMU      b_n = first argmin_k of sum_d m_nd (x_nd - w_kd)^2  =  q_n + s_nk,   q_n = sum_d m_nd x_nd^2 (the same for every
             unit),  s_nk = c2_nk - 2 c1_nk,  c1 = sum_d x~_nd w_kd,  c2 = sum_d m_nd w_kd^2
    update   num[k,d] = sum_n g(b_n, k) m_nd x~_nd      den[k,d] = sum_n g(b_n, k) m_nd      (sample weights w_n multiply both)
             W[k,d] = num / den where den != 0, else unchanged
    QE       mean_n sqrt(sum_d m_nd (x_nd - w_{b_n,d})^2), a row with nothing observed adds 0 and is counted

`masked_scores` returns s and the bound E on the kernel's float32 evaluation of it: each of c1 and c2 is a k-ordered fma
chain of D terms, the squares w^2 are rounded once before they enter c2, and one fma joins the two --
E = gamma(D + 3) (2 sum_d |x~_d w_d| + sum_d m_d w_d^2) with query_ref.gamma; picks are checked with query_ref.check_picks
(a per-row constant q_n shifts a row's scores and its cap alike, so s serves in place of the full distance).

The update model is tests/update_ref.py's `reference_update` (tests/weights_ref.py's weighted one) applied to the AUGMENTED
rows [x~ | m] of width 2 D: its first D columns are num, its last D are den, and the magnitudes are split the same way.  The
device forms one rounding per row and per MFMA step on those columns exactly as on ordinary features, so update_ref.TOL and
the magnitude-relative form of its check apply as they stand.  `brute_force_update` -- a loop over the rows, straight from
the definition -- pins the model itself.
"""
import numpy as np

from oracle import som_oracle as O
from tests import query_ref as Q
from tests import update_ref as U
from tests import weights_ref as R

F32, F64 = np.float32, np.float64
PATTERNS = ("none", "random30", "feature", "row", "halves", "payload")


def _rows64(x):
    """float32 rows as float64 (a signalling NaN raises the invalid flag when it is widened: of no interest here)."""
    with np.errstate(invalid="ignore"):
        return np.asarray(x, F32).astype(F64)


# ------------------------------------------------------------------------------------------------------ the split
def split(x):
    """(x~, m) in float64 of float32 rows: x where observed and 0 where NaN; 1 where observed and 0 where NaN."""
    x = np.asarray(x, F32)
    seen = ~np.isnan(x)
    return np.where(seen, x, F32(0)).astype(F64), seen.astype(F64)


def augmented(x):
    """The rows [x~ | m], float64 (N, 2 D)."""
    xt, m = split(x)
    return np.hstack([xt, m])


# ------------------------------------------------------------------------------------------------------ the search
def masked_scores(x, w):
    """(s, E): s_nk = c2 - 2 c1 in float64, (n, K), and the bound on the kernel's float32 evaluation of it."""
    xt, m = split(x)
    w = np.asarray(w, F32).astype(F64)
    D = w.shape[1]
    c1 = xt @ w.T
    c2 = m @ (w * w).T
    S = np.abs(xt) @ np.abs(w).T
    return c2 - 2 * c1, Q.gamma(D + 3) * (2 * S + c2)


def masked_sq_dist(x, w):
    """sum_d m_nd (x_nd - w_kd)^2 as the definition reads, float64 (n, K), in row chunks."""
    x = _rows64(x)
    w = np.asarray(w, F32).astype(F64)
    out = np.zeros((len(x), len(w)))
    step = max(1, (1 << 22) // max(1, w.size))
    for s in range(0, len(x), step):
        d = x[s:s + step, None, :] - w[None, :, :]
        out[s:s + step] = np.where(np.isnan(d), 0.0, d * d).sum(axis=2)
    return out


def masked_bmu(x, w):
    """The first minimum of the masked squared distance per row (int64)."""
    return np.argmin(masked_sq_dist(x, w), axis=1)


def qe_reference(x, w, ids):
    """mean_n sqrt(sum_d m_nd (x_nd - w[ids_n, d])^2), float64."""
    x = _rows64(x)
    w = np.asarray(w, F32).astype(F64)
    d = x - w[np.asarray(ids, np.int64)]
    return float(np.sqrt(np.where(np.isnan(d), 0.0, d * d).sum(axis=1)).mean())


def check_qe(qe, x, w, ids, what=""):
    """query_ref.check_qe's form on the masked definition: the kernel sums fma'd squares of rounded differences and takes a
    float32 sqrt per row, relative error <= gamma(D + 10) per row.  Returns err / bound."""
    ref = qe_reference(x, w, ids)
    bound = Q.gamma(np.asarray(w).shape[1] + 10) * ref
    err = abs(float(qe) - ref)
    ratio = 0.0 if err == 0 else (err / bound if bound > 0 else np.inf)
    assert ratio <= 1.0, "%s: masked QE %r, float64 definition %r (bound %r)" % (what, qe, ref, bound)
    return ratio


# ------------------------------------------------------------------------------------------------------ the update
def reference_update_masked(data, bmu, X, Y, eta, sigma, *, wide, weights=None, neighbourhood="gaussian",
                            topology="rectangular", compact=False, std_coeff=0.5):
    """(num, den, mag_num, mag_den), each float64 (K, D): update_ref.reference_update (with `weights`:
    weights_ref.reference_update_weighted) on the augmented rows, split into its first and last D columns."""
    D = np.asarray(data).shape[1]
    aug = augmented(data)
    kw = dict(wide=wide, neighbourhood=neighbourhood, topology=topology, compact=compact, std_coeff=std_coeff)
    if topology == "toroidal":                              # (no reference has one: tests/torus_ref.py's direct form)
        from tests import torus_ref as T
        assert weights is None
        del kw["topology"]
        num, _, mag, _ = T.reference_update(aug, bmu, X, Y, eta, sigma, **kw)
    elif weights is None:
        num, _, mag, _ = U.reference_update(aug, bmu, X, Y, eta, sigma, **kw)
    else:
        num, _, mag, _ = R.reference_update_weighted(aug, bmu, weights, X, Y, eta, sigma, **kw)
    return num[:, :D], num[:, D:], mag[:, :D], mag[:, D:]


def brute_force_update(data, bmu, X, Y, eta, sigma, *, wide, weights=None, neighbourhood="gaussian", topology="rectangular",
                       compact=False, std_coeff=0.5):
    """(num (K, D), den (K, D)) as the definition reads: one neighbourhood row per data row, a Python loop, float64."""
    fn = O.NEIGHBOURHOODS[U.oracle_key(neighbourhood, topology)]
    eta_t = F64(eta) if wide else float(eta)
    xt, m = split(data)
    K = X * Y
    num, den = np.zeros((K, xt.shape[1])), np.zeros((K, xt.shape[1]))
    for n in range(len(xt)):
        wn = 1.0 if weights is None else float(weights[n])
        if wn == 0:
            continue
        b = np.array([bmu[n]], np.int64)
        g = np.asarray(fn(X, Y, std_coeff, compact, b // Y, b % Y, sigma, wide) * eta_t, F64).reshape(K)
        num += wn * g[:, None] * (m[n] * xt[n])[None, :]
        den += wn * g[:, None] * m[n][None, :]
    return num, den


def check_accumulators(num, den, ref, what=""):
    """update_ref.check_accumulators' form on a numerator and a denominator that are both (K, D); returns the worst ratio."""
    rnum, rden, mnum, mden = ref
    K, D = rnum.shape
    num, den = np.asarray(num).reshape(K, D), np.asarray(den).reshape(K, D)
    a, ia = U.accum_ratio(num, rnum, mnum)
    b, ib = U.accum_ratio(den, rden, mden)
    assert a <= 1.0, "%s num: err/bound %.3g at unit %d feature %d: got %r, ref %r, mag %r" % (
        what, a, ia // D, ia % D, float(num.flat[ia]), rnum.flat[ia], mnum.flat[ia])
    assert b <= 1.0, "%s den: err/bound %.3g at unit %d feature %d: got %r, ref %r, mag %r" % (
        what, b, ib // D, ib % D, float(den.flat[ib]), rden.flat[ib], mden.flat[ib])
    return max(a, b)


def merge(w_old, num, den):
    """float32 W' = num / den where den != 0, else the old value, elementwise."""
    w_old, num, den = (np.asarray(a, F32) for a in (w_old, num, den))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den != 0, num / den, w_old).astype(F32)


def merge_bound(ref, mexican=False):
    """(ok, W_ref, bound): update_ref.check_merge's bound elementwise -- where |den_ref| >= 1e-30 (mexican hat: also above
    1e-3 of the largest), |W' - W_ref| <= (e_num + |W_ref| e_den) / |den_ref| with e = update_ref.accum_bound(mag)."""
    rnum, rden, mnum, mden = ref
    ad = np.abs(rden)
    ok = ad >= 1e-30
    if mexican and ad.size:
        ok &= ad > 1e-3 * ad.max()
    with np.errstate(divide="ignore", invalid="ignore"):
        wr = np.where(ok, rnum / np.where(ok, rden, 1.0), 0.0)
        bound = np.where(ok, (U.accum_bound(mnum) + np.abs(wr) * U.accum_bound(mden)) / np.where(ok, ad, 1.0), np.inf)
    return ok, wr, bound


def check_merge(w_old, w_new, num, den, ref, mexican=False, what=""):
    """The merge after an accumulate: bit for bit merge(w_old, num, den) of the engine's own accumulators, and within
    merge_bound of the reference.  Returns the worst ratio."""
    K, D = ref[0].shape
    w_new = np.asarray(w_new, F32).reshape(K, D)
    want = merge(np.asarray(w_old).reshape(K, D), np.asarray(num).reshape(K, D), np.asarray(den).reshape(K, D))
    bad = np.flatnonzero(want.view(np.uint32) != w_new.view(np.uint32))
    assert len(bad) == 0, "%s merge: %d elements differ from float32(num/den) / the old value, first (%d, %d)" % (
        what, len(bad), bad[0] // D, bad[0] % D)
    ok, wr, bound = merge_bound(ref, mexican)
    if not ok.any():
        return 0.0
    err = np.abs(w_new.astype(F64) - wr)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(ok & (err > 0), err / bound, 0.0)
    i = int(np.argmax(r))
    assert r.flat[i] <= 1.0, "%s merge vs reference: err/bound %.3g at unit %d feature %d" % (what, r.flat[i], i // D, i % D)
    return float(r.flat[i])


# ------------------------------------------------------------------------------------------------------ the large grid
# The forced-update grid of tests/test_gpu_missing_large.py, kept here so that the GPU module and the coverage test of
# tests/test_missing_cpu.py read one table.  A masked handle's rows are UD = 2 D wide, so these are the smallest shapes at
# which every width the host's dispatch decides on (update_ref.update_paths(..., masked=True)) crosses its boundary.
# family (update_ref.FAMILIES or "torus_gaussian"), X, Y, D, N, BMU pattern, missing pattern, sigma, wide
LARGE_FORCED = [
    ("gaussian", 129, 5, 64, 1000, "spread", "random30", 2.0, False),     # two row blocks, one-row last block, UD = 128 per column
    ("gaussian", 257, 3, 65, 2100, "skewed", "payload", 1.2, True),       # three blocks, UD = 130 narrow2, counting sort, odd D
    ("gaussian", 5, 130, 128, 1000, "spread", "halves", 2.0, False),      # stage 1 over two blocks, UD = 256: two column tiles
    ("gaussian", 1, 300, 3, 2047, "spread", "row", 1.5, True),            # degenerate axis, three stage-1 blocks, UD = 6: narrow only
    ("mexican_hat_compact", 66, 66, 3, 5000, "spread", "random30", 3.0, True),   # swapped order, 128-row tile without ranges, D1p = 8
    # (the swapped order's column stage is D1p wide: at D1p = 8 it is a narrow tile alone, and only D1p = 132 gives it a
    #  128-row MFMA tile AND a narrow tile of 4 columns -- no other row reaches s2.tile128 or s2.narrow2)
    ("mexican_hat_compact", 66, 66, 64, 5000, "spread", "random30", 3.0, False),
    ("mexican_hat", 129, 5, 6, 300, "spread", "random30", 2.0, True),     # two terms, two blocks
    ("hex_mexican_hat_compact", 40, 34, 6, 2047, "spread", "random30", 2.0, False),   # sixteen term copies
    ("hex_gaussian", 129, 34, 33, 5000, "spread", "feature", 1.5, False),  # three classes, an unobserved feature stays bit for bit
    ("bubble", 129, 40, 1, 5200, "spread", "random30", 3.0, False),       # UD = 2, whole tiles of a table zero
    ("triangle_compact", 40, 129, 4, 5200, "spread", "random30", 3.5, False),    # UD = 8
    ("torus_gaussian", 129, 40, 67, 5200, "spread", "random30", 1.2, False),     # wrap kernel, band across the seam, UD = 134 narrow4
    ("torus_gaussian", 40, 129, 64, 5200, "spread", "payload", 4.0, True),       # wrap kernel, per-column stage 2
    ("gaussian", 5, 7, 600, 300, "skewed", "random30", 2.0, True),        # 4 waves
    ("gaussian", 5, 7, 1100, 300, "spread", "random30", 2.0, False),      # 2 waves
    ("gaussian", 5, 7, 2046, 300, "skewed", "random30", 2.0, True),       # 1 wave (direct slots), even D
    ("gaussian", 5, 7, 2047, 129, "spread", "halves", 2.0, False),        # 1 wave, odd D
    ("gaussian", 8, 8, 2, 300000, "skewed", "random30", 1.5, True),       # three run-sum levels
    ("gaussian", 129, 64, 4, 8300, "spread", "random30", 2.0, False),     # K = 8256 > CS_MAX_K: radix sort
]
LARGE_ETA, LARGE_STD = 0.5, 0.5
MIN_MERGE_SHARE = 0.95      # of the (unit, feature) elements: what merge_bound must cover on every row of the grid
_large_cache = {}


def family_of(fam):
    """(neighbourhood, topology, compact) of a family of the grids."""
    return ("gaussian", "toroidal", False) if fam == "torus_gaussian" else U.FAMILIES[fam]


def large_id(row):
    return "%s-%dx%dx%d-n%d-%s-%s" % row[:7]


def large_forced_case(row, missing=None, weighted=False):
    """{data, bmu, weights, w0, ref, kw, mexican} of a LARGE_FORCED row, computed once and never changed.  `missing`
    replaces the row's missing pattern; `weighted` adds weights_ref.make_weights and sets one row of weight 0 to inf
    (a row of weight 0 is not read)."""
    key = (row, missing, weighted)
    if key not in _large_cache:
        fam, X, Y, D, N, bpat, mpat, sigma, wide = row
        neigh, topo, compact = family_of(fam)
        rs = np.random.RandomState(X * Y + D + N)
        bmu = U.make_bmu(bpat, X, Y, N, rs)
        data = punch(U.make_data(N, D, 1.0, 70 + D), missing or mpat, 9, bmu)
        w = None
        if weighted:
            w = R.make_weights(N, 5 + D)
            data[np.flatnonzero(w == 0)[0]] = np.inf
        ref = reference_update_masked(data, bmu, X, Y, LARGE_ETA, sigma, wide=wide, weights=w, neighbourhood=neigh,
                                      topology=topo, compact=compact, std_coeff=LARGE_STD)
        for a in (data, bmu, *ref):
            a.setflags(write=False)
        _large_cache[key] = dict(
            data=data, bmu=bmu, weights=w, ref=ref, mexican=neigh == "mexican_hat",
            w0=O.default_codebook(X, Y, D, 3).astype(F32).reshape(X * Y, D),
            kw=dict(neighborhood=neigh, topology=topo, compact_support=compact, std_coeff=LARGE_STD))
    return _large_cache[key]


def merge_share(ref, mexican=False):
    """The share of the (unit, feature) elements merge_bound checks against the reference (from the reference alone)."""
    ok, _, _ = merge_bound(ref, mexican)
    return float(ok.mean()) if ok.size else 1.0


def update_from_unit_rows(rows, X, Y, eta, sigma, *, wide, neighbourhood="gaussian", topology="rectangular", compact=False,
                          std_coeff=0.5):
    """(num, den), each float64 (K, D): the masked update from the per-unit rows [S (D) | C (D)] (K, 2 D) that level 0 hands
    to the transform, H^T rows with the neighbourhood rows update_ref.reference_update builds (rectangular and hexagonal
    topologies).  With the rows of the true segment sums this is reference_update_masked; the named mutants of
    tests/test_missing_cpu.py feed it rows a wrong kernel would have left."""
    rows = np.asarray(rows, F64)
    K, D = X * Y, rows.shape[1] // 2
    fn = O.NEIGHBOURHOODS[U.oracle_key(neighbourhood, topology)]
    eta_t = F64(eta) if wide else float(eta)

    def h_of(u):
        return fn(X, Y, std_coeff, compact, u // Y, u % Y, sigma, wide) * eta_t

    num, _, _, _ = U.accumulate(rows, np.abs(rows), np.zeros(K), np.arange(K), K, h_of)
    return num[:, :D], num[:, D:]


def unit_rows(data, bmu, K):
    """The dense per-unit rows [S | C | count] (K, 2 D + 1), float64, of the augmented rows: what level 0 leaves in SC."""
    units, S, _, c = U.segment_sums(augmented(data), bmu)
    out = np.zeros((K, S.shape[1] + 1))
    out[units, :-1] = S
    out[units, -1] = c
    return out


# ------------------------------------------------------------------------------------------------------ data
def punch(x, pattern, seed, bmu=None):
    """A copy of float32 rows `x` with holes of a pattern:
      none       nothing missing
      random30   30 % of the values at random
      feature    feature D // 2 missing in every row (D >= 2; with D == 1 the pattern is `row`)
      row        row N // 2 entirely missing (plus 10 % at random elsewhere)
      halves     the rows of one unit (`bmu` given: its most frequent id; else every row) observe disjoint halves of the
                 features in turn: even rows the first half, odd rows the second (D >= 2)
      payload    30 % at random, written as NaNs of both signs and with a nonzero payload"""
    x = np.array(x, dtype=F32, copy=True)
    N, D = x.shape
    rs = np.random.RandomState(seed)
    if pattern == "none":
        return x
    if pattern == "random30":
        x[rs.rand(N, D) < 0.3] = np.nan
    elif pattern == "feature" and D >= 2:
        x[:, D // 2] = np.nan
    elif pattern in ("row", "feature"):
        x[rs.rand(N, D) < 0.1] = np.nan
        x[N // 2] = np.nan
    elif pattern == "halves":
        rows = np.arange(N) if bmu is None else np.flatnonzero(np.asarray(bmu) == np.bincount(bmu).argmax())
        if D >= 2:
            x[rows[0::2], D // 2:] = np.nan
            x[rows[1::2], :D // 2] = np.nan
    elif pattern == "payload":
        hole = rs.rand(N, D) < 0.3
        pats = np.array([0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFF800001, 0x7FA00000], np.uint32)
        v = x.view(np.uint32)
        v[hole] = pats[rs.randint(0, len(pats), int(hole.sum()))]
        assert np.isnan(x[hole]).all()
    else:
        raise ValueError(pattern)
    return x


def exact_case(N, K, D, seed, holes=True):
    """Rows and units whose every masked score is exact in float32: small integers / 8; the last units repeat the first
    ones (ties: the lowest id must win), some units are zero, some rows are all-equal, and -- with `holes` -- 30 % of the
    values are missing and one row entirely.  Every product is a multiple of 1 / 64 below 2^12, every sum stays far below
    2^24 / 64."""
    rs = np.random.RandomState(seed)
    x = (rs.randint(-8, 9, (N, D)) / 8.0).astype(F32)
    w = (rs.randint(-8, 9, (K, D)) / 8.0).astype(F32)
    dup = max(1, K // 4)
    w[K - dup:] = w[:dup]
    w[rs.randint(0, K, max(1, K // 8))] = 0
    if N > 2:
        x[1] = x[1, 0]
        x[N - 1] = 0.5
    if holes:
        x[rs.rand(N, D) < 0.3] = np.nan
        x[N // 2] = np.nan
    return x, w
