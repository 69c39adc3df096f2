"""The float64 model of the row moments (som_row_moments*, include/somhip.h; csrc/moments.hpp) and the bound the kernels must stay
inside.  No GPU, no library call except the pure host arithmetic of som_debug_moments_plan, which exports the kernels' constants.

The model: float32 inputs widened to float64, d = x - p NOT rounded, direct sums; rows of weight 0 are left out.

The bound is derived from the kernels' chain, per entry, as c * sum_n w_n |d_na| |d_nb| (s1: c1 * sum_n w_n |d_na|):
  u = 2^-24  the float32 subtraction d^ = fl(x - p) = d (1 + e1) -- once per operand -- and the float32 product fl(w d^_a) of the A
             operand: three factors (1 + e), |e| <= u
  gamma_R    the float32 chain of one chunk of R rows from zero: every term carries at most R roundings, gamma_R = R u / (1 - R u)
             (Higham, Accuracy and Stability of Numerical Algorithms, 3.1); R = SOM_MOMENTS_CHUNK_ROWS, read from the library.
             This ASSUMES that v_mfma_f32_32x32x2_f32 is a FUSED multiply-add per k step -- one rounding per product-and-add, the
             product itself unrounded -- so that the first term is rounded R times and not R + 1.  That is what the float32 parity
             mode rests on and pins on the device: its distances are NumPy's / OpenBLAS' fma chain bit for bit (csrc/bmu_f32.hpp,
             tests/test_gpu_parity.py); emulate() below states the same chain.  A separately rounded product would make it
             gamma_{R + 1}
  2^-53      the double additions: a chunk result passes through at most m of them -- the chunks of its split, the splits, the
             three joins of the waves -- so gamma64_m with m = chunks + 2 056 (no grid has more than 2 048 workgroups) bounds any order the kernels may use
  and the reference's own error: a float64 matrix product of n terms, gamma64_{n + 2} of the same absolute sum.
s1 and wsum are exact double products added in double: u for the subtraction (s1 only) and gamma64 of the number of additions."""
import ctypes as C

import numpy as np

F32, F64 = np.float32, np.float64
U32 = 2.0 ** -24
U64 = 2.0 ** -53


def plan(n_rows, D):
    """{R, tiles, splits, round (chunks in one round of the row split), sum_grid, max_features} of the kernels' launch geometry."""
    from xpysom_dask_amd import _lib
    out = (C.c_int64 * 6)()
    assert _lib.load().som_debug_moments_plan(int(n_rows), int(D), out) == 0
    return dict(zip(("R", "tiles", "splits", "round", "sum_grid", "max_features"), (int(v) for v in out)))


def chunk_rows():
    return plan(1, 1)["R"]


def gamma(k, u):
    assert k * u < 1
    return k * u / (1 - k * u)


def _inputs(x, w, p):
    x = np.asarray(x, dtype=F32)
    n, D = x.shape
    w = np.ones(n, F32) if w is None else np.asarray(w, dtype=F32)
    p = np.zeros(D, F32) if p is None else np.asarray(p, dtype=F32)
    live = w != 0                                         # a row of weight 0 is left out, whatever it holds
    return x[live].astype(F64) - p.astype(F64), w[live].astype(F64), n


def model(x, w=None, p=None):
    """(wsum, s1, gram) in float64 and the absolute sums (sum w |d_a|, sum w |d_a| |d_b|) the bounds scale with."""
    d, w, _ = _inputs(x, w, p)
    wd = w[:, None] * d
    return (w.sum(), wd.sum(axis=0), wd.T @ d), (np.abs(wd).sum(axis=0), np.abs(wd).T @ np.abs(d))


def bounds(x, w=None, p=None, R=None):
    """(bound on wsum, on s1 (D,), on gram (D, D)): what |kernel - model| may be, reference error included."""
    R = R or chunk_rows()
    d, w, n = _inputs(x, w, p)
    awd = np.abs(w[:, None] * d)
    a1, a2 = awd.sum(axis=0), awd.T @ np.abs(d)
    m = (n + R - 1) // R + 2048 + 8                       # double additions a chunk result may pass through
    c_gram = (1 + U32) ** 3 * (1 + gamma(R, U32)) * (1 + gamma(m, U64)) - 1 + gamma(n + 2, U64)
    c_s1 = (1 + U32) * (1 + gamma(n + 2048 + 8, U64)) - 1 + gamma(n + 2, U64)
    c_w = 2 * gamma(n + 2048 + 8, U64)
    return c_w * w.sum(), c_s1 * a1, c_gram * a2


def check_moments(got, x, w=None, p=None, what=""):
    """got = (wsum, s1, gram or None) of a kernel (or of anything that claims to compute them) against the model, entry by entry."""
    (wsum, s1, gram), _ = model(x, w, p)
    bw, b1, b2 = bounds(x, w, p)
    g_wsum, g_s1, g_gram = got
    assert abs(g_wsum - wsum) <= bw, "%s wsum: %r against %r (bound %g)" % (what, g_wsum, wsum, bw)
    err = np.abs(np.asarray(g_s1, F64) - s1)
    bad = np.argwhere(~(err <= b1))
    assert len(bad) == 0, "%s s1: %d entries outside the bound, first %r: %r against %r (bound %g)" % (
        what, len(bad), bad[0], g_s1[tuple(bad[0])], s1[tuple(bad[0])], b1[tuple(bad[0])])
    if g_gram is not None:
        err = np.abs(np.asarray(g_gram, F64) - gram)
        bad = np.argwhere(~(err <= b2))
        assert len(bad) == 0, "%s gram: %d entries outside the bound, first %r: %r against %r (error %g, bound %g)" % (
            what, len(bad), bad[0], g_gram[tuple(bad[0])], gram[tuple(bad[0])], err[tuple(bad[0])], b2[tuple(bad[0])])
    return float(np.max(err / np.maximum(b2, 1e-300))) if g_gram is not None else 0.0


def central(wsum, s1, gram):
    """The shifted-data formula: sum w (x - mean)(x - mean)^T = gram - s1 s1^T / wsum for moments about ANY pivot."""
    return gram - np.outer(s1, s1) / wsum


def central_bound(x, w=None, p=None):
    """What |central(kernel moments) - central(model moments)| may be, from the bounds above: the Gram matrix's own, and s1's
    carried through the product (|s1_a| b_b + |s1_b| b_a + b_a b_b) / wsum (wsum's error is orders below both and is folded into a
    factor 1 + 4 u64 n)."""
    (wsum, s1, _), _ = model(x, w, p)
    _, b1, b2 = bounds(x, w, p)
    a = np.abs(s1)
    return (b2 + (np.outer(a, b1) + np.outer(b1, a) + np.outer(b1, b1)) / wsum) * (1 + 1e-9)


def emulate(x, w=None, p=None, R=None):
    """The Gram kernel's order in NumPy: float32 d = x - p, float32 w * d, a float32 fma chain over each chunk of R rows from zero
    (the fma as a float64 product-and-add rounded once to float32: the product of two float32 is exact in float64), the chunks'
    results widened and added in float64.  s1 and wsum as exact products added in float64."""
    R = R or chunk_rows()
    x = np.asarray(x, dtype=F32)
    n, D = x.shape
    w = np.ones(n, F32) if w is None else np.asarray(w, dtype=F32)
    p = np.zeros(D, F32) if p is None else np.asarray(p, dtype=F32)
    live = w != 0
    d = np.where(live[:, None], x - p[None, :], F32(0)).astype(F32)
    a = (w[:, None] * d).astype(F32)
    gram = np.zeros((D, D), F64)
    for r0 in range(0, n, R):
        acc = np.zeros((D, D), F32)
        for r in range(r0, min(r0 + R, n)):
            acc = (acc.astype(F64) + np.outer(a[r].astype(F64), d[r].astype(F64))).astype(F32)
        gram += acc.astype(F64)
    return float(w.astype(F64).sum()), (w.astype(F64)[:, None] * d.astype(F64)).sum(axis=0), gram


# ---- data and float64 moments for the initialisers' tests ----
def spectrum_rows(n, D, seed, lam=(16.0, 9.0, 4.0), mean=3.0):
    """Rows whose covariance has the leading eigenvalues `lam` on a rotated basis and the rest <= 1."""
    rs = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rs.normal(size=(D, D)))
    scale = np.concatenate([np.sqrt(lam[:D]), rs.uniform(0.3, 1.0, max(D - len(lam), 0))])[:D]
    return (mean + (rs.normal(size=(n, D)) * scale) @ q.T).astype(F32)


def moments64(x, w=None):
    x = np.asarray(x, F64)
    w = np.ones(len(x)) if w is None else np.asarray(w, F64)
    mean = (w[:, None] * x).sum(axis=0) / w.sum()
    c = x - mean
    return w.sum(), mean, (w[:, None] * c).T @ c / w.sum()


def linear_tolerance(x, w, pivot, cast=True):
    """How far (Euclidean norm, per unit) a linear codebook built from the device moments of (x, w) about `pivot` may lie from
    _linear_codebook of the float64 moments -- derived, not measured.  With |c| <= 1 on both axes a unit moves by at most
        |d mean| + sum_{k = 1, 2} ( |d sqrt(l_k)| + sqrt(l_k) |d v_k| )
      |d mean|       s1's bound over wsum (the mean is pivot + s1 / wsum, the pivot exact)
      |dC|_2         <= the Frobenius norm of central_bound / wsum (the moments bound, not the result), plus eigh's own
                     backward error, D * 2^-52 |C|
      |d l_k|        <= |dC|_2 (Weyl), so |d sqrt(l_k)| <= |dC|_2 / sqrt(l_k - |dC|_2)
      |d v_k|        <= 2 sqrt(2) |dC|_2 / gap_k (Davis-Kahan), gap_k the distance of l_k to the nearest other eigenvalue
      cast           the codebook is stored in float32: u |W| per unit."""
    wsum, mean, cov = moments64(x, w)
    _, b1, _ = bounds(x, w, pivot)
    D = cov.shape[0]
    dC = np.linalg.norm(central_bound(x, w, pivot)) / wsum + D * 2.0 ** -52 * np.linalg.norm(cov)
    lam = np.linalg.eigvalsh(cov)
    tol = np.linalg.norm(b1) / wsum
    for k in (D - 1, D - 2):
        gap = np.min(np.abs(np.delete(lam, k) - lam[k]))
        assert gap > 100 * dC and lam[k] > 100 * dC, "the test's data must have a separated spectrum"
        tol += dC / np.sqrt(lam[k] - dC) + np.sqrt(lam[k]) * 2 * np.sqrt(2) * dC / gap
    if cast:
        tol += U32 * (np.linalg.norm(mean) + np.sqrt(lam[-1]) + np.sqrt(lam[-2]))
    return tol
