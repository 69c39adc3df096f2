"""A float64 reference of the 16-bit masked BMU search (`missing='nan', missing_search='bf16' | 'f16'`; csrc/bmu_masked_half.hpp)
ON THE IMAGES THE KERNEL CONSUMES, and a derived bound on what its float32 accumulation may add.

Shared by tests/test_masked_half_cpu.py and tests/test_gpu_masked_half.py (not a conftest).  Rounding, KAPPA, gamma and the checks
are tests/half_ref.py's; the split of a row into (x~, m) and the hole patterns are tests/missing_ref.py's.

    s[n,k] = sum_d m_nd (hi_kd + lo_kd)  -  sum_d x~_nd w~_kd
    w~ = round(w), x~ = round(x) with 0 at the holes, h = float32(w~ w~) / 2 (exact), hi = bf16(h), lo = bf16(h - hi)

`images` builds w~, hi, lo as prep_masked_half_kernel defines them; `scores` evaluates s in float64 and returns the bound E:

  MFMA accumulation   KAPPA n_mfma 2^-23 A[n,k]: n_mfma = 3 ceil(D / 32) MFMAs are chained per unit into one accumulator that starts
                      at zero, half_ref's KAPPA ulps of the largest partial magnitude each; every partial is at most
                      A = sum m (|hi| + |lo|) + sum |x~||w~|.  There is no offset, no epilogue (c = 0: the accumulator itself is
                      compared) and no key truncation (plain float compares).
  operand uncertainty IEEE-half elements of x~ and w~ that are subnormal after rounding may be read as they are or as zero
                      (half_ref's allowance): sum |x~_d||w~_d| over the elements where either side is subnormal.  hi and lo are
                      bf16 in both modes: no half-typed image.

`operand_bound`: against the UNROUNDED float64 masked distance d = sum m (x - w)^2 = sum m x^2 + tau, tau = sum m w^2 - 2 sum x w
(x with 0 at the holes): |s - tau / 2| <= e := sum m |dq| / 2 + sum |dx||w~| + sum |x||dw| with the rounding errors measured,
dx = x~ - x, dw = w~ - w, dq = 2 (hi + lo) - w^2; a pick p against any unit b has s_p - E_p <= s_b + E_b, hence
d_p <= d_b + 2 (e_p + e_b) + 2 (E_p + E_b).
"""
import numpy as np

from tests import missing_ref as M
from tests.half_ref import F32, F64, HALF_MIN_NORMAL, KAPPA, check_picks, check_ties, round_operand

# csrc/bmu_masked_half.hpp: rows per workgroup, units per stage, features per step, steps of the register-resident kernel
WG_SAMPLES, STAGE_UNITS, STEP, RES_KS = 256, 64, 32, 4
KINDS = ("bf16", "f16")


def images(w, kind):
    """(w~, hi, lo) as float64 values: the rounded codebook and the two bf16 images of w~ w~ / 2."""
    wr = round_operand(w, kind)[0]
    w32 = wr.astype(F32)
    with np.errstate(over="ignore", under="ignore"):
        h = F32(0.5) * (w32 * w32)
    hi = round_operand(h, "bf16")[0]
    lo = round_operand((h.astype(F64) - hi).astype(F32), "bf16")[0]
    return wr, hi, lo


def scores(x, w, kind):
    """(s, E) of the module docstring for float32 rows `x` (NaN: not observed) against the codebook `w`."""
    xt, m = M.split(x)
    xr = round_operand(xt, kind)[0]
    wr, hi, lo = images(w, kind)
    n_mfma = 3 * -(-wr.shape[1] // STEP)
    ax, aw = np.abs(xr), np.abs(wr)
    s = m @ (hi + lo).T - xr @ wr.T
    A = m @ (np.abs(hi) + np.abs(lo)).T + ax @ aw.T
    E = KAPPA * n_mfma * 2.0 ** -23 * A
    if kind == "f16":
        xs, ws = (ax > 0) & (ax < HALF_MIN_NORMAL), (aw > 0) & (aw < HALF_MIN_NORMAL)
        if xs.any() or ws.any():
            E = E + (ax * xs) @ aw.T + (ax * ~xs) @ (aw * ws).T
    return s, E


def operand_bound(x, w, kind):
    """e[n,k] of the module docstring."""
    xt, m = M.split(x)
    w64 = np.asarray(w, F32).astype(F64)
    xr = round_operand(xt, kind)[0]
    wr, hi, lo = images(w, kind)
    dq = 2 * (hi + lo) - w64 * w64
    return 0.5 * m @ np.abs(dq).T + np.abs(xr - xt) @ np.abs(wr).T + np.abs(xt) @ np.abs(wr - w64).T


def check_operand_bound(ids, x, w, kind, E, what=""):
    """d_pick <= d_best + 2 (e_pick + e_best) + 2 (E_pick + E_best) on the unrounded float64 masked distances (formed as
    sum m x^2 - 2 x.w + sum m w^2; float64's own cancellation, (D + 4) 2^-52 of the terms, is added).  Returns excess / allowance."""
    ids = np.asarray(ids, np.int64)
    xt, m = M.split(x)
    w64 = np.asarray(w, F32).astype(F64)
    mag = (xt * xt).sum(1)[:, None] + m @ (w64 * w64).T
    d = mag - 2 * (xt @ w64.T)
    e = operand_bound(x, w, kind)
    r, b = np.arange(len(ids)), np.argmin(d, axis=1)
    allow = 2 * (e[r, ids] + e[r, b] + E[r, ids] + E[r, b]) + (w64.shape[1] + 4) * 2.0 ** -52 * (mag[r, ids] + mag[r, b])
    over = d[r, ids] - d[r, b]
    with np.errstate(divide="ignore", invalid="ignore"):
        rat = np.where(over <= 0, 0.0, over / allow)
    i = int(np.argmax(rat)) if len(rat) else 0
    assert not len(rat) or rat[i] <= 1.0, "%s: row %d picks unit %d at %r, unit %d is at %r: excess / allowance %.3g" % (
        what, i, ids[i], d[i, ids[i]], b[i], d[i, b[i]], rat[i])
    return float(rat[i]) if len(rat) else 0.0


def check(ids, x, w, kind, what=""):
    """Admissible picks, all-missing rows on unit 0, and the operand bound; returns the two worst ratios."""
    ids = np.asarray(ids)
    assert ids.shape == (len(x),) and ((ids >= 0) & (ids < len(w))).all(), "%s: a pick outside the map" % what
    s, E = scores(x, w, kind)
    assert np.isfinite(E).all()
    pick = check_picks(ids, s, E, what)
    assert (ids[np.isnan(x).all(axis=1)] == 0).all(), "%s: a row with nothing observed must take unit 0" % what
    return pick, check_operand_bound(ids, x, w, kind, E, what)


# ------------------------------------------------------------------------------------------------ the GPU module's grid
# (N, X, Y, D): one row / unit / feature; one past a workgroup, two stages and a step; tails below them; the register-resident
# kernel's widest instance over 65 stages with a one-unit tail; the streamed kernel over five chunks of two stages, and over 19
# chunks (past many turns of its two-slot ring) with an odd row count
SHAPES = [(1, 1, 1, 1), (257, 3, 43, 33), (300, 15, 17, 31), (513, 17, 241, 128), (129, 5, 13, 160), (130, 6, 6, 600)]
# (data kind of half_ref.make_half_data, hole pattern of missing_ref.PATTERNS); `tiny` (subnormal halves) runs under f16 only
DATA = [("blobs", "none"), ("blobs", "random30"), ("offset30", "row"), ("blobs", "feature"), ("blobs", "halves"),
        ("blobs", "payload"), ("tiny", "random30")]
_cache = {}


def case(shape, data, pattern):
    """(x, w) of one grid point, computed once and never changed."""
    key = (shape, data, pattern)
    if key not in _cache:
        from tests.half_ref import make_half_data
        N, X, Y, D = shape
        x, w = make_half_data(data, N, X * Y, D, 5 + D, dup=min(3, X * Y - 1))
        x = M.punch(x, pattern, 7)
        for a in (x, w):
            a.setflags(write=False)
        _cache[key] = (x, w)
    return _cache[key]


__all__ = ["DATA", "KINDS", "RES_KS", "SHAPES", "STAGE_UNITS", "STEP", "WG_SAMPLES", "case", "check", "check_operand_bound",
           "check_picks", "check_ties", "images", "operand_bound", "scores"]
