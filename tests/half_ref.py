"""A float64 reference of the 16-bit BMU search (precision 'bf16' / 'f16') ON THE ROUNDED OPERANDS, a rigorous bound on what
the kernels' float32 arithmetic may add to it, the checks built on the two, and a label mirror of the host's dispatch.

Shared by tests/test_half_ref_cpu.py, tests/test_gpu_half_ref.py and tests/fuzz/fuzz_half.py (not a conftest).

csrc/bmu_bf16.hpp: d'(n,k) = B + |w~_k|^2/2 - x~_n . w~_k is "a true distance in the rounded space".  The rounding of the
operands is deterministic (cvt<> of som_common.hpp: round-to-nearest-even to bf16, or to IEEE half after a clip to
+-65504), so the reference rounds them itself (`round_operand`) and only the kernel's float32 arithmetic stays behind the
bound.  B is common to a launch's units, so picks are compared on

    s[n,k] = |w~_k|^2/2 - x~_n . w~_k      (cosine: -x~_n . w~_k on the rounded UNIT-LENGTH operands, no norm term)

computed in float64.  `half_scores` returns s and a per-element bound E on the kernel's evaluation of s + B, in d' units.
With u = 2^-24, gamma(n) = n u / (1 - n u):

  MFMA accumulation   (KAPPA n_mfma + 1) 2^-23 Bm.  n_mfma = ceil(D / 32) 16x16x32 MFMAs are chained per unit; the project
                      charges KAPPA = 6 ulps of the largest magnitude among accumulator, result and sum of |products| per
                      MFMA (measured <= 2.4 by test_gpu_exact's som_debug_mfma16 test), the "+ 1" is the
                      rounding of the initial accumulator fma(0.5, |w~|^2, B).  Every such magnitude is below
                      Bm = 2.01 B + |w~|max^2 / 2 with B = |x~|max |w~|max (1 + 2^-9): the kernel's own B carries 1 + 2^-10
                      and float32 norms (relative error gamma(D) / 2 each, far inside the spare 2^-10).  The maxima are
                      over the rows of the LAUNCH (resident set, query batch, streamed chunk): pass exactly those rows.
  norm term           |w~_k|^2 is a float32 fma chain of D exact squares in one of several orders (prep_wnorm_kernel: in
                      order; rownorm_bf16_kernel: 64 lanes and a butterfly; merge_prep_*: quads, then waves): any order
                      is within gamma(D) of the sum, the halving fma adds one rounding (charged above), so
                      gamma(D + 2) |w~_k|^2 / 2 covers every preparation kernel.
  key truncation      the argmin key is (bits & ~IDX_MASK) | index with IDX_MASK = 15 (bmu_bf16_k16.hpp:239,
                      bmu_bf16_tiled.hpp:131) or 7 (bmu_bf16_wide.hpp:197): the positive value is floored by fewer than
                      16 (8) ulps, an ulp being at most 2^-23 Bm.
  operand uncertainty IEEE-half elements that are subnormal after rounding (|v| < 2^-14): the MFMA may read them as they
                      are or as zero (half_operand_error of bmu_bf16.hpp makes the same allowance), so sum_d |x~_d||w~_d|
                      over the elements where either side is subnormal.  Cosine: see `round_operand`; an ambiguous
                      element may have gone to the neighbouring 16-bit value, so (hi - lo)_d times the other operand's
                      element, summed.

The checks:
  admissible pick   query_ref.check_picks on (s, E): s_pick <= min_j (s_j + E_j) + E_pick, and every pick is < K (a
                    padding unit carries BF_PAD_NORM = 1e30 and can never be admissible).
  exact ties        `pin_int_norms` makes small-integer data on which B itself is an integer: every operand is exact in
                    bf16 and half, every d' a half-integer below 2^23 and therefore exact whatever the MFMA's internal
                    order, distinct values are >= 0.5 apart (a 16-ulp floor is < 2^-4 there) -- the pick IS the
                    lowest-index argmin (query_ref.check_ties).
  operand bound     `operand_bound`: the statement a user reads ("near-best within the operand rounding"), made rigorous
                    against the UNROUNDED float64 distances, with the rounding errors measured rather than modelled:
                    tau_k = |w_k|^2 - 2 x.w_k,  |s_k - tau_k/2| <= e_k := |dx||w~_k| + |x||dw_k| + |dw_k|(|w_k| + |w~_k|)/2
                    (dx = x~ - x, dw = w~ - w; Cauchy-Schwarz on x~.w~ - x.w = dx.w~ + x.dw and on
                    |w~|^2 - |w|^2 = dw.(w~ + w)), and the kernel's pick p against any unit b has s_p - E_p <= s_b + E_b, so
                    |x - w_p|^2 <= |x - w_b|^2 + 2 (e_p + e_b) + 2 (E_p + E_b).  Valid on un-centred rows too.

`half_paths` mirrors launch_bmu_half and the launchers below it as labels, so that tests/test_half_ref_cpu.py can show
that the GPU module's grid reaches every one.
"""
import numpy as np

from tests.query_ref import F32, F64, U, _cdiv, check_picks, check_ties, gamma, make_rows, make_units, pick_ratio

KAPPA = 6                                   # exact_bound()'s charge per MFMA, DESIGN 3.0 (E2)
BF_PAD_NORM = 1.0e30                        # bmu_bf16.hpp:18
HALF_MAX = 65504.0
HALF_MIN_NORMAL = 2.0 ** -14
K16_STAGE_UNITS, K16_WG_SAMPLES = 64, 256   # bmu_bf16_k16.hpp:25,28
WD_STAGE_UNITS, WD_WG_SAMPLES = 32, 256     # bmu_bf16_wide.hpp:26,29
TL_BK = 32                                  # bmu_bf16_tiled.hpp:24
KEY_ULPS = {"k16": 16, "tiled": 16, "wide": 8}
KINDS = ("bf16", "f16")


# ------------------------------------------------------------------------------------------------ operand rounding
def _rne_bf16(a32):
    """float32 -> bfloat16 by round-to-nearest-even on the bit pattern, as float64 values (finite inputs)."""
    bits = np.ascontiguousarray(a32, F32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(F32).astype(F64)


def _round16(a32, kind):
    a32 = np.asarray(a32, F32)
    if kind == "bf16":
        return _rne_bf16(a32)
    if kind == "f16":
        with np.errstate(over="ignore"):
            return np.clip(a32, -HALF_MAX, HALF_MAX).astype(np.float16).astype(F64)
    raise ValueError(kind)


def unit_scale_error(D):
    """Relative error of the kernels' float32 unit-length scaling x_d * (1 / sqrt(q)), q a float32 sum of D squares.  The
    error of a sum of positive terms is at most gamma(h), h the longest chain of roundings one addend passes through.  The
    preparation kernels sum in three orders, none of which the reference copies: 64 lanes striding the row and a six-level
    butterfly (prep_x_bf16_kernel: h <= D / 64 + 7), NumPy's pairwise order (row_sq_f32_kernel: eight accumulators over
    blocks of at most 128, h <= 31 up to 1024 features), and a lane's fma chain over at most 7 chunks of 8 features, two
    shuffles and two additions (merge_prep_wide_kernel: h <= 60).  So h <= min(D + 1, 64) for every one of them, half of
    it survives the square root, and one rounding each comes from the root, the quotient and the product (hipcc's default
    float32 divide and sqrt are correctly rounded) and, twice, from this module's own float32 bracket values."""
    assert D <= 1024
    return (0.5 * min(D + 1, 64) + 5.0) * U


def round_operand(a, kind, unit=False):
    """(r, amb): the float64 value of every float32 element of `a` after the kernel's conversion to `kind`, and how far the
    kernel's value may sit from it (0 where the conversion is determined).

    unit (cosine): the float32 row is first scaled by a float32 1 / sqrt(sum of squares) whose summation order differs
    between the preparation kernels; the reference scales in float64 and does not copy any of them.  The float32 product f
    lies within y (1 +- unit_scale_error(D)) of the float64-scaled y, rounding is monotone, so the kernel's 16-bit value
    lies between lo = round(y (1 - d)) and hi = round(y (1 + d)); where they differ the element is AMBIGUOUS: r is either
    of the two and amb = hi - lo (one 16-bit ulp).  A zero row stays zero."""
    a = np.asarray(a, F32)
    if not unit:
        return _round16(a, kind), np.zeros(a.shape)
    a64 = a.astype(F64)
    q = (a64 * a64).sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = np.where(q > 0, a64 / np.sqrt(q), 0.0)
    d = unit_scale_error(a.shape[1])
    lo = _round16((np.abs(y) * (1 - d)).astype(F32), kind)
    hi = _round16((np.abs(y) * (1 + d)).astype(F32), kind)
    r = np.copysign(_round16(np.abs(y).astype(F32), kind), y)
    return r, hi - lo


# ------------------------------------------------------------------------------------------------ scores and bound
def half_terms(x, w, kind, dist, key_ulps=16):
    """Everything half_scores is made of, as a dict: s, the four terms of E (mfma, norm, key, operand), B, Bm and the
    rounded operands xr, wr.  `x`: the rows of ONE launch."""
    unit = dist == "cosine"
    xr, xa = round_operand(x, kind, unit)
    wr, wa = round_operand(w, kind, unit)
    D = wr.shape[1]
    n_mfma = _cdiv(D, 32)
    c = xr @ wr.T
    wq = (wr * wr).sum(1)
    xmax = float(np.sqrt((xr * xr).sum(1).max())) if len(xr) else 0.0
    wmax = float(np.sqrt(wq.max()))
    B = xmax * wmax * (1 + 2.0 ** -9)
    Bm = 2.01 * B + 0.5 * wmax * wmax
    s = -c if unit else 0.5 * wq[None, :] - c
    t = dict(s=s, B=B, Bm=Bm, xr=xr, wr=wr)
    t["mfma"] = (KAPPA * n_mfma + 1) * 2.0 ** -23 * Bm
    t["key"] = key_ulps * 2.0 ** -23 * Bm
    t["norm"] = np.zeros(len(wr)) if unit else gamma(D + 2) * 0.5 * wq
    op = np.zeros(s.shape)
    ax, aw = np.abs(xr), np.abs(wr)
    if kind == "f16":
        xs = (ax > 0) & (ax < HALF_MIN_NORMAL)
        ws = (aw > 0) & (aw < HALF_MIN_NORMAL)
        if xs.any() or ws.any():
            op += (ax * xs) @ aw.T + (ax * ~xs) @ (aw * ws).T
    if unit:
        op += xa @ (aw + wa).T + ax @ wa.T
    t["operand"] = op
    return t


def half_scores(x, w, kind, dist, key_ulps=16):
    """(s, E) of the module docstring for the rows `x` of one launch against the codebook `w` (both float32)."""
    t = half_terms(x, w, kind, dist, key_ulps)
    return t["s"], t["mfma"] + t["key"] + t["norm"][None, :] + t["operand"]


def operand_bound(x, w, kind):
    """e[n,k] of the module docstring (euclidean): |s_k - tau_k / 2| <= e[n,k], from the measured rounding errors."""
    x64, w64 = np.asarray(x, F32).astype(F64), np.asarray(w, F32).astype(F64)
    xr, wr = round_operand(x, kind)[0], round_operand(w, kind)[0]
    ndx, nx = np.linalg.norm(xr - x64, axis=1), np.linalg.norm(x64, axis=1)
    ndw, nw, nwr = np.linalg.norm(wr - w64, axis=1), np.linalg.norm(w64, axis=1), np.linalg.norm(wr, axis=1)
    return ndx[:, None] * nwr[None, :] + nx[:, None] * ndw[None, :] + (0.5 * ndw * (nw + nwr))[None, :]


def sq_distances(x, w):
    """(d2, err): |x_n - w_k|^2 in float64 from the UNROUNDED float32 operands, as |x|^2 - 2 x.w + |w|^2, and a bound on what
    float64's own cancellation cost it: 2 gamma64(D + 4) (|x|^2 + |w|^2), which the callers add to their allowance."""
    x64, w64 = np.asarray(x, F32).astype(F64), np.asarray(w, F32).astype(F64)
    xq, wq = (x64 * x64).sum(1)[:, None], (w64 * w64).sum(1)[None, :]
    d2 = xq - 2 * (x64 @ w64.T) + wq
    return d2, (x64.shape[1] + 4) * 2.0 ** -52 * (xq + wq)


def check_operand_bound(ids, x, w, kind, E, what=""):
    """|x - w_pick|^2 <= |x - w_best|^2 + 2 (e_pick + e_best) + 2 (E_pick + E_best) against the unrounded float64 distances;
    returns the worst excess / allowance."""
    ids = np.asarray(ids, np.int64)
    if not len(ids):
        return 0.0
    assert ids.min() >= 0 and ids.max() < len(w), "%s: a pick outside the map" % what
    d2, d2err = sq_distances(x, w)
    e = operand_bound(x, w, kind)
    r = np.arange(len(ids))
    b = np.argmin(d2, axis=1)
    allow = 2 * (e[r, ids] + e[r, b]) + 2 * (E[r, ids] + E[r, b]) + d2err[r, ids] + d2err[r, b]
    over = d2[r, ids] - d2[r, b]
    with np.errstate(divide="ignore", invalid="ignore"):
        rat = np.where(over <= 0, 0.0, over / allow)
    i = int(np.argmax(rat))
    assert rat[i] <= 1.0, "%s: row %d picks unit %d at |x-w|^2 %r, unit %d is at %r: excess / allowance %.3g" % (
        what, i, ids[i], d2[i, ids[i]], b[i], d2[i, b[i]], rat[i])
    return float(rat[i])


def check_half(ids, x, w, kind, dist, key_ulps=16, ties=False, what=""):
    """All the checks of one launch's picks; returns {"pick": ..., "operand": ...} worst ratios."""
    ids = np.asarray(ids)
    assert ids.shape == (len(x),), "%s: %r ids for %d rows" % (what, ids.shape, len(x))
    assert ((ids >= 0) & (ids < len(w))).all(), "%s: a pick outside the map (a padding unit won?)" % what
    s, E = half_scores(x, w, kind, dist, key_ulps)
    out = {"pick": check_picks(ids, s, E, what)}
    if ties:
        check_ties(ids, s, what)
    if dist == "euclidean":
        out["operand"] = check_operand_bound(ids, x, w, kind, E, what)
    return out


# ------------------------------------------------------------------------------------------------ data
DATA_KINDS = ("blobs", "int", "offset30", "offset300", "tiny", "huge")


def pin_int_norms(x, w):
    """Small-integer rows and units (in place) made EXACT for the kernels: the last row and the last unit become
    (m, 0, 0, ...) with m in {32, 64, 96} and m^2 >= 9 D >= every other squared norm, so both maxima are m^2, their float32
    roots are m, and B = m m (1 + 2^-10) is an integer (m m is a multiple of 1024).  Every d' is then a half-integer below
    2^23."""
    D = x.shape[1]
    m = 32.0 if 9 * D <= 1024 else 64.0 if 9 * D <= 4096 else 96.0
    assert 9 * D <= m * m
    for a in (x, w):
        a[-1] = 0
        a[-1, 0] = m
    return x, w


def clear_of_boundaries(a, kind, rounds=30):
    """Cosine data the reference can decide: every element of the float32 rows `a` whose unit-length value is AMBIGUOUS for
    `kind` (round_operand) is moved, by 8 times the bracket's relative half-width (~2e-5 of the element or less), towards the
    16-bit value the reference rounds it to, i.e. away from the rounding boundary; repeated, since a moved element shifts
    its row's norm and with it the neighbours by a 1/D-th of that.  Deterministic per row (duplicate rows stay duplicates).
    Random blobs keep 0.05 - 0.7 % of their elements ambiguous whatever the seed, and below ~500 features ONE such element
    outweighs the float32 terms of E on every pair it takes part in -- the same rows a few float32 ulps aside do not.
    Returns the rows; whatever stays ambiguous after `rounds` is simply charged by half_scores."""
    a = np.array(a, F32)
    step = 8 * unit_scale_error(a.shape[1])
    for _ in range(rounds):
        r, amb = round_operand(a, kind, unit=True)
        bad = amb > 0
        if not bad.any():
            break
        a64 = a.astype(F64)
        q = np.sqrt((a64 * a64).sum(axis=1, keepdims=True))
        with np.errstate(divide="ignore", invalid="ignore"):
            y = np.where(q > 0, a64 / q, 0.0)
        grow = np.where(np.abs(r) > np.abs(y), 1.0 + step, 1.0 - step)
        a = np.where(bad, (a64 * grow), a64).astype(F32)
    return a


def make_half_data(kind, n, K, D, seed, dup=0, query=True, unit_kind=None):
    """(x, w) float32.  unit_kind ('bf16' / 'f16': the cosine cases pass their precision): rows and units go through
    clear_of_boundaries.  blobs / int / offset30 / offset300: query_ref's (int: pinned by pin_int_norms); tiny: blobs scaled
    by 2^-12, where a tenth of the elements round to SUBNORMAL halves; huge: blobs scaled so that norms reach 6e4 and,
    in query batches (set_data refuses such rows), elements at and beyond +-65504 that the half conversion saturates."""
    base = kind if kind in ("blobs", "int", "offset30", "offset300") else "blobs"
    x = make_rows(base, n, D, seed)
    w = make_units(base, x, K, D, seed, dup)
    if kind == "int":
        pin_int_norms(x, w)
    elif kind == "tiny":
        x, w = (x * F32(2.0 ** -12)), (w * F32(2.0 ** -12))
    elif kind == "huge":
        sc = F32(6.0e4 / max(np.linalg.norm(x.astype(F64), axis=1).max(), np.linalg.norm(w.astype(F64), axis=1).max()))
        x, w = x * sc, w * sc
        if query:
            rs = np.random.RandomState(seed + 2)
            for v in (65504.0, -65504.0, 65520.0, -7.0e4, 1.0e6):
                x[rs.randint(0, n), rs.randint(0, D)] = v
    if unit_kind is not None:
        x, w = clear_of_boundaries(x, unit_kind), clear_of_boundaries(w, unit_kind)
    return np.ascontiguousarray(x, F32), np.ascontiguousarray(w, F32)


# ------------------------------------------------------------------------------------------ the host's dispatch
def half_paths(X, Y, D, n, prec, dist, env=None, epochs=0):
    """Labels of what one BMU launch of n rows reaches on an X x Y x D map of precision 'bf16' / 'f16' (csrc/somhip.hip):

      k16.ks{1..4}.{bf16,f16} / wide.ks{5..25}.{bf16,f16} / tiled.{4x2x2,8x2x4}.{bf16,f16}
                  the kernel family with KS32 or the tile configuration, and the operand type.  som_create:1371-1388:
                  beyond 128 features the two-sided tiling, 8x2x4 from 4096 units on, and from there the wide kernel up
                  to 25 chunks of 32 features unless SOM_BF16_WIDE=0; launch_bmu_half:797-812, launch_bmu_bf16_tiled:777-794
      {family}.{euclidean,cosine}
      {family}.parts.{one,several,forced}
                  the part count where it is known beforehand: SOM_BF16_PARTS (forced; k16:701 takes it as it is, the
                  others clamp it to their unit blocks / stages: 727, 761); one stage or unit block: one; otherwise
                  choose_parts:666-689 (k16:700, tiled:723-725) or the wide launcher's own rule (750-759) split a grid of
                  fewer workgroups than resident slots -- there are at least 256 slots, so fewer than 256 workgroups
                  always split: several.  Larger grids depend on the occupancy: no label.
      {family}.prep.{separate,fused}
                  epochs > 0: the images came from som_epoch_merge:1862-1863 -- merge_prep_k16_kernel (k16, euclidean) or
                  merge_prep_wide_kernel (wide) unless SOM_FUSE_MERGE=0; otherwise, and after set_weights, from
                  prep_codebook_half:470-537."""
    env = env or {}
    K = X * Y
    out = set()
    if D <= 128:
        fam, ks = "k16", _cdiv(D, 32)
        name = "k16.ks%d" % ks
        blocks, units = _cdiv(n, K16_WG_SAMPLES), _cdiv(K, K16_STAGE_UNITS)
    else:
        big = K >= 4096
        ks = _cdiv(D, TL_BK)
        if big and ks <= 25 and env.get("SOM_BF16_WIDE", "1") != "0":
            fam, name = "wide", "wide.ks%d" % ks
            blocks, units = _cdiv(n, WD_WG_SAMPLES), _cdiv(K, WD_STAGE_UNITS)
        else:
            fam, name = "tiled", "tiled.%s" % ("8x2x4" if big else "4x2x2")
            bm = bn = 256 if big else 128
            blocks, units = _cdiv(n, bm), _cdiv(K, bn)
    out.add("%s.%s" % (name, prec))
    out.add("%s.%s" % (fam, dist))
    forced = int(env.get("SOM_BF16_PARTS", "0") or 0)
    if forced > 0:
        out.add(fam + ".parts.forced")
    elif units == 1:
        out.add(fam + ".parts.one")
    elif blocks < 256:
        out.add(fam + ".parts.several")
    fusable = (fam == "k16" and dist == "euclidean") or fam == "wide"
    fused = epochs > 0 and fusable and env.get("SOM_FUSE_MERGE", "1") != "0"
    out.add("%s.prep.%s" % (fam, "fused" if fused else "separate"))
    return out


def family_of(labels):
    return sorted(labels)[0].split(".")[0]


def required_type(ks):
    """The operand type the grid must cover for KS32 = ks: the two alternate."""
    return "bf16" if ks % 2 else "f16"


ALL_LABELS = ({"k16.ks%d.%s" % (k, required_type(k)) for k in range(1, 5)}
              | {"wide.ks%d.%s" % (k, required_type(k)) for k in range(5, 26)}
              | {"tiled.%s.%s" % (c, t) for c in ("4x2x2", "8x2x4") for t in KINDS}
              | {"%s.%s" % (f, d) for f in ("k16", "tiled", "wide") for d in ("euclidean", "cosine")}
              | {"%s.parts.%s" % (f, p) for f in ("k16", "tiled") for p in ("one", "several", "forced")}
              | {"wide.parts.several", "wide.parts.forced"}
              | {"k16.prep.separate", "k16.prep.fused", "wide.prep.separate", "wide.prep.fused", "tiled.prep.separate"})

__all__ = ["ALL_LABELS", "BF_PAD_NORM", "DATA_KINDS", "F32", "F64", "KAPPA", "KEY_ULPS", "check_half", "check_operand_bound",
           "check_picks", "check_ties", "clear_of_boundaries", "family_of", "half_paths", "half_scores", "half_terms", "make_half_data",
           "operand_bound", "pick_ratio", "pin_int_norms", "required_type", "round_operand", "sq_distances",
           "unit_scale_error"]
