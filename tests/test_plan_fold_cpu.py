"""The folded plan's split of a row threshold (plan_fold_scale, plan_split_threshold, csrc/exact_skip.hpp) without a GPU, through
the library's test hook som_debug_plan_split (include/somhip_test.h): the host side of the __host__ __device__ functions the plan
kernels call in their prologue.

The plan kernels subtract P~ = c (p1 + p2 + p3) from every accumulator inside the extra MFMA step and test a sign, so the plan is
sound iff P~ >= P in REAL arithmetic for every P, with p1..p3 values the operand type holds as NORMAL numbers (or zero) and c a power
of two of that type.  Both are checked here in exact rational arithmetic, for IEEE half and bfloat16 operands, together with how
tight the split is:  P~ <= P + |P| 2^-19 + c MINN  (MINN: the type's smallest normal value -- the part a positive remainder below it
is rounded up to) wherever |P / c| is inside the type's range.  Beyond the range a positive P gives +inf (the row needs everything),
a negative one the type's most negative value (still >= P)."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from xpysom_dask_amd import _lib

FMT = {  # mantissa bits, smallest normal, largest finite, the exponents c may take
    "f16": dict(flag=0, m=10, minn=2.0 ** -14, maxv=65504.0, cmin=-14, cmax=15),
    "bf16": dict(flag=1, m=7, minn=2.0 ** -126, maxv=float(np.float32(2.0 ** 127) * np.float32(2.0 - 2.0 ** -7)), cmin=-100, cmax=100),
}
# S'Bm' of a level: ~2^27 .. 2^30 under the scales' normal working (the longest norms land in [2^13, 2^14)); the extremes are what
# the scales' exponent clamp (+-100) and float32 leave: from the smallest product the kernels accept to the largest finite one
S_BMAG = [2.0 ** -119, 2.0 ** -40, 1.0, 2.0 ** 26, 1.37 * 2.0 ** 28, 2.0 ** 30 * 0.99, 2.0 ** 31, 2.0 ** 60, 2.0 ** 119]


def split(fmt, P, s_bmag):
    lib = _lib.load()
    P = np.ascontiguousarray(P, dtype=np.float32)
    sb = np.ascontiguousarray(np.broadcast_to(np.float32(s_bmag), P.shape), dtype=np.float32)
    out = np.empty((P.size, 4), dtype=np.float32)
    fp = C.POINTER(C.c_float)
    rc = lib.som_debug_plan_split(FMT[fmt]["flag"], P.size, P.ctypes.data_as(fp), sb.ctypes.data_as(fp), out.ctypes.data_as(fp))
    assert rc == 0
    return out


def is_value_of(fmt, v):
    """v (a float32) is zero or a NORMAL number of the operand type."""
    f = FMT[fmt]
    if v == 0.0:
        return True
    if not math.isfinite(v):
        return True
    bits = np.float32(v).view(np.uint32)
    return (int(bits) & ((1 << (23 - f["m"])) - 1)) == 0 and f["minn"] <= abs(v) <= f["maxv"]


def sweep(s_bmag):
    """float32 thresholds around a level of scale s_bmag: a logarithmic sweep of both signs with odd mantissas from far below the
    smallest part to beyond the type's range, the edges of the range, and values whose second or third part would be subnormal."""
    rng = np.random.default_rng(17)
    vals = []
    for k in np.arange(-60.0, 4.0, 0.37):
        mant = 1.0 + rng.random()
        vals += [s_bmag * mant * 2.0 ** k, -s_bmag * mant * 2.0 ** k]
    for e in range(-30, 3):                                     # a leading part and a tail far below it
        vals += [s_bmag * 2.0 ** e * (1.0 + 2.0 ** -20), s_bmag * 2.0 ** e * (1.0 - 2.0 ** -22), -s_bmag * 2.0 ** e * (1.0 + 2.0 ** -23)]
    vals += [0.0, -0.0, 1e-45, -1e-45]
    v = np.array(vals, dtype=np.float64)
    v = v[np.abs(v) < 3.0e38]
    return v.astype(np.float32)


@pytest.mark.parametrize("fmt", sorted(FMT))
@pytest.mark.parametrize("s_bmag", S_BMAG)
def test_split_is_never_below_the_threshold_and_is_tight(fmt, s_bmag):
    f = FMT[fmt]
    P = sweep(s_bmag)
    out = split(fmt, P, s_bmag)
    c = float(out[0, 0])
    assert np.all(out[:, 0] == out[0, 0])
    m, e = math.frexp(c)
    assert m == 0.5 and f["cmin"] <= e - 1 <= f["cmax"], "c is a power of two the operand type holds: %g" % c
    # the level's scale covers every accumulator (<= S'Bm') unless the type's powers of two run out
    if f["cmin"] < e - 1 < f["cmax"]:
        assert 65504.0 * c >= 1.01 * s_bmag * (1 - 2.0 ** -20) and 65504.0 * c <= 2.03 * s_bmag
    for p, (_, p1, p2, p3) in zip(P, out):
        p, p1, p2, p3 = float(p), float(p1), float(p2), float(p3)
        assert is_value_of(fmt, p1) and is_value_of(fmt, p2) and is_value_of(fmt, p3), (p, p1, p2, p3)
        if p1 == math.inf:
            # beyond the type's range: everything is needed -- only for a P above the range, never for one inside it
            assert p2 == 0.0 and p3 == 0.0 and p / c > f["maxv"] * (1.0 - 2.0 ** -(f["m"] + 2)), (p, c)
            continue
        assert math.isfinite(p1) and math.isfinite(p2) and math.isfinite(p3)
        tilde = Fraction(c) * (Fraction(p1) + Fraction(p2) + Fraction(p3))
        assert tilde > Fraction(p) or (tilde == 0 and p <= 0), "P~ below (or at) P: %r -> %r" % (p, (c, p1, p2, p3))
        if abs(p) / c <= f["maxv"]:
            # (one float32 step up is part of the split: 2^-23 |P|, or the smallest float32 at zero)
            hi = Fraction(p) + abs(Fraction(p)) * Fraction(1, 2 ** 19) + Fraction(c) * Fraction(f["minn"]) + Fraction(2.0 ** -149)
            assert tilde <= hi, "P~ looser than P (1 + 2^-19) + c MINN: %r -> %r" % (p, (c, p1, p2, p3))
        elif p < 0:
            assert p1 == -f["maxv"]                              # (below the range: the type's most negative value, still >= P)


@pytest.mark.parametrize("fmt", sorted(FMT))
def test_infinities_and_nan(fmt):
    P = np.array([np.inf, -np.inf, np.nan, np.float32(3.4e38)], dtype=np.float32)
    for s_bmag in S_BMAG:
        out = split(fmt, P, s_bmag)
        assert out[0, 1] == np.inf and out[0, 2] == 0 and out[0, 3] == 0          # +inf stays +inf
        assert out[1, 1] == -np.inf and out[1, 2] == 0 and out[1, 3] == 0         # -inf stays -inf
        assert out[2, 1] == np.inf and out[2, 2] == 0 and out[2, 3] == 0          # a NaN needs everything
        assert out[3, 1] == np.inf or Fraction(float(out[3, 0])) * sum(Fraction(float(v)) for v in out[3, 1:]) >= Fraction(float(P[3]))


@pytest.mark.parametrize("fmt", sorted(FMT))
def test_a_scale_that_is_not_a_number_is_still_a_power_of_two(fmt):
    for s in (0.0, -1.0, np.inf, np.nan, 1e-45):
        out = split(fmt, np.array([1.0, -3.5], dtype=np.float32), s)
        c = float(out[0, 0])
        assert math.frexp(c)[0] == 0.5
        for p, row in zip((1.0, -3.5), out):
            assert row[1] == np.inf or Fraction(c) * sum(Fraction(float(v)) for v in row[1:]) >= Fraction(p)


@pytest.mark.parametrize("fmt", sorted(FMT))
def test_parts_that_would_be_subnormal(fmt):
    """t = P / c with a tail below the type's smallest normal value: the tail is not dropped, it is rounded up to that value."""
    f = FMT[fmt]
    s_bmag = 2.0 ** 28
    c = float(split(fmt, np.array([1.0], dtype=np.float32), s_bmag)[0, 0])
    if fmt == "f16":
        t = np.array([1.0 + 2.0 ** -20, 2.0 ** -13 * (1 + 2.0 ** -12), 2.0 ** -16, 3.0 * 2.0 ** -14 + 2.0 ** -30], dtype=np.float64)
    else:
        t = np.array([2.0 ** -120 * (1 + 2.0 ** -10), 2.0 ** -125 * (1 + 2.0 ** -20)], dtype=np.float64)
    P = (t * c).astype(np.float32)
    out = split(fmt, P, s_bmag)
    for p, (_, p1, p2, p3) in zip(P, out):
        assert all(is_value_of(fmt, float(v)) for v in (p1, p2, p3))
        tilde = Fraction(c) * (Fraction(float(p1)) + Fraction(float(p2)) + Fraction(float(p3)))
        assert tilde > Fraction(float(p))
        assert tilde <= Fraction(float(p)) * (1 + Fraction(1, 2 ** 19)) + Fraction(c) * Fraction(f["minn"])
