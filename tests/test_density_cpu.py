"""The data density per unit without a device: the float64 model and its band (tests/density_ref.py) against a brute-force count,
the band's width on every input the GPU module uses, the scan's launch geometry (som_debug_density_plan) against a Python
restatement, the argument checks that run before an engine exists, the U*-matrix formula, and the new symbols."""
import ctypes as C

import numpy as np
import pytest

from tests import density_ref as R

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def case_models():
    """Per GPU band case: (x, w, pivot, s, E, radii, lo, hi), computed once."""
    out = {}
    for c in R.CASES:
        x, w = R.case_data(c)
        pivot = R.midrange(w)
        s, E = R.model(x, w, pivot)
        radii = R.percentile_radii(s)
        lo, hi = R.band(s, E, radii)
        out[c["id"]] = (x, w, pivot, s, E, radii, lo, hi)
    return out


@pytest.mark.parametrize("c", R.CASES, ids=[c["id"] for c in R.CASES])
def test_band_holds_the_brute_force_count_and_is_narrow(c, case_models):
    x, w, pivot, s, E, radii, lo, hi = case_models[c["id"]]
    n, K = c["N"], c["X"] * c["Y"]
    assert len(radii) == 7 and radii[0] == 0 and (np.diff(radii) >= 0).all()
    brute = R.brute_counts(x, w, pivot, radii)
    assert R.check_counts(brute, lo, hi, c["id"]) >= 0
    share = R.band_share(lo, hi, n)
    print("%s: undecided pairs per radius %s of %d" % (c["id"], (hi - lo).sum(axis=1).tolist(), n * K))
    assert (share <= R.MAX_SHARE).all(), "%s: the band leaves %s of the pairs open" % (c["id"], share)
    # the counts are what the radii were chosen for: nothing at 0 on continuous data, every pair at twice the maximum
    assert (hi[0] == 0).all() or c["kind"] == "int"
    assert (lo[-1] == n).all() and (hi[-1] == n).all()
    assert abs(brute[4].sum() / (n * K) - 0.5) < 0.01


def test_uncentred_offset_rows_cannot_be_counted_and_centred_ones_can():
    """Why the pivot: on rows of spread 1e-3 around 30 the float32 bound of the un-centred GEMM form exceeds every distance; about the
    midrange of the codebook it is a fraction of a per cent of it."""
    c = R.CASES[2]
    assert c["kind"] == "offset30"
    x, w = R.case_data(c)
    s0, E0 = R.model(x, w, None)
    assert (E0 > s0).all()
    s, E = R.model(x, w, R.midrange(w))
    assert (E / s).max() < 0.0023


def test_uncentred_blobs_band_is_narrow():
    """pivot = NULL on centred blobs (the GPU module's case): the un-centred model's band is as narrow."""
    c = R.CASES[1]
    x, w = R.case_data(c)
    s, E = R.model(x, w, None)
    radii = R.percentile_radii(s)
    lo, hi = R.band(s, E, radii)
    assert (R.band_share(lo, hi, c["N"]) <= R.MAX_SHARE).all()
    R.check_counts(R.brute_counts(x, w, None, radii), lo, hi, "uncentred blobs")


@pytest.mark.parametrize("c", R.TIE_CASES, ids=[c["id"] for c in R.TIE_CASES])
def test_integer_data_is_exact_and_sits_on_the_radii(c):
    """Small integers about a half-integer pivot: every operand, product and sum is exact in float32 (E's terms are bounds, the
    values are integers and quarters below 2^24), so the count is the float64 count exactly -- and pairs sit ON every radius,
    thousands in all, so `<` in place of `<=` gives another answer at each of them."""
    x, w = R.case_data(c)
    pivot = R.midrange(w)
    assert (np.abs(pivot * 2 - np.round(pivot * 2)) == 0).all()
    xc, wc = R.centred(x, w, pivot)
    assert ((xc.astype(F64) == x.astype(F64) - pivot.astype(F64)).all() and (wc.astype(F64) == w.astype(F64) - pivot.astype(F64)).all())
    s, _ = R.model(x, w, pivot)
    plain = ((x.astype(F64)[:, None, :] - w.astype(F64)[None, :, :]) ** 2).sum(axis=2)
    assert np.array_equal(s, plain)                       # (float64 GEMM form of quarter-integers: exact too)
    incl = R.brute_counts(x, w, pivot, R.TIE_RADII, inclusive=True)
    strict = R.brute_counts(x, w, pivot, R.TIE_RADII, inclusive=False)
    on_radius = (incl - strict).sum(axis=1)
    print("%s: pairs exactly on each radius %s" % (c["id"], on_radius.tolist()))
    assert (on_radius > 0).all() and on_radius.sum() >= 1000


def test_nonfinite_rows_are_in_neither_count():
    c = R.CASES[1]
    x, w = R.case_data(c)
    x = x[:64].copy()
    x[3, 5] = np.nan
    x[10, 0] = np.inf
    x[11, 36] = -np.inf
    pivot = R.midrange(w)
    s, E = R.model(x, w, pivot)
    radii = np.array([1e3], F32)
    lo, hi = R.band(s, E, radii)
    assert (lo == 61).all() and (hi == 61).all()


def _plan(n, K, slots, forced=0):
    from xpysom_dask_amd import _lib
    lib = _lib.load()
    out = (C.c_int64 * 4)()
    assert lib.som_debug_density_plan(n, K, slots, forced, out) == 0
    return tuple(out)


def test_density_plan_matches_its_restatement():
    seen = set()
    for n in (1, 127, 128, 129, 517, 1000, 70000, 1 << 20, (1 << 31) - 1):
        for K in (1, 128, 129, 200, 333, 4096, 65536):
            for slots in (1, 3, 512, 1024):
                for forced in (0, 1, 3, 64):
                    got = _plan(n, K, slots, forced)
                    assert got == R.plan(n, K, slots, forced), (n, K, slots, forced)
                    ut, rt, slabs, per = got
                    assert 1 <= slabs <= rt and (slabs - 1) * per < rt <= slabs * per     # every slab holds a row tile, all are covered
                    seen.add((ut == 1, slabs == rt, forced > 0, slots < ut))
    # K = 1, slabs clamped to the row tiles, a forced count, fewer slots than unit tiles: all reached
    assert {a for a, _, _, _ in seen} == {True, False} and {b for _, b, _, _ in seen} == {True, False}
    assert {d for _, _, _, d in seen} == {True, False}
    assert _plan(517, 1, 512) == (1, 5, 5, 1)                  # one unit: the rows alone fill what they can
    assert _plan(1000, 200, 512) == (2, 8, 8, 1)               # small map: clamped to the row tiles
    assert _plan(1000, 200, 512, 3) == (2, 8, 3, 3)            # forced
    assert _plan(1000, 200, 512, 64) == (2, 8, 8, 1)           # forced, clamped
    assert _plan(1 << 20, 65536, 512) == (512, 8192, 1, 8192)  # the flagship map: one slab, the unit tiles fill the chip
    assert _plan(1 << 20, 65536, 3) == (512, 8192, 1, 8192)    # fewer slots than unit tiles
    assert _plan(1 << 20, 4096, 512) == (32, 8192, 16, 512)
    from xpysom_dask_amd import _lib
    lib = _lib.load()
    out = (C.c_int64 * 4)()
    for bad in ((0, 4, 8, 0), (5, 0, 8, 0), (5, 4, 0, 0), (5, 4, 8, -1), (1 << 31, 4, 8, 0)):
        assert lib.som_debug_density_plan(*bad, out) != 0, bad
    assert lib.som_debug_density_plan(5, 4, 8, 0, None) != 0


@pytest.fixture
def no_engine(monkeypatch):
    """Any attempt to create an engine fails the test: the refusals below must come first."""
    from xpysom_dask_amd import engine

    def boom(*a, **k):
        raise AssertionError("an engine was created before the arguments were checked")
    monkeypatch.setattr(engine, "HipEngine", boom)


@pytest.mark.parametrize("radius", [-1.0, float("nan"), float("inf"), 1e30, [], [1, 2, 3, 4, 5, 6, 7, 8, 9], [1.0, -0.5], "a"],
                         ids=["negative", "nan", "inf", "square-overflows", "empty", "nine", "one-negative", "text"])
def test_bad_radii_are_refused_before_an_engine_exists(radius, no_engine):
    from xpysom_dask_amd import XPySom
    som = XPySom(4, 5, 3, random_seed=1)
    data = np.zeros((6, 3), F32)
    with pytest.raises(ValueError):
        som.density_map(data, radius)
    if np.ndim(radius) == 0:
        with pytest.raises(ValueError):
            som.ustar_map(data, radius)


def test_ustar_takes_one_radius(no_engine):
    from xpysom_dask_amd import XPySom
    som = XPySom(4, 5, 3, random_seed=1)
    with pytest.raises(ValueError, match="one radius"):
        som.ustar_map(np.zeros((6, 3), F32), [1.0, 2.0])


def test_missing_nan_is_refused_before_an_engine_exists(no_engine):
    from xpysom_dask_amd import XPySom
    som = XPySom(4, 5, 3, random_seed=1, missing="nan")
    for call in (som.density_map, som.ustar_map):
        with pytest.raises(NotImplementedError, match=call.__name__.split("_")[0]):
            call(np.zeros((6, 3), F32), 1.0)


def test_check_radii_accepts_what_the_contract_allows():
    from xpysom_dask_amd.engine import check_radii
    assert check_radii(0).tolist() == [0.0] and check_radii(-0.0).tolist() == [0.0]
    r = check_radii([0, 1.5, 1e19])
    assert r.dtype == F32 and r.shape == (3,)
    assert len(check_radii(range(8))) == 8
    with pytest.raises(ValueError):
        check_radii(2e19)                                  # 4e38 > float32's largest


def test_ustar_formula():
    from xpysom_dask_amd.xpysom import _ustar
    u = np.arange(1.0, 10.0).reshape(3, 3)
    p = np.array([[0, 4, 8], [4, 4, 4], [2, 6, 4]], np.int64)        # mean 4, max 8
    got = _ustar(u, p)
    assert got.dtype == F64
    want = u * np.array([[2.0, 1.0, 0.0], [1.0, 1.0, 1.0], [1.5, 0.5, 1.0]])
    np.testing.assert_array_equal(got, want)
    assert got[0, 2] == 0 and (got[1] == u[1]).all()         # 0 where the density is highest, U where it is average
    flat = _ustar(u, np.full((3, 3), 7))
    np.testing.assert_array_equal(flat, u)
    assert flat is not u
    with pytest.raises(ValueError):
        _ustar(u, np.zeros((2, 3)))


def test_new_symbols_resolve():
    from xpysom_dask_amd import _lib
    lib = _lib.load()
    F, I64 = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    assert _lib.SIGNATURES["som_unit_density"] == (C.c_int, [C.c_void_p, F, C.c_int64, F, F, C.c_int32, I64])
    assert _lib.SIGNATURES["som_unit_density_device"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, F, F, C.c_int32, I64])
    assert _lib.SIGNATURES["som_debug_density_plan"] == (C.c_int, [C.c_int64, C.c_int32, C.c_int64, C.c_int32, I64])
    for name in ("som_unit_density", "som_unit_density_device", "som_debug_density_plan"):
        assert hasattr(lib, name)
    # a NULL handle is refused, not dereferenced
    r = (C.c_float * 1)(1.0)
    out = (C.c_int64 * 4)()
    assert lib.som_unit_density(None, None, 0, None, r, 1, out) != 0
    from xpysom_dask_amd.engine import HipEngine
    from xpysom_dask_amd.xpysom import XPySom
    for owner, names in ((HipEngine, ("unit_density", "unit_density_device")), (XPySom, ("density_map", "ustar_map"))):
        for n in names:
            assert callable(getattr(owner, n))
