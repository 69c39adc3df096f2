"""The data density per unit on the device -- som_unit_density / som_unit_density_device, XPySom.density_map / ustar_map -- against
the float64 model and the band of tests/density_ref.py.  GPU only (`-m gpu`).

Rows and units come from query_ref's generators with seed 3; the radii are 0, the 1st, 5th, 20th, 50th and 90th percentile of the
model's distances and twice the maximum; the pivot is the midrange of the codebook.  Checked:
  band cases   lo <= P <= hi for every unit and radius, on shapes that reach every tail of the 128 x 128 x 32 tiling, with the
               band itself held to 0.5 % of the pairs
  exact ties   small integers: P is the float64 count of |x - w|^2 <= r^2 exactly, inclusive (pairs sit on every radius, thousands in all)
  geometry     SOM_DENSITY_SLABS = 1, 3 and 64 give identical arrays; 1 .. 8 radii equal the rows of the eight-radius call
  rows         a NaN or an infinity in a row: counted nowhere; pivot = NULL passes the un-centred band
  entries      host rows = device rows, through the C ABI and through XPySom.density_map; n_parallel chunks add up; the counts
               follow the codebook after train; ustar_map is _ustar of the two maps; a missing='nan' engine refuses by name."""
import numpy as np
import pytest

from tests import density_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def engine(X, Y, D, **kw):
    from xpysom_dask_amd.engine import HipEngine
    kw.setdefault("precision", "f32")
    return HipEngine(X, Y, D, **kw)


def _device_rows(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, F32)).cuda()


_MODELS = {}


def case_model(c):
    """(x, w, pivot, radii, lo, hi) of a band case, computed once per session and never written to."""
    if c["id"] not in _MODELS:
        x, w = R.case_data(c)
        pivot = R.midrange(w)
        s, E = R.model(x, w, pivot)
        radii = R.percentile_radii(s)
        lo, hi = R.band(s, E, radii)
        _MODELS[c["id"]] = (x, w, pivot, radii, lo, hi)
    return _MODELS[c["id"]]


@pytest.mark.parametrize("c", R.CASES, ids=[c["id"] for c in R.CASES])
def test_band_case(c):
    x, w, pivot, radii, lo, hi = case_model(c)
    n = c["N"]
    share = R.band_share(lo, hi, n)
    assert (share <= R.MAX_SHARE).all(), "%s: the band leaves %s of the pairs open" % (c["id"], share)
    e = engine(c["X"], c["Y"], c["D"])
    try:
        e.set_weights(w)
        got = e.unit_density(x, pivot, radii)
        open_entries = R.check_counts(got, lo, hi, c["id"])
        print("%s: %d of %d entries not pinned by the band; counts per radius %s" % (
            c["id"], open_entries, got.size, got.sum(axis=1).tolist()))
        assert (got[0] == 0).all() and (got[-1] == n).all()
        again = e.unit_density(x, pivot, radii)
        assert np.array_equal(again, got), "%s: a second call differs" % c["id"]
        t = _device_rows(x)
        dev = e.unit_density_device(t.data_ptr(), n, pivot, radii)
        assert np.array_equal(dev, got), "%s: the device entry differs from the host entry" % c["id"]
    finally:
        e.close()


@pytest.mark.parametrize("c", R.TIE_CASES, ids=[c["id"] for c in R.TIE_CASES])
def test_exact_ties(c):
    x, w = R.case_data(c)
    pivot = R.midrange(w)
    want = R.brute_counts(x, w, None, R.TIE_RADII, inclusive=True)          # |x - w|^2 <= r^2 on the integers themselves
    strict = R.brute_counts(x, w, None, R.TIE_RADII, inclusive=False)
    assert ((want - strict).sum(axis=1) > 0).all()           # pairs sit ON every radius: `<` would count fewer at each
    e = engine(c["X"], c["Y"], c["D"])
    try:
        e.set_weights(w)
        got = e.unit_density(x, pivot, np.array(R.TIE_RADII, F32))
        assert got.dtype == np.int64 and np.array_equal(got, want), "%s: %d entries differ from the exact count" % (
            c["id"], (got != want).sum())
    finally:
        e.close()


@pytest.mark.parametrize("c", [R.CASES[1], R.CASES[3]], ids=[R.CASES[1]["id"], R.CASES[3]["id"]])
def test_slab_and_radius_count_independence(c, monkeypatch):
    x, w, pivot, radii, lo, hi = case_model(c)
    radii8 = np.concatenate([radii, radii[3:4] * F32(1.5)]).astype(F32)
    e = engine(c["X"], c["Y"], c["D"])
    try:
        e.set_weights(w)
        monkeypatch.delenv("SOM_DENSITY_SLABS", raising=False)
        base = e.unit_density(x, pivot, radii8)
        R.check_counts(base[:7], lo, hi, c["id"])
        for slabs in ("1", "3", "64"):
            monkeypatch.setenv("SOM_DENSITY_SLABS", slabs)
            assert np.array_equal(e.unit_density(x, pivot, radii8), base), "%s: SOM_DENSITY_SLABS=%s changes the counts" % (c["id"], slabs)
        monkeypatch.delenv("SOM_DENSITY_SLABS")
        for r in range(1, 8):                                # every instance of the kernel: 1, 2, 4 and 8 counters, with spare ones
            part = e.unit_density(x, pivot, radii8[8 - r:])
            assert part.shape == (r, c["X"] * c["Y"]) and np.array_equal(part, base[8 - r:]), "%s: %d radii differ from their rows" % (c["id"], r)
        assert np.array_equal(e.unit_density(x, pivot, radii8[2:3]), base[2:3])
    finally:
        e.close()


def test_nonfinite_rows_add_nothing():
    c = R.CASES[1]
    x, w, pivot, radii, lo, hi = case_model(c)
    bad = x[:300].copy()
    bad[::3, 5] = np.nan
    bad[1::3, 0] = np.inf
    bad[2::3, 36] = -np.inf
    bad[7] = np.nan
    e = engine(c["X"], c["Y"], c["D"])
    try:
        e.set_weights(w)
        clean = e.unit_density(x, pivot, radii)
        both = e.unit_density(np.concatenate([x[:500], bad, x[500:]]), pivot, radii)
        assert np.array_equal(both, clean)
        assert (e.unit_density(bad, pivot, radii) == 0).all()
    finally:
        e.close()


def test_null_pivot_passes_the_uncentred_band():
    c = R.CASES[1]
    x, w = R.case_data(c)
    s, E = R.model(x, w, None)
    radii = R.percentile_radii(s)
    lo, hi = R.band(s, E, radii)
    assert (R.band_share(lo, hi, c["N"]) <= R.MAX_SHARE).all()
    e = engine(c["X"], c["Y"], c["D"])
    try:
        e.set_weights(w)
        R.check_counts(e.unit_density(x, None, radii), lo, hi, "pivot=NULL")
        t = _device_rows(x)
        R.check_counts(e.unit_density_device(t.data_ptr(), c["N"], None, radii), lo, hi, "pivot=NULL, device rows")
    finally:
        e.close()


def test_precision_and_distance_do_not_matter():
    """Always Euclidean, always float32: a bf16 / cosine handle and the default (exact) handle count what the f32 handle counts."""
    c = R.CASES[4]
    x, w, pivot, radii, lo, hi = case_model(c)
    got = []
    for kw in (dict(precision="f32"), dict(precision="bf16", distance="cosine"), dict(precision="exact")):
        e = engine(c["X"], c["Y"], c["D"], **kw)
        try:
            e.set_weights(w)
            got.append(e.unit_density(x, pivot, radii))
        finally:
            e.close()
    R.check_counts(got[0], lo, hi, c["id"])
    assert np.array_equal(got[1], got[0]) and np.array_equal(got[2], got[0])


def test_empty_and_refusals():
    from xpysom_dask_amd.engine import SomHipError
    e = engine(4, 5, 3)
    try:
        z = e.unit_density(np.zeros((0, 3), F32), None, [1.0, 2.0])
        assert z.dtype == np.int64 and z.shape == (2, 20) and (z == 0).all()
        with pytest.raises(ValueError):
            e.unit_density(np.zeros((2, 3), F32), None, [-1.0])
        with pytest.raises(ValueError):
            e.unit_density(np.zeros((2, 3), F32), np.zeros(4, F32), [1.0])
    finally:
        e.close()
    m = engine(4, 5, 3, missing="nan")
    try:
        with pytest.raises(SomHipError, match="som_unit_density:.*SOM_MISSING_NAN"):
            m.unit_density(np.zeros((2, 3), F32), None, [1.0])
        t = _device_rows(np.zeros((2, 3), F32))
        with pytest.raises(SomHipError, match="som_unit_density_device:.*SOM_MISSING_NAN"):
            m.unit_density_device(t.data_ptr(), 2, None, [1.0])
    finally:
        m.close()


def test_density_map_and_ustar_map():
    from xpysom_dask_amd import XPySom
    from xpysom_dask_amd.xpysom import _ustar
    c = R.CASES[1]
    x, w, pivot, radii, lo, hi = case_model(c)
    X, Y, D, n = c["X"], c["Y"], c["D"], c["N"]
    som = XPySom(X, Y, D, random_seed=5, precision="f32", topology="toroidal")
    som._weights = w.reshape(X, Y, D).astype(F64)
    assert np.array_equal(som._density_pivot(), pivot)
    maps = som.density_map(x, radii)
    assert maps.dtype == np.int64 and maps.shape == (7, X, Y)
    R.check_counts(maps.reshape(7, X * Y), lo, hi, "density_map")
    one = som.density_map(x, float(radii[3]))
    assert one.shape == (X, Y) and np.array_equal(one, maps[3])
    assert np.array_equal(som.density_map(x, [radii[3]]), maps[3:4])
    # device rows: counted where they are, the host rows' counts
    t = _device_rows(x)
    assert np.array_equal(som.density_map(t, radii), maps)
    # chunks of 256 rows add up to one chunk's counts
    chunked = XPySom(X, Y, D, random_seed=5, precision="f32", topology="toroidal", n_parallel=256)
    chunked._weights = som._weights.copy()
    assert np.array_equal(chunked.density_map(x, radii), maps)
    # U*: the host formula on the two maps
    us = som.ustar_map(x, float(radii[3]))
    assert us.dtype == F64 and np.array_equal(us, _ustar(som.distance_map(), maps[3]))
    assert us.min() == 0 and (us[maps[3] == maps[3].max()] == 0).all()
    # freshness: after train the counts are those of the new codebook
    before = som.density_map(x, float(radii[4]))
    som.train(x, 2)
    w2 = np.asarray(som._weights, F32).reshape(X * Y, D)
    assert not np.array_equal(w2, w)
    s2, E2 = R.model(x, w2, R.midrange(w2))
    lo2, hi2 = R.band(s2, E2, radii[4:5])
    after = som.density_map(x, float(radii[4]))
    R.check_counts(after.reshape(1, X * Y), lo2, hi2, "density_map after train")
    assert not np.array_equal(after, before)
    with pytest.raises(NotImplementedError, match="density_map"):
        XPySom(X, Y, D, random_seed=5, missing="nan").density_map(x, 1.0)
