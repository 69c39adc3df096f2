"""The map diagnostics on the device -- som_bmu_distances / som_unit_stats and XPySom.quantization_distances / unit_statistics --
against the float64 model and the bounds of tests/diag_ref.py.  GPU only (`-m gpu`).

Every case is teacher-forced: set a codebook, query rows, compare with the model computed from the codebook the engine holds.
For every case of diag_ref.CASES (the smallest shapes that cross each boundary of the kernels: one lane, odd widths, one and two
fma steps a lane, beyond 128 features, the 16-bit searches, the exact mode's screen + window path on >= 4096 units, segments of
more than a thousand rows, missing values; and past one turn: three turns of the persistent row loop, the mask on a lane's second
and third fma step, the per-unit kernels behind the counting sort at its ceiling of 8 192 units and behind the radix sort above it):
  (a) the ids are e.bmu(x, quantization=True)'s of the same handle bit for bit (exact handles: also a float32 handle's)
  (b) the distances, counts, maxima and sums are within diag_ref's bounds
  (c) the device entry point returns the host entry point's bits
  (d) a second call returns the same bits
  (e) sum_k sum_k / n agrees with quantization_error to 1e-12
  (f) on an exact handle whose screen serves, every call advances qe_stats() by n rows: the fast path served it."""
import ctypes as C

import numpy as np
import pytest

from tests import diag_ref as R
from tests import query_ref as Q

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def engine(X, Y, D, **kw):
    from xpysom_dask_amd.engine import HipEngine
    return HipEngine(X, Y, D, **kw)


def _device_rows(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, F32)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, "%s: %s %r against %s %r" % (what, a.dtype, a.shape, b.dtype, b.shape)
    bad = np.flatnonzero(_bits(a) != _bits(b))
    assert len(bad) == 0, "%s: %d entries differ, first at %d: %r against %r" % (what, len(bad), bad[0], a[bad[0]], b[bad[0]])


@pytest.fixture
def env_of(monkeypatch):
    def set_env(c):
        monkeypatch.delenv("SOM_EXACT_SKIP", raising=False)
        for k, v in c["env"].items():
            monkeypatch.setenv(k, v)
    return set_env


@pytest.mark.parametrize("c", R.CASES, ids=[c["id"] for c in R.CASES])
def test_diag_case(c, env_of):
    env_of(c)
    X, Y, D, n = c["X"], c["Y"], c["D"], c["n"]
    K, masked, what = X * Y, bool(c["missing"]), c["id"]
    x, w0 = R.case_data(c)
    kw = dict(precision=c["prec"])
    if masked:
        kw["missing"] = c["missing"]
    e = engine(X, Y, D, **kw)
    try:
        e.set_weights(w0)
        w = e.get_weights()
        t = _device_rows(x)
        fast = Q.is_exact(X, Y, D, c["prec"], "euclidean") and not masked
        served = [e.qe_stats()[0]] if fast else None

        def advanced(call):                                 # (f)
            if fast:
                served.append(e.qe_stats()[0])
                assert served[-1] - served[-2] == n, "%s: %s advanced qe_stats by %d rows, not %d" % (
                    what, call, served[-1] - served[-2], n)

        ids, d = e.bmu_distances(x)
        advanced("bmu_distances")
        assert ids.dtype == np.int32 and ids.shape == (n,)
        # (a)
        want_ids = e.bmu(x, quantization=True)
        _same_bits(ids, want_ids, what + " ids against som_bmu QUANTIZATION")
        if c["prec"] == "exact":
            f = engine(X, Y, D, **dict(kw, precision="f32"))
            try:
                f.set_weights(w0)
                _same_bits(ids, f.bmu(x, quantization=True), what + " ids against a float32 handle's")
            finally:
                f.close()
        # (b) the distances
        worst_d = R.check_distances(d, x, w, ids, masked=masked, what=what)
        if c["data"] == "weights":
            assert (d == 0).all(), "%s: rows that are units must be at distance 0 exactly" % what
        if c["data"] == "int":
            s, _ = Q.scores(x, w, "sqrt")
            Q.check_ties(ids, s, what)                        # NumPy's first argmin; duplicate units go to the lowest id
            sq = ((x.astype(F64) - w.astype(F64)[ids]) ** 2).sum(axis=1)
            _same_bits(d, np.sqrt(sq.astype(F32)), what + " distances against the rounded sqrt of the integer")
        if masked:
            assert ids[0] == 0 and d[0] == 0, "%s: a row with nothing observed has unit 0 and distance 0" % what
        # (b) the per-unit statistics
        st = e.unit_stats(x)
        advanced("unit_stats")
        print("%s: worst err / bound of the distances %.3g, of the unit sums %.3g" % (
            what, worst_d, R.check_unit_stats(st, ids, d, K, what=what)))
        if c["data"] == "three":
            assert (st[0] > 1000).sum() == 3 and (st[0] == 0).sum() == K - 3
        if K >= 8192:                                       # both sorts at scale: thousands of segments beside thousands of empty units
            assert (st[0] > 0).sum() > 1000 and (st[0] == 0).sum() > 3000, "%s: %d units with rows" % (what, (st[0] > 0).sum())
        # (c)
        ids_dev, d_dev = e.bmu_distances_device(t.data_ptr(), n)
        advanced("bmu_distances_device")
        _same_bits(ids_dev, ids, what + " device ids")
        _same_bits(d_dev, d, what + " device distances")
        st_dev = e.unit_stats_device(t.data_ptr(), n)
        advanced("unit_stats_device")
        for name, a, b in zip(("count", "sum", "sumsq", "max"), st_dev, st):
            _same_bits(a, b, "%s device %s" % (what, name))
        # (d)
        ids2, d2 = e.bmu_distances(x)
        advanced("bmu_distances again")
        _same_bits(ids2, ids, what + " second call ids")
        _same_bits(d2, d, what + " second call distances")
        for name, a, b in zip(("count", "sum", "sumsq", "max"), e.unit_stats_device(t.data_ptr(), n), st):
            _same_bits(a, b, "%s second call %s" % (what, name))
        advanced("unit_stats_device again")
        assert e.unit_sort_stats() == ((3, 0) if R.sort_path(c) == "counting" else (0, 3)), "%s: not the sort the rule names" % what
        # (e)
        R.check_qe_agreement(st[1], n, e.quantization_error(x), what)
    finally:
        e.close()


def test_c_abi_refusals_and_no_rows():
    from xpysom_dask_amd.engine import SomHipError
    X, Y, D = 5, 7, 3
    K = X * Y
    e = engine(X, Y, D, precision="f32")
    try:
        lib, h = e._lib, e._h
        e.set_weights(np.random.RandomState(0).normal(0, 1, (K, D)).astype(F32))
        x = np.random.RandomState(1).normal(0, 1, (9, D)).astype(F32)
        t = _device_rows(x)
        ids, d = np.full(9, -7, np.int32), np.full(9, -7, F32)
        cnt, tot, sq, mx = np.full(K, -7, np.int64), np.full(K, -7.0), np.full(K, -7.0), np.full(K, -7, F32)
        ip, fp = e._ip, e._fp
        lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        dev = C.c_void_p(t.data_ptr())

        def refused(rc, msg):
            assert rc != 0
            assert lib.som_last_error(h).decode() == msg

        # no rows: distances touch nothing, the statistics are K zeros -- whatever the row pointer
        assert lib.som_bmu_distances(h, None, 0, ip(ids), fp(d)) == 0
        assert lib.som_bmu_distances_device(h, None, 0, ip(ids), fp(d)) == 0
        assert (ids == -7).all() and (d == -7).all()
        for fn in (lib.som_unit_stats, lib.som_unit_stats_device):
            cnt[:], tot[:], sq[:], mx[:] = -7, -7, -7, -7
            assert fn(h, None, 0, lp(cnt), dp(tot), dp(sq), fp(mx)) == 0
            assert not cnt.any() and not tot.any() and not sq.any() and not mx.any()
        # refusals
        refused(lib.som_bmu_distances(h, fp(x), -1, ip(ids), fp(d)), "som_bmu_distances: bad argument")
        refused(lib.som_bmu_distances_device(h, dev, -1, ip(ids), fp(d)), "som_bmu_distances_device: bad argument")
        refused(lib.som_bmu_distances(h, None, 9, ip(ids), fp(d)), "som_bmu_distances: bad argument")
        refused(lib.som_bmu_distances_device(h, None, 9, ip(ids), fp(d)), "som_bmu_distances_device: bad argument")
        refused(lib.som_bmu_distances(h, fp(x), 9, None, None), "som_bmu_distances: bad argument")
        refused(lib.som_bmu_distances_device(h, dev, 9, None, None), "som_bmu_distances_device: bad argument")
        refused(lib.som_bmu_distances_device(h, dev, 2 ** 31, ip(ids), fp(d)), "som_bmu_distances_device: more than 2^31-1 rows in one call")
        refused(lib.som_unit_stats(h, fp(x), -1, lp(cnt), dp(tot), dp(sq), fp(mx)), "som_unit_stats: bad argument")
        refused(lib.som_unit_stats_device(h, dev, -1, lp(cnt), dp(tot), dp(sq), fp(mx)), "som_unit_stats_device: bad argument")
        refused(lib.som_unit_stats(h, None, 9, lp(cnt), dp(tot), dp(sq), fp(mx)), "som_unit_stats: bad argument")
        refused(lib.som_unit_stats_device(h, None, 9, lp(cnt), dp(tot), dp(sq), fp(mx)), "som_unit_stats_device: bad argument")
        refused(lib.som_unit_stats(h, fp(x), 9, None, dp(tot), dp(sq), fp(mx)), "som_unit_stats: bad argument")
        refused(lib.som_unit_stats(h, fp(x), 9, lp(cnt), dp(tot), dp(sq), None), "som_unit_stats: bad argument")
        refused(lib.som_unit_stats_device(h, dev, 2 ** 31, lp(cnt), dp(tot), dp(sq), fp(mx)),
                "som_unit_stats_device: more than 2^31-1 rows in one call")
        assert (ids == -7).all() and (d == -7).all()
        with pytest.raises(ValueError):
            e.bmu_distances(np.zeros((4, D + 1), F32))
        with pytest.raises(ValueError):
            e.unit_stats(np.zeros((4, D + 1), F32))
        # one output of the pair may be NULL; the handle is still good after the refusals
        want_ids, want_d = e.bmu_distances(x)
        assert lib.som_bmu_distances(h, fp(x), 9, ip(ids), None) == 0
        assert lib.som_bmu_distances_device(h, dev, 9, None, fp(d)) == 0
        _same_bits(ids, want_ids, "ids alone")
        _same_bits(d, want_d, "distances alone")
        assert lib.som_unit_stats(h, fp(x), 9, lp(cnt), dp(tot), dp(sq), fp(mx)) == 0
        R.check_unit_stats((cnt, tot, sq, mx), want_ids, want_d, K)
        assert isinstance(SomHipError("x"), RuntimeError)
    finally:
        e.close()


def test_xpysom_host_chunks_equal_device_rows():
    from xpysom_dask_amd import UnitStatistics, XPySom
    X, Y, D, n = 12, 11, 33, 300
    x = Q.make_rows("blobs", n, D, 11)
    som = XPySom(X, Y, D, random_seed=4, n_parallel=97, precision="f32")
    som._weights = Q.make_units("blobs", x, X * Y, D, 11).reshape(X, Y, D)
    t = _device_rows(x)
    ids, d = som.quantization_distances(x)                  # four chunks: 97, 97, 97, 9
    ids_dev, d_dev = som.quantization_distances(t)
    assert ids.dtype == np.int64 and d.dtype == F32
    _same_bits(ids, ids_dev, "ids of host chunks against device rows")
    _same_bits(d, d_dev, "distances of host chunks against device rows")
    np.testing.assert_array_equal(ids, som.predict(x))
    host, dev = som.unit_statistics(x), som.unit_statistics(t)
    assert isinstance(host, UnitStatistics) and isinstance(dev, UnitStatistics)
    for st in (host, dev):
        assert st.hits.shape == st.sum.shape == st.sumsq.shape == st.max.shape == (X, Y)
        assert st.hits.sum() == n
        R.check_unit_stats((st.hits.reshape(-1), st.sum.reshape(-1), st.sumsq.reshape(-1), st.max.reshape(-1)), ids, d, X * Y)
        assert np.array_equal(np.isnan(st.mean), st.hits == 0) and np.array_equal(np.isnan(st.std), st.hits == 0)
        mean, std = R.mean_std(st.hits, st.sum, st.sumsq)
        np.testing.assert_array_equal(st.mean[st.hits > 0], mean[st.hits > 0])
        np.testing.assert_array_equal(st.std[st.hits > 0], std[st.hits > 0])
    np.testing.assert_array_equal(host.hits, dev.hits)
    _same_bits(host.max, dev.max, "max of host chunks against device rows")
    one_ids, one_d = som.quantization_distances(x[7])      # a 1-D row is one sample
    assert one_ids.shape == (1,) and one_ids[0] == ids[7] and one_d[0] == d[7]
    with pytest.raises(ValueError, match="Received %d features, expected %d" % (D - 1, D)):
        som.unit_statistics(x[:, :-1])
    # missing='nan': both methods are defined (over the observed features)
    xm = x.copy()
    xm[np.random.RandomState(2).random_sample(xm.shape) < 0.3] = np.nan
    xm[5] = np.nan
    msom = XPySom(X, Y, D, random_seed=4, n_parallel=97, precision="f32", missing="nan")
    msom._weights = som._weights.copy()
    mids, md = msom.quantization_distances(xm)
    R.check_distances(md, xm, msom._weights.reshape(X * Y, D), mids, masked=True, what="missing='nan'")
    assert mids[5] == 0 and md[5] == 0
    mst = msom.unit_statistics(_device_rows(xm))
    mids_dev, md_dev = msom.quantization_distances(_device_rows(xm))
    _same_bits(mids, mids_dev, "masked ids")
    _same_bits(md, md_dev, "masked distances")
    R.check_unit_stats((mst.hits.reshape(-1), mst.sum.reshape(-1), mst.sumsq.reshape(-1), mst.max.reshape(-1)), mids, md, X * Y)


def test_a_nan_row_without_missing_poisons_only_its_unit():
    X, Y, D, n = 5, 7, 3, 127
    K = X * Y
    x = Q.make_rows("blobs", n, D, 21)
    w0 = Q.make_units("blobs", x, K, D, 21)
    bad = 50
    xn = x.copy()
    xn[bad, 1] = np.nan
    e = engine(X, Y, D, precision="f32")
    try:
        e.set_weights(w0)
        clean_ids, clean_d = e.bmu_distances(x)
        clean = e.unit_stats(x)
        ids, d = e.bmu_distances(xn)
        _same_bits(ids, e.bmu(xn, quantization=True), "ids with a NaN row")
        assert np.array_equal(np.flatnonzero(np.isnan(d)), [bad])
        others = np.arange(n) != bad
        _same_bits(ids[others], clean_ids[others], "ids of the other rows")
        _same_bits(d[others], clean_d[others], "distances of the other rows")
        st = e.unit_stats(xn)
        R.check_unit_stats(st, ids, d, K, what="NaN row")
        k = int(ids[bad])
        assert np.isnan(st[1][k]) and np.isnan(st[2][k])
        np.testing.assert_array_equal(st[0], np.bincount(ids, minlength=K))
        assert np.array_equal(np.flatnonzero(np.isnan(st[1])), [k]) and np.array_equal(np.flatnonzero(np.isnan(st[2])), [k])
        rest = np.ones(K, bool)
        rest[[k, int(clean_ids[bad])]] = False                # (the row may have changed units: both are affected)
        for name, a, b in zip(("count", "sum", "sumsq", "max"), st, clean):
            _same_bits(a[rest], b[rest], "%s of the units without the NaN row" % name)
    finally:
        e.close()
