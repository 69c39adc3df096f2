"""The label and value maps on the device -- som_unit_label_counts / som_unit_value_sums and XPySom.label_counts / unit_means /
classify -- against the float64 model and the bound of tests/project_ref.py.  GPU only (`-m gpu`).

Every case is teacher-forced: set a codebook, query rows, compare with the model computed from e.bmu(x) of the same handle.
Every case runs through the host and the device entry point and checks
  (a) the counts equal the model's exactly
  (b) the sums pass project_ref.check_value_sums
  (c) the device entry point returns the host entry point's bits
  (d) a second call returns the same bits.
The shapes are the smallest that cross each boundary of the two kernels (csrc/project.hpp): one row, odd sizes, a full wave of
columns, one over, two column blocks and a tail, the widest row-slot layouts (1 and 2 columns), segments of more than a thousand
rows beside thousands of empty units, one segment holding every row, and every kind of search the ids can come from."""
import ctypes as C

import numpy as np
import pytest

from tests import diag_ref as R
from tests import project_ref as P
from tests import query_ref as Q
from tests import update_ref as U

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def engine(X, Y, D, **kw):
    from xpysom_dask_amd.engine import HipEngine
    return HipEngine(X, Y, D, **kw)


def _dev(a, dtype=F32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, "%s: %s %r against %s %r" % (what, a.dtype, a.shape, b.dtype, b.shape)
    bad = np.argwhere(_bits(a) != _bits(b))
    assert len(bad) == 0, "%s: %d entries differ, first at %r: %r against %r" % (what, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


# ------------------------------------------------------------------------------------------------------ the cases
def _case(X, Y, D, n, C, prec="f32", data="blobs", distance="euclidean", missing=None, tag=""):
    c = dict(X=X, Y=Y, D=D, n=n, C=C, prec=prec, data=data, distance=distance, missing=missing)
    c["id"] = "%dx%dx%d-n%d-C%d-%s-%s%s%s%s" % (X, Y, D, n, C, prec, data, "-cosine" if distance == "cosine" else "",
                                              "-nan" if missing else "", tag)
    return c


CASES = (
    [_case(5, 7, 3, 1, 1),                                  # one row, 34 empty units
     _case(5, 7, 3, 127, 3)]                                # odd everything
    + [_case(12, 11, 65, 300, C) for C in (63, 64, 65, 130)]     # a full wave of columns, one over, two blocks and a tail
    + [_case(12, 11, 65, 300, C) for C in (1, 2)]           # the widest row-slot layouts
    + [_case(64, 64, 32, 5000, 5, prec="exact", data="three")]   # three segments of > 1000 rows, 4093 empty units
    + [_case(5, 7, 3, 20000, C, data="one") for C in (1, 7)]     # one segment holds every row
    + [_case(12, 11, 9, 300, 4, data="scaled", distance="cosine")]     # the ACTIVATION ids, not the quantization ids
    + [_case(12, 11, 33, 300, 6, prec=prec, missing="nan") for prec in ("f32", "exact")]
    + [_case(12, 11, 65, 300, 5, prec="bf16")]
    + [_case(5, 7, 3, 127, 4, data="blobs", tag="-holes")]  # values: 30 % NaN, an all-NaN column, an all-NaN row, a +Inf
    #                                                         labels: -1 and >= C mixed in
    # behind both sorts at scale: K = 8 256 (radix, 14 key bits) and K = 8 192 = CS_MAX_K (the counting sort's ceiling)
    + [_case(129, 64, 4, 5000, 3), _case(128, 64, 4, 5000, 3)]
    + [_case(5, 7, 3, 70000, 2, data="one")]                # one segment of 70 000 rows, 32 row slots x 2 columns: the longest walk
)
HOLES = next(c for c in CASES if c["id"].endswith("-holes"))


def case_data(c):
    """(rows, codebook, labels int32 (n,), values float32 (n, C)) of a case."""
    X, Y, D, n, C = c["X"], c["Y"], c["D"], c["n"], c["C"]
    K = X * Y
    d = R._case(X, Y, D, n, prec=c["prec"], data=c["data"] if c["data"] in ("blobs", "three") else "blobs", missing=c["missing"])
    x, w = R.case_data(d)
    rs = np.random.RandomState(R.case_seed(d) + 7 * C)
    if c["data"] == "one":
        x = np.ascontiguousarray(np.repeat(w[17:18], n, axis=0))
    elif c["data"] == "scaled":                             # un-normalised rows: the cosine's unit is not the nearest one
        x = (x * rs.uniform(0.05, 20.0, (n, 1))).astype(F32)
    labels = rs.randint(0, C, n).astype(np.int32)
    values = rs.normal(0, 10, (n, C)).astype(F32)
    if c["id"].endswith("-holes"):
        labels = rs.randint(-1, C + 2, n).astype(np.int32)
        labels[3], labels[4] = -9, 2 ** 31 - 1
        values[rs.random_sample(values.shape) < 0.3] = np.nan
        values[:, 1] = np.nan
        values[6] = np.nan
        values[9, 0] = np.inf
        values[10, 2], values[11, 2] = 3e38, 3e38           # float32's largest magnitudes: their squares still fit a double
    return x, w, labels, values


def test_case_list_covers_the_issue_table():
    assert len({c["id"] for c in CASES}) == len(CASES) == 2 + 4 + 2 + 1 + 2 + 1 + 2 + 1 + 1 + 2 + 1
    assert {(c["X"], c["Y"], c["D"], c["n"], c["C"]) for c in CASES} >= {
        (5, 7, 3, 1, 1), (5, 7, 3, 127, 3), (12, 11, 65, 300, 63), (12, 11, 65, 300, 64), (12, 11, 65, 300, 65),
        (12, 11, 65, 300, 130), (12, 11, 65, 300, 1), (12, 11, 65, 300, 2), (64, 64, 32, 5000, 5), (5, 7, 3, 20000, 1),
        (5, 7, 3, 20000, 7), (129, 64, 4, 5000, 3), (128, 64, 4, 5000, 3), (5, 7, 3, 70000, 2)}
    sorts = {c["X"] * c["Y"]: R.sort_path(c) for c in CASES if c["n"] == 5000 and c["D"] == 4}
    assert sorts == {8256: "radix", 8192: "counting"}       # (the threshold cannot move the cases quietly)
    for c in CASES:
        assert "sort." + R.sort_path(c) in U.update_paths(c["X"], c["Y"], c["D"], "gaussian", "rectangular", False, c["n"]), c["id"]
    assert [c["data"] for c in CASES if c["n"] == 70000] == ["one"]
    assert {c["prec"] for c in CASES if c["missing"]} == {"f32", "exact"}
    assert any(c["prec"] == "bf16" for c in CASES) and any(c["distance"] == "cosine" for c in CASES)
    x, _w, labels, values = case_data(HOLES)
    assert np.isnan(values[:, 1]).all() and np.isnan(values[6]).all() and np.isinf(values).sum() == 1
    assert 0.2 < np.isnan(values).mean() < 0.6 and (labels < 0).any() and (labels >= HOLES["C"]).any()


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_project_case(c, monkeypatch):
    monkeypatch.delenv("SOM_EXACT_SKIP", raising=False)
    X, Y, D, n, Cc = c["X"], c["Y"], c["D"], c["n"], c["C"]
    K, what = X * Y, c["id"]
    x, w0, labels, values = case_data(c)
    kw = dict(precision=c["prec"], distance=c["distance"])
    if c["missing"]:
        kw["missing"] = c["missing"]
    e = engine(X, Y, D, **kw)
    try:
        e.set_weights(w0)
        ids = e.bmu(x)
        if c["distance"] == "cosine":                       # the data must tell the two searches apart
            assert (ids != e.bmu(x, quantization=True)).any(), "%s: the cosine and the Euclidean units agree on every row" % what
        if c["data"] == "one":
            assert (ids == ids[0]).all()
        if c["data"] == "three":
            seg = np.bincount(ids, minlength=K)
            assert (seg > 1000).sum() == 3 and (seg == 0).sum() == K - 3
        if K >= 8192:                                       # both sorts at scale: thousands of segments, thousands of empty units
            seg = np.bincount(ids, minlength=K)
            assert (seg > 0).sum() > 1000 and (seg == 0).sum() > 3000, "%s: %d units with rows" % (what, (seg > 0).sum())
        if c["missing"]:
            assert np.isnan(x[0]).all() and 0.25 < np.isnan(x).mean()
        tx, tl, tv = _dev(x), _dev(labels, np.int32), _dev(values)
        # (a)
        counts = e.label_counts(x, labels, Cc)
        assert counts.dtype == np.int64 and counts.shape == (K, Cc)
        want = P.label_counts_model(ids, labels, K, Cc)
        assert np.array_equal(counts, want), "%s: label counts differ from the model at %r" % (what, np.argwhere(counts != want)[:5].tolist())
        assert counts.sum() == ((labels >= 0) & (labels < Cc)).sum()
        # (b)
        sums = e.value_sums(x, values)
        print("%s: worst err / bound of the sums %.3g" % (what, P.check_value_sums(sums, ids, values, K, what=what)))
        # (c)
        _same_bits(e.label_counts_device(tx.data_ptr(), tl.data_ptr(), n, Cc), counts, what + " device label counts")
        sums_dev = e.value_sums_device(tx.data_ptr(), tv.data_ptr(), n, Cc)
        for name, a, b in zip(("count", "sum", "sumsq"), sums_dev, sums):
            _same_bits(a, b, "%s device %s" % (what, name))
        # (d)
        _same_bits(e.label_counts(x, labels, Cc), counts, what + " second call label counts")
        _same_bits(e.label_counts_device(tx.data_ptr(), tl.data_ptr(), n, Cc), counts, what + " second device call label counts")
        for second in (e.value_sums(x, values), e.value_sums_device(tx.data_ptr(), tv.data_ptr(), n, Cc)):
            for name, a, b in zip(("count", "sum", "sumsq"), second, sums):
                _same_bits(a, b, "%s second call %s" % (what, name))
        assert e.unit_sort_stats() == ((8, 0) if R.sort_path(c) == "counting" else (0, 8)), "%s: not the sort the rule names" % what
    finally:
        e.close()


def test_c_abi_refusals_and_no_rows():
    X, Y, D, n, Cc = 5, 7, 3, 9, 3
    K = X * Y
    e = engine(X, Y, D, precision="f32")
    big = engine(129, 128, 2, precision="f32")              # 16 512 units: x * y * 4096 > 2^26
    try:
        lib, h = e._lib, e._h
        e.set_weights(np.random.RandomState(0).normal(0, 1, (K, D)).astype(F32))
        x = np.random.RandomState(1).normal(0, 1, (n, D)).astype(F32)
        labels = (np.arange(n) % Cc).astype(np.int32)
        values = np.random.RandomState(2).normal(0, 1, (n, Cc)).astype(F32)
        tx, tl, tv = _dev(x), _dev(labels, np.int32), _dev(values)
        cnt, tot, sq = np.full((K, Cc), -7, np.int64), np.full((K, Cc), -7.0), np.full((K, Cc), -7.0)
        ip, fp = e._ip, e._fp
        lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        vp = lambda t: C.c_void_p(t.data_ptr())

        def refused(rc, msg, handle=h):
            assert rc != 0
            assert lib.som_last_error(handle).decode() == msg

        # no rows: zeros, whatever the row pointers
        for fn in (lib.som_unit_label_counts, lib.som_unit_label_counts_device):
            cnt[:] = -7
            assert fn(h, None, None, 0, Cc, lp(cnt)) == 0
            assert not cnt.any()
        for fn in (lib.som_unit_value_sums, lib.som_unit_value_sums_device):
            cnt[:], tot[:], sq[:] = -7, -7, -7
            assert fn(h, None, None, 0, Cc, lp(cnt), dp(tot), dp(sq)) == 0
            assert not cnt.any() and not tot.any() and not sq.any()
        cnt[:], tot[:], sq[:] = -7, -7, -7
        # the label counts
        for name, fn, rows, lab in (("som_unit_label_counts", lib.som_unit_label_counts, fp(x), ip(labels)),
                                    ("som_unit_label_counts_device", lib.som_unit_label_counts_device, vp(tx), vp(tl))):
            refused(fn(h, None, lab, n, Cc, lp(cnt)), name + ": bad argument")
            refused(fn(h, rows, None, n, Cc, lp(cnt)), name + ": bad argument")
            refused(fn(h, rows, lab, n, Cc, None), name + ": bad argument")
            refused(fn(h, rows, lab, -1, Cc, lp(cnt)), name + ": bad argument")
            refused(fn(h, rows, lab, n, 0, lp(cnt)), name + ": n_classes must be between 1 and 4096")
            refused(fn(h, rows, lab, n, 4097, lp(cnt)), name + ": n_classes must be between 1 and 4096")
            refused(fn(h, rows, lab, 2 ** 31, Cc, lp(cnt)), name + ": more than 2^31-1 rows in one call")
            refused(fn(big._h, rows, lab, n, 4096, lp(cnt)), name + ": x * y * n_classes exceeds 2^26 (analysis call: fewer columns at a time)",
                    big._h)
        # the value sums
        for name, fn, rows, val in (("som_unit_value_sums", lib.som_unit_value_sums, fp(x), fp(values)),
                                    ("som_unit_value_sums_device", lib.som_unit_value_sums_device, vp(tx), vp(tv))):
            out = (lp(cnt), dp(tot), dp(sq))
            refused(fn(h, None, val, n, Cc, *out), name + ": bad argument")
            refused(fn(h, rows, None, n, Cc, *out), name + ": bad argument")
            for hole in range(3):
                refused(fn(h, rows, val, n, Cc, *[None if i == hole else o for i, o in enumerate(out)]), name + ": bad argument")
            refused(fn(h, rows, val, -1, Cc, *out), name + ": bad argument")
            refused(fn(h, rows, val, n, 0, *out), name + ": n_cols must be between 1 and 4096")
            refused(fn(h, rows, val, n, 4097, *out), name + ": n_cols must be between 1 and 4096")
            refused(fn(h, rows, val, 2 ** 31, Cc, *out), name + ": more than 2^31-1 rows in one call")
            refused(fn(big._h, rows, val, n, 4096, *out), name + ": x * y * n_cols exceeds 2^26 (analysis call: fewer columns at a time)", big._h)
        assert (cnt == -7).all() and (tot == -7).all() and (sq == -7).all()          # a refused call writes nothing
        for call in (lambda: e.label_counts(np.zeros((4, D + 1), F32), np.zeros(4, np.int32), Cc),
                     lambda: e.label_counts(x, labels[:-1], Cc), lambda: e.label_counts(x, labels, 0),
                     lambda: e.value_sums(np.zeros((4, D + 1), F32), np.zeros((4, 2), F32)),
                     lambda: e.value_sums(x, values[:-1]), lambda: e.value_sums(x, values[:, :0])):
            with pytest.raises(ValueError):
                call()
        # the handle is still good: the next calls are correct, through both entry points
        ids = e.bmu(x)
        want = P.label_counts_model(ids, labels, K, Cc)
        assert lib.som_unit_label_counts(h, fp(x), ip(labels), n, Cc, lp(cnt)) == 0
        assert np.array_equal(cnt, want)
        cnt[:] = -7
        assert lib.som_unit_label_counts_device(h, vp(tx), vp(tl), n, Cc, lp(cnt)) == 0
        assert np.array_equal(cnt, want)
        assert lib.som_unit_value_sums_device(h, vp(tx), vp(tv), n, Cc, lp(cnt), dp(tot), dp(sq)) == 0
        P.check_value_sums((cnt, tot, sq), ids, values, K)
        host = e.value_sums(x, values)
        for a, b in zip(host, (cnt, tot, sq)):
            _same_bits(a, b, "host against device after the refusals")
    finally:
        e.close()
        big.close()


def test_unit_stats_keeps_its_bits_around_label_counts():
    """som_unit_stats and the label / value calls share the sort's buffers and the segment starts: neither disturbs the other."""
    X, Y, D, n, Cc = 12, 11, 33, 300, 5
    K = X * Y
    x = Q.make_rows("blobs", n, D, 31)
    labels = np.random.RandomState(5).randint(0, Cc, n).astype(np.int32)
    values = np.random.RandomState(6).normal(0, 1, (n, Cc)).astype(F32)
    e = engine(X, Y, D, precision="f32", distance="cosine")  # (the two calls sort by DIFFERENT ids on this handle)
    try:
        e.set_weights(Q.make_units("blobs", x, K, D, 31))
        before = e.unit_stats(x)
        counts = e.label_counts(x, labels, Cc)
        after = e.unit_stats(x[:200])                       # ... and fewer rows in between
        sums = e.value_sums(x, values)
        again = e.unit_stats(x)
        for name, a, b in zip(("count", "sum", "sumsq", "max"), before, again):
            _same_bits(a, b, "unit_stats %s after label_counts and value_sums" % name)
        ids, d = e.bmu_distances(x)
        R.check_unit_stats(again, ids, d, K)
        R.check_unit_stats(after, ids[:200], d[:200], K)
        act = e.bmu(x)
        assert np.array_equal(counts, P.label_counts_model(act, labels, K, Cc))
        assert np.array_equal(e.label_counts(x, labels, Cc), counts)
        P.check_value_sums(sums, act, values, K)
    finally:
        e.close()


def test_xpysom_device_rows_and_labels():
    from xpysom_dask_amd import UnitMeans, XPySom
    X, Y, D, n, Cc = 12, 11, 33, 300, 4
    x = Q.make_rows("blobs", n, D, 11)
    labels = np.random.RandomState(3).randint(0, Cc, n)
    som = XPySom(X, Y, D, random_seed=4, n_parallel=97, precision="f32")
    som._weights = Q.make_units("blobs", x, X * Y, D, 11).reshape(X, Y, D)
    tx, tl = _dev(x), _dev(labels, np.int32)
    lm = som.labels_map(x, labels)                          # the host's Counters
    want = np.zeros((X, Y, Cc), np.int64)
    for (i, j), counter in lm.items():
        for c, m in counter.items():
            want[i, j, c] = m
    dev = som.label_counts(tx, tl, n_classes=Cc)
    assert dev.dtype == np.int64 and dev.shape == (X, Y, Cc)
    np.testing.assert_array_equal(dev, want)
    np.testing.assert_array_equal(som.label_counts(x, labels), want)           # four host chunks: 97, 97, 97, 9
    np.testing.assert_array_equal(som.label_counts(tx, labels, n_classes=Cc), want)      # host labels beside device rows
    with pytest.raises(ValueError, match="n_classes is required"):
        som.label_counts(tx, tl)
    with pytest.raises(ValueError, match="data and labels must have the same length."):
        som.label_counts(tx, tl[:-1], n_classes=Cc)
    with pytest.raises(ValueError, match="need data in device memory"):
        som.label_counts(x, tl, n_classes=Cc)
    # classify on the training rows: the host rule applied to predict
    ids = som.predict(x)
    got = som.classify(tx, dev)
    np.testing.assert_array_equal(got, P.classify_model(ids, want))
    np.testing.assert_array_equal(som.classify(x, dev), got)
    assert (got == labels).mean() > 1.0 / Cc                # (better than chance on its own training rows)
    # unit_means: device rows whole, host rows in chunks
    values = np.random.RandomState(8).normal(0, 5, (n, 3)).astype(F32)
    values[np.random.RandomState(9).random_sample(values.shape) < 0.3] = np.nan
    um_dev, um_host = som.unit_means(tx, _dev(values)), som.unit_means(x, values)
    assert isinstance(um_dev, UnitMeans) and um_dev.count.shape == (X, Y, 3)
    for um in (um_dev, um_host, som.unit_means(tx, values)):
        P.check_value_sums((um.count.reshape(-1, 3), um.sum.reshape(-1, 3), um.sumsq.reshape(-1, 3)), ids, values, X * Y)
        assert np.array_equal(np.isnan(um.mean), um.count == 0)
    np.testing.assert_array_equal(um_dev.count, um_host.count)
