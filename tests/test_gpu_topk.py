"""The k nearest units on the device -- som_bmu_topk / som_bmu_topk_device, som_unit_rank_counts*, XPySom.nearest_units / rank_hits /
smoothed_hits -- against the oracle and the checks of tests/topk_ref.py.  GPU only (`-m gpu`).

Rows and units come from query_ref's generators with seed 3 (topk_ref.CASES: the smallest shapes that reach each tail of the
128 x 128 x 32 tiling); every check runs for k in 1, 2, 3, 4, 5, 8 (both instances of the kernel, with spare slots and full).
  exact       ids == topk_lowest(activate(x), k) and the scores == the gathered entries of activate(x), bit for bit, on 'euclidean',
              'euclidean_no_opt' and 'cosine' handles (activate() is existing code, pinned to float64 by test_gpu_query_ref.py); on
              integer data ids == the stable argsort of the exact integer scores; duplicate units: the lower id first
  float64     check_topk passes (the worst err/bound is printed); on the rows the bounds pin, ids == the float64 order
  distances   every filled slot within gamma(D + 10) relative of the float64 distance; column 0 == quantization_distances' bits
              where the two ids agree
  slot 0      == predict(x) on precision 'f32' and 'exact'
  geometry    SOM_TOPK_PARTS = 1, 3, 64 identical; a second call identical; a k = 3 call == the first columns of the k = 8 call;
              more rows than one pass holds
  rows        NaN rows, a NaN feature, all but three units infinite
  entries     host == device rows through the C ABI and through nearest_units; n_parallel chunks; rank_hits == bincount of
              nearest_units' columns; rank_hits(x, 1)[0] == activation_response(x); smoothed_hits == topk_ref.sdh; refusals by name."""
import ctypes as C

import numpy as np
import pytest

from tests import query_ref as Q
from tests import topk_ref as T

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DISTANCES = ("euclidean", "euclidean_no_opt", "cosine")
ALL_CASES = T.CASES + T.TIE_CASES + [T.DUP_CASE]


def engine(X, Y, D, **kw):
    from xpysom_dask_amd.engine import HipEngine
    kw.setdefault("precision", "f32")
    return HipEngine(X, Y, D, **kw)


def _device_rows(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, F32)).cuda()


_REF = {}


def reference(c, distance):
    """(x, w, act, s, E) of a case under a distance: the float32 matrix activate() returns (existing code, through an engine of its
    own) and query_ref's float64 scores with their bounds -- computed once per session, shared, never written to."""
    key = (c["id"], distance)
    if key not in _REF:
        x, w = T.case_data(c)
        e = engine(c["X"], c["Y"], c["D"], distance=distance)
        try:
            e.set_weights(w)
            act = e.distance_matrix(x)
        finally:
            e.close()
        s, E = Q.scores(x, w, T.MODE_OF[distance])
        for a in (x, w, act, s, E):
            a.setflags(write=False)
        _REF[key] = (x, w, act, s, E)
    return _REF[key]


@pytest.mark.parametrize("distance", DISTANCES)
@pytest.mark.parametrize("c", ALL_CASES, ids=[c["id"] for c in ALL_CASES])
def test_lists_are_the_stable_argsort_of_activate(c, distance):
    x, w, act, s, E = reference(c, distance)
    e = engine(c["X"], c["Y"], c["D"], distance=distance)
    try:
        e.set_weights(w)
        for k in T.ks_of(c):
            ids, score, dist = e.bmu_topk(x, k)
            assert ids.dtype == np.int32 and ids.shape == (c["N"], k) and score.dtype == F32 and dist.dtype == F32
            want = T.topk_lowest(act, k)
            bad = np.flatnonzero((ids != want).any(axis=1))
            assert len(bad) == 0, "%s %s k=%d: %d rows differ from the stable argsort of activate(), first row %d: %s vs %s" % (
                c["id"], distance, k, len(bad), bad[0], ids[bad[0]].tolist(), want[bad[0]].tolist())
            assert T.same_bits_or_nan(score, T.gather(act, want)), "%s %s k=%d: scores are not activate()'s entries" % (c["id"], distance, k)
            assert (ids >= 0).all()                          # finite rows and units: every slot filled
    finally:
        e.close()


@pytest.mark.parametrize("c", T.TIE_CASES, ids=[c["id"] for c in T.TIE_CASES])
def test_integer_data_is_the_exact_stable_argsort(c):
    x, w = T.case_data(c)
    x64, w64 = x.astype(F64), w.astype(F64)
    exact = {"euclidean": (w64 * w64).sum(1)[None, :] - 2 * x64 @ w64.T}                     # integers: exact in float32 too
    exact["euclidean_no_opt"] = exact["euclidean"] + (x64 * x64).sum(1)[:, None]
    ties = int((np.sort(exact["euclidean"], axis=1)[:, 1:9] == np.sort(exact["euclidean"], axis=1)[:, :8]).sum())
    assert ties > c["N"]                                     # ties among the eight lowest of nearly every row
    for distance, sc in exact.items():
        e = engine(c["X"], c["Y"], c["D"], distance=distance)
        try:
            e.set_weights(w)
            for k in T.KS:
                ids, score, _ = e.bmu_topk(x, k, dist=False)
                want = np.argsort(sc, axis=1, kind="stable")[:, :k]
                assert np.array_equal(ids, want), "%s %s k=%d" % (c["id"], distance, k)
                assert np.array_equal(score.astype(F64), np.take_along_axis(sc, want, axis=1))
        finally:
            e.close()


def test_duplicate_units_list_the_lower_id_first():
    c = T.DUP_CASE
    x, w, act, s, E = reference(c, "euclidean")
    K = c["X"] * c["Y"]
    e = engine(c["X"], c["Y"], c["D"])
    try:
        e.set_weights(w)
        ids, score, _ = e.bmu_topk(x, 8, dist=False)
    finally:
        e.close()
    twin = {u: K - c["dup"] + u for u in range(c["dup"])}
    pairs = 0
    for n in range(c["N"]):
        row = ids[n].tolist()
        for j, u in enumerate(row):
            if u in twin and j + 1 < 8:                      # a duplicated unit not in the last slot: its twin follows it at once
                assert row[j + 1] == twin[u] and score[n, j] == score[n, j + 1], "row %d: %s" % (n, row)
                pairs += 1
            if u >= K - c["dup"]:                            # a twin: its original sits right in front of it
                assert j > 0 and row[j - 1] == u - (K - c["dup"]), "row %d: the twin %d without its original in front: %s" % (n, u, row)
    assert pairs > 100


@pytest.mark.parametrize("distance", DISTANCES)
@pytest.mark.parametrize("c", T.CASES, ids=[c["id"] for c in T.CASES])
def test_float64_admissible_and_pinned_rows(c, distance):
    x, w, act, s, E = reference(c, distance)
    e = engine(c["X"], c["Y"], c["D"], distance=distance)
    try:
        e.set_weights(w)
        worst = 0.0
        for k in T.ks_of(c):
            ids = e.bmu_topk(x, k, score=False, dist=False)[0].astype(np.int64)
            worst = max(worst, T.check_topk(ids, s, E, k, "%s %s k=%d" % (c["id"], distance, k)))
            pin = T.pinned_rows(s, E, k)
            want = np.argsort(s, axis=1, kind="stable")[:, :k]
            assert np.array_equal(ids[pin], want[pin]), "%s %s k=%d: a pinned row differs from the float64 order" % (c["id"], distance, k)
        print("%s %s: worst err/bound %.3g; %.1f %% of the rows pinned at k = %d" % (
            c["id"], distance, worst, 100 * pin.mean(), T.ks_of(c)[-1]))
    finally:
        e.close()


@pytest.mark.parametrize("c", T.CASES + [T.TIE_CASES[1]], ids=[c["id"] for c in T.CASES + [T.TIE_CASES[1]]])
def test_distances(c):
    x, w = T.case_data(c)
    x64, w64 = x.astype(F64), w.astype(F64)
    g = Q.gamma(c["D"] + 10)
    for distance in ("euclidean", "cosine"):
        e = engine(c["X"], c["Y"], c["D"], distance=distance)
        try:
            e.set_weights(w)
            qi, qd = e.bmu_distances(x)
            for k in (T.ks_of(c)[0], T.ks_of(c)[-1]):
                ids, _, dist = e.bmu_topk(x, k, score=False)
                ref = np.linalg.norm(x64[:, None, :] - w64[ids.astype(np.int64)], axis=2)
                err = np.abs(dist.astype(F64) - ref)
                assert (err <= g * ref).all(), "%s %s k=%d: a distance off by %.3g of its bound" % (
                    c["id"], distance, k, float((err / np.maximum(g * ref, 1e-300)).max()))
                agree = ids[:, 0] == qi
                if distance == "euclidean" and c["kind"] in ("blobs", "int"):
                    assert agree.mean() > 0.9                # (the two searches differ in |x|^2 and the sqrt: near-ties only)
                assert T.same_bits(dist[agree, 0], qd[agree]), "%s %s k=%d: column 0 is not quantization_distances' value" % (c["id"], distance, k)
        finally:
            e.close()


@pytest.mark.parametrize("precision", ("f32", "exact"))
@pytest.mark.parametrize("c", [T.CASES[2], T.CASES[3], T.CASES[4], T.TIE_CASES[0]], ids=lambda c: c["id"])
def test_slot_0_is_predict(c, precision):
    x, w = T.case_data(c)
    for distance in ("euclidean", "cosine"):
        e = engine(c["X"], c["Y"], c["D"], distance=distance, precision=precision)
        try:
            e.set_weights(w)
            bmu = e.bmu(x)
            for k in (1, 8):
                ids = e.bmu_topk(x, k, score=False, dist=False)[0]
                assert np.array_equal(ids[:, 0], bmu), "%s %s %s k=%d" % (c["id"], precision, distance, k)
        finally:
            e.close()


@pytest.mark.parametrize("c", [T.CASES[2], T.CASES[4]], ids=lambda c: c["id"])
def test_precision_does_not_matter(c):
    """Always float32: a bf16 handle and the default (exact) handle list what the f32 handle lists, bit for bit."""
    x, w = T.case_data(c)
    got = []
    for kw in (dict(precision="f32"), dict(precision="bf16"), dict(precision="exact")):
        e = engine(c["X"], c["Y"], c["D"], distance="cosine", **kw)       # (a distance every precision implements)
        try:
            e.set_weights(w)
            got.append(e.bmu_topk(x, 5))
        finally:
            e.close()
    for other in got[1:]:
        assert np.array_equal(other[0], got[0][0]) and T.same_bits(other[1], got[0][1]) and T.same_bits(other[2], got[0][2])


@pytest.mark.parametrize("c", [T.CASES[2], T.CASES[4], T.CASES[3]], ids=lambda c: c["id"])
def test_geometry_does_not_matter(c, monkeypatch):
    x, w, act, s, E = reference(c, "cosine")
    e = engine(c["X"], c["Y"], c["D"], distance="cosine")
    try:
        e.set_weights(w)
        monkeypatch.delenv("SOM_TOPK_PARTS", raising=False)
        base = {k: e.bmu_topk(x, k) for k in T.KS}
        assert np.array_equal(base[8][0], T.topk_lowest(act, 8))
        for k in T.KS:                                       # a shorter list: the first columns of the longest
            for a, b in zip(base[k], base[8]):
                assert np.array_equal(a.view(np.uint32), np.ascontiguousarray(b[:, :k]).view(np.uint32)), "%s: k=%d is not the head of k=8" % (c["id"], k)
        for parts in ("1", "3", "64"):
            monkeypatch.setenv("SOM_TOPK_PARTS", parts)
            for k in (3, 8):
                for a, b in zip(e.bmu_topk(x, k), base[k]):
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: SOM_TOPK_PARTS=%s changes the k=%d result" % (c["id"], parts, k)
            assert np.array_equal(e.unit_rank_counts(x, 8), np.stack([np.bincount(base[8][0][:, j], minlength=c["X"] * c["Y"]) for j in range(8)]))
        monkeypatch.delenv("SOM_TOPK_PARTS")
        for a, b in zip(e.bmu_topk(x, 8), base[8]):         # a second call
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finally:
        e.close()


def test_more_rows_than_one_pass():
    """Two passes (262 144 rows each at most) and a tail: the lists and the counts are those of the rows taken alone."""
    n, D, X, Y = T.PASS_ROWS + 333, 2, 1, 5
    rs = np.random.RandomState(11)
    x = rs.normal(0, 1, (n, D)).astype(F32)
    w = rs.normal(0, 1, (X * Y, D)).astype(F32)
    e = engine(X, Y, D, distance="euclidean_no_opt")
    try:
        e.set_weights(w)
        act = np.concatenate([e.distance_matrix(x[a:a + 65536]) for a in range(0, n, 65536)])
        want = T.topk_lowest(act, 3)
        ids, score, dist = e.bmu_topk(x, 3)
        assert np.array_equal(ids, want) and T.same_bits(score, T.gather(act, want))
        tail = e.bmu_topk(x[T.PASS_ROWS - 5:], 3)
        assert np.array_equal(tail[0], ids[T.PASS_ROWS - 5:]) and T.same_bits(tail[2], dist[T.PASS_ROWS - 5:])
        t = _device_rows(x)
        dev = e.bmu_topk_device(t.data_ptr(), n, 3)
        assert np.array_equal(dev[0], ids) and T.same_bits(dev[1], score) and T.same_bits(dev[2], dist)
        counts = e.unit_rank_counts_device(t.data_ptr(), n, 3)
        assert np.array_equal(counts, np.stack([np.bincount(ids[:, j], minlength=X * Y) for j in range(3)]))
        assert counts.sum() == 3 * n
    finally:
        e.close()


@pytest.mark.parametrize("distance", DISTANCES)
def test_rows_and_units_that_do_not_enter(distance):
    c = T.CASES[2]
    x, w = T.case_data(c)
    K = c["X"] * c["Y"]
    bad = x[:200].copy()
    bad[::4] = np.nan                                        # a row that is all NaN
    bad[1::4, 36] = np.nan                                   # a row with one NaN feature (the feature tail's)
    bad[2::4, 0] = np.nan
    rows = np.concatenate([x[:300], bad, x[300:]])
    e = engine(c["X"], c["Y"], c["D"], distance=distance)
    try:
        e.set_weights(w)
        act = e.distance_matrix(rows)
        for k in (2, 8):
            ids, score, dist = e.bmu_topk(rows, k)
            want = T.topk_lowest(act, k)
            assert np.array_equal(ids, want) and T.same_bits_or_nan(score, T.gather(act, want))
            # a distance is NaN where nothing is listed -- and where the row itself holds a NaN (cosine lists such a row)
            assert np.array_equal(np.isnan(dist), (ids < 0) | np.isnan(rows).any(axis=1)[:, None])
            nanrow = np.zeros(len(rows), bool)
            nanrow[300:500] = np.arange(200) % 4 != 3
            if distance != "cosine":                         # (cosine: nan_to_num turns the NaN quotient into score 1, as in activate)
                assert (ids[nanrow] == -1).all() and np.isnan(score[nanrow]).all() and np.isnan(dist[nanrow]).all()
            assert (ids[~nanrow] >= 0).all()
            clean = e.bmu_topk(np.concatenate([x[:300], x[300:]]), k)
            assert np.array_equal(np.concatenate([ids[:300], ids[500:]]), clean[0])      # a row reaches no other row's list
        # all but three units infinite: three scores below +inf
        w3 = w.copy()
        keep = [5, 130, 199]
        w3[[u for u in range(K) if u not in keep]] = np.inf
        e.set_weights(w3)
        act3 = e.distance_matrix(x)
        ids, score, dist = e.bmu_topk(x, 8)
        want = T.topk_lowest(act3, 8)
        assert np.array_equal(ids, want) and T.same_bits_or_nan(score, T.gather(act3, want))
        if distance != "cosine":
            assert (np.sort(ids[:, :3], axis=1) == np.array(keep)).all() and (ids[:, 3:] == -1).all()
            assert np.isnan(score[:, 3:]).all() and np.isnan(dist[:, 3:]).all() and np.isfinite(dist[:, :3]).all()
            counts = e.unit_rank_counts(x, 8)
            assert counts.sum() == 3 * c["N"] and (counts[3:] == 0).all()
    finally:
        e.close()


def test_host_rows_equal_device_rows_and_empty_calls():
    c = T.CASES[4]
    x, w = T.case_data(c)
    K = c["X"] * c["Y"]
    e = engine(c["X"], c["Y"], c["D"])
    try:
        e.set_weights(w)
        t = _device_rows(x)
        for k in (1, 4, 8):
            host, dev = e.bmu_topk(x, k), e.bmu_topk_device(t.data_ptr(), c["N"], k)
            for a, b in zip(host, dev):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            assert np.array_equal(e.unit_rank_counts(x, k), e.unit_rank_counts_device(t.data_ptr(), c["N"], k))
        only = e.bmu_topk(x, 4, score=False, dist=False)
        assert only[1] is None and only[2] is None and np.array_equal(only[0], e.bmu_topk(x, 4)[0])
        z = e.bmu_topk(np.zeros((0, c["D"]), F32), 3)
        assert z[0].shape == (0, 3) and z[1].shape == (0, 3)
        zc = e.unit_rank_counts(np.zeros((0, c["D"]), F32), 3)
        assert zc.dtype == np.int64 and zc.shape == (3, K) and (zc == 0).all()
    finally:
        e.close()


def test_refusals_name_the_reason():
    from xpysom_dask_amd.engine import SomHipError
    x = np.zeros((4, 3), F32)
    ids = np.zeros((4, 9), np.int32)
    cnt = np.zeros((9, 20), np.int64)
    t = _device_rows(x)
    e = engine(4, 5, 3)
    try:
        for k in (0, 9):
            with pytest.raises(ValueError, match="k must be between 1 and 8"):
                e.bmu_topk(x, k)
            with pytest.raises(ValueError, match="k must be between 1 and 8"):
                e.unit_rank_counts_device(t.data_ptr(), 4, k)
            # ... and by the library itself
            assert e._lib.som_bmu_topk(e._h, e._fp(x), 4, k, e._ip(ids), None, None) != 0
            assert "som_bmu_topk: k must be between 1 and SOM_TOPK_MAX = 8" in e._lib.som_last_error(e._h).decode()
            assert e._lib.som_unit_rank_counts_device(e._h, C.c_void_p(t.data_ptr()), 4, k, cnt.ctypes.data_as(C.POINTER(C.c_int64))) != 0
            assert "som_unit_rank_counts_device: k must be between 1 and SOM_TOPK_MAX = 8" in e._lib.som_last_error(e._h).decode()
        assert e._lib.som_bmu_topk(e._h, e._fp(x), 4, 2, None, None, None) != 0
        assert "som_bmu_topk: bad argument" in e._lib.som_last_error(e._h).decode()
    finally:
        e.close()
    small = engine(1, 3, 3)
    try:
        with pytest.raises(ValueError, match="k = 4 exceeds the map's 3 units"):
            small.bmu_topk(x, 4)
        assert small._lib.som_bmu_topk_device(small._h, C.c_void_p(t.data_ptr()), 4, 4, small._ip(ids), None, None) != 0
        assert "som_bmu_topk_device: k = 4 exceeds the map's 3 units" in small._lib.som_last_error(small._h).decode()
        assert small.bmu_topk(x, 3)[0].shape == (4, 3)
    finally:
        small.close()
    m = engine(4, 5, 3, missing="nan")
    try:
        with pytest.raises(SomHipError, match="som_bmu_topk:.*SOM_MISSING_NAN"):
            m.bmu_topk(x, 2)
        with pytest.raises(SomHipError, match="som_bmu_topk_device:.*SOM_MISSING_NAN"):
            m.bmu_topk_device(t.data_ptr(), 4, 2)
        with pytest.raises(SomHipError, match="som_unit_rank_counts:.*SOM_MISSING_NAN"):
            m.unit_rank_counts(x, 2)
    finally:
        m.close()
    man = engine(4, 5, 3, distance="manhattan")
    try:
        with pytest.raises(SomHipError, match="som_bmu_topk:.*GEMM-form distances"):
            man.bmu_topk(x, 2)
        with pytest.raises(SomHipError, match="som_unit_rank_counts_device:.*GEMM-form distances"):
            man.unit_rank_counts_device(t.data_ptr(), 4, 2)
    finally:
        man.close()


def test_nearest_units_rank_hits_smoothed_hits():
    from xpysom_dask_amd import XPySom
    c = T.CASES[2]
    x, w, act, s, E = reference(c, "euclidean")
    X, Y, D, n = c["X"], c["Y"], c["D"], c["N"]
    som = XPySom(X, Y, D, random_seed=5, precision="f32")
    som._weights = w.reshape(X, Y, D).astype(F64)
    want = T.topk_lowest(act, 8)
    ids, dist = som.nearest_units(x, 8)
    assert ids.dtype == np.int64 and dist.dtype == F32 and ids.shape == dist.shape == (n, 8)
    assert np.array_equal(ids, want)
    assert np.array_equal(som.nearest_units(x, 3, return_distance=False), want[:, :3])
    assert np.array_equal(ids[:, 0], som.predict(x))
    # device rows: searched where they are, the host rows' lists
    t = _device_rows(x)
    dids, ddist = som.nearest_units(t, 8)
    assert np.array_equal(dids, ids) and T.same_bits(ddist, dist)
    # chunks of 256 rows concatenate
    chunked = XPySom(X, Y, D, random_seed=5, precision="f32", n_parallel=256)
    chunked._weights = som._weights.copy()
    cids, cdist = chunked.nearest_units(x, 8)
    assert np.array_equal(cids, ids) and T.same_bits(cdist, dist)
    # rank hits: the bincount of every column
    for k in (1, 5, 8):
        hits = som.rank_hits(x, k)
        assert hits.dtype == np.int64 and hits.shape == (k, X, Y)
        assert np.array_equal(hits.reshape(k, X * Y), np.stack([np.bincount(ids[:, j], minlength=X * Y) for j in range(k)]))
        assert np.array_equal(som.rank_hits(t, k), hits) and np.array_equal(chunked.rank_hits(x, k), hits)
    assert np.array_equal(som.rank_hits(x, 1)[0].astype(float), som.activation_response(x))
    for sm in (1, 3, 8):
        sh = som.smoothed_hits(x, sm)
        assert sh.dtype == F64 and sh.shape == (X, Y) and np.array_equal(sh, T.sdh(som.rank_hits(x, sm), sm))
        assert abs(sh.sum() - n) < 1e-9 * n
    assert np.array_equal(som.smoothed_hits(x, 1), som.activation_response(x))
    # one sample, and none
    one_ids, one_dist = som.nearest_units(x[7], 4)
    assert one_ids.shape == (1, 4) and np.array_equal(one_ids[0], ids[7, :4]) and T.same_bits(one_dist[0], dist[7, :4])
    none = som.nearest_units(np.zeros((0, D), F32), 4)
    assert none[0].shape == (0, 4) and none[0].dtype == np.int64 and none[1].shape == (0, 4)
    assert (som.rank_hits(np.zeros((0, D), F32), 2) == 0).all()
    # the default handle (precision 'exact'): the same lists, and predict in column 0
    ex = XPySom(X, Y, D, random_seed=5)
    ex._weights = som._weights.copy()
    eids = ex.nearest_units(x, 8, return_distance=False)
    assert np.array_equal(eids, ids) and np.array_equal(eids[:, 0], ex.predict(x))
    assert np.array_equal(ex.rank_hits(x, 1)[0].astype(float), ex.activation_response(x))
    # freshness: after train the lists are those of the new codebook
    som.train(x, 2)
    w2 = np.asarray(som._weights, F32).reshape(X * Y, D)
    assert not np.array_equal(w2, w)
    s2, E2 = Q.scores(x, w2, "part")
    T.check_topk(som.nearest_units(x, 8, return_distance=False), s2, E2, 8, "nearest_units after train")
    # refusals, by name
    with pytest.raises(ValueError, match="k must be between 1 and 8"):
        som.nearest_units(x, 9)
    with pytest.raises(NotImplementedError, match="nearest_units"):
        XPySom(X, Y, D, random_seed=5, missing="nan").nearest_units(x, 2)
    with pytest.raises(NotImplementedError, match="smoothed_hits.*manhattan"):
        XPySom(X, Y, D, random_seed=5, activation_distance="manhattan").smoothed_hits(x, 2)
