"""The k nearest rows of every unit on the device -- som_unit_nearest_rows*, XPySom.nearest_samples -- against a float64 model of the
definition in include/somhip.h and against activate().  GPU only (`-m gpu`).  Shapes: the smallest that reach each tail of the
128 units x 128 rows x 32 features tiling, more than one unit tile, more than one row stage and part, k on both kernel instances."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def engine(X, Y, D, **kw):
    from xpysom_dask_amd.engine import HipEngine
    kw.setdefault("precision", "f32")
    return HipEngine(X, Y, D, **kw)


def ranking(score, k):
    """(K, k) ids: per column of the (n, K) scores the k lowest rows by (score, row id), scores below +inf only; -1 where none is left."""
    n = score.shape[0]
    order = np.argsort(score, axis=0, kind="stable")
    order = np.where(np.take_along_axis(score, order, axis=0) < np.inf, order, -1)
    return np.concatenate([order, np.full((max(k - n, 0), score.shape[1]), -1)])[:k].T


def gather(a, ids):
    """a[ids[u, j], u], NaN where ids is -1"""
    return np.where(ids >= 0, a[np.maximum(ids, 0), np.arange(a.shape[1])[:, None]], np.nan)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32)[~np.isnan(a)], np.asarray(b, F32).view(np.uint32)[~np.isnan(b)]) and \
        np.array_equal(np.isnan(a), np.isnan(b))


INT_CASES = [((1, 1), 1, 1, 1), ((1, 1), 33, 1, 4), ((1, 1), 70, 127, 8), ((3, 11), 1, 300, 5), ((3, 11), 33, 129, 1), ((3, 11), 70, 1, 8),
             ((3, 11), 33, 300, 8), ((10, 13), 1, 127, 4), ((10, 13), 33, 300, 4), ((10, 13), 70, 129, 8), ((10, 13), 70, 300, 5),
             ((10, 13), 33, 1, 5), ((10, 13), 1, 300, 1)]


@pytest.mark.parametrize("shape,D,N,k", INT_CASES)
def test_integer_data_is_the_exact_stable_ranking(shape, D, N, k, monkeypatch):
    """Integers in -8 .. 8: every float32 sum is exact, so the lists are the float64 model's with no tolerance, ties included; the
    same lists for every part count."""
    rs = np.random.RandomState(N * 1000 + D * 10 + k)
    K = shape[0] * shape[1]
    x = rs.randint(-8, 9, (N, D)).astype(F32)
    w = rs.randint(-8, 9, (K, D)).astype(F32)
    for j in range(0, N - 40, 7):                            # twins: in the other lane half of a tile, and in another part
        x[j + 37] = x[j]
        x[N - 1 - j // 7] = x[j]
    x64, w64 = x.astype(F64), w.astype(F64)
    exact = (x64 * x64).sum(1)[:, None] - 2 * x64 @ w64.T + (w64 * w64).sum(1)[None, :]
    want = ranking(exact, k)
    assert N < 100 or (np.sort(exact, axis=0)[1:k + 1] == np.sort(exact, axis=0)[:k]).any()                # ties inside the lists
    e = engine(*shape, D)
    try:
        e.set_weights(w)
        for parts in ("1", "2", "3"):
            monkeypatch.setenv("SOM_EXEMPLAR_PARTS", parts)
            ids, score, dist = e.unit_nearest_rows(x, k)
            assert ids.dtype == np.int32 and ids.shape == score.shape == dist.shape == (K, k)
            assert np.array_equal(ids, want), "parts=%s: unit %d" % (parts, np.flatnonzero((ids != want).any(axis=1))[0])
            assert np.array_equal(np.nan_to_num(score.astype(F64), nan=-1.0), np.nan_to_num(gather(exact, want), nan=-1.0))
            assert np.array_equal(np.isnan(dist), want < 0)
            if k > N:
                assert (ids[:, N:] == -1).all() and np.isnan(score[:, N:]).all() and (ids[:, :N] >= 0).all()
    finally:
        e.close()


_GAUSS = {}


def gauss():
    if not _GAUSS:
        rs = np.random.RandomState(5)
        _GAUSS["x"], _GAUSS["w"] = rs.normal(0, 1, (300, 70)).astype(F32), rs.normal(0, 1, (130, 70)).astype(F32)
        for a in _GAUSS.values():
            a.setflags(write=False)
    return _GAUSS["x"], _GAUSS["w"]


@pytest.mark.parametrize("distance", ("euclidean_no_opt", "cosine"))
def test_scores_are_activate_bit_for_bit(distance):
    x, w = gauss()
    e = engine(10, 13, 70, distance=distance)
    try:
        e.set_weights(w)
        act = e.distance_matrix(x)
        for k in (3, 8):
            ids, score, _ = e.unit_nearest_rows(x, k)
            assert np.array_equal(ids, ranking(act, k))
            assert same_bits(score, gather(act, ids)) and (ids >= 0).all()
    finally:
        e.close()
    if distance == "euclidean_no_opt":
        e = engine(10, 13, 70, distance="euclidean")
        try:
            e.set_weights(w)
            assert np.array_equal(e.unit_nearest_rows(x, 8)[0], ids)
        finally:
            e.close()


def test_row_sources_give_the_same_arrays(monkeypatch):
    import torch
    from xpysom_dask_amd import XPySom
    x, w = gauss()
    som = XPySom(10, 13, 70, random_seed=5, precision="f32")
    som._weights = w.reshape(10, 13, 70).astype(F64)
    ids, dist = som.nearest_samples(x, 5)
    assert ids.dtype == np.int64 and dist.dtype == F32 and ids.shape == dist.shape == (10, 13, 5)
    dids, ddist = som.nearest_samples(torch.from_numpy(np.array(x)).cuda(), 5)
    assert np.array_equal(dids, ids) and same_bits(ddist, dist)
    chunked = XPySom(10, 13, 70, random_seed=5, precision="f32", n_parallel=64)
    chunked._weights = som._weights.copy()
    cids, cdist = chunked.nearest_samples(x, 5)
    assert np.array_equal(cids, ids) and same_bits(cdist, dist)
    assert np.array_equal(som.nearest_samples(x, 5, return_distance=False), ids)
    assert np.array_equal(som.nearest_samples(x)[0], ids[:, :, :1])
    monkeypatch.setenv("SOM_EXEMPLAR_PASS_ROWS", "128")      # the library's own passes over host rows: three of them
    pids, pdist = som.nearest_samples(x, 5)
    assert np.array_equal(pids, ids) and same_bits(pdist, dist)
    none = som.nearest_samples(np.zeros((0, 70), F32), 2)
    assert (none[0] == -1).all() and np.isnan(none[1]).all() and none[0].shape == (10, 13, 2)


def test_non_finite_rows_distances_and_state():
    """Worst distance error seen on the device: see profiles/exemplars.md (the bound: 4 ulp of float32 against float64)."""
    from xpysom_dask_amd import XPySom
    x, w = gauss()
    x = x.copy()
    x[17, 40], x[150, 3] = np.nan, np.inf
    som = XPySom(10, 13, 70, random_seed=5, precision="f32")
    som.train(np.nan_to_num(x, posinf=0.0), 2)
    w0, p0 = np.array(som._weights, copy=True), som.predict(x[200:])
    ids, dist = som.nearest_samples(x, 8)
    assert not np.isin(ids, (17, 150)).any() and (ids >= 0).all()
    ref = np.linalg.norm(x.astype(F64)[ids] - np.asarray(w0, F32).astype(F64).reshape(10, 13, 1, 70), axis=3)
    ulps = np.abs(dist.astype(F64) - ref) / np.spacing(ref.astype(F32)).astype(F64)
    print("nearest_samples: worst distance error %.3f ulp" % ulps.max())
    assert ulps.max() <= 4
    qi, qd = som.quantization_distances(x[ids[:, :, 0].ravel()])                 # where the unit is the row's BMU: the same bits
    own = qi == np.arange(130)
    assert own.any() and same_bits(dist[:, :, 0].ravel()[own], qd[own])
    assert np.array_equal(np.asarray(som._weights), w0) and np.array_equal(som.predict(x[200:]), p0)
