"""The label and value maps without a GPU: tests/project_ref.py's models against brute force, what its checker must catch,
the C ABI's declarations, and XPySom.label_counts / unit_means / classify over a NumPy-backed test double of the engine."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import project_ref as P
from tests.oracle_engine import OracleEngine

F32, F64 = np.float32, np.float64
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------ the model
def _ids(kind, n, K, rs):
    if kind == "random":                                    # K > n: most units are empty
        return rs.randint(0, K, n)
    if kind == "few":                                       # three units share the rows, the others are empty
        return rs.choice([1, K // 2, K - 1], n)
    assert kind == "one"                                    # one unit holds everything
    return np.full(n, K - 2)


@pytest.mark.parametrize("kind", ["random", "few", "one"])
@pytest.mark.parametrize("n,K,C", [(1, 35, 1), (127, 35, 3), (300, 500, 65), (200, 7, 5)])
def test_label_model_equals_brute_force(kind, n, K, C):
    rs = np.random.RandomState(n + K + C)
    ids = _ids(kind, n, K, rs)
    labels = rs.randint(-1, C + 2, n)                       # -1 and >= C mixed in
    labels[0] = -5 if n > 1 else 0
    got = P.label_counts_model(ids, labels, K, C)
    assert got.dtype == np.int64 and got.shape == (K, C)
    np.testing.assert_array_equal(got, P.brute_force_label_counts(ids, labels, K, C))
    assert got.sum() == ((labels >= 0) & (labels < C)).sum()
    if kind == "one":
        assert not np.delete(got, K - 2, axis=0).any()
    if kind == "few":
        assert (got.sum(axis=1) == 0).sum() >= K - 3


def _holey_values(n, C, rs):
    """30 % NaN, the last column observed by nobody, row 0 with nothing observed."""
    v = rs.normal(0, 10, (n, C)).astype(F32)
    v[rs.random_sample(v.shape) < 0.3] = np.nan
    v[:, C - 1] = np.nan
    v[0] = np.nan
    return v


@pytest.mark.parametrize("kind", ["random", "few", "one"])
@pytest.mark.parametrize("n,K,C", [(1, 35, 1), (127, 35, 3), (300, 500, 7), (200, 7, 5)])
def test_value_model_equals_brute_force(kind, n, K, C):
    rs = np.random.RandomState(n + K + C + 1)
    ids = _ids(kind, n, K, rs)
    v = _holey_values(n, C, rs)
    got = P.value_sums_model(ids, v, K)
    bf = P.brute_force_value_sums(ids, v, K)
    for a, b in zip(got, bf):
        assert a.shape == (K, C) and np.array_equal(a, b)   # (fsum is the correctly rounded exact sum)
    assert not got[0][:, C - 1].any() and not got[1][:, C - 1].any()         # the column nobody observes
    assert got[0].sum() == (~np.isnan(v)).sum()
    assert P.check_value_sums(got, ids, v, K) == 0.0
    if C > 1:                                               # a 1-D array is one column
        one = P.value_sums_model(ids, v[:, 0], K)
        for a, b in zip(one, got):
            assert a.shape == (K, 1) and np.array_equal(a[:, 0], b[:, 0])


def test_value_model_infinities():
    ids = np.array([0, 0, 1, 1, 2, 2, 2])
    v = np.array([np.inf, 1.0, np.inf, -np.inf, -np.inf, np.nan, 2.0], F32)
    got = P.value_sums_model(ids, v, 4)
    bf = P.brute_force_value_sums(ids, v, 4)
    np.testing.assert_array_equal(got[0][:, 0], [2, 2, 2, 0])
    for a, b in zip(got, bf):
        np.testing.assert_array_equal(a, b)
    assert got[1][0, 0] == np.inf and np.isnan(got[1][1, 0]) and got[1][2, 0] == -np.inf and got[1][3, 0] == 0
    assert (got[2][:3, 0] == np.inf).all()
    P.check_value_sums(got, ids, v, 4)
    bad = [a.copy() for a in got]
    bad[1][1, 0] = np.inf                                   # NaN expected
    with pytest.raises(AssertionError):
        P.check_value_sums(bad, ids, v, 4)
    bad = [a.copy() for a in got]
    bad[1][2, 0] = np.inf                                   # the other infinity
    with pytest.raises(AssertionError):
        P.check_value_sums(bad, ids, v, 4)


def test_checker_catches_what_it_must():
    assert P.gamma(3) == 3 * 2.0 ** -53 / (1 - 3 * 2.0 ** -53)
    rs = np.random.RandomState(4)
    n, K, C = 400, 5, 3
    ids = rs.randint(0, K, n)
    v = rs.normal(0, 3, (n, C)).astype(F32)
    v[rs.random_sample(v.shape) < 0.3] = np.nan
    good = P.value_sums_model(ids, v, K)
    sa, sq = P.abs_sums(ids, v, K)
    g = P.gamma(good[0])
    assert P.check_value_sums(good, ids, v, K) == 0.0
    bad = [a.copy() for a in good]
    bad[0][2, 1] += 1                                       # a count off by one
    with pytest.raises(AssertionError):
        P.check_value_sums(bad, ids, v, K)
    for which, scale in ((1, sa), (2, sq)):
        for sign in (1, -1):
            bad = [a.copy() for a in good]
            bad[which][3, 2] += sign * 2 * g[3, 2] * scale[3, 2]            # twice the bound
            with pytest.raises(AssertionError):
                P.check_value_sums(bad, ids, v, K)
        near = [a.copy() for a in good]
        near[which][3, 2] += 0.5 * g[3, 2] * scale[3, 2]                     # inside it
        assert 0 < P.check_value_sums(near, ids, v, K) <= 1
    # a cell with one value: nothing was added, only the value itself passes
    one_ids, one_v = np.array([0]), np.array([[0.1]], F32)
    P.check_value_sums(P.value_sums_model(one_ids, one_v, 2), one_ids, one_v, 2)
    bad = [a.copy() for a in P.value_sums_model(one_ids, one_v, 2)]
    bad[1][0, 0] = np.nextafter(bad[1][0, 0], 1) + 1e-15
    with pytest.raises(AssertionError):
        P.check_value_sums(bad, one_ids, one_v, 2)
    with pytest.raises(AssertionError):                     # float32 sums are not what the contract says
        P.check_value_sums((good[0], good[1].astype(F32), good[2]), ids, v, K)


# ------------------------------------------------------------------------------------------------------ the C ABI
def _prototype_args(header, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert m, "include/somhip.h does not declare %s" % name
    return [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in m.group(1).split(",")]


def test_header_and_binding_declare_the_four_calls():
    from xpysom_dask_amd import _lib
    from xpysom_dask_amd.engine import HipEngine
    header = open(REPO + "/include/somhip.h").read()
    out = ["int64_t*", "double*", "double*"]
    want = {"som_unit_label_counts": ["som_handle*", "const float*", "const int32_t*", "int64_t", "int32_t", "int64_t*"],
            "som_unit_label_counts_device": ["som_handle*", "const void*", "const void*", "int64_t", "int32_t", "int64_t*"],
            "som_unit_value_sums": ["som_handle*", "const float*", "const float*", "int64_t", "int32_t"] + out,
            "som_unit_value_sums_device": ["som_handle*", "const void*", "const void*", "int64_t", "int32_t"] + out}
    ctype_of = {"som_handle*": C.c_void_p, "const void*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32,
                "const float*": C.POINTER(C.c_float), "const int32_t*": C.POINTER(C.c_int32), "int64_t*": C.POINTER(C.c_int64),
                "double*": C.POINTER(C.c_double)}
    for name, types in want.items():
        assert _prototype_args(header, name) == types, name
        assert name in _lib.SIGNATURES, "%s is not bound in _lib.py" % name
        res, argtypes = _lib.SIGNATURES[name]
        assert res is C.c_int and argtypes == [ctype_of[t] for t in types], (name, argtypes)
    for method in ("label_counts", "label_counts_device", "value_sums", "value_sums_device"):
        assert hasattr(HipEngine, method)


# ------------------------------------------------------------------------------------------------------ the host class
class ProjectOracleEngine(OracleEngine):
    """OracleEngine + the label and value calls answered from tests/project_ref.py's model on the engine's own bmu(), recording
    the chunk sizes it was handed.  missing='nan': the BMU is the first minimum over a row's observed features."""
    calls = []

    def __init__(self, *a, missing=None, **kw):
        super().__init__(*a, **kw)
        self.device = 0
        self.missing = missing

    def sync_producer(self, stream=None):
        pass

    def bmu(self, x, quantization=False):
        if self.missing is None:
            return super().bmu(x, quantization=quantization)
        with np.errstate(invalid="ignore"):
            d = np.asarray(x, F32).astype(F64)[:, None, :] - self.W.astype(F64)[None, :, :]
        return np.argmin(np.where(np.isnan(d), 0.0, d * d).sum(axis=2), axis=1).astype(np.int32)

    def _rows(self, x):
        x = np.ascontiguousarray(x, F32)
        if x.ndim != 2 or x.shape[1] != self.D:
            raise ValueError("x must be (n, %d), got %r" % (self.D, x.shape))
        ProjectOracleEngine.calls.append(len(x))
        return x

    def label_counts(self, x, labels, n_classes):
        x = self._rows(x)
        assert labels.dtype == np.int32 and labels.shape == (len(x),)
        return P.label_counts_model(self.bmu(x), labels, self.K, n_classes)

    def value_sums(self, x, values):
        x = self._rows(x)
        assert values.dtype == F32 and values.ndim == 2 and len(values) == len(x)
        return P.value_sums_model(self.bmu(x), values, self.K)


def _som(monkeypatch, **kw):
    from xpysom_dask_amd import XPySom, engine
    monkeypatch.setattr(engine, "HipEngine", ProjectOracleEngine)
    ProjectOracleEngine.calls = []
    s = XPySom(6, 5, 4, random_seed=3, **kw)
    s._weights = np.random.RandomState(1).normal(0, 1, (6, 5, 4)).astype(F32)
    return s


def _rows(n, seed=5):
    return np.random.RandomState(seed).normal(0, 1, (n, 4)).astype(F32)


def test_label_counts_chunks_equal_one_chunk_and_labels_map(monkeypatch):
    x = _rows(127)
    labels = np.random.RandomState(2).randint(0, 4, 127)
    chunked = _som(monkeypatch, n_parallel=50).label_counts(x, labels)
    assert ProjectOracleEngine.calls == [50, 50, 27]
    assert chunked.dtype == np.int64 and chunked.shape == (6, 5, 4)          # n_classes inferred: max + 1
    som = _som(monkeypatch, n_parallel=1000)
    whole = som.label_counts(x, labels)
    assert ProjectOracleEngine.calls == [127]
    np.testing.assert_array_equal(chunked, whole)
    assert whole.sum() == 127
    lm = som.labels_map(x, labels)                          # the Counters, entry for entry
    want = np.zeros((6, 5, 4), np.int64)
    for (i, j), counter in lm.items():
        for c, m in counter.items():
            want[i, j, c] = m
    np.testing.assert_array_equal(whole, want)
    np.testing.assert_array_equal(whole.sum(axis=2), som.activation_response(x).astype(np.int64))
    # more classes than the labels show; lists; negative codes are unlabelled
    wide = som.label_counts(x, labels.tolist(), n_classes=6)
    assert wide.shape == (6, 5, 6) and not wide[:, :, 4:].any()
    np.testing.assert_array_equal(wide[:, :, :4], whole)
    holes = labels.copy()
    holes[::3] = -1
    holes[1] = -7
    part = som.label_counts(x, holes, n_classes=4)
    ids = som.predict(x)
    np.testing.assert_array_equal(part.reshape(30, 4), P.label_counts_model(ids, holes, 30, 4))
    assert part.sum() == (holes >= 0).sum()
    one = som.label_counts(x[3], [2], n_classes=4)          # a 1-D row is one sample
    assert one.sum() == 1 and one.reshape(30, 4)[ids[3], 2] == 1
    empty = som.label_counts(np.zeros((0, 4), F32), [], n_classes=3)
    assert empty.shape == (6, 5, 3) and empty.dtype == np.int64 and not empty.any()


def test_label_counts_refusals(monkeypatch):
    som = _som(monkeypatch, n_parallel=50)
    x = _rows(20)
    labels = np.arange(20) % 3
    with pytest.raises(ValueError, match="data and labels must have the same length."):
        som.label_counts(x, labels[:-1])
    with pytest.raises(ValueError, match="data and labels must have the same length."):
        som.label_counts(x, labels.reshape(4, 5))
    with pytest.raises(ValueError, match="labels must be < n_classes = 2, got 2"):
        som.label_counts(x, labels, n_classes=2)
    with pytest.raises(ValueError, match="integer class codes"):
        som.label_counts(x, labels.astype(F64))
    with pytest.raises(ValueError, match="n_classes cannot be inferred"):
        som.label_counts(x, np.full(20, -1))
    with pytest.raises(ValueError, match="n_classes cannot be inferred"):
        som.label_counts(np.zeros((0, 4), F32), [])
    for bad in (0, 4097, 2.5, True):
        with pytest.raises(ValueError, match="n_classes must be an integer between 1 and 4096"):
            som.label_counts(x, np.zeros(20, np.int64), n_classes=bad)
    with pytest.raises(ValueError, match="Received 3 features, expected 4"):
        som.label_counts(np.zeros((5, 3), F32), np.zeros(5, np.int64))
    assert ProjectOracleEngine.calls == []                  # refused before any engine call


def test_label_counts_with_missing_values(monkeypatch):
    som = _som(monkeypatch, n_parallel=50, missing="nan")
    x = _rows(127, seed=9)
    x[np.random.RandomState(3).random_sample(x.shape) < 0.3] = np.nan
    x[5] = np.nan
    labels = np.random.RandomState(4).randint(-1, 3, 127)
    got = som.label_counts(x, labels, n_classes=3)
    ids = som._engine().bmu(x)
    assert ids[5] == 0                                      # a row with nothing observed: unit 0
    np.testing.assert_array_equal(got.reshape(30, 3), P.label_counts_model(ids, labels, 30, 3))
    assert got.sum() == (labels >= 0).sum()


def test_unit_means_chunks_one_column_and_refusals(monkeypatch):
    from xpysom_dask_amd import UnitMeans
    x = _rows(127, seed=6)
    v = _holey_values(127, 3, np.random.RandomState(7))
    som = _som(monkeypatch, n_parallel=50)
    um = som.unit_means(x, v)
    assert ProjectOracleEngine.calls == [50, 50, 27]
    assert isinstance(um, UnitMeans)
    assert um.count.dtype == np.int64 and um.sum.dtype == F64 and um.sumsq.dtype == F64
    assert um.count.shape == um.sum.shape == um.sumsq.shape == (6, 5, 3)
    eng = som._engine()
    count, tot, sq = np.zeros((30, 3), np.int64), np.zeros((30, 3)), np.zeros((30, 3))
    for s in range(0, 127, 50):                             # chunk order, float64: bit for bit
        c, t, q = eng.value_sums(x[s:s + 50], v[s:s + 50])
        count += c
        tot += t
        sq += q
    for got, ref in zip((um.count, um.sum, um.sumsq), (count, tot, sq)):
        assert np.array_equal(got.reshape(30, 3), ref)
    ids = som.predict(x)
    P.check_value_sums((um.count.reshape(30, 3), um.sum.reshape(30, 3), um.sumsq.reshape(30, 3)), ids, v, 30)
    whole = _som(monkeypatch, n_parallel=1000).unit_means(x, v)
    np.testing.assert_array_equal(whole.count, um.count)
    P.check_value_sums((whole.count.reshape(30, 3), whole.sum.reshape(30, 3), whole.sumsq.reshape(30, 3)), ids, v, 30)
    # a 1-D values array is one column; float64 and integer values are taken as float32
    col = som.unit_means(x, v[:, 0].astype(F64))
    assert col.count.shape == (6, 5, 1)
    np.testing.assert_array_equal(col.count[:, :, 0], um.count[:, :, 0])
    assert np.array_equal(col.sum[:, :, 0], um.sum[:, :, 0]) and np.array_equal(col.sumsq[:, :, 0], um.sumsq[:, :, 0])
    assert som.unit_means(x, np.arange(127)).count.sum() == 127
    one = som.unit_means(x[3], [2.5])                       # a 1-D row is one sample
    assert one.count.sum() == 1 and one.sum.reshape(30)[ids[3]] == 2.5
    empty = som.unit_means(np.zeros((0, 4), F32), np.zeros((0, 2), F32))
    assert empty.count.shape == (6, 5, 2) and not empty.count.any() and np.isnan(empty.mean).all()
    calls = list(ProjectOracleEngine.calls)
    with pytest.raises(ValueError, match="data and values must have the same length."):
        som.unit_means(x, v[:-1])
    with pytest.raises(ValueError, match="data and values must have the same length."):
        som.unit_means(x, np.zeros((127, 2, 2), F32))
    with pytest.raises(ValueError, match="between 1 and 4096 columns"):
        som.unit_means(x, np.zeros((127, 0), F32))
    with pytest.raises(ValueError, match="between 1 and 4096 columns"):
        som.unit_means(x, np.zeros((127, 4097), F32))
    with pytest.raises(ValueError, match="real dtype"):
        som.unit_means(x, np.zeros(127, np.complex64))
    with pytest.raises(ValueError, match="Received 3 features, expected 4"):
        som.unit_means(np.zeros((5, 3), F32), np.zeros(5, F32))
    assert ProjectOracleEngine.calls == calls


def test_unit_means_mean_and_std():
    from xpysom_dask_amd import UnitMeans
    count = np.array([[[0, 1], [2, 4]]], np.int64)
    tot = np.array([[[0.0, 2.5], [3.0, 8.0]]])
    sq = np.array([[[0.0, 6.25], [5.0, 16.0 - 1e-15]]])     # [0, 1, 1]: a variance rounding below zero
    um = UnitMeans(count, tot, sq)
    assert np.array_equal(np.isnan(um.mean), count == 0) and np.array_equal(np.isnan(um.std), count == 0)
    assert um.mean[0, 0, 1] == 2.5 and um.std[0, 0, 1] == 0.0
    assert um.mean[0, 1, 0] == 1.5 and um.std[0, 1, 0] == 0.5               # the population formula
    assert um.mean[0, 1, 1] == 2.0 and um.std[0, 1, 1] == 0.0
    assert um.mean.dtype == F64 and um.std.dtype == F64
    both = UnitMeans(count + count, tot + tot, sq + sq)     # the raw quantities add across shards
    np.testing.assert_array_equal(both.mean[count > 0], um.mean[count > 0])


def test_classify_rule(monkeypatch):
    som = _som(monkeypatch, n_parallel=50)
    x = _rows(127, seed=11)
    ids = som.predict(x)
    counts = np.zeros((30, 3), np.int64)
    used = np.unique(ids)
    assert len(used) >= 4
    counts[used[0]] = [2, 5, 5]                             # a tie: the lowest code of the maximum
    counts[used[1]] = [0, 0, 1]
    counts[used[2]] = [3, 3, 3]
    # used[3:] stay empty: default
    got = som.classify(x, counts.reshape(6, 5, 3))
    assert got.dtype == np.int64 and got.shape == (127,)
    np.testing.assert_array_equal(got, P.classify_model(ids, counts))
    assert (got[ids == used[0]] == 1).all() and (got[ids == used[1]] == 2).all() and (got[ids == used[2]] == 0).all()
    # totals are [5, 8, 9]: class 2; with a tie in the totals the lowest code
    assert (got[ids == used[3]] == 2).all()
    counts[used[1]] = [0, 1, 0]                             # totals [5, 9, 8]
    assert (som.classify(x, counts.reshape(6, 5, 3))[ids == used[3]] == 1).all()
    counts[used[1]] = [4, 0, 0]                             # totals [9, 8, 8]
    counts[used[2]] = [3, 4, 4]                             # totals [9, 9, 9]: the lowest code
    assert (som.classify(x, counts.reshape(6, 5, 3))[ids == used[3]] == 0).all()
    np.testing.assert_array_equal(som.classify(x, counts.reshape(6, 5, 3)), P.classify_model(ids, counts))
    forced = som.classify(x, counts.reshape(6, 5, 3), default=-1)
    assert (forced[np.isin(ids, used[3:])] == -1).all() and (forced[np.isin(ids, used[:3])] >= 0).all()
    np.testing.assert_array_equal(forced, P.classify_model(ids, counts, default=-1))
    assert som.classify(x[3], counts.reshape(6, 5, 3)).shape == (1,)
    assert som.classify(np.zeros((0, 4), F32), counts.reshape(6, 5, 3)).shape == (0,)
    # the training rows through their own label map
    labels = np.random.RandomState(12).randint(0, 3, 127)
    lc = som.label_counts(x, labels)
    np.testing.assert_array_equal(som.classify(x, lc), P.classify_model(ids, lc))
    with pytest.raises(ValueError, match=r"counts must be \(6, 5, n_classes\)"):
        som.classify(x, counts)
    with pytest.raises(ValueError, match="Received 3 features, expected 4"):
        som.classify(np.zeros((5, 3), F32), counts.reshape(6, 5, 3))
