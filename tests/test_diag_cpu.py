"""The map diagnostics without a GPU: tests/diag_ref.py's model against brute force on the GPU module's case list, the bounds'
arithmetic, and XPySom.quantization_distances / unit_statistics over a NumPy-backed test double of the engine."""
import math

import numpy as np
import pytest

from tests import diag_ref as R
from tests import query_ref as Q
from tests.oracle_engine import OracleEngine

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------ the model
def _model_ids(c, x, w):
    """First minimum of the float64 (masked) squared distance: the model's ids for the case."""
    with np.errstate(invalid="ignore"):
        x64 = np.asarray(x, F32).astype(F64)
    out = np.empty(len(x), np.int64)
    w64 = w.astype(F64)
    for s in range(0, len(x), 256):
        d = x64[s:s + 256, None, :] - w64[None, :, :]
        sq = d * d
        if c["missing"]:
            sq = np.where(np.isnan(sq), 0.0, sq)
        out[s:s + 256] = np.argmin(sq.sum(axis=2), axis=1)
    return out


@pytest.mark.parametrize("c", [c for c in R.CASES if not c["env"]], ids=[c["id"] for c in R.CASES if not c["env"]])
def test_model_equals_brute_force_on_the_case_list(c):
    x, w = R.case_data(c)
    K, n = c["X"] * c["Y"], c["n"]
    assert x.shape == (n, c["D"]) and w.shape == (K, c["D"]) and x.dtype == F32 and w.dtype == F32
    ids = _model_ids(c, x, w)
    ref = R.row_distances(x, w, ids, masked=bool(c["missing"]))
    # straight from the definition, row by row
    rows = range(n) if n <= 300 else range(0, n, 17)
    for i in rows:
        seen = ~np.isnan(x[i]) if c["missing"] else np.ones(c["D"], bool)
        want = math.sqrt(math.fsum(((float(a) - float(b)) ** 2 for a, b in zip(x[i][seen], w[ids[i]][seen]))))
        assert abs(ref[i] - want) <= 4 * R.U64 * want * c["D"]
    d = ref.astype(F32)                                    # a float32 rounding of the reference is within the bound
    R.check_distances(d, x, w, ids, masked=bool(c["missing"]), what=c["id"])
    got = R.unit_stats_model(ids, d, K)
    if n < 20000:                                          # the exact-rational loop: too slow beyond; the float64 model runs on all
        bf = R.brute_force_unit_stats(ids, d, K)
        for a, b in zip(got, bf):
            assert np.array_equal(a, b)                    # (fsum is the correctly rounded exact sum)
    else:
        assert np.array_equal(got[0], np.bincount(ids, minlength=K)) and np.allclose(got[1].sum(), d.astype(F64).sum(), rtol=1e-12)
    assert R.check_unit_stats(got, ids, d, K, what=c["id"]) == 0.0
    assert got[0].sum() == n
    if c["data"] == "weights":
        assert (d == 0).all()
    if c["data"] == "three":
        assert (got[0] > 1000).sum() <= 3 and (got[0] == 0).sum() >= K - 3
    if c["missing"]:
        assert np.isnan(x[0]).all() and ids[0] == 0 and d[0] == 0 and np.isnan(x[:, -1]).all()
    if c["data"] == "int":                                 # exact arithmetic: the distance is the rounded sqrt of an integer
        sq = ((x.astype(F64) - w.astype(F64)[ids]) ** 2).sum(axis=1)
        assert (sq == np.round(sq)).all() and np.array_equal(d, np.sqrt(sq.astype(F32)))
        assert (ids < K - c["dup"]).all()                  # duplicate units: the lowest id


def test_case_list_covers_the_issue_table():
    ids = {c["id"] for c in R.CASES}
    assert len(ids) == len(R.CASES) == 7 + 8 + 1 + 4 + 6
    assert {(c["X"], c["Y"], c["D"], c["n"]) for c in R.CASES} == {
        (5, 7, 1, 1), (5, 7, 3, 127), (5, 7, 64, 129), (12, 11, 65, 300), (12, 11, 130, 1031), (16, 16, 260, 257),
        (64, 64, 32, 5000), (12, 11, 33, 300),
        (5, 7, 3, 40003), (12, 11, 130, 16389), (128, 64, 4, 5000), (129, 64, 4, 5000)}
    exact = [c for c in R.CASES if c["prec"] == "exact" and not c["missing"]]
    assert {c["data"] for c in exact} == {"blobs", "offset30", "offset300", "weights"}
    assert {c["env"].get("SOM_EXACT_SKIP") for c in exact} == {None, "2"}
    assert {(c["prec"], c["D"]) for c in R.CASES if c["missing"]} == {("f32", 33), ("exact", 33), ("f32", 3), ("exact", 3),
                                                                      ("f32", 130), ("exact", 130), ("f32", 65)}
    assert sorted((c["X"], c["D"], c["n"]) for c in R.CASES if c["missing"] and c["D"] >= 65) == [(12, 65, 300), (12, 130, 16389),
                                                                                                 (12, 130, 16389)]


def test_case_list_goes_past_one_turn_and_behind_both_sorts():
    """What the cases added for the persistent loop and the sorts reach, restated from the launch code: bmu_dist_kernel's waves
    take rows r, r + 16 384, ...; the sort is update_ref.update_paths' rule (and diag_ref.sort_path's)."""
    from tests import update_ref as U
    turns = {c["id"]: -(-c["n"] // R.DIST_WAVES) for c in R.CASES}
    assert max(turns.values()) == 3 and turns["5x7x3-n40003-f32-blobs"] == 3 and 40003 % R.DIST_WAVES not in (0, R.DIST_WAVES - 1)
    assert {c["prec"] for c in R.CASES if c["missing"] and c["n"] > R.DIST_WAVES} == {"f32", "exact"}
    assert {c["D"] for c in R.CASES if c["missing"] and c["n"] > R.DIST_WAVES} == {130}          # three fma steps on lanes 0 and 1
    assert all(c["n"] - R.DIST_WAVES == 5 for c in R.CASES if c["missing"] and c["n"] > R.DIST_WAVES)   # waves 0 ... 4 turn twice
    for c in R.CASES:
        label = "sort." + R.sort_path(c)
        assert label in U.update_paths(c["X"], c["Y"], c["D"], "gaussian", "rectangular", False, c["n"]), c["id"]
    by_units = {}
    for c in R.CASES:
        by_units.setdefault(R.sort_path(c), set()).add(c["X"] * c["Y"])
    assert max(by_units["counting"]) == 8192 and max(by_units["radix"]) == 8256          # the ceiling, and just past it
    big = [c for c in R.CASES if c["X"] * c["Y"] > 8192]
    assert len(big) == 1 and big[0]["n"] >= 2048                            # (enough rows for the counting sort: only K decides)
    assert R.sort_path(dict(big[0], X=128)) == "counting"
    assert (8256 - 1).bit_length() == 14                                    # the radix sort's key bits


# ------------------------------------------------------------------------------------------------------ the bounds
def test_bounds_arithmetic():
    assert Q.gamma(74) == 74 * 2.0 ** -24 / (1 - 74 * 2.0 ** -24)
    assert R.dist_bound(64) == Q.gamma(74)
    np.testing.assert_array_equal(R.sum_bound([0, 1, 2, 1000]), [0.0, 0.0, 2 * 2.0 ** -53, 1000 * 2.0 ** -53])
    # a distance one float32 ulp off is inside gamma(D + 10); one part in 1e4 off is not
    x = np.array([[3.0, 4.0]], F32)
    w = np.zeros((1, 2), F32)
    R.check_distances(np.array([np.nextafter(F32(5), F32(6))], F32), x, w, [0])
    with pytest.raises(AssertionError):
        R.check_distances(np.array([5.0005], F32), x, w, [0])
    # a row that equals its unit: only 0 passes
    R.check_distances(np.array([0.0], F32), x, x, [0])
    with pytest.raises(AssertionError):
        R.check_distances(np.array([1e-30], F32), x, x, [0])
    # NaN rows: NaN expected without the mask, the observed features with it
    xn = np.array([[np.nan, 4.0]], F32)
    R.check_distances(np.array([np.nan], F32), xn, w, [0])
    R.check_distances(np.array([4.0], F32), xn, w, [0], masked=True)
    with pytest.raises(AssertionError):
        R.check_distances(np.array([4.0], F32), xn, w, [0])


def test_unit_stats_check_catches_what_it_must():
    ids = np.array([2, 0, 2, 2, 1], np.int64)
    d = np.array([1.0, 0.5, 0.1, 3.0, np.nan], F32)
    good = R.unit_stats_model(ids, d, 4)
    np.testing.assert_array_equal(good[0], [1, 1, 3, 0])
    assert good[1][0] == 0.5 and np.isnan(good[1][1]) and np.isnan(good[2][1]) and good[3][1] == 0 and good[3][2] == 3.0
    assert good[1][3] == 0 and good[2][3] == 0 and good[3][3] == 0
    assert good[2][2] == math.fsum([1.0, float(F32(0.1)) ** 2, 9.0])
    R.check_unit_stats(good, ids, d, 4)
    for which, unit, value in ((0, 3, 1), (1, 0, np.nextafter(0.5, 1)), (1, 2, good[1][2] * (1 + 8 * R.U64)), (1, 1, 0.0),
                               (2, 2, good[2][2] * (1 - 8 * R.U64)), (3, 2, np.nextafter(F32(3), F32(4))), (3, 3, F32(1e-9))):
        bad = [a.copy() for a in good]
        bad[which][unit] = value
        with pytest.raises(AssertionError):
            R.check_unit_stats(bad, ids, d, 4)
    # inside the bound: three terms, one ulp of the double sum
    near = [a.copy() for a in good]
    near[1][2] = np.nextafter(good[1][2], np.inf)
    assert 0 < R.check_unit_stats(near, ids, d, 4) <= 1
    R.check_qe_agreement([1.0, 2.0, 3.0], 4, 1.5)
    with pytest.raises(AssertionError):
        R.check_qe_agreement([1.0, 2.0, 3.0], 4, 1.5 * (1 + 1e-11))


# ------------------------------------------------------------------------------------------------------ the host class
class FakeDeviceRows:
    """Stands for rows in HBM: XPySom sees `__cuda_array_interface__`, the test double finds the rows by their pointer."""
    table = {}

    def __init__(self, x):
        self.x = np.ascontiguousarray(x, F32)
        self.shape = self.x.shape
        self.__cuda_array_interface__ = {"shape": self.x.shape, "typestr": "<f4", "data": (self.x.ctypes.data, False),
                                         "version": 2, "strides": None, "stream": None}
        FakeDeviceRows.table[self.x.ctypes.data] = self.x


class DiagOracleEngine(OracleEngine):
    """OracleEngine + the four diagnostic calls answered from NumPy (float32 distances; sums over a unit's rows in ascending
    order), recording the chunk sizes it was handed."""
    calls = []

    def __init__(self, *a, missing=None, **kw):
        super().__init__(*a, **kw)
        self.device = 0
        self.uploads = 0

    def set_weights(self, w):
        super().set_weights(w)
        self.uploads += 1

    def sync_producer(self, stream=None):
        pass

    def bmu_distances(self, x):
        x = np.ascontiguousarray(x, F32)
        if x.ndim != 2 or x.shape[1] != self.D:
            raise ValueError("x must be (n, %d), got %r" % (self.D, x.shape))
        DiagOracleEngine.calls.append(len(x))
        ids = self.bmu(x, quantization=True) if len(x) else np.zeros(0, np.int32)
        return ids, np.sqrt(((x - self.W[ids]) ** 2).sum(axis=1, dtype=F32)).astype(F32)

    def unit_stats(self, x):
        ids, d = self.bmu_distances(x)
        return R.unit_stats_model(ids, d, self.K)

    def bmu_distances_device(self, ptr, n):
        return self.bmu_distances(FakeDeviceRows.table[ptr][:n])

    def unit_stats_device(self, ptr, n):
        return self.unit_stats(FakeDeviceRows.table[ptr][:n])


@pytest.fixture
def som(monkeypatch):
    from xpysom_dask_amd import XPySom, engine
    monkeypatch.setattr(engine, "HipEngine", DiagOracleEngine)
    DiagOracleEngine.calls = []
    s = XPySom(6, 5, 4, random_seed=3, n_parallel=97)
    s._weights = np.random.RandomState(1).normal(0, 1, (6, 5, 4)).astype(F32)
    return s


def _rows(n, seed=5):
    return np.random.RandomState(seed).normal(0, 1, (n, 4)).astype(F32)


def test_quantization_distances_chunks_and_device_rows(som):
    x = _rows(300)
    ids, d = som.quantization_distances(x)
    assert DiagOracleEngine.calls == [97, 97, 97, 9]                        # n_parallel chunks, concatenated in order
    assert ids.dtype == np.int64 and d.dtype == F32 and ids.shape == d.shape == (300,)
    np.testing.assert_array_equal(ids, som.predict(x))                      # raveled as in predict (euclidean)
    eng = som._engine()
    whole = eng.bmu_distances(x)
    np.testing.assert_array_equal(ids, whole[0])
    np.testing.assert_array_equal(d.view(np.uint32), whole[1].view(np.uint32))
    DiagOracleEngine.calls = []
    uploads = eng.uploads
    ids_d, d_d = som.quantization_distances(FakeDeviceRows(x))              # device rows: whole, one upload of the codebook
    assert DiagOracleEngine.calls == [300] and eng.uploads == uploads + 1
    np.testing.assert_array_equal(ids_d, ids)
    np.testing.assert_array_equal(d_d.view(np.uint32), d.view(np.uint32))
    assert ids_d.dtype == np.int64


def test_one_dimensional_wrong_width_and_empty_input(som):
    x = _rows(3)
    ids, d = som.quantization_distances(x[1])                               # a 1-D row is one sample
    assert ids.shape == d.shape == (1,)
    ref = som.quantization_distances(x)
    assert ids[0] == ref[0][1] and d[0] == ref[1][1]
    st = som.unit_statistics(x[1])
    assert st.hits.sum() == 1 and st.hits.shape == (6, 5)
    for call in (som.quantization_distances, som.unit_statistics):
        with pytest.raises(ValueError, match="Received 3 features, expected 4"):
            call(np.zeros((5, 3), F32))
        with pytest.raises(ValueError, match="Received 3 features, expected 4"):
            call(FakeDeviceRows(np.zeros((5, 3), F32)))
    ids, d = som.quantization_distances(np.zeros((0, 4), F32))
    assert ids.shape == d.shape == (0,) and ids.dtype == np.int64 and d.dtype == F32
    ids, d = som.quantization_distances(FakeDeviceRows(np.zeros((0, 4), F32)))
    assert ids.shape == d.shape == (0,) and ids.dtype == np.int64 and d.dtype == F32
    for empty in (np.zeros((0, 4), F32), FakeDeviceRows(np.zeros((0, 4), F32))):
        st = som.unit_statistics(empty)
        assert st.hits.shape == (6, 5) and st.hits.dtype == np.int64 and not st.hits.any()
        assert not st.sum.any() and not st.sumsq.any() and not st.max.any()
        assert np.isnan(st.mean).all() and np.isnan(st.std).all()


def test_unit_statistics_combines_chunks_in_order(som):
    from xpysom_dask_amd import UnitStatistics
    x = _rows(300, seed=8)
    st = som.unit_statistics(x)
    assert DiagOracleEngine.calls == [97, 97, 97, 9]
    assert isinstance(st, UnitStatistics)
    assert st.hits.dtype == np.int64 and st.sum.dtype == F64 and st.sumsq.dtype == F64 and st.max.dtype == F32
    assert st.hits.shape == st.sum.shape == st.sumsq.shape == st.max.shape == (6, 5)
    eng = som._engine()
    parts = [eng.unit_stats(x[s:s + 97]) for s in range(0, 300, 97)]
    want = R.combine(parts, 30)
    for got, ref in zip((st.hits, st.sum, st.sumsq, st.max), want):
        assert np.array_equal(got.reshape(-1), ref)                          # chunk order, float64, np.maximum: bit for bit
    ids, d = som.quantization_distances(x)
    R.check_unit_stats((st.hits.reshape(-1), st.sum.reshape(-1), st.sumsq.reshape(-1), st.max.reshape(-1)), ids, d, 30)
    assert st.hits.sum() == 300
    dev = som.unit_statistics(FakeDeviceRows(x))                            # whole: the engine's own sums
    whole = eng.unit_stats(x)
    for got, ref in zip((dev.hits, dev.sum, dev.sumsq, dev.max), whole):
        assert np.array_equal(got.reshape(-1), ref)
    np.testing.assert_array_equal(dev.hits, st.hits)
    np.testing.assert_array_equal(dev.max, st.max)


def test_unit_statistics_mean_and_std():
    from xpysom_dask_amd import UnitStatistics
    hits = np.array([[0, 1, 2], [4, 0, 3]], np.int64)
    tot = np.array([[0.0, 2.5, 3.0], [8.0, 0.0, 3.0]])
    sq = np.array([[0.0, 6.25, 5.0], [16.0 - 1e-15, 0.0, 3.5]])             # [1, 0]: a variance rounding below zero
    st = UnitStatistics(hits, tot, sq, np.zeros((2, 3), F32))
    mean, std = R.mean_std(hits, tot, sq)
    assert np.array_equal(np.isnan(st.mean), hits == 0) and np.array_equal(np.isnan(st.std), hits == 0)
    np.testing.assert_array_equal(st.mean[hits > 0], mean[hits > 0])
    np.testing.assert_array_equal(st.std[hits > 0], std[hits > 0])
    assert st.mean[0, 1] == 2.5 and st.std[0, 1] == 0.0 and st.std[1, 0] == 0.0
    assert st.mean[0, 2] == 1.5 and st.std[0, 2] == 0.5
    assert st.mean.dtype == F64 and st.std.dtype == F64
    # the raw quantities add: two shards' statistics summed by the caller give the whole's mean
    a = UnitStatistics(hits, tot, sq, np.zeros((2, 3), F32))
    both = UnitStatistics(a.hits + hits, a.sum + tot, a.sumsq + sq, np.maximum(a.max, 0))
    np.testing.assert_array_equal(both.mean[hits > 0], mean[hits > 0])
