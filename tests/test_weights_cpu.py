"""Per-row sample weights, the part that needs no GPU: `train`'s validation of `sample_weight` (refused with ValueError
before any engine is created), the values it accepts, rows and weights cut alike under a process group, and the float64
model of tests/weights_ref.py against the definition."""
import numpy as np
import pytest

from tests import weights_ref as R
from xpysom_dask_amd import distributed as dist_mod
from xpysom_dask_amd import xpysom as xp_mod
from xpysom_dask_amd.xpysom import XPySom

F32 = np.float32
N, D = 40, 3


def rows(n=N, d=D):
    return np.random.RandomState(0).rand(n, d).astype(F32)


class NoEngine:
    """Stands where the engine would be created: reaching it means the validation let the call through."""

    def __call__(self):
        raise AssertionError("the engine was asked for before sample_weight was refused")


def som_without_engine(monkeypatch):
    s = XPySom(4, 4, D, random_seed=1)
    monkeypatch.setattr(s, "_engine", NoEngine())
    return s


@pytest.mark.parametrize("bad, what", [
    (np.ones((N, 1)), "1-dimensional"),
    (np.ones((2, N // 2)), "1-dimensional"),
    (np.float32(1.0), "1-dimensional"),
    (np.ones(N - 1), "%d values for %d rows" % (N - 1, N)),
    (np.ones(N + 1), "%d values for %d rows" % (N + 1, N)),
    (np.ones(N, dtype=np.complex64), "real dtype"),
    (np.ones(N, dtype=bool), "real dtype"),
    (np.array(["1"] * N), "real dtype"),
    (np.r_[np.ones(N - 1), np.nan], r"sample_weight\[%d\]" % (N - 1)),
    (np.r_[np.ones(7), np.inf, np.ones(N - 8)], r"sample_weight\[7\]"),
    (np.r_[1.0, -1e-30, np.ones(N - 2)], r"sample_weight\[1\]"),
    (np.r_[np.ones(N - 1), 1e39], r"sample_weight\[%d\]" % (N - 1)),          # finite in float64, infinite as float32
])
def test_train_refuses_bad_sample_weight_before_the_engine(monkeypatch, bad, what):
    s = som_without_engine(monkeypatch)
    with pytest.raises(ValueError, match=what):
        s.train(rows(), 1, sample_weight=bad)


def test_sample_weight_is_keyword_only():
    """The reference's positional surface of train() is unchanged: a sixth positional argument is still an error."""
    s = XPySom(4, 4, D, random_seed=1)
    with pytest.raises(TypeError):
        s.train(rows(), 1, 0, None, False, np.ones(N))


class FakeEngine:
    """Records what train() hands to the engine."""
    device = 0

    def __init__(self):
        self.data, self.weights, self.epochs, self.n_rows = None, "never set", 0, 0

    def set_weights(self, w):
        self.codebook = np.array(w, F32)

    def get_weights(self):
        return self.codebook.reshape(-1, self.codebook.shape[-1])

    def set_data(self, data):
        self.data, self.n_rows = np.array(data), len(data)
        self.weights = None                       # the library drops the old rows' weights

    def set_sample_weights(self, w):
        self.weights = None if w is None else np.array(w)


def fake_train(monkeypatch, data, sample_weight, rank=0, world=1, **kw):
    eng = FakeEngine()
    s = XPySom(4, 4, data.shape[1], random_seed=1, **kw)
    monkeypatch.setattr(s, "_engine", lambda: eng)
    monkeypatch.setattr(dist_mod, "dist_info", lambda: (rank, world))
    monkeypatch.setattr(dist_mod, "epoch", lambda engine, *a, **k: setattr(engine, "epochs", engine.epochs + 1))
    if sample_weight is None:
        s.train(data, 2)
    else:
        s.train(data, 2, sample_weight=sample_weight)
    assert eng.epochs == 2
    return eng


@pytest.mark.parametrize("make", [
    lambda: np.arange(N, dtype=np.int64) % 5,
    lambda: (np.arange(N) % 5).astype(np.int8),
    lambda: np.linspace(0.0, 2.0, N),                      # float64
    lambda: [float(i % 3) for i in range(N)],              # a list
    lambda: tuple(range(N)),
    lambda: np.zeros(N, F32),                              # all rows left out: allowed
])
def test_train_accepts_real_array_likes(monkeypatch, make):
    w = make()
    eng = fake_train(monkeypatch, rows(), w)
    assert eng.weights.dtype == F32 and eng.weights.shape == (N,)
    assert np.array_equal(eng.weights, np.asarray(w, dtype=F32))


def test_train_without_sample_weight_sets_none(monkeypatch):
    """Weights are an argument of the call, not state: an unweighted train() sets the rows and no weights (the
    library drops the weights of earlier rows in set_data)."""
    eng = fake_train(monkeypatch, rows(), None)
    assert eng.weights is None
    s = XPySom(4, 4, D, random_seed=1)
    assert not any("weight" in k and "sample" in k for k in s.__getstate__())


@pytest.mark.parametrize("shard", ["contiguous", "strided"])
@pytest.mark.parametrize("world", [2, 3])
def test_rows_and_weights_are_cut_alike(monkeypatch, shard, world):
    """601 rows whose first feature is the row's index and whose weight is index + 0.5: on every rank each weight
    sits next to its own row, and the ranks together hold every row once."""
    n = 601
    data = np.zeros((n, D), F32)
    data[:, 0] = np.arange(n)
    w = np.arange(n) + 0.5
    seen = []
    for rank in range(world):
        eng = fake_train(monkeypatch, data, w, rank=rank, world=world, shard=shard)
        assert len(eng.data) == len(eng.weights) > 0
        assert np.array_equal(eng.weights, eng.data[:, 0] + F32(0.5))
        ref = dist_mod.shard_rows(np.arange(n), rank, world, shard)
        assert np.array_equal(eng.data[:, 0], ref)
        seen.append(eng.data[:, 0])
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(n))


def test_sharded_input_keeps_this_ranks_own_weights(monkeypatch):
    data, w = rows(), np.arange(N, dtype=F32)
    eng = fake_train(monkeypatch, data, w, rank=1, world=2, sharded_input=True)
    assert np.array_equal(eng.data, data) and np.array_equal(eng.weights, w)


def test_stream_chunks_must_not_mix_forms():
    """engine.stream_epoch_accumulate: rows and (rows, weights) pairs in one epoch raise ValueError (checked on a
    stand-in library: the refusal comes before the second chunk is handed over)."""
    from xpysom_dask_amd.engine import HipEngine

    class Lib:
        calls = []

        def __getattr__(self, name):
            def f(*a):
                Lib.calls.append(name)
                return 0
            return f

    e = HipEngine.__new__(HipEngine)
    e._lib, e._h, e.D, e.K = Lib(), None, D, 16
    x = rows()
    with pytest.raises(ValueError, match="not a mix"):
        e.stream_epoch_accumulate([x[:10], (x[10:], np.ones(N - 10))], 1.0, 0.5, False)
    with pytest.raises(ValueError, match="not a mix"):
        e.stream_epoch_accumulate([(x[:10], np.ones(10)), x[10:]], 1.0, 0.5, False)
    with pytest.raises(ValueError, match="one value per row"):
        e.stream_epoch_accumulate([(x[:10], np.ones(9))], 1.0, 0.5, False)
    Lib.calls.clear()
    e.stream_epoch_accumulate([(x[:10], np.ones(10)), (x[10:], np.ones(N - 10))], 1.0, 0.5, False)
    assert Lib.calls.count("som_stream_rows_weighted") == 2 and "som_stream_rows" not in Lib.calls


@pytest.mark.parametrize("neighbourhood, topology, wide", [("gaussian", "rectangular", False), ("gaussian", "rectangular", True),
                                                           ("bubble", "rectangular", False), ("gaussian", "hexagonal", True),
                                                           ("triangle", "rectangular", True)])
def test_float64_model_against_the_definition(neighbourhood, topology, wide):
    """weights_ref.reference_update_weighted (segment sums, then H^T [S | c]) against sum_n w_n h(bmu_n -> k) x_n
    row by row on a 5 x 4 map: float64 both, equal to a few ulps of the magnitude sum."""
    X, Y, d, n = 5, 4, 3, 200
    rs = np.random.RandomState(7)
    x = rs.randn(n, d)
    bmu = rs.randint(0, X * Y, n)
    w = R.make_weights(n, 3).astype(np.float64)
    assert (w == 0).sum() >= 1
    x[np.flatnonzero(w == 0)[0]] = np.nan                 # a row of weight 0 is absent, whatever it holds
    num, den, mnum, mden = R.reference_update_weighted(x, bmu, w, X, Y, 0.5, 1.5, wide=wide, neighbourhood=neighbourhood,
                                                       topology=topology)
    bnum, bden = R.brute_force_update(x, bmu, w, X, Y, 0.5, 1.5, wide=wide, neighbourhood=neighbourhood, topology=topology)
    assert np.isfinite(num).all() and np.isfinite(den).all()
    assert (np.abs(num - bnum) <= 1e-13 * mnum + 1e-300).all()
    assert (np.abs(den - bden) <= 1e-13 * mden + 1e-300).all()
    assert den.max() > 0


def test_model_with_unit_weights_is_the_unweighted_model():
    from tests import update_ref as U
    rs = np.random.RandomState(2)
    x, bmu = rs.randn(300, 4), rs.randint(0, 20, 300)
    a = R.reference_update_weighted(x, bmu, np.ones(300), 5, 4, 0.3, 2.0, wide=True)
    b = U.reference_update(x, bmu, 5, 4, 0.3, 2.0, wide=True)
    for p, q in zip(a, b):
        assert np.array_equal(p, q)


def test_check_sample_weight_returns_float32_host_array():
    w = xp_mod._check_sample_weight([1, 2, 3], 3, False)
    assert isinstance(w, np.ndarray) and w.dtype == F32 and w.flags.c_contiguous
