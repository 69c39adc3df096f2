"""The training monitor without a GPU: XPySom.train / train_streaming (monitor=, callback=), distributed.epoch(metrics=) and
the history over a NumPy-backed test double of the engine (tests/monitor_worker.py), against tests/monitor_ref.py."""
import math
import pickle

import numpy as np
import pytest

from tests import monitor_ref as R
from tests.monitor_worker import MonitorOracleEngine, data_rows, stop_at, worker
from xpysom_dask_amd.decays import DECAY_FUNCTIONS

F32 = np.float32
EPOCH_CALLS = ["accumulate", "measure_rows", "measure_shift", "merge", "metrics"]


@pytest.fixture
def XPySom(monkeypatch):
    from xpysom_dask_amd import XPySom, engine
    monkeypatch.setattr(engine, "HipEngine", MonitorOracleEngine)
    MonitorOracleEngine.log = []
    MonitorOracleEngine.instances = 0
    return XPySom


def _som(XPySom, **kw):
    return XPySom(8, 7, 5, random_seed=3, **kw)


def test_six_monitored_epochs_equal_the_model(XPySom):
    data = data_rows()
    som = _som(XPySom).train(data, 6, monitor=True)
    h = som.history
    assert type(h) is list and len(h) == 6 and [r.iteration for r in h] == list(range(6))
    f = DECAY_FUNCTIONS["exponential"]
    eng = som._engine()
    assert len(eng.epochs) == 6
    prev = None
    for t, (rec, (w0, ids, w1)) in enumerate(zip(h, eng.epochs)):
        assert all(type(v) in (int, float) or v is None for v in rec)        # plain Python numbers
        assert rec.sigma == float(f(som._sigma, som._sigmaN, t, 6))
        assert rec.learning_rate == float(f(som._learning_rate, som._learning_rateN, t, 6))
        ref = R.row_metrics(data, w0, ids, prev=prev)
        assert rec.rows == 300 and rec.weight == 300.0
        assert rec.bmu_changed == (None if t == 0 else ref["changed"])
        assert rec.quantization_error == R.qe_of(ref)
        sumsq, mx = R.shift(w0, w1)
        assert rec.codebook_shift == math.sqrt(sumsq) and rec.codebook_shift_max == float(mx)
        prev = ids
    assert any(r.bmu_changed for r in h[1:])                                 # (the counts are not trivially zero)
    assert np.array_equal(som._weights.reshape(-1, 5), eng.epochs[-1][2])


def test_engine_calls_per_epoch_are_counted(XPySom):
    data = data_rows()
    _som(XPySom).train(data, 3, monitor=True)
    assert MonitorOracleEngine.log == ["monitor_on"] + EPOCH_CALLS * 3
    MonitorOracleEngine.log = []
    som = _som(XPySom).train(data, 3)
    assert MonitorOracleEngine.log == ["accumulate", "merge"] * 3 and som.history == []
    # an unmonitored schedule on an engine whose monitor an earlier call switched on switches it off, and launches nothing for it
    MonitorOracleEngine.log = []
    som = _som(XPySom).train(data, 1, monitor=True)
    som.train(data, 2)
    assert MonitorOracleEngine.log == ["monitor_on"] + EPOCH_CALLS + ["monitor_off"] + ["accumulate", "merge"] * 2
    assert len(som.history) == 1


def test_callback_stops_the_schedule(XPySom):
    data = data_rows()
    seen = []

    def cb(rec):
        seen.append(rec)
        return rec.iteration == 2

    som = _som(XPySom).train(data, 6, callback=cb)                           # (a callback implies monitor)
    assert len(som.history) == 3 and seen == som.history
    assert MonitorOracleEngine.log.count("accumulate") == 3                  # later epochs are not run
    plain = _som(XPySom).train(data, 6, iter_end=3)
    assert np.array_equal(som._weights, plain._weights)
    # a falsy return goes on
    som = _som(XPySom).train(data, 4, callback=lambda rec: 0)
    assert len(som.history) == 4


def test_resumed_schedule_appends_to_the_history(XPySom):
    data = data_rows()
    som = _som(XPySom)
    som.train(data, 6, iter_end=3, monitor=True)
    som.train(data, 6, iter_beg=3, monitor=True)
    whole = _som(XPySom).train(data, 6, monitor=True)
    assert [r.iteration for r in som.history] == list(range(6))
    assert som.history[3].bmu_changed is None                                # a new train call sets the rows again
    strip = lambda h: [r._replace(bmu_changed=None) for r in h]
    assert strip(som.history) == strip(whole.history)
    assert np.array_equal(som._weights, whole._weights)


def test_mexican_hat_zero_sigma_keeps_the_completed_epochs(XPySom):
    som = XPySom(8, 7, 5, random_seed=3, neighborhood_function="mexican_hat", decay_function="linear", sigmaN=0)
    with pytest.raises(ZeroDivisionError):
        som.train(data_rows(), 3, monitor=True)                              # the linear schedule ends at sigma 0: iteration 2 raises
    assert [r.iteration for r in som.history] == [0, 1] and som._weights.dtype == F32
    assert np.array_equal(som._weights.reshape(-1, 5), som._engine().epochs[-1][2])


def test_pickle_round_trip(XPySom):
    som = _som(XPySom).train(data_rows(), 2, monitor=True)
    back = pickle.loads(pickle.dumps(som))
    assert back.history == som.history and type(back.history) is list and type(back.history[0]).__name__ == "EpochRecord"
    state = som.__getstate__()
    del state["history"]                                                     # a pickle from before the monitor
    old = object.__new__(type(som))
    old.__setstate__(state)
    assert old.history == []


@pytest.mark.parametrize("kw,exc", [(dict(monitor=1), TypeError), (dict(monitor="yes"), TypeError), (dict(monitor=None), TypeError),
                                    (dict(callback=3), TypeError), (dict(callback="cb"), TypeError)])
def test_bad_arguments_are_refused_before_an_engine_exists(XPySom, kw, exc):
    som = _som(XPySom)
    with pytest.raises((TypeError, ValueError)) as e:
        som.train(data_rows(), 2, **kw)
    assert isinstance(e.value, exc)
    with pytest.raises((TypeError, ValueError)):
        som.train_streaming(lambda: [data_rows()], 2, **kw)
    assert MonitorOracleEngine.instances == 0 and som.history == []


def test_sample_weights(XPySom):
    data = data_rows()
    w = np.ones(300, F32)
    w[[0, 17, 299]] = 0
    a = _som(XPySom).train(data, 3, monitor=True, sample_weight=w)
    keep = w > 0
    b = _som(XPySom).train(data[keep], 3, monitor=True)
    for ra, rb in zip(a.history, b.history):                                 # a weight-0 row changes neither rows nor QE
        assert ra.rows == rb.rows == 297 and ra.weight == 297.0
        assert ra.quantization_error == rb.quantization_error
        assert ra.codebook_shift == rb.codebook_shift
    wi = np.random.RandomState(4).randint(0, 4, 300).astype(F32)
    a = _som(XPySom).train(data, 3, monitor=True, sample_weight=wi)
    b = _som(XPySom).train(np.repeat(data, wi.astype(int), axis=0), 3, monitor=True)
    for ra, rb in zip(a.history, b.history):                                 # an integer weight is the row repeated
        assert ra.rows == int((wi > 0).sum()) and rb.rows == int(wi.sum()) and ra.weight == rb.weight == float(wi.sum())
        assert ra.quantization_error == pytest.approx(rb.quantization_error, rel=1e-12)
        assert ra.codebook_shift == rb.codebook_shift and ra.codebook_shift_max == rb.codebook_shift_max
    assert np.array_equal(a._weights, b._weights)
    none = _som(XPySom).train(data, 1, monitor=True, sample_weight=np.zeros(300, F32))
    assert none.history[0].rows == 0 and none.history[0].weight == 0 and math.isnan(none.history[0].quantization_error)


def test_streamed_epochs_equal_resident_ones(XPySom):
    data = data_rows()
    cuts = [0, 130, 131, 300]
    som = _som(XPySom).train_streaming(lambda: (data[a:b] for a, b in zip(cuts[:-1], cuts[1:])), 4, monitor=True)
    res = _som(XPySom).train(data, 4, monitor=True)
    assert len(som.history) == 4
    for rs, rr in zip(som.history, res.history):
        assert rs.bmu_changed is None
        assert rs._replace(bmu_changed=None) == rr._replace(bmu_changed=None)
    assert MonitorOracleEngine.log.count("stream") == 4
    stopped = _som(XPySom).train_streaming(lambda: [data], 4, callback=stop_at(1))
    assert len(stopped.history) == 2


def _spawn(tmp_path, name, world, stop):
    import torch.multiprocessing as mp
    d = tmp_path / name
    d.mkdir()
    mp.spawn(worker, args=(world, str(d), stop), nprocs=world, join=True)
    out = []
    for r in range(world):
        with open(d / ("h%d.pkl" % r), "rb") as f:
            out.append(pickle.load(f))
    return out


def test_two_gloo_ranks_hold_the_one_rank_records(tmp_path):
    (h1, w1), = _spawn(tmp_path, "one", 1, None)
    (ha, wa), (hb, wb) = _spawn(tmp_path, "two", 2, None)
    assert ha == hb and len(ha) == 6 and np.array_equal(wa, wb)             # identical records on both ranks
    for r2, r1 in zip(ha, h1):
        r2, r1 = dict(zip(R_FIELDS, r2)), dict(zip(R_FIELDS, r1))
        for k in ("iteration", "sigma", "learning_rate", "rows", "weight", "bmu_changed", "codebook_shift", "codebook_shift_max"):
            assert r2[k] == r1[k], k
        assert r2["quantization_error"] == pytest.approx(r1["quantization_error"], rel=1e-12)
    assert ha[0][R_FIELDS.index("bmu_changed")] is None and ha[1][R_FIELDS.index("bmu_changed")] is not None
    (sa, wsa), (sb, wsb) = _spawn(tmp_path, "stop", 2, 2)                    # a stopping callback stops both ranks at the same epoch
    assert sa == sb == ha[:3] and np.array_equal(wsa, wsb)


from xpysom_dask_amd import EpochRecord  # noqa: E402  (fails on a tree without the monitor, as every test here does)

R_FIELDS = EpochRecord._fields
