"""The training monitor without a GPU: XPySom.train / train_streaming (monitor=, callback=), distributed.epoch(metrics=) and
the history over a NumPy-backed test double of the engine (tests/monitor_worker.py), against tests/monitor_ref.py."""
import math
import pickle

import numpy as np
import pytest

from tests import monitor_ref as R
from tests import query_ref as Q
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


# ------------------------------------------------------------------------------------------ the launch geometry and its cases
def _brute_rows_paths(N, weights=None):
    """monitor_rows_kernel's loops replayed wave by wave (csrc/monitor.hpp), written without monitor_ref."""
    g = min((N + 3) // 4, 4096)
    waves = 4 * g
    out = set()
    for wave in range(min(waves, N)):
        turns = 0
        row0 = wave
        while row0 < N:
            turns += 1
            below = [row0 + j * waves < N for j in range(4)]
            live = [b and (weights is None or weights[row0 + j * waves] != 0) for j, b in enumerate(below)]
            if all(live):
                out.add("turn.all")
            if not all(below):
                out.add("turn.tail")
            if all(below) and not all(live) and any(live):
                out.add("turn.zero_weight")
            row0 += waves * 4
        if turns > 1:
            out.add("second_turn")
    return out | _brute_reduce(g)


def _brute_reduce(g):
    """The reduction's runs: thread t adds the partials [t c, min((t + 1) c, g))."""
    c = (g + 255) // 256
    runs = [min((t + 1) * c, g) - t * c for t in range(256) if t * c < g]
    return {"reduce.c=%d" % c} | ({"reduce.ragged"} if runs[-1] < c else set())


def _brute_shift_paths(K, D):
    """monitor_shift_kernel's walk replayed thread by thread."""
    total = K * D
    g = min((total + 1023) // 1024, 2048)
    stride = g * 256
    sk = stride // D
    sd = stride - sk * D
    out = set()
    if (total + 1023) // 1024 > 2048:
        out.add("grid.capped")
    if g >= 2:
        out.add("grid.multi")
    if sk == 0:
        out.add("sk.zero")
    if sd != 0:
        out.add("sd.nonzero")
    for i0 in range(min(stride, total)):
        i, k, d = i0, i0 // D, i0 % D
        while i < total:
            if d >= D:
                d -= D
                k += 1
                out.add("carry")
            assert (k, d) == divmod(i, D)
            i, k, d = i + stride, k + sk, d + sd
    return out | _brute_reduce(g)


ROW_SIZES = (1, 4, 1003, 1025, 16384, 16385, 20000, 65535, 65536, 65537, 81925)


@pytest.mark.parametrize("N", ROW_SIZES)
def test_rows_paths_equal_the_enumeration(N):
    assert R.rows_paths(N) == _brute_rows_paths(N)
    rs = np.random.RandomState(N)
    for share in (0.1, 0.9):                                                 # few holes; mostly holes
        w = (rs.rand(N) * 2).astype(F32)
        w[rs.rand(N) < share] = 0
        assert R.rows_paths(N, w) == _brute_rows_paths(N, w.tolist()), share
    assert R.rows_paths(N, np.zeros(N, F32)) == _brute_rows_paths(N, [0.0] * N)
    assert "turn.all" not in R.rows_paths(N, np.zeros(N, F32))


def test_rows_paths_at_the_boundaries_the_issue_names():
    p = {N: R.rows_paths(N) for N in ROW_SIZES}
    assert all("turn.all" not in p[N] for N in ROW_SIZES if N <= 3 * 16384)  # today's largest case, 20 000 rows, included
    assert R.rows_paths(3 * 16384) == {"turn.tail", "reduce.c=16"} and "turn.all" in R.rows_paths(3 * 16384 + 1)   # wave 0's fourth row
    assert p[65535] == {"turn.all", "turn.tail", "reduce.c=16"}
    assert p[65536] == {"turn.all", "reduce.c=16"}                           # exactly one all-live turn, nothing else
    assert p[65537] == {"turn.all", "turn.tail", "second_turn", "reduce.c=16"}
    assert p[1025] == {"turn.tail", "reduce.c=2", "reduce.ragged"} and p[1003] == {"turn.tail", "reduce.c=1"}
    assert p[4] == {"turn.tail", "reduce.c=1"}                               # (one live row per wave is a tail turn)
    w = np.ones(65536, F32)
    assert "turn.zero_weight" not in R.rows_paths(65536, w)
    w[40000] = 0                                                             # one hole inside one full turn
    assert R.rows_paths(65536, w) == {"turn.all", "turn.zero_weight", "reduce.c=16"}
    assert R.rows_paths(0) == set() and R.shift_paths(0, 3) == set()


@pytest.mark.parametrize("K,D", [(1, 1), (20, 3), (120, 7), (3, 1500), (576, 65), (4096, 160), (4096, 512), (16384, 129)])
def test_shift_paths_equal_the_enumeration(K, D):
    assert R.shift_paths(K, D) == _brute_shift_paths(K, D)


def test_shift_paths_at_the_boundaries_the_issue_names():
    assert "grid.capped" not in R.shift_paths(4096, 160)                     # today's largest map: 640 workgroups
    assert R.shift_paths(4096, 160) >= {"grid.multi", "reduce.c=3", "reduce.ragged"}
    assert R.shift_paths(4096, 512) == {"grid.multi", "reduce.c=8"}          # exactly the cap: 2 048 workgroups, sd == 0
    assert R.shift_paths(16384, 129) == {"grid.capped", "grid.multi", "sd.nonzero", "carry", "reduce.c=8"}
    assert R.shift_paths(3, 1500) >= {"sk.zero", "sd.nonzero", "carry"}
    assert R.shift_paths(1, 1) == {"reduce.c=1"}


# what the issue's table says each case reaches
BIG_ROWS = {
    "f32-n81925": {"turn.all", "second_turn", "turn.tail", "reduce.c=16"},
    "f32-n65536-d130": {"turn.all", "reduce.c=16"},
    "weighted-n81925": {"turn.zero_weight", "turn.all", "second_turn", "turn.tail"},
    "masked-weighted-n70001-d65": {"turn.all", "turn.zero_weight", "second_turn", "turn.tail"},
    "exact-skip-n81925": {"turn.all", "second_turn", "turn.tail"},
    "f32-n1025": {"reduce.c=2", "reduce.ragged"},
    "shift-128x128x129": set(),
    "shift-masked-24x24x65": set(),
}
BIG_SHIFT = {
    "shift-128x128x129": {"grid.capped", "sd.nonzero", "carry", "reduce.c=8"},
    "shift-masked-24x24x65": {"grid.multi", "sd.nonzero", "carry"},
}


def test_big_cases_reach_the_paths_they_name():
    assert set(R.BIG_CASES) == set(BIG_ROWS)
    reached_rows, reached_shift = set(), set()
    for name, c in R.BIG_CASES.items():
        wt = R.big_case_weights(name)
        assert (wt is None) == (c["weights"] is None) and (wt is None or wt.shape == (c["n"],)), name
        rows = R.rows_paths(c["n"], wt)
        assert BIG_ROWS[name] <= rows, (name, rows)
        reached_rows |= rows
        sh = R.shift_paths(c["X"] * c["Y"], c["D"])
        assert BIG_SHIFT.get(name, set()) <= sh, (name, sh)
        reached_shift |= sh
    assert R.rows_paths(81925) == BIG_ROWS["f32-n81925"] and R.rows_paths(65536) == BIG_ROWS["f32-n65536-d130"]
    assert reached_rows >= {"turn.all", "turn.tail", "turn.zero_weight", "second_turn", "reduce.c=2", "reduce.c=16", "reduce.ragged"}
    assert reached_shift >= {"grid.capped", "grid.multi", "sd.nonzero", "carry", "reduce.c=8"}
    # the shapes and handles of the table
    assert {n: (c["X"], c["Y"], c["D"], c["n"]) for n, c in R.BIG_CASES.items()} == {
        "f32-n81925": (12, 10, 3, 81925), "f32-n65536-d130": (12, 10, 130, 65536), "weighted-n81925": (12, 10, 7, 81925),
        "masked-weighted-n70001-d65": (16, 16, 65, 70001), "exact-skip-n81925": (64, 64, 32, 81925), "f32-n1025": (12, 10, 7, 1025),
        "shift-128x128x129": (128, 128, 129, 300), "shift-masked-24x24x65": (24, 24, 65, 500)}
    assert {n for n, c in R.BIG_CASES.items() if c["masked"]} == {"masked-weighted-n70001-d65", "shift-masked-24x24x65"}
    assert [n for n, c in R.BIG_CASES.items() if c["kw"]["precision"] != "f32"] == ["exact-skip-n81925"]
    assert R.BIG_CASES["exact-skip-n81925"]["env"] == {"SOM_EXACT_SKIP": "2"}
    assert all(c["epochs"] == (4 if n == "exact-skip-n81925" else 2) for n, c in R.BIG_CASES.items())
    # 81 925 rows: waves 0 ... 4 hold two live rows in their second turn, the others one
    second = [sum(65536 + w + j * 16384 < 81925 for j in range(4)) for w in range(16384)]
    assert second[:5] == [2] * 5 and set(second[5:]) == {1}
    wt = R.big_case_weights("weighted-n81925")
    assert 0.05 * len(wt) < (wt == 0).sum() < 0.15 * len(wt)                 # a tenth zero
    x, wm = R.big_case_data("masked-weighted-n70001-d65")
    assert x.shape == (70001, 65) and np.isnan(x[7]).all() and wm[7] == 1 and set(np.unique(wm)) == {0.0, 1.0, 2.0}
    assert 0.25 < np.isnan(x).mean() < 0.35
    assert R.shift_grid(128 * 128 * 129) == 2048 and 2048 * 256 - (2048 * 256 // 129) * 129 == 32


# ------------------------------------------------------------------------------------------ the tight row check
def _emulated_record(d32, w, order):
    """sum_wd as a device could form it: the exact products added one by one in float64, in the given order."""
    terms = (np.ones(len(d32)) if w is None else w.astype(np.float64)) * d32.astype(np.float64)
    s = 0.0
    for v in terms[order].tolist():
        s += v
    return {"sum_wd": s}


@pytest.mark.parametrize("weighted", [False, True])
def test_check_rows_tight_accepts_any_order_and_rejects_one_wrong_row(weighted):
    n = 80000
    rs = np.random.RandomState(7 + weighted)
    d32 = np.sqrt(rs.chisquare(7, n)).astype(F32)                            # distances of 7-feature rows
    w = None
    if weighted:
        w = (rs.rand(n) * 2).astype(F32)
        w[rs.rand(n) < 0.1] = 0
    live = np.arange(n) if w is None else np.flatnonzero(w != 0)
    for seed in range(3):
        order = np.random.RandomState(seed).permutation(live)
        assert R.check_rows_tight(_emulated_record(d32, w, order), d32, w) <= 1.0
    assert R.check_rows_tight(_emulated_record(d32, w, live), d32, w) <= 1.0  # ascending
    assert R.check_rows_tight(_emulated_record(d32, w, live[::-1]), d32, w) <= 1.0
    heavy = live if w is None else live[w[live] >= 1]                        # (a row whose weight does not hide it)
    a, b = int(heavy[1234]), int(heavy[4321])
    assert d32[a] != d32[b]
    swapped = d32.copy()
    swapped[a] = d32[b]                                                      # one row's distance replaced by another row's
    wrong = {"one row's distance is another row's": _emulated_record(swapped, w, live),
             "one row left out": _emulated_record(d32, w, live[live != a]),
             "one row added twice": _emulated_record(d32, w, np.append(live, a))}
    for what, m in wrong.items():
        with pytest.raises(AssertionError, match="sum_wd"):
            R.check_rows_tight(m, d32, w, what)
    # one row's distance off by one part in 10^4: a hundredth of what gamma(D + 10) on the mean lets through, and caught here
    near = d32.copy()
    near[a] = F32(d32[a] * (1 + 1e-4))
    m = _emulated_record(near, w, live)
    ref = _emulated_record(d32, w, live)["sum_wd"]
    assert 0 < abs(m["sum_wd"] - ref) < 1e-2 * Q.gamma(7 + 10) * ref
    with pytest.raises(AssertionError, match="sum_wd"):
        R.check_rows_tight(m, d32, w)
    if weighted:                                                             # a zero-weight row read after all
        hole = int(np.flatnonzero(w == 0)[0])
        m = _emulated_record(d32, np.where(np.arange(n) == hole, F32(1), w), np.append(live, hole))
        with pytest.raises(AssertionError, match="sum_wd"):
            R.check_rows_tight(m, d32, w)
    assert R.check_rows_tight({"sum_wd": 0.0}, np.zeros(5, F32)) == 0.0
    with pytest.raises(AssertionError):
        R.check_rows_tight({"sum_wd": 1e-300}, np.zeros(5, F32))


def test_check_near_ties_accepts_a_tie_and_rejects_another_unit():
    rs = np.random.RandomState(0)
    x, w = rs.normal(0, 1, (50, 9)).astype(F32), rs.normal(0, 1, (30, 9)).astype(F32)
    ids = np.argmin(((x[:, None].astype(np.float64) - w[None]) ** 2).sum(axis=2), axis=1)
    other = (ids + 1) % 30
    with pytest.raises(AssertionError, match="no tie"):
        R.check_near_ties(x, w, ids, other, np.arange(5))
    tie = w.copy()
    tie[other[0]] = w[ids[0]]
    tie[other[0], 2] = np.nextafter(tie[other[0], 2], F32(9))                # one float32 ulp in one feature
    R.check_near_ties(x, tie, ids, other, np.arange(1))
    xm = x.copy()
    xm[0, 2] = np.nan                                                        # masked: the feature they differ in is not observed
    far = tie.copy()
    far[other[0], 2] += 100
    R.check_near_ties(xm, far, ids, other, np.arange(1), masked=True)
    with pytest.raises(AssertionError, match="no tie"):
        R.check_near_ties(x, far, ids, other, np.arange(1))


from xpysom_dask_amd import EpochRecord  # noqa: E402  (fails on a tree without the monitor, as every test here does)

R_FIELDS = EpochRecord._fields
