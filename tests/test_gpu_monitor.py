"""The training monitor on the device (som_monitor / som_epoch_measure_rows / som_epoch_measure_shift / som_epoch_metrics).
GPU only (`-m gpu`).

Every case runs at engine level, stage by stage: epoch_accumulate, epoch_fetch for the ids the epoch's own search found,
epoch_measure_rows, epoch_measure_shift, get_weights before and after epoch_merge, epoch_metrics -- and holds the record against
tests/monitor_ref.py's float64 model on those ids and codebooks:
  rows, changed   exact
  QE              within gamma(D + 10) ref (query_ref.check_qe's bound)
  shift_max       exactly float32's max |W' - W|
  shift_sumsq     within K D 2^-52 relative of the float64 sum of the squares
Shapes: the smallest that reach each path (named at the case list).  monitor_ref.BIG_CASES are the shapes past one turn of the
kernels' loops -- the all-live instance of the unrolled row chains, a second turn, a zero-weight row inside a full turn, the
capped shift grid, a ragged reduction --; there the Euclidean record's sum_wd is also held to the float32 distances
bmu_distances returns for the same rows, within 2 rows 2^-53 (monitor_ref.check_rows_tight): one misread row fails it.  Then
three equalities bit for bit -- two monitored runs, the XPySom history against the stage-by-stage replay, the monitored against
the unmonitored codebook -- and the state errors."""
import contextlib
import math
import os

import numpy as np
import pytest

from oracle import som_oracle as O
from tests import monitor_ref as R
from tests import query_ref as Q

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SCHEDULE = ((3.0, 0.5, 1), (2.0, 0.4, 0), (1.5, 0.3, 1), (1.0, 0.2, 0), (0.8, 0.1, 1))   # (sigma, eta, neigh_f64) per epoch


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def engine(X, Y, D, env=None, **kw):
    from xpysom_dask_amd.engine import HipEngine
    with _env(**(env or {})):                                # (the library reads its switches in som_create)
        return HipEngine(X, Y, D, **kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def codebook(X, Y, D, seed=3):
    return O.default_codebook(X, Y, D, seed).astype(F32).reshape(X * Y, D)


def record_bits(m):
    """A record as comparable bits (NaN-safe)."""
    return (np.array([m["sum_wd"], m["sum_w"], m["shift_sumsq"]], F64).tobytes(), m["rows"], m["changed"],
            np.array([m["shift_max"]], F32).tobytes())


def replay(e, x, w0, epochs=4, weights=None, masked=False, check=True, monitored=True, tight=False, what=""):
    """`epochs` epochs stage by stage on engine `e`; every record checked against the model.  tight: also against the float32
    distances e.bmu_distances(x) returns under the epoch's codebook (distances_under).  Returns (records, final codebook)."""
    e.set_weights(w0)
    e.set_data(x)
    if weights is not None:
        e.set_sample_weights(weights)
    if monitored:
        e.monitor(True)
    prev, out = None, []
    for t in range(epochs):
        sigma, eta, f64 = SCHEDULE[t]
        w_old = e.get_weights()
        if tight and check and monitored:
            q_ids, q_d = e.bmu_distances(x)                  # (the query's own row set: the resident rows are untouched)
        e.epoch_accumulate(sigma, eta, f64)
        if not monitored:
            e.epoch_merge()
            continue
        num, den, ids = e.epoch_fetch_masked() if masked else e.epoch_fetch()
        e.epoch_measure_rows()
        e.epoch_measure_shift()
        e.epoch_merge()
        w_new = e.get_weights()
        m = e.epoch_metrics()
        out.append(m)
        if check:
            tag = "%s epoch %d" % (what, t)
            assert (ids >= 0).all() and (ids < e.K).all()
            qr = R.check_rows(m, x, w_old, ids, weights, prev, masked, tag)
            assert np.array_equal(bits(w_new), bits(R.merged(w_old, num, den))), tag + ": the merge is not num / den"
            sr = R.check_shift(m, w_old, w_new, tag)
            print("%s: rows %d changed %d QE %.9g (err/bound %.3g) shift %.9g max %.9g (err/bound %.3g)"
                  % (tag, m["rows"], m["changed"], R.qe_of(m), qr, math.sqrt(m["shift_sumsq"]), m["shift_max"], sr))
            if tight:
                d32, ties = distances_under(x, w_old, ids, q_ids, q_d, masked, tag)
                print("%s: sum_wd against the float32 distances: err/bound %.3g (%d rows re-scored at the epoch's unit)"
                      % (tag, R.check_rows_tight(m, d32, weights, tag), ties))
            assert m["shift_sumsq"] > 0 or len(x) == 0
        prev = ids
    return out, e.get_weights()


def distances_under(x, w, ids, q_ids, q_d, masked, what):
    """bmu_dist_kernel's float32 distance of every row to the unit the EPOCH gave it.  bmu_distances names the quantization
    search's unit (the differences themselves), the epoch the training search's (|w|^2 - 2 x.w): on a tie at float32's
    resolution the two may differ.  Such a row is held to be a tie (monitor_ref.check_near_ties) and its distance is taken
    again from the same kernel on a 5 x 4 handle whose every unit is the epoch's unit -- the float32 depends on the row, the unit
    and D alone.  Returns (distances, rows re-scored)."""
    diff = np.flatnonzero(q_ids != ids)
    if len(diff) == 0:
        return q_d, 0
    R.check_near_ties(x, w, ids, q_ids, diff, masked, what)
    d32 = q_d.copy()
    D = x.shape[1]
    f = engine(5, 4, D, precision="f32", **({"missing": "nan"} if masked else {}))
    try:
        for k in np.unique(ids[diff]):
            rows = diff[ids[diff] == k]
            f.set_weights(np.repeat(w[k][None, :], 20, axis=0))
            d32[rows] = f.bmu_distances(x[rows])[1]
    finally:
        f.close()
    return d32, len(diff)


def _masked_case(n=500, D=9, seed=5):
    return R.masked_rows(n, D, seed)                         # 30 % missing, row 7 entirely; weights 0, 1, 2


# name: (X, Y, D, n, engine keywords, environment)
CASES = {
    # odd D; 1 003 rows: tails against the 4 rows of a workgroup and the 256 partials' runs
    "f32": (12, 10, 7, 1003, dict(precision="f32"), {}),
    # the exact mode under a plan: block skipping and the resident sorted pass (SOM_EXACT_SKIP=2: planned from the first epoch)
    "exact-skip": (64, 64, 32, 20000, dict(precision="exact"), {"SOM_EXACT_SKIP": "2"}),
    "exact-wide": (64, 64, 160, 2048, dict(precision="exact"), {}),
    "bf16": (20, 20, 64, 777, dict(precision="bf16"), {}),
    "cosine-mexican": (9, 9, 6, 300, dict(precision="f32", distance="cosine", neighborhood="mexican_hat"), {}),
    "torus-bubble": (8, 8, 3, 257, dict(precision="f32", topology="toroidal", neighborhood="bubble"), {}),
    "one-row": (5, 4, 3, 1, dict(precision="f32"), {}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_records_against_the_model(name):
    X, Y, D, n, kw, env = CASES[name]
    x = O.gaussian_blobs(n, D, seed=11) if name.startswith("exact") else Q.make_rows("blobs", n, D, 11 + D)
    e = engine(X, Y, D, env, **kw)
    try:
        recs, _ = replay(e, x, codebook(X, Y, D), what=name)
        if name == "exact-skip":
            planned, sorts = e.exact_resident_stats()
            run, total = e.exact_skip_stats()
            assert planned >= 3 and sorts >= 1 and run < total, (planned, sorts, run, total)
    finally:
        e.close()
    assert [m["changed"] >= 0 for m in recs] == [False, True, True, True]
    assert all(m["rows"] == n and m["sum_w"] == float(n) for m in recs)
    if n > 100:
        assert any(m["changed"] > 0 for m in recs[1:])


@pytest.mark.parametrize("name", list(R.BIG_CASES))
def test_records_past_one_turn(name):
    """monitor_ref.BIG_CASES: what each reaches is pinned by tests/test_monitor_cpu.py.  Every epoch holds check_rows, check_shift,
    exact rows and changed, the merge, and sum_wd against the float32 distances of bmu_distances."""
    c = R.BIG_CASES[name]
    X, Y, D, n, epochs = c["X"], c["Y"], c["D"], c["n"], c["epochs"]
    x, wt = R.big_case_data(name)
    assert x.shape == (n, D)
    e = engine(X, Y, D, c["env"], **c["kw"])
    try:
        recs, _ = replay(e, x, codebook(X, Y, D), epochs=epochs, weights=wt, masked=c["masked"], tight=True, what=name)
        if name.startswith("exact-skip"):
            planned, sorts = e.exact_resident_stats()
            run, total = e.exact_skip_stats()
            assert planned >= 3 and sorts >= 1 and run < total, (planned, sorts, run, total)
    finally:
        e.close()
    assert len(recs) == epochs and [m["changed"] >= 0 for m in recs] == [False] + [True] * (epochs - 1)
    if wt is None:
        assert all(m["rows"] == n and m["sum_w"] == float(n) for m in recs)
    else:
        assert all(m["rows"] == int((wt != 0).sum()) for m in recs)          # the non-zero weights, exactly
        if c["weights"] == "012":                            # small integers: their double sum is exact in any order
            assert all(m["sum_w"] == float(wt.sum(dtype=F64)) for m in recs)
    assert any(m["changed"] > 0 for m in recs[1:])


def test_missing_values_with_weights():
    x, w = _masked_case()
    e = engine(16, 16, 9, precision="f32", missing="nan")
    try:
        recs, _ = replay(e, x, codebook(16, 16, 9), weights=w, masked=True, what="masked")
    finally:
        e.close()
    assert all(m["rows"] == int((w > 0).sum()) and m["sum_w"] == float(w.sum()) for m in recs)


def test_staged_blocks():
    """130 x 4 x 3: two 128-row blocks.  measure_shift is refused until the last block is done, and the record equals the
    monolithic epoch's bit for bit."""
    from xpysom_dask_amd.engine import SomHipError
    X, Y, D, n = 130, 4, 3, 600
    x, w0 = Q.make_rows("blobs", n, D, 14), codebook(X, Y, D)
    a, b = engine(X, Y, D, precision="f32"), engine(X, Y, D, precision="f32")
    try:
        mono, w_mono = replay(a, x, w0, what="staged/mono")
        b.set_weights(w0)
        b.set_data(x)
        b.monitor(True)
        for t in range(4):
            sigma, eta, f64 = SCHEDULE[t]
            b.epoch_accumulate_begin(sigma, eta, f64)
            b.epoch_measure_rows()
            nb = b.epoch_block_count()
            assert nb == 2
            for blk in range(nb):
                with pytest.raises(SomHipError, match="staged blocks"):
                    b.epoch_measure_shift()
                b.epoch_accumulate_block(blk)
            b.epoch_measure_shift()
            b.epoch_merge()
            assert record_bits(b.epoch_metrics()) == record_bits(mono[t]), t
        assert np.array_equal(bits(b.get_weights()), bits(w_mono))
    finally:
        a.close()
        b.close()


def test_graph_replays_are_followed_by_the_eager_launches():
    """SOM_GRAPH=1, five epochs: the first runs eagerly, the second is captured, epochs 3 to 5 are replays.  Every record is checked
    against the model and equals the eager engine's bit for bit."""
    X, Y, D, n, kw, _ = CASES["f32"]
    x, w0 = Q.make_rows("blobs", n, D, 11 + D), codebook(X, Y, D)
    g, e = engine(X, Y, D, {"SOM_GRAPH": "1"}, **kw), engine(X, Y, D, {"SOM_GRAPH": "0"}, **kw)
    try:
        rg, wg = replay(g, x, w0, epochs=5, what="graph")
        re_, we = replay(e, x, w0, epochs=5, check=False)
    finally:
        g.close()
        e.close()
    assert [record_bits(m) for m in rg] == [record_bits(m) for m in re_]
    assert np.array_equal(bits(wg), bits(we))


@pytest.mark.parametrize("pinned", [False, True])
def test_streamed_chunks(pinned):
    """Chunks of 700, 1 and 1 300 rows on 10 x 10 x 5: the epoch's totals are the model's over the concatenation (ids: the same
    handle's search of the same rows under the same codebook), `changed` stays unknown."""
    X, Y, D = 10, 10, 5
    x = Q.make_rows("blobs", 2001, D, 17)
    cuts = [0, 700, 701, 2001]
    e = engine(X, Y, D, precision="f32")
    try:
        e.set_weights(codebook(X, Y, D))
        e.monitor(True)
        bufs = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            buf = e.pinned_empty((b - a, D)) if pinned else np.empty((b - a, D), F32)
            buf[:] = x[a:b]
            bufs.append(buf)
        for t in range(4):
            sigma, eta, f64 = SCHEDULE[t]
            w_old = e.get_weights()
            ids = e.bmu(x)
            e.stream_epoch_accumulate(iter(bufs), sigma, eta, f64)
            e.epoch_measure_shift()
            e.epoch_merge()
            w_new = e.get_weights()
            m = e.epoch_metrics()
            tag = "streamed%s epoch %d" % ("/pinned" if pinned else "", t)
            assert m["changed"] == -1
            qr = R.check_rows(m, x, w_old, ids, what=tag)
            sr = R.check_shift(m, w_old, w_new, tag)
            print("%s: rows %d QE %.9g (err/bound %.3g) shift %.9g (err/bound %.3g)" % (tag, m["rows"], R.qe_of(m), qr,
                                                                                     math.sqrt(m["shift_sumsq"]), sr))
    finally:
        e.close()


def test_empty_row_set():
    """A rank's empty shard: rows 0, sums 0, and NaN as the quantization error at Python level; the shift is 0 (nothing merged)."""
    from xpysom_dask_amd import XPySom
    som = XPySom(5, 4, 3, random_seed=3, precision="f32").train(np.zeros((0, 3), F32), 2, monitor=True)
    assert len(som.history) == 2
    for r in som.history:
        assert r.rows == 0 and r.weight == 0.0 and math.isnan(r.quantization_error)
        assert r.codebook_shift == 0.0 and r.codebook_shift_max == 0.0
    assert som.history[0].bmu_changed is None and som.history[1].bmu_changed == 0


EQ_CASES = {
    "f32": (CASES["f32"], False),
    "exact": (CASES["exact-skip"], False),
    "masked": ((16, 16, 9, 500, dict(precision="exact", missing="nan"), {}), True),
    # the all-live chains and a second turn: their tree, run twice
    "f32-n81925": (tuple(R.BIG_CASES["f32-n81925"][k] for k in ("X", "Y", "D", "n", "kw", "env")), False),
}


@pytest.mark.parametrize("name", list(EQ_CASES))
def test_two_monitored_runs_and_the_unmonitored_codebook(name):
    """(a) two monitored runs return identical records; (c) the monitored schedule trains the unmonitored codebook, bit for bit."""
    (X, Y, D, n, kw, env), masked = EQ_CASES[name]
    if masked:
        x, wt = _masked_case(n, D)
    else:
        x, wt = (O.gaussian_blobs(n, D, seed=11) if name == "exact" else Q.make_rows("blobs", n, D, 11 + D)), None
    w0 = codebook(X, Y, D)
    epochs = R.BIG_CASES[name]["epochs"] if name in R.BIG_CASES else 4
    runs = []
    for monitored in (True, True, False):
        e = engine(X, Y, D, env, **kw)
        try:
            runs.append(replay(e, x, w0, epochs=epochs, weights=wt, masked=masked, check=False, monitored=monitored))
        finally:
            e.close()
    assert len(runs[0][0]) == epochs and [record_bits(m) for m in runs[0][0]] == [record_bits(m) for m in runs[1][0]]
    assert np.array_equal(bits(runs[0][1]), bits(runs[1][1]))
    assert np.array_equal(bits(runs[0][1]), bits(runs[2][1])), "the monitor changed the trained codebook"


@pytest.mark.parametrize("precision", ["f32", "exact"])
def test_history_equals_the_stage_by_stage_replay(precision):
    """(b) XPySom.train(..., monitor=True).history is what the engine-level calls return for the same schedule, bit for bit."""
    from xpysom_dask_amd import XPySom
    from xpysom_dask_amd.xpysom import _epoch_record
    X, Y, D, n, T = 12, 10, 7, 1003, 4
    x = Q.make_rows("blobs", n, D, 18)
    som = XPySom(X, Y, D, random_seed=3, precision=precision)
    w0 = np.asarray(som._weights, F32).reshape(X * Y, D)
    som.train(x, T, monitor=True)
    unmon = XPySom(X, Y, D, random_seed=3, precision=precision).train(x, T)
    assert np.array_equal(bits(som._weights), bits(unmon._weights)) and unmon.history == []
    e = engine(X, Y, D, precision=precision)
    try:
        e.set_weights(w0)
        e.set_data(x)
        e.monitor(True)
        want = []
        for t in range(T):
            eta = som._decay_function(som._learning_rate, som._learning_rateN, t, T)
            sig = som._decay_function(som._sigma, som._sigmaN, t, T)
            e.epoch_accumulate(sig, eta, isinstance(sig, np.generic))
            e.epoch_measure_rows()
            e.epoch_measure_shift()
            e.epoch_merge()
            want.append(_epoch_record(t, sig, eta, e.epoch_metrics()))
        assert np.array_equal(bits(e.get_weights()), bits(som._weights).reshape(X * Y, D))
    finally:
        e.close()
    assert som.history == want and som.history[0].bmu_changed is None and som.history[1].bmu_changed is not None
    assert all(r.quantization_error > 0 and r.codebook_shift >= r.codebook_shift_max > 0 for r in som.history)


def test_state_errors():
    from xpysom_dask_amd.engine import SomHipError
    X, Y, D = 6, 5, 4
    x = Q.make_rows("blobs", 50, D, 3)
    e = engine(X, Y, D, precision="f32")
    try:
        e.set_weights(codebook(X, Y, D))
        e.set_data(x)
        e.epoch_accumulate(2.0, 0.5, 0)
        for call in (e.epoch_measure_rows, e.epoch_measure_shift, e.epoch_metrics):
            with pytest.raises(SomHipError, match="monitor is off"):
                call()
        e.epoch_merge()
        e.monitor(True)
        with pytest.raises(SomHipError, match="no search"):              # nothing searched since the merge
            e.epoch_measure_rows()
        e.epoch_accumulate(2.0, 0.5, 0)
        e.epoch_measure_rows()
        e.epoch_measure_shift()
        e.epoch_merge()
        m = e.epoch_metrics()
        assert m["rows"] == 50 and m["changed"] == -1
        with pytest.raises(SomHipError, match="no search"):
            e.epoch_measure_rows()
        e.set_data(x)                                                    # new rows: last epoch's ids are not theirs
        e.epoch_accumulate(1.5, 0.5, 0)
        e.epoch_measure_rows()
        e.epoch_measure_shift()
        e.epoch_merge()
        assert e.epoch_metrics()["changed"] == -1
        e.monitor(False)
        with pytest.raises(SomHipError, match="monitor is off"):
            e.epoch_metrics()
    finally:
        e.close()
