"""The exact mode's scratch on the device: what the handle's four owners HOLD (som_debug_exact_scratch_held) is what the rule of
csrc/exact_scratch.hpp says for the geometry the handle reports (som_debug_exact_scratch_sizes), case by case; the ids are the
float32 engine's; and the process's device bytes after every step of three sequences are the parent commit's, to the byte.
GPU only (`-m gpu`)."""
import gc

import numpy as np
import pytest

from oracle import som_oracle as O
from tests import exact_scratch_ref as E

pytestmark = pytest.mark.gpu
F32 = np.float32


def engine(X, Y, D, precision):
    from xpysom_dask_amd.engine import HipEngine
    return HipEngine(X, Y, D, precision=precision)


def device_bytes():
    import ctypes as C
    from xpysom_dask_amd import _lib
    v = C.c_int64()
    assert _lib.load().som_debug_device_bytes(C.byref(v)) == 0
    return v.value


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    for k in ("SOM_EXACT_SKIP", "SOM_EXACT_PASS_ROWS", "SOM_EXACT_DEBUG_REFUSE_ABOVE", "SOM_EXACT_DEBUG_REFUSE_SKIP", "SOM_EXACT_PAIRS"):
        monkeypatch.delenv(k, raising=False)


def rule(x, rows, stride=0):
    """The rule's block for `rows` rows at first_stride(rows, stride), on the geometry the handle reports."""
    return E.sizes(E.held(x)["geometry"], rows, stride)[2]


def assert_sorted(got, want, second_half):
    """A held sorted pass against the rule's: every buffer, the second half image held or not."""
    assert got == dict(want, Xl_s=want["Xl_s"] if second_half else 0), (got, want)


NOTHING_SORTED = dict.fromkeys(E.SORTED, 0)


# ------------------------------------------------------------------------------------------ the sequences
# Each yields (step, engine) after every step; the exact engine is the only live one while it runs, so the process's device bytes
# above the start are the handle's.  PARENT_BYTES holds those totals as the parent commit (c1dfa1a) reported them.
def seq_refused(ids):
    """32 x 32 x 24, 9 000 rows, a device that refuses passes above 2 500 rows (the caller sets the hook)."""
    X, Y, D, n = 32, 32, 24, 9000
    data = O.gaussian_blobs(n, D, seed=12)
    w = O.default_codebook(X, Y, D, 3).astype(F32)
    x = engine(X, Y, D, "exact")
    yield "create", x
    x.set_weights(w); x.set_data(data)
    yield "set_data", x
    x.epoch_accumulate(3.0, 0.4, True)
    ids["epoch"] = x.epoch_fetch()[2]
    yield "epoch", x
    ids["query"] = x.bmu(data[:777])
    yield "query", x
    x.close()


def seq_resident(ids):
    """64 x 64 x 32 under SOM_EXACT_SKIP=2 (the caller sets it): 20 000 resident rows, three epochs, a 5 000-row query."""
    X, Y, D, n = 64, 64, 32, 20000
    data = O.gaussian_blobs(n, D, seed=4)
    x = engine(X, Y, D, "exact")
    x.set_weights(O.default_codebook(X, Y, D, 6).astype(F32))
    yield "create", x
    x.set_data(data)
    yield "set_data", x
    for t in range(3):
        x.epoch_accumulate(O.exponential_decay(X / 2.0, 1.0, t, 6), O.exponential_decay(0.5, 0.01, t, 6), True)
        ids["epoch%d" % t] = x.epoch_fetch()[2]
        x.epoch_merge()
        yield "epoch%d" % t, x
    ids["query"] = x.bmu(data[:5000])
    yield "query", x
    x.close()


def seq_closed(ids):
    """test_closed_engines_give_back_every_device_byte's exact engine (tests/test_gpu_exact.py), step by step."""
    X, Y, D, n = 64, 64, 32, 20000
    data = O.gaussian_blobs(n, D, seed=4)
    x = engine(X, Y, D, "exact")
    x.set_weights(O.default_codebook(X, Y, D, 6).astype(F32))
    x.set_data(data)
    yield "set_data", x
    T = 6
    for t in range(T):
        x.epoch_accumulate(O.exponential_decay(X / 2.0, 1.0, t, T), O.exponential_decay(0.5, 0.01, t, T), True)
        x.epoch_merge()
    yield "epochs", x
    x.bmu(data[:5000])
    yield "query", x
    bufs = [x.pinned_empty((1000, D)), x.pinned_empty((1000, D))]

    def chunks():
        for i, lo in enumerate(range(0, 6000, 1000)):
            bufs[i & 1][:] = data[lo:lo + 1000]
            yield bufs[i & 1]
    x.stream_epoch_accumulate(chunks(), 1.0, 0.1, True)
    yield "streamed", x
    x.set_verify(64)
    x.epoch_accumulate(1.0, 0.1, True)
    yield "verified", x
    x.close()


SEQUENCES = {"refused": (seq_refused, {"SOM_EXACT_DEBUG_REFUSE_ABOVE": "2500"}),
             "resident": (seq_resident, {"SOM_EXACT_SKIP": "2"}),
             "closed": (seq_closed, {"SOM_EXACT_SKIP": "2"})}

# device bytes above the start after every step, as the parent commit c1dfa1a's library reported them for these same generators
PARENT_BYTES = {
    "refused": {"create": 888960, "set_data": 3073668, "epoch": 3147396, "query": 3458692},
    "resident": {"create": 4210848, "set_data": 25514080, "epoch0": 26972256, "epoch1": 26972256, "epoch2": 26972256, "query": 29536352},
    "closed": {"set_data": 25514080, "epochs": 26972256, "query": 29536352, "streamed": 30817240, "verified": 30826216},
}


def f32_ids(name):
    """The float32 engine's ids at the steps of a sequence that fetch some."""
    if name == "refused":
        X, Y, D, n = 32, 32, 24, 9000
        data = O.gaussian_blobs(n, D, seed=12)
        f = engine(X, Y, D, "f32")
        f.set_weights(O.default_codebook(X, Y, D, 3).astype(F32)); f.set_data(data)
        f.epoch_accumulate(3.0, 0.4, True)
        out = {"epoch": f.epoch_fetch()[2], "query": f.bmu(data[:777])}
    else:
        X, Y, D, n = 64, 64, 32, 20000
        data = O.gaussian_blobs(n, D, seed=4)
        f = engine(X, Y, D, "f32")
        f.set_weights(O.default_codebook(X, Y, D, 6).astype(F32)); f.set_data(data)
        out = {}
        for t in range(3):
            f.epoch_accumulate(O.exponential_decay(X / 2.0, 1.0, t, 6), O.exponential_decay(0.5, 0.01, t, 6), True)
            out["epoch%d" % t] = f.epoch_fetch()[2]
            f.epoch_merge()
        out["query"] = f.bmu(data[:5000])
    f.close()
    return out


def run(name, monkeypatch, check=None):
    """One sequence: ({step: device bytes above the start}, the ids it fetched); check(step, engine) after every step."""
    fn, env = SEQUENCES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gc.collect()                                          # (engines of earlier tests still waiting for their __del__)
    start = device_bytes()
    got, ids = {}, {}
    for step, x in fn(ids):
        got[step] = device_bytes() - start
        if check is not None:
            check(step, x)
    assert device_bytes() == start
    return got, ids


def same_ids(ids, ref):
    assert sorted(ids) == sorted(ref)
    for k in ids:
        assert np.array_equal(ids[k], ref[k]), (k, int((ids[k] != ref[k]).sum()))


# ------------------------------------------------------------------------------------------ held == rule
def test_refused_passes_hold_the_scratch_of_the_stride_that_fitted(monkeypatch):
    ref = f32_ids("refused")

    def check(step, x):
        h = E.held(x)
        if step == "create":
            assert h["pass"]["stride"] == 0 and h["pass"]["gmin"] == 0 and h["levels"] == 0
            return
        # 9 216 and 4 608 are refused, 2 304 fits; the 777-row query fits the same scratch.  A 32 x 32 map plans nothing by default
        want = rule(x, 9000, 2304)
        assert want["pass"]["stride"] == 2304 and E.sizes(h["geometry"], 9000)[0][:3] == [9216, 4608, 2304]
        assert h["pass"] == want["pass"], step
        assert h["levels"] == 0 and h["sorted"] == NOTHING_SORTED and h["plan"]["stride"] == 0 and h["plan"]["items"] == 0
    got, ids = run("refused", monkeypatch, check)
    same_ids(ids, ref)
    print("device bytes, refused:", got)
    assert got == PARENT_BYTES["refused"]


def test_resident_rows_a_query_and_the_parents_bytes(monkeypatch):
    ref = f32_ids("resident")

    def check(step, x):
        h = E.held(x)
        if step == "create":
            assert h["pass"]["stride"] == 0 and h["levels"] == 0 and h["sorted"] == NOTHING_SORTED and h["plan"]["stride"] == 0
            return
        want = rule(x, 20000)
        assert want["pass"]["stride"] == 20224 and want["sorted"]["cap"] == 20224 and want["levels"] == 2
        assert h["pass"] == want["pass"] and h["levels"] == 2 and h["cen"] == want["cen"] and h["plan"] == want["plan"], step
        # the second half image: not before a launch refines; SOM_EXACT_SKIP=2 refines in every planned launch, the first one included
        assert_sorted(h["sorted"], want["sorted"], second_half=step != "set_data")
        if step == "query":
            # the transient pass at the query's size (it refines too); nothing before
            assert_sorted(h["sorted1"], rule(x, 5000)["sorted"], second_half=True)
            assert h["sorted1"]["cap"] == 5120
        else:
            assert h["sorted1"] == NOTHING_SORTED
        assert h["fbX"] == 0 or h["fbX"] % (1024 * 32) == 0
    got, ids = run("resident", monkeypatch, check)
    same_ids(ids, ref)
    print("device bytes, resident:", got)
    assert got == PARENT_BYTES["resident"]


def test_the_closed_engines_sequence_holds_the_parents_bytes(monkeypatch):
    got, _ = run("closed", monkeypatch)
    print("device bytes, closed:", got)
    assert got == PARENT_BYTES["closed"]


def test_a_launch_that_samples_tiles_holds_the_transient_pass_for_them():
    """Default switches, 192 x 192 x 128, 65 792 query rows (tests/scout_ref.py's built data: the smallest launch whose forecast
    asks the sample tiles): srt[1] holds the query's pass, which covers the 128 sample tiles."""
    from tests import scout_ref as R
    w, rows = R.build(192, 192, 128)["commit"]
    f, x = engine(192, 192, 128, "f32"), engine(192, 192, 128, "exact")
    f.set_weights(w); x.set_weights(w)
    assert np.array_equal(f.bmu(rows), x.bmu(rows))
    assert x.exact_last_plan()["sample_tiles"] and x.exact_forecast()["n_st"] == 128
    h = E.held(x)
    want = rule(x, len(rows))
    assert h["sorted1"]["cap"] == want["sorted"]["cap"] >= 128 * 256 and h["sorted"] == NOTHING_SORTED
    assert {k: v for k, v in h["sorted1"].items() if k != "Xl_s"} == {k: v for k, v in want["sorted"].items() if k != "Xl_s"}
    assert h["pass"] == want["pass"] and h["plan"] == want["plan"] and h["cen"] == want["cen"]
    # a small query next: the pass of the sample tiles is the least the transient pass ever holds from here on
    assert np.array_equal(f.bmu(rows[:3000]), x.bmu(rows[:3000]))
    assert E.held(x)["sorted1"]["cap"] >= 128 * 256
    f.close(); x.close()


def test_refused_skipping_holds_no_sorted_pass_no_plan_and_no_centroids(monkeypatch):
    monkeypatch.setenv("SOM_EXACT_SKIP", "2")
    monkeypatch.setenv("SOM_EXACT_DEBUG_REFUSE_SKIP", "1")
    X, Y, D, n = 32, 32, 16, 4000
    data = O.gaussian_blobs(n, D, seed=3)
    w = O.default_codebook(X, Y, D, 2).astype(F32)
    f, x = engine(X, Y, D, "f32"), engine(X, Y, D, "exact")
    for e in (f, x):
        e.set_weights(w); e.set_data(data)
    for sig in (4.0, 2.0):
        f.epoch_accumulate(sig, 0.4, True); x.epoch_accumulate(sig, 0.4, True)
        assert np.array_equal(f.epoch_fetch()[2], x.epoch_fetch()[2])
        f.epoch_merge(); x.epoch_merge()
        h = E.held(x)
        assert h["levels"] == 0 and all(v == 0 for c in h["cen"] for v in c.values())
        assert h["sorted"] == NOTHING_SORTED and h["sorted1"] == NOTHING_SORTED
        assert all(v == 0 for v in h["plan"].values())
        assert h["pass"] == rule(x, n)["pass"]
    run_, total = x.exact_skip_stats()
    assert run_ == total > 0
    f.close(); x.close()


def test_a_wide_map_holds_one_centroid_level_and_the_plans_float32_scores(monkeypatch):
    monkeypatch.setenv("SOM_EXACT_SKIP", "2")
    X, Y, D, n = 64, 64, 136, 3000
    data = O.gaussian_blobs(n, D, seed=8)
    w = O.default_codebook(X, Y, D, 4).astype(F32)
    f, x = engine(X, Y, D, "f32"), engine(X, Y, D, "exact")
    for e in (f, x):
        e.set_weights(w); e.set_data(data)
    for sig in (6.0, 3.0):
        f.epoch_accumulate(sig, 0.4, True); x.epoch_accumulate(sig, 0.4, True)
        assert np.array_equal(f.epoch_fetch()[2], x.epoch_fetch()[2])
        f.epoch_merge(); x.epoch_merge()
    assert x.exact_resident_stats()[0] > 0                    # (an epoch ran under the wide plan)
    h = E.held(x)
    want = rule(x, n)
    assert h["geometry"]["wide"] == 1 and h["levels"] == want["levels"] == 1
    assert h["cen"] == want["cen"] and all(v == 0 for v in h["cen"][1].values())
    assert h["plan"] == want["plan"] and h["plan"]["tq"] == 3072 and h["plan"]["need2"] == 1
    assert h["pass"] == want["pass"]
    assert_sorted(h["sorted"], want["sorted"], second_half=False)     # (no refinement pass beyond 128 features)
    f.close(); x.close()


def test_more_rows_on_the_same_handle_grow_every_owner_to_the_rule(monkeypatch):
    monkeypatch.setenv("SOM_EXACT_SKIP", "2")
    X, Y, D = 64, 64, 16
    w = O.default_codebook(X, Y, D, 5).astype(F32)
    f, x = engine(X, Y, D, "f32"), engine(X, Y, D, "exact")
    for e in (f, x):
        e.set_weights(w)
    held_rows = 0
    for n in (5000, 12000, 7000):
        data = O.gaussian_blobs(n, D, seed=n)
        for e in (f, x):
            e.set_data(data)
        held_rows = max(held_rows, n)                         # (the owners only ever grow)
        for step in ("set_data", "epoch"):
            if step == "epoch":
                f.epoch_accumulate(4.0, 0.3, True); x.epoch_accumulate(4.0, 0.3, True)
                assert np.array_equal(f.epoch_fetch()[2], x.epoch_fetch()[2]), n
                f.epoch_merge(); x.epoch_merge()
            h, want = E.held(x), rule(x, held_rows)
            assert h["pass"] == want["pass"] and h["plan"] == want["plan"] and h["cen"] == want["cen"], (n, step)
            # (a grown sorted pass is a new one: its second half image comes back with the next launch that refines)
            assert_sorted(h["sorted"], want["sorted"], second_half=step == "epoch" or n == 7000)
    f.close(); x.close()
