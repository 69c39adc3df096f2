"""Exact mode, euclidean, under a plan: the candidate selection inside the listed screen's launch (the select tail of
csrc/bmu_bf16_k16.hpp, the default) against the launch of exact_select_kernel behind the screen that it replaces
(SOM_EXACT_FUSE_SELECT=0).

The tail decides what the kernel decides: the same threshold from the same float expression, the same walk over the same
masks and values.  Every case runs the same seeded epochs on two fresh engines, one per setting, both under SOM_EXACT_SKIP=2
(small maps are planned, and the measured-cost decisions are out of the policy: both engines plan alike), and asserts epoch
by epoch and bit for bit: the BMU ids, the codebook after the merge, exact_skip_stats(), exact_stats(),
exact_resident_stats(), exact_refine_stats() and exact_last_counts() -- the rows' candidate counts of the last pass, the
selection's direct output.  (The order inside a group's row list depends on the order of atomics on either path and is not
compared.)  exact_select_stats() says which path ran: a planned pass of the fused engine selects in its screen and launches
no select kernel, the reference engine does the reverse.  Shapes: the smallest that reach each branch."""
import contextlib
import os

import numpy as np
import pytest

from xpysom_dask_amd.synthetic import gaussian_blobs

pytestmark = pytest.mark.gpu

N_ROWS = 4096
TILE = 256                                   # rows per tile of the plan (SK_TILE)
SIGMAS8 = (6.0, 4.0, 3.0, 2.0, 1.5, 1.2, 1.0, 0.8)
SIGMAS6 = (6.0, 4.0, 3.0, 2.0, 1.5, 1.0)


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


def _engine(fused, x, y, d, env, precision="exact", **kw):
    from xpysom_dask_amd.engine import HipEngine
    # (the library reads the switches in som_create; SOM_EXACT_FUSE_SELECT and the hooks in `env` only under SOM_TEST_HOOKS=1,
    #  which conftest sets)
    with _env(SOM_EXACT_FUSE_SELECT="1" if fused else "0", SOM_EXACT_SKIP="2", **(env or {})):
        return HipEngine(x, y, d, precision=precision, **kw)


def _codebook(x, y, d, seed):
    return np.random.default_rng(seed).normal(0.0, 2.0, size=(x * y, d)).astype(np.float32)


def _state(eng, ids, n_last, epoch=True):
    """n_last: the rows of the launch's last pass (what exact_last_counts can give); epoch: a training step (planned)."""
    return {"ids": ids, "w": eng.get_weights(), "skip": eng.exact_skip_stats(), "stats": eng.exact_stats(),
            "resident": eng.exact_resident_stats(), "refine": eng.exact_refine_stats(), "counts": eng.exact_last_counts(n_last),
            "select": eng.exact_select_stats(), "epoch": epoch}


def _last_pass_rows(n, env):
    p = int((env or {}).get("SOM_EXACT_PASS_ROWS", "0"))
    return n if p <= 0 else n - (n - 1) // p * p


def _run(fused, x, y, d, *, rows, w0, sigmas, env=None, between=None, precision="exact", **kw):
    """The record of one engine, a step per epoch.  between = (epoch, fn): fn(engine, record) runs after that epoch's merge."""
    eng = _engine(fused, x, y, d, env, precision=precision, **kw)
    rec = []
    n_last = _last_pass_rows(len(rows), env)
    try:
        eng.set_weights(w0)
        eng.set_data(rows)
        for e, sigma in enumerate(sigmas):
            eng.epoch_accumulate(sigma, 0.5, 1)
            ids = eng.epoch_fetch()[2]
            eng.epoch_merge()
            rec.append(_state(eng, ids, n_last) if precision == "exact" else {"ids": ids, "w": eng.get_weights()})
            if between is not None and between[0] == e:
                n_last = between[1](eng, rec) or n_last
    finally:
        eng.close()
    return rec


def _same_bits(a, b):
    return a.shape == b.shape and a.view(np.uint32).tobytes() == b.view(np.uint32).tobytes()


def _deltas(rec, key):
    """Per step, what the step added to the counters of `key`."""
    prev = None
    out = []
    for r in rec:
        cur = np.array(r[key], dtype=np.int64)
        out.append(cur - (0 if prev is None else prev))
        prev = cur
    return out


def _compare(x, y, d, *, queue=True, **kw):
    """Both engines' records, compared; returns the fused engine's.  queue False: the grid path -- no tail on either engine."""
    ref, got = _run(False, x, y, d, **kw), _run(True, x, y, d, **kw)
    assert len(ref) == len(got)
    for e, (r, g) in enumerate(zip(ref, got)):
        assert np.array_equal(r["ids"], g["ids"]), "step %d: BMU ids differ in %d rows" % (e, int((r["ids"] != g["ids"]).sum()))
        assert _same_bits(r["w"], g["w"]), "step %d: the codebooks differ" % e
        for key in ("skip", "stats", "resident", "refine"):
            assert r[key] == g[key], "step %d: exact_%s_stats %r != %r" % (e, key, g[key], r[key])
        assert np.array_equal(r["counts"], g["counts"]), \
            "step %d: the candidate counts differ in %d rows" % (e, int((r["counts"] != g["counts"]).sum()))
    # which path ran: every screen pass either selected in its screen or launched the select kernel; the planned passes of the
    # fused engine did the former -- on the work queue --, every pass of the reference engine the latter
    d_ref, d_got = _deltas(ref, "select"), _deltas(got, "select")
    d_pass = [int(v[2]) for v in _deltas(got, "stats")]
    for e, (r, g) in enumerate(zip(d_ref, d_got)):
        print("step %d: passes %d, select stats (fused, launched, ticket tiles): fused engine %s, reference %s"
              % (e, d_pass[e], tuple(g), tuple(r)))
        assert r[0] == 0 and r[2] == 0, "step %d: the reference engine selected in its screen: %r" % (e, tuple(r))
        if not got[e]["epoch"]:
            continue
        assert r[1] == d_pass[e] > 0, "step %d: the reference engine launched %d select kernels in %d passes" % (e, r[1], d_pass[e])
        if queue:
            assert g[0] == d_pass[e] and g[1] == 0, "step %d: the fused engine's planned passes: %r of %d" % (e, tuple(g), d_pass[e])
        else:
            assert tuple(g) == (0, d_pass[e], 0), "step %d: the grid path keeps the launched select: %r" % (e, tuple(g))
    return got


def _planned_throughout(rec):
    run, total = rec[-1]["skip"]
    planned, sorted_ = rec[-1]["resident"]
    assert 0 < run <= total and planned == len(rec), (rec[-1]["skip"], rec[-1]["resident"])


# 1: 4 groups and 16 tiles; the default schedule (on maps this small it sorts and scouts in most epochs) and an order kept for
#    three epochs -- and the float32 mode trains the same map (the mode's invariant)
@pytest.mark.parametrize("env", [{}, {"SOM_EXACT_RESORT": "3"}])
def test_fused_small_map(env):
    rows = gaussian_blobs(N_ROWS, 16, seed=31)
    w0 = _codebook(16, 16, 16, 3)
    got = _compare(16, 16, 16, rows=rows, w0=w0, sigmas=SIGMAS8, env=env)
    _planned_throughout(got)
    f32 = _run(True, 16, 16, 16, rows=rows, w0=w0, sigmas=SIGMAS8, precision="f32")
    assert _same_bits(f32[-1]["w"], got[-1]["w"]), "precision='exact' left the float32 trajectory"
    assert all(np.array_equal(a["ids"], b["ids"]) for a, b in zip(f32, got))


# 2: the TICKET path.  With 16 tiles an item's length is the 32-block floor (exact_list_totals_body): every tile that lists more
#    than 32 of its 16-unit blocks is cut (32 x 32: 64 blocks a tile, two parts; 64 x 64: 256 blocks, up to eight parts).  Both
#    kinds of tile must occur: cut ones (selected by the last part to arrive) and whole ones (selected by the workgroup that
#    walked them).  The random codebook of the first epoch lists everything; rows from 16 well separated blobs (a tile of the
#    sorted rows is about one blob) then leave tiles with short lists beside tiles that straddle blobs -- with the 64 blobs of
#    the other cases every tile of these maps stayed above 32 blocks in every epoch (measured: 16 of 16 tiles cut throughout).
#    SOM_EXACT_QUEUE=25: an item's length as 25 % of the mean list (the floor still holds at this size).
@pytest.mark.parametrize("x,y,d,env", [(32, 32, 16, {}), (64, 64, 32, {}), (64, 64, 32, {"SOM_EXACT_QUEUE": "25"})])
def test_fused_ticket_path(x, y, d, env):
    rows = gaussian_blobs(N_ROWS, d, seed=32, centres=16)
    got = _compare(x, y, d, rows=rows, w0=_codebook(x, y, d, 4), sigmas=SIGMAS8, env=env)
    _planned_throughout(got)
    tiles = N_ROWS // TILE
    ticket = [int(v[2]) for v in _deltas(got, "select")]
    print("ticket tiles per epoch (of %d tiles): %r" % (tiles, ticket))
    assert all(0 <= t <= tiles for t in ticket), ticket
    assert any(t > 0 for t in ticket), "no epoch cut a tile into parts: %r" % (ticket,)
    assert any(t < tiles for t in ticket), "no epoch had a tile with a single item: %r" % (ticket,)


# ... and the grid path (SOM_EXACT_QUEUE=0: a workgroup per tile and part, no queue): it keeps the launched select
def test_fused_grid_path_keeps_the_select_kernel():
    rows = gaussian_blobs(N_ROWS, 32, seed=32, centres=16)
    got = _compare(64, 64, 32, rows=rows, w0=_codebook(64, 64, 32, 4), sigmas=SIGMAS6, env={"SOM_EXACT_QUEUE": "0"}, queue=False)
    _planned_throughout(got)


# 3: three passes an epoch (passes of 1 024 rows over 3 000 rows): the last pass's last tile and its last 64-row block are
#    partial -- rows >= N select nothing and write nothing (the counts and the pass's pair totals stay equal)
def test_fused_several_passes_partial_tile():
    rows = gaussian_blobs(3000, 16, seed=33)
    got = _compare(16, 16, 16, rows=rows, w0=_codebook(16, 16, 16, 6), sigmas=SIGMAS6,
                   env={"SOM_EXACT_RESORT": "3", "SOM_EXACT_PASS_ROWS": "1024"})
    _planned_throughout(got)
    assert got[-1]["stats"][2] == len(SIGMAS6) * 3            # (screen passes)
    assert got[-1]["select"][0] == len(SIGMAS6) * 3


# 4: the refinement pass on and off (SOM_EXACT_REFINE): with it rowmin2 starts from the tail's all-ones
def test_fused_refinement_on_and_off():
    rows = gaussian_blobs(N_ROWS, 32, seed=34)
    w0 = _codebook(32, 32, 32, 5)
    on = _compare(32, 32, 32, rows=rows, w0=w0, sigmas=SIGMAS6, env={"SOM_EXACT_RESORT": "3", "SOM_EXACT_REFINE": "1"})
    off = _compare(32, 32, 32, rows=rows, w0=w0, sigmas=SIGMAS6, env={"SOM_EXACT_RESORT": "3", "SOM_EXACT_REFINE": "0"})
    on_x, off_x = on[-1]["refine"], off[-1]["refine"]
    assert on_x[0] > 0 and 0 < on_x[1] <= on_x[0] and off_x == (0, 0), (on_x, off_x)
    for a, b in zip(on, off):
        assert np.array_equal(a["ids"], b["ids"]) and _same_bits(a["w"], b["w"])


# 5: a row of NaN, a row of infinities: thresholds that are not finite, rows for the float32 fallback kernel in every epoch
#    (bubble: the two rows poison the units in their reach only)
def test_fused_fallback_rows():
    rows = gaussian_blobs(N_ROWS, 16, seed=35)
    rows[7] = np.nan
    rows[9] = np.inf
    got = _compare(16, 16, 16, rows=rows, w0=_codebook(16, 16, 16, 7), sigmas=(2.0, 1.5, 1.5, 1.2, 1.0, 1.0),
                   env={"SOM_EXACT_RESORT": "1000"}, neighborhood="bubble")
    fb = [g["stats"][1] for g in got]
    assert fb[0] > 0 and all(b > a for a, b in zip(fb, fb[1:])), fb        # (rows fell back in every epoch)


# 6: four 32-feature steps: the headline's instance of the listed screen
def test_fused_128_features():
    rows = gaussian_blobs(N_ROWS, 128, seed=36)
    got = _compare(32, 32, 128, rows=rows, w0=_codebook(32, 32, 128, 9), sigmas=SIGMAS6, env={"SOM_EXACT_RESORT": "3"})
    _planned_throughout(got)


# 7: between two epochs set_weights, a query over other rows (a transient pass under a plan), quantization_error; later a
#    second set_data with other rows
def test_fused_between_epochs():
    rows = gaussian_blobs(N_ROWS, 16, seed=37)
    other = gaussian_blobs(2500, 16, seed=38)
    w0 = _codebook(16, 16, 16, 8)

    def moved(eng, rec):
        eng.set_weights(w0[::-1].copy())
        rec.append(_state(eng, eng.bmu(other[:300]), 300, epoch=False))
        qe = eng.quantization_error(rows[:500])
        rec.append(_state(eng, np.array([qe], dtype=np.float64).view(np.int64), 300, epoch=False))

    def new_rows(eng, rec):
        eng.set_data(other)
        return len(other)

    got = _compare(16, 16, 16, rows=rows, w0=w0, sigmas=SIGMAS8, env={"SOM_EXACT_RESORT": "1000"}, between=(2, moved))
    # (the query over other rows ran under a plan: its pass selected in its screen too)
    assert _deltas(got, "select")[3][0] >= 1, _deltas(got, "select")[3]
    _compare(16, 16, 16, rows=rows, w0=w0, sigmas=SIGMAS8, env={"SOM_EXACT_RESORT": "1000"}, between=(3, new_rows))


# 8: the two hooks compose: with SOM_EXACT_CHAIN=0 the lists come from exact_lists_kernel, which clears the tickets as well
@pytest.mark.parametrize("x,y,d", [(16, 16, 16), (64, 64, 32)])
def test_fused_with_the_unchained_launches(x, y, d):
    rows = gaussian_blobs(N_ROWS, d, seed=39)
    got = _compare(x, y, d, rows=rows, w0=_codebook(x, y, d, 10), sigmas=SIGMAS6, env={"SOM_EXACT_CHAIN": "0", "SOM_EXACT_RESORT": "3"})
    _planned_throughout(got)
    if x == 64:
        assert got[-1]["select"][2] > 0, "no tile was cut: the tickets of the unchained lists were not exercised"
