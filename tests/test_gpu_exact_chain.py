"""Exact mode, euclidean, under a plan: the chain of small launches between the big kernels of a planned epoch, shortened
(default) against the launch sequence it replaces (SOM_EXACT_CHAIN=0):

  1. the sorted rows' last-BMU positions left behind by exact_finalize_kernel instead of gathered by exact_lastpos_kernel;
  2. the tiles' lists and their totals / work items in one launch (exact_lists_totals_kernel: the last workgroup sums);
  3. the need2 words cleared by the level-1 plan workgroups, rowmin2 initialised by exact_select_kernel, instead of two fills;
  4. exact_tiles_kernel on sixteen workgroups instead of one;
  5. the codebook's 16-bit image and the centroid images in one grid (exact_prep_images_kernel).

None of them changes what is computed.  Every case runs the same seeded epochs on two fresh engines, one per setting, both
under SOM_EXACT_SKIP=2 (small maps are planned, and the measured-cost decisions are out of the policy: both engines plan
alike), and asserts epoch by epoch and bit for bit: the BMU ids, the codebook after the merge, exact_skip_stats(),
exact_stats() and exact_resident_stats().  Shapes: the smallest that reach each branch."""
import contextlib
import os

import numpy as np
import pytest

from xpysom_dask_amd.synthetic import gaussian_blobs

pytestmark = pytest.mark.gpu

N_ROWS = 4096
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


def _engine(chain, x, y, d, env, precision="exact", **kw):
    from xpysom_dask_amd.engine import HipEngine
    # (the library reads the switches in som_create; SOM_EXACT_CHAIN and the hooks in `env` only under SOM_TEST_HOOKS=1,
    #  which conftest sets)
    with _env(SOM_EXACT_CHAIN="1" if chain else "0", SOM_EXACT_SKIP="2", **(env or {})):
        return HipEngine(x, y, d, precision=precision, **kw)


def _codebook(x, y, d, seed):
    return np.random.default_rng(seed).normal(0.0, 2.0, size=(x * y, d)).astype(np.float32)


def _state(eng, ids):
    return (ids, eng.get_weights(), eng.exact_skip_stats(), eng.exact_stats(), eng.exact_resident_stats(), eng.exact_chain_stats())


def _carried(rec):
    """Per epoch of a record: did its launch take the rows' last-BMU positions from the epoch before?"""
    c = [r[5] for r in rec]
    return [b - a for a, b in zip([0] + c[:-1], c)]


def _run(chain, x, y, d, *, rows, w0, sigmas, env=None, between=None, precision="exact", **kw):
    """The record of one engine, a step per epoch: (BMU ids, codebook after the merge, the three counters).
    between = (epoch, fn): fn(engine, record) runs after that epoch's merge."""
    eng = _engine(chain, x, y, d, env, precision=precision, **kw)
    rec = []
    try:
        eng.set_weights(w0)
        eng.set_data(rows)
        for e, sigma in enumerate(sigmas):
            eng.epoch_accumulate(sigma, 0.5, 1)
            ids = eng.epoch_fetch()[2]
            eng.epoch_merge()
            rec.append(_state(eng, ids) if precision == "exact" else (ids, eng.get_weights()))
            if between is not None and between[0] == e:
                between[1](eng, rec)
        extra = eng.exact_refine_stats() if precision == "exact" else None
    finally:
        eng.close()
    return rec, extra


def _same_bits(a, b):
    return a.shape == b.shape and a.view(np.uint32).tobytes() == b.view(np.uint32).tobytes()


def _compare(x, y, d, **kw):
    (ref, ref_x), (got, got_x) = _run(False, x, y, d, **kw), _run(True, x, y, d, **kw)
    assert len(ref) == len(got)
    for e, (r, g) in enumerate(zip(ref, got)):
        assert np.array_equal(r[0], g[0]), "step %d: BMU ids differ in %d rows" % (e, int((r[0] != g[0]).sum()))
        assert _same_bits(r[1], g[1]), "step %d: the codebooks differ" % e
        assert r[2] == g[2], "step %d: exact_skip_stats %r != %r" % (e, g[2], r[2])
        assert r[3] == g[3], "step %d: exact_stats %r != %r" % (e, g[3], r[3])
        assert r[4] == g[4], "step %d: exact_resident_stats %r != %r" % (e, g[4], r[4])
    assert ref_x == got_x, "exact_refine_stats %r != %r" % (got_x, ref_x)
    assert ref[-1][5] == 0, "SOM_EXACT_CHAIN=0 carried positions"
    return got, got_x


def _planned_throughout(rec):
    run, total = rec[-1][2]
    planned, sorted_ = rec[-1][4]
    assert 0 < run <= total and planned == len(rec), (rec[-1][2], rec[-1][4])
    return planned, sorted_


# 1: 4 groups and 16 tiles -- the plan's grid has four parts a tile (pgrid.y > 1: every part clears its own slice of need2);
#    24 x 20: sides no multiples of 8 (partial groups, a strip-ordered patch).  An order kept for three epochs
#    (SOM_EXACT_RESORT=3: the carried positions are used, then replaced by a re-sort) and the default schedule, which on maps
#    this small sorts and scouts in most epochs (the scout's picks in lastpos_s, the real last BMUs beside them).
@pytest.mark.parametrize("x,y,d,env", [(16, 16, 16, {"SOM_EXACT_RESORT": "3"}), (16, 16, 16, {}),
                                       (24, 20, 12, {"SOM_EXACT_RESORT": "3"}), (24, 20, 12, {})])
def test_chain_small_maps(x, y, d, env):
    rows = gaussian_blobs(N_ROWS, d, seed=21)
    w0 = _codebook(x, y, d, 3)
    got, _ = _compare(x, y, d, rows=rows, w0=w0, sigmas=SIGMAS8, env=env)
    _planned_throughout(got)
    if (x, env) == (16, {"SOM_EXACT_RESORT": "3"}):
        # ... and the float32 mode trains the same map
        f32, _ = _run(True, x, y, d, rows=rows, w0=w0, sigmas=SIGMAS8, precision="f32")
        assert _same_bits(f32[-1][1], got[-1][1]), "precision='exact' left the float32 trajectory"
        assert all(np.array_equal(a[0], b[0]) for a, b in zip(f32, got))


# 2: the carried positions across a re-sort: an order kept for three epochs, rebuilt once in the middle, kept again
def test_chain_carried_positions_across_a_resort():
    rows = gaussian_blobs(N_ROWS, 16, seed=22)
    got, _ = _compare(32, 32, 16, rows=rows, w0=_codebook(32, 32, 16, 4), sigmas=SIGMAS8, env={"SOM_EXACT_RESORT": "4"})
    planned, sorted_ = _planned_throughout(got)
    # (epoch 0 sorts, epochs 1-3 keep, epoch 4 sorts, epochs 5-7 keep)
    assert sorted_ >= 2 and planned - sorted_ >= 4, (planned, sorted_)
    # (the positions are carried exactly into the epochs that keep the order: every epoch stores them, a re-sort ignores them)
    sorts = [b[4][1] - a[4][1] for a, b in zip([(0, 0, 0, 0, (0, 0))] + got[:-1], got)]
    assert _carried(got) == [1 - s for s in sorts] and sum(_carried(got)) >= 4, (_carried(got), sorts)


# 3: the refinement pass on and off (SOM_EXACT_REFINE): with it the launch has a second exact_tiles_kernel and rowmin2 starts
#    from the select kernel's all-ones; without it the select kernel gets no such pointer
def test_chain_refinement_on_and_off():
    rows = gaussian_blobs(N_ROWS, 32, seed=23)
    w0 = _codebook(32, 32, 32, 5)
    on, on_x = _compare(32, 32, 32, rows=rows, w0=w0, sigmas=SIGMAS6, env={"SOM_EXACT_RESORT": "3", "SOM_EXACT_REFINE": "1"})
    off, off_x = _compare(32, 32, 32, rows=rows, w0=w0, sigmas=SIGMAS6, env={"SOM_EXACT_RESORT": "3", "SOM_EXACT_REFINE": "0"})
    assert on_x[0] > 0 and 0 < on_x[1] <= on_x[0] and off_x == (0, 0), (on_x, off_x)
    for a, b in zip(on, off):
        assert np.array_equal(a[0], b[0]) and _same_bits(a[1], b[1])


# 4: several passes per epoch (passes of 1 024 rows; 3 000 rows: three passes, the last one partial): the positions are
#    complete only behind the last pass
@pytest.mark.parametrize("n", [N_ROWS, 3000])
def test_chain_several_passes(n):
    rows = gaussian_blobs(n, 16, seed=24)
    got, _ = _compare(16, 16, 16, rows=rows, w0=_codebook(16, 16, 16, 6), sigmas=SIGMAS6,
                      env={"SOM_EXACT_RESORT": "3", "SOM_EXACT_PASS_ROWS": "1024"})
    _planned_throughout(got)
    assert got[-1][3][2] == len(SIGMAS6) * -(-n // 1024)      # (screen passes)
    # (SOM_EXACT_RESORT=3: epochs 0 and 3 sort; the others find every pass's slice stored by the epoch before)
    assert _carried(got) == [0, 1, 1, 0, 1, 1], _carried(got)


# 5: fallback rows -- a row of NaN, a row of infinities: the positions of an epoch with fallback rows are not carried, the
#    next epoch gathers them again (bubble: the two rows poison the units in their reach only)
def test_chain_fallback_rows():
    rows = gaussian_blobs(N_ROWS, 16, seed=25)
    rows[7] = np.nan
    rows[9] = np.inf
    got, _ = _compare(16, 16, 16, rows=rows, w0=_codebook(16, 16, 16, 7), sigmas=(2.0, 1.5, 1.5, 1.2, 1.0, 1.0),
                      env={"SOM_EXACT_RESORT": "1000"}, neighborhood="bubble")
    fb = [g[3][1] for g in got]
    assert fb[0] > 0 and all(b > a for a, b in zip(fb, fb[1:])), fb        # (rows fell back in every epoch)
    assert _carried(got) == [0] * len(got), _carried(got)                  # (... so no epoch's positions were good for the next)


# 6: between two epochs set_weights, a query over other rows, quantization_error; later a second set_data with other rows
def test_chain_between_epochs():
    rows = gaussian_blobs(N_ROWS, 16, seed=26)
    other = gaussian_blobs(2500, 16, seed=27)
    w0 = _codebook(16, 16, 16, 8)

    def moved(eng, rec):
        eng.set_weights(w0[::-1].copy())
        rec.append(_state(eng, eng.bmu(other[:300])))
        qe = eng.quantization_error(rows[:500])
        rec.append(_state(eng, np.array([qe], dtype=np.float64).view(np.int64)))

    def new_rows(eng, rec):
        eng.set_data(other)

    got, _ = _compare(16, 16, 16, rows=rows, w0=w0, sigmas=SIGMAS8, env={"SOM_EXACT_RESORT": "1000"}, between=(2, moved))
    # (a new codebook and queries over other rows leave the resident ids and their order alone; two more steps in the record)
    assert _carried(got) == [0, 1, 1, 0, 0, 1, 1, 1, 1, 1], _carried(got)
    got, _ = _compare(16, 16, 16, rows=rows, w0=w0, sigmas=SIGMAS8, env={"SOM_EXACT_RESORT": "1000"}, between=(3, new_rows))
    assert _carried(got) == [0, 1, 1, 1, 0, 1, 1, 1], _carried(got)      # (new rows: nothing to carry into their first epoch)


# 7: four 32-feature steps (the headline's instance of the plan, of the image kernels)
def test_chain_128_features():
    rows = gaussian_blobs(N_ROWS, 128, seed=28)
    got, _ = _compare(32, 32, 128, rows=rows, w0=_codebook(32, 32, 128, 9), sigmas=SIGMAS6, env={"SOM_EXACT_RESORT": "3"})
    _planned_throughout(got)


# 8: beyond 128 features the wide plan launches the same lists kernel (the smallest shape of tests/test_gpu_skip_wide.py)
def test_chain_wide_plan():
    rows = gaussian_blobs(5000, 129, seed=29)
    got, _ = _compare(64, 72, 129, rows=rows, w0=_codebook(64, 72, 129, 10), sigmas=SIGMAS6, env={"SOM_EXACT_RESORT": "3"})
    _planned_throughout(got)
    assert got[-1][5] == 0                                   # (the wide plan keeps its own gather of the last BMUs)
