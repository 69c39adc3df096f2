"""Exact mode, euclidean, up to 128 features, under a plan: levels 1 and 2 of the plan and the tiles' lists in one launch
(exact_plan_fused_kernel of csrc/exact_skip.hpp, the default) against the three launches it replaces (SOM_EXACT_FUSE_PLAN=0:
exact_plan_kernel at both levels, exact_lists_totals_kernel).

The fused kernel calls the device functions the split kernels call: the same tests on the same operands, so the same need
bits, the same lists, the same work items.  Every case runs the same seeded epochs on two fresh engines, one per setting,
both under SOM_EXACT_SKIP=2 (small maps are planned, and the measured-cost decisions are out of the policy: both engines plan
alike), and asserts epoch by epoch and bit for bit: the BMU ids, the codebook after the merge, exact_skip_stats() (blocks run
of blocks in all: the lists), exact_stats(), exact_resident_stats(), exact_refine_stats(), exact_select_stats() and
exact_last_counts().  exact_plan_stats() says which path ran, exact_last_plan() what the policy asked of the launch: the fused
engine plans in one launch exactly where the launch has level 2, no scout and no timed phases (the launches the policy times
keep the split pair, whose level 2 its events bracket), the split engine never.

The fused launch serves passes planned by one workgroup per tile -- 1 024 tiles and more, or a single centroid stage.  The
cases here have 16 tiles or fewer; where the map has more than one stage of groups, SOM_EXACT_PLAN_PARTS=1 (a test hook, set
for BOTH engines) gives their plans the one-workgroup-per-tile grid of a large pass.  Shapes: the smallest that reach each
branch."""
import contextlib
import os

import numpy as np
import pytest

from xpysom_dask_amd.synthetic import gaussian_blobs

pytestmark = pytest.mark.gpu

N_ROWS = 4096
SIGMAS8 = (6.0, 4.0, 3.0, 2.0, 1.5, 1.2, 1.0, 0.8)
SIGMAS6 = (6.0, 4.0, 3.0, 2.0, 1.5, 1.0)
# (the order of the first sort is kept: no later epoch sorts or scouts, so the epochs between two timed launches are there)
KEEP_ORDER = {"SOM_EXACT_RESORT": "1000"}


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
    # (the library reads the switches in som_create; SOM_EXACT_FUSE_PLAN and the hooks in `env` only under SOM_TEST_HOOKS=1,
    #  which conftest sets)
    with _env(SOM_EXACT_FUSE_PLAN="1" if fused else "0", SOM_EXACT_SKIP="2", **(env or {})):
        return HipEngine(x, y, d, precision=precision, **kw)


def _codebook(x, y, d, seed):
    return np.random.default_rng(seed).normal(0.0, 2.0, size=(x * y, d)).astype(np.float32)


def _last_pass_rows(n, env):
    p = int((env or {}).get("SOM_EXACT_PASS_ROWS", "0"))
    return n if p <= 0 else n - (n - 1) // p * p


def _run(fused, x, y, d, *, rows, w0, sigmas, env=None, precision="exact", **kw):
    """The record of one engine, a step per epoch."""
    eng = _engine(fused, x, y, d, env, precision=precision, **kw)
    rec = []
    n_last = _last_pass_rows(len(rows), env)
    try:
        eng.set_weights(w0)
        eng.set_data(rows)
        for sigma in sigmas:
            eng.epoch_accumulate(sigma, 0.5, 1)
            ids = eng.epoch_fetch()[2]
            eng.epoch_merge()
            if precision != "exact":
                rec.append({"ids": ids, "w": eng.get_weights()})
                continue
            rec.append({"ids": ids, "w": eng.get_weights(), "skip": eng.exact_skip_stats(), "stats": eng.exact_stats(),
                        "resident": eng.exact_resident_stats(), "refine": eng.exact_refine_stats(), "select": eng.exact_select_stats(),
                        "counts": eng.exact_last_counts(n_last), "plan": eng.exact_plan_stats(), "asked": eng.exact_last_plan()})
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


def _compare(x, y, d, *, fusable=True, **kw):
    """Both engines' records, compared; returns the fused engine's.  fusable False: no launch of the case may take the fused plan."""
    ref, got = _run(False, x, y, d, **kw), _run(True, x, y, d, **kw)
    assert len(ref) == len(got)
    for e, (r, g) in enumerate(zip(ref, got)):
        assert np.array_equal(r["ids"], g["ids"]), "step %d: BMU ids differ in %d rows" % (e, int((r["ids"] != g["ids"]).sum()))
        assert _same_bits(r["w"], g["w"]), "step %d: the codebooks differ" % e
        for key in ("skip", "stats", "resident", "refine", "select"):
            assert r[key] == g[key], "step %d: exact_%s_stats %r != %r" % (e, key, g[key], r[key])
        assert np.array_equal(r["counts"], g["counts"]), \
            "step %d: the candidate counts differ in %d rows" % (e, int((r["counts"] != g["counts"]).sum()))
        assert r["asked"] == g["asked"], "step %d: the policy decided differently: %r != %r" % (e, g["asked"], r["asked"])
    # which path ran.  The reference engine: never the fused launch.  The fused engine: as many plans as the reference engine, each
    # pass's in one launch where the launch has level 2, no scout and no timed phases, as three launches everywhere else
    d_ref, d_got = _deltas(ref, "plan"), _deltas(got, "plan")
    fused_epochs = 0
    for e, (r, g) in enumerate(zip(d_ref, d_got)):
        asked = got[e]["asked"]
        print("step %d: plan stats (fused, split): fused engine %s, reference %s; asked %s"
              % (e, tuple(g), tuple(r), ",".join(k for k, v in asked.items() if v)))
        assert r[0] == 0, "step %d: the reference engine planned in one launch: %r" % (e, tuple(r))
        assert g[0] + g[1] == r[1], "step %d: %r plans against the reference engine's %r" % (e, tuple(g), tuple(r))
        if asked["skip"]:
            assert r[1] > 0, "step %d: a planned launch without a plan" % e
        if fusable and asked["skip"] and asked["level2"] and not asked["scout"] and not asked["time_phases"]:
            assert tuple(g) == (r[1], 0), "step %d: an untimed launch with level 2 planned in %r launches" % (e, tuple(g))
            fused_epochs += 1
        else:
            # (a launch the policy timed, or one with a scout or without level 2, is counted as split)
            assert g[0] == 0, "step %d: the fused launch ran where it must not (asked %r): %r" % (e, asked, tuple(g))
    if fusable:
        assert fused_epochs > 0 and got[-1]["plan"][0] > 0, "no launch of the run took the fused plan: %r" % (got[-1]["plan"],)
        # (... and the timed launches in between stayed split: the first planned launches and every fourth one after that)
        assert any(a["asked"]["skip"] and a["asked"]["time_phases"] for a in got), "no planned launch of the run was timed"
    else:
        assert got[-1]["plan"][0] == 0
    return got


def _planned_throughout(rec, first=0, skips=True):
    """Every epoch from `first` on ran under a plan (skips: ... that skipped blocks somewhere in the run)."""
    run, total = rec[-1]["skip"]
    planned, sorted_ = rec[-1]["resident"]
    assert 0 < run <= total and (run < total or not skips) and planned >= len(rec) - first, (rec[-1]["skip"], rec[-1]["resident"])


# 1: 64 groups = ONE centroid stage; level 2's list holds at most 64 groups = four chunks of sixteen -- and the float32 mode trains
#    the same map (the mode's invariant): ids identical on every row in every epoch
def test_one_stage_and_f32_beside():
    rows = gaussian_blobs(N_ROWS, 32, seed=41)
    w0 = _codebook(64, 64, 32, 3)
    got = _compare(64, 64, 32, rows=rows, w0=w0, sigmas=SIGMAS8, env=KEEP_ORDER)
    _planned_throughout(got)
    f32 = _run(True, 64, 64, 32, rows=rows, w0=w0, sigmas=SIGMAS8, precision="f32")
    for e, (a, b) in enumerate(zip(f32, got)):
        assert np.array_equal(a["ids"], b["ids"]), "step %d: %d ids differ from float32's" % (e, int((a["ids"] != b["ids"]).sum()))
    assert _same_bits(f32[-1]["w"], got[-1]["w"]), "precision='exact' left the float32 trajectory"


# 2: 72 groups: two stages, the second one partial (8 groups of 64); four 32-feature steps: the headline's instance
def test_two_stages_128_features():
    rows = gaussian_blobs(N_ROWS, 128, seed=42)
    got = _compare(72, 64, 128, rows=rows, w0=_codebook(72, 64, 128, 4), sigmas=SIGMAS6, env=dict(KEEP_ORDER, SOM_EXACT_PLAN_PARTS="1"))
    _planned_throughout(got)


# 3: sides that are no multiples of 8 (2 x 8 sub-blocks) and a partial last group: 561 units = 8 groups and 49 units
def test_odd_sides_partial_group():
    rows = gaussian_blobs(N_ROWS, 128, seed=43)
    got = _compare(33, 17, 128, rows=rows, w0=_codebook(33, 17, 128, 5), sigmas=SIGMAS6, env=KEEP_ORDER)
    _planned_throughout(got)


# 4: three features: one 32-feature step (KS32 = 1)
def test_three_features():
    rows = gaussian_blobs(N_ROWS, 3, seed=44)
    got = _compare(64, 64, 3, rows=rows, w0=_codebook(64, 64, 3, 6), sigmas=SIGMAS8, env=KEEP_ORDER)
    _planned_throughout(got)


# 5: three passes an epoch (passes of 1 024 rows over 2 537 rows): the last pass's last tile is partial -- rows behind the pass
#    need nothing -- and every pass plans on its own
def test_several_passes_partial_tile():
    rows = gaussian_blobs(2537, 32, seed=45)
    got = _compare(64, 64, 32, rows=rows, w0=_codebook(64, 64, 32, 7), sigmas=SIGMAS8, env=dict(KEEP_ORDER, SOM_EXACT_PASS_ROWS="1024"))
    _planned_throughout(got)
    assert got[-1]["stats"][2] == len(SIGMAS8) * 3            # (screen passes)
    assert got[-1]["plan"][0] % 3 == 0 and got[-1]["plan"][0] >= 3, got[-1]["plan"]   # (a fused launch per pass of a fused epoch)


# 6: level 2 off (SOM_EXACT_SUBBLOCKS=0): the plan stops at the groups, the fused launch is never chosen, the ids stay equal
def test_without_sub_blocks_the_split_plan_stays():
    rows = gaussian_blobs(N_ROWS, 32, seed=46)
    got = _compare(64, 64, 32, rows=rows, w0=_codebook(64, 64, 32, 8), sigmas=SIGMAS6, env=dict(KEEP_ORDER, SOM_EXACT_SUBBLOCKS="0"),
                   fusable=False)
    _planned_throughout(got, skips=False)       # (64 groups of a random codebook: the groups alone drop nothing in six epochs)
    assert not any(g["asked"]["level2"] for g in got)


# 7: a row holding a NaN, a row holding an infinite feature: thresholds that are not finite -- the row needs everything, its tile
#    lists every block -- and rows for the float32 fallback kernel in every epoch (bubble: the two rows poison the units in
#    their reach only)
def test_nan_and_infinite_rows():
    rows = gaussian_blobs(N_ROWS, 32, seed=47)
    rows[7, 3] = np.nan
    rows[9, 5] = np.inf
    got = _compare(64, 64, 32, rows=rows, w0=_codebook(64, 64, 32, 9), sigmas=(2.0, 1.5, 1.5, 1.2, 1.0, 1.0, 1.0, 0.8),
                   env=KEEP_ORDER, neighborhood="bubble")
    fb = [g["stats"][1] for g in got]
    assert fb[0] > 0 and all(b > a for a, b in zip(fb, fb[1:])), fb        # (rows fell back in every epoch)
