"""precision='exact' under the DEFAULT switches (SOM_EXACT_SKIP unset): the forecast every large launch without a trusted recent
plan goes through before it commits to one -- the 128-row sample (exact_scout_rowneed_kernel), the sample tiles through srt[1]
(exact_sample_tiles), and the decline that cancels the plan in the middle of pass 0 -- on the smallest shapes that reach each of
them, against the float64 model and the built data of tests/scout_ref.py.  GPU only (`-m gpu`).

WHAT MAY BE ASSERTED.  Nothing here depends on a measured time.  A decision is asserted only where one of two arguments fixes it:
  FRESH    a fresh handle has no costs on record, so its first launch decides from what the device counted alone: the row sample
           declines iff need > 0.9 (PlanState::rows_sampled), the sample tiles decline iff est > 0.8 (commit_scouted_plan, unpriced).
  PRICED   after one launch without a plan commit_scouted_plan is share * blocks * blk + over < 0.97 full_total with
           blk = 1.05 full_screen / blocks and over = full_total - 0.8 full_screen, i.e. share < (0.8 - 0.03 full_total / full_screen)
           / 1.05: it declines for every share >= 0.77 whatever the times, and commits a share s while full_total / full_screen
           < (0.8 - 1.05 s) / 0.03 (s = 0.2: 19.7 -- a launch spends most of its time in its screen: the ratio is printed).
  MEMORY   within eight launches of a decline by the tiles the row sample declines wherever need >= 0.9 x the need it saw then.
Every test compares the ids with a precision='f32' engine on every row and holds the float32 fallback to <= 1 % of the rows."""
import ctypes as C

import numpy as np
import pytest

from tests import scout_ref as R
from tests import skip_ref as S

pytestmark = pytest.mark.gpu
F32 = np.float32
MAIN = (192, 192, 128)
SIG, ETA = 1.0, 0.01


def engine(shape, precision):
    from xpysom_dask_amd.engine import HipEngine
    return HipEngine(shape[0], shape[1], shape[2], precision=precision)


class Pair:
    """A fresh exact handle beside a float32 one, the same codebook (and resident rows) in both."""

    def __init__(self, shape, w, resident=None):
        self.shape, self.G = shape, S.n_groups(shape[0] * shape[1])
        self.f, self.x = engine(shape, "f32"), engine(shape, "exact")
        self.load(w, resident)

    def load(self, w, resident=None):
        for e in (self.f, self.x):
            e.set_weights(w)
            if resident is not None:
                e.set_data(resident)

    def snap(self):
        x = self.x
        scouted, transient = x.exact_scout_stats()
        run, total = x.exact_skip_stats()
        rows, fb, passes = x.exact_stats()
        return dict(scouted=scouted, transient=transient, run=run, total=total, rows=rows, fb=fb, passes=passes,
                    declined=x.exact_forecast()["scout_declined"])

    def launch(self, mode, rows=None):
        """One BMU launch in both engines: 'query' (bmu), 'accumulate' (a resident epoch's search, the codebook left alone) or
        'epoch' (search, update, merge).  Returns (what the launch added to the counters, its plan, its forecast, the ids)."""
        before = self.snap()
        if mode == "query":
            a, b = self.f.bmu(rows), self.x.bmu(rows)
        else:
            for e in (self.f, self.x):
                e.epoch_accumulate(SIG, ETA, True)
            a, b = self.f.epoch_fetch()[2], self.x.epoch_fetch()[2]
        plan, fc = self.x.exact_last_plan(), self.x.exact_forecast()
        if mode == "epoch":
            self.f.epoch_merge()
            self.x.epoch_merge()
        after = self.snap()
        d = {k: after[k] - before[k] for k in after}
        self.last_f32 = a
        assert np.array_equal(a, b), "ids differ from float32's on %d rows (first: %s)" % (int((a != b).sum()), np.flatnonzero(a != b)[:8])
        assert d["fb"] <= d["rows"] // 100, "float32 fallback on %d of %d rows" % (d["fb"], d["rows"])
        return d, plan, fc, b

    def row_sample_against_float64(self, rows, fc, label=""):
        """The device's count of needed (row, group) pairs within the float64 model's interval, the model fed the device's own
        level-1 centroids and radii (current: no merge since the launch)."""
        cen, rad, _ = self.x.debug_exact_centroids(0)
        sure, maybe = R.rowneed_ref(rows, cen, rad, self.G)
        pairs = 128 * self.G
        count = fc["need"] * pairs
        print("%s need %.6f (%d pairs of %d) model [%d, %d] maybe %d" % (label, fc["need"], round(count), pairs, sure, sure + maybe, maybe))
        assert fc["rows"] == 128
        assert abs(count - round(count)) < 1e-6 and sure <= round(count) <= sure + maybe
        assert maybe <= 0.01 * pairs

    def close(self):
        self.f.close()
        self.x.close()


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    monkeypatch.delenv("SOM_EXACT_SKIP", raising=False)
    monkeypatch.delenv("SOM_EXACT_PASS_ROWS", raising=False)


def share(d):
    return d["run"] / d["total"]


def assert_commit(d, plan, fc, tiles_asked=True, wide=False):
    # FRESH: need <= 0.9 and est <= 0.8 commit the plan
    assert plan["skip"] and plan["scout"] and plan["estimate"] and plan["sample_tiles"] == (not wide), plan
    assert d["scouted"] == 1 and d["declined"] == 0, d
    assert 0.0 <= fc["need"] <= 0.9 and fc["rows"] == 128, fc
    if tiles_asked:
        assert 0.0 < fc["est"] <= 0.8 and fc["est"] <= fc["est1"] and fc["n_st"] == 128, fc
    else:
        assert fc["est"] == -1.0 and fc["n_st"] == -1, fc
    assert share(d) < 0.6, share(d)


def assert_rows_decline(d, plan, fc):
    # FRESH: need > 0.9 declines before the scout, the sort and the tiles
    assert not plan["skip"] and not plan["scout"] and not plan["estimate"], plan
    assert fc["need"] > 0.9 and fc["rows"] == 128 and fc["est"] == -1.0 and fc["n_st"] == -1, fc
    assert d["run"] == d["total"] and d["scouted"] == 0 and d["declined"] == 1, d


def assert_tiles_decline(d, plan, fc):
    # FRESH: est > 0.8 declines in the middle of pass 0
    assert not plan["skip"] and not plan["scout"] and not plan["estimate"], plan
    assert 0.0 <= fc["need"] <= 0.9 and fc["est"] > 0.8 and fc["n_st"] == 128 and fc["blocks_run"] > 0, fc
    assert d["run"] == d["total"] and d["scouted"] == 0 and d["declined"] == 1, d


ASSERT = {"commit": assert_commit, "rows_decline": assert_rows_decline, "tiles_decline": assert_tiles_decline}


# ------------------------------------------------------------------------------------------ the row sample against float64
ROW_SAMPLE_CASES = [(s, d, False) for s in sorted(R.SHAPES) if s[2] <= 128 for d in ("commit", "tiles_decline")]
ROW_SAMPLE_CASES += [(MAIN, "commit", True), (MAIN, "tiles_decline", True)]       # a NaN row at a sampled index


@pytest.mark.parametrize("shape,data,nan_row", ROW_SAMPLE_CASES,
                         ids=["%dx%dx%d-%s%s" % (s + (d, "-nan" if n else "")) for s, d, n in ROW_SAMPLE_CASES])
def test_the_row_sample_counts_what_the_float64_model_counts(shape, data, nan_row):
    b = R.build(*shape, nan_row=nan_row)
    w, rows = b[data]
    p = Pair(shape, w)
    d, plan, fc, _ = p.launch("query", rows)
    p.row_sample_against_float64(rows, fc, "%s %s%s:" % (shape, data, " (NaN row)" if nan_row else ""))
    p.close()


# ------------------------------------------------------------------------------------------ the three branches
@pytest.mark.parametrize("mode", ["query", "first_epoch", "last_bmus"])
@pytest.mark.parametrize("branch", ["commit", "rows_decline", "tiles_decline"])
def test_three_branches_on_a_fresh_handle(branch, mode):
    """192 x 192 x 128, 65 792 rows = 257 tiles, st = 2: as a query, as a resident first epoch, and as two resident epochs (search,
    update, merge) of which the second has last BMUs."""
    b = R.build(*MAIN)
    w, rows = b[branch]
    p = Pair(MAIN, w, None if mode == "query" else rows)
    d, plan, fc, ids = p.launch("query" if mode == "query" else "accumulate" if mode == "first_epoch" else "epoch", rows)
    print(branch, mode, "need %.4f est %.4f est1 %.4f share %.4f" % (fc["need"], fc["est"], fc["est1"], share(d)))
    ASSERT[branch](d, plan, fc)
    assert d["transient"] == (1 if mode == "query" and branch == "commit" else 0)
    if branch == "tiles_decline":
        # the sample wrote best64[0 .. 128 * 256): those rows' ids on their own (launch() has compared every row)
        assert np.array_equal(ids[:32768], p.last_f32[:32768])
    if mode != "last_bmus":
        p.row_sample_against_float64(rows, fc, "%s %s:" % (branch, mode))
    else:
        s1 = share(d)
        d2, plan2, fc2, _ = p.launch("epoch")
        print(branch, "second epoch: plan", plan2, "need %.4f est %.4f share %.4f" % (fc2["need"], fc2["est"], share(d2)))
        if branch == "commit":
            # begin(): the order is valid and the rows have last BMUs, so the launch is fresh for the default policy -- sorts,
            # scouts and asks the samples again -- only while the last share was >= 0.25 (no scout wins are on record yet)
            assert (fc2["need"] >= 0.0) == (s1 >= 0.25), (fc2, s1)
            if s1 < 0.25:
                # (resort is not begin()'s alone: the first launch that refines rebuilds the order -- LaunchPlan::force_sort)
                assert plan2["skip"] and not plan2["scout"] and not plan2["estimate"], plan2
                assert d2["declined"] == 0 and d2["scouted"] == 0 and d2["run"] < d2["total"]
            elif not fc2["need"] > 0.9 and 0.0 <= fc2["est"] <= 0.8:
                # (asked again: no launch without a plan is on record, so FRESH applies once more)
                assert plan2["skip"] and plan2["resort"] and plan2["scout"] and plan2["estimate"], plan2
                assert d2["declined"] == 0 and d2["scouted"] == 1 and d2["run"] < d2["total"]
        else:
            # the first epoch declined: no valid order, so this one is fresh and asks again, now PRICED and with MEMORY -- the
            # codebook has moved, so the branch follows from what the device counted this time
            assert fc2["need"] >= 0.0 and fc2["rows"] == 128, fc2
            mem = branch == "tiles_decline" and fc2["need"] >= 0.9 * fc["need"]
            if fc2["need"] > 0.9 or mem:
                assert fc2["est"] == -1.0 and d2["declined"] == 1 and d2["run"] == d2["total"] and not plan2["skip"]
            elif fc2["est"] >= 0.77:
                assert d2["declined"] == 1 and d2["run"] == d2["total"] and not plan2["skip"]
    p.close()


@pytest.mark.parametrize("shape,n,branch,mode", [
    (MAIN, 65791, "commit", "query"),                         # 256 tiles: the row sample only, the plan commits unasked
    ((192, 192, 126), None, "commit", "query"),               # the scalar branch of the row sample, a partial last tile, dp != D
    ((192, 192, 126), None, "tiles_decline", "first_epoch"),
    ((256, 256, 64), None, "commit", "first_epoch"),          # 1 024 groups: four turns of the need loop
    ((256, 256, 64), None, "tiles_decline", "query"),
    ((256, 256, 64), None, "rows_decline", "query"),
    ((128, 128, 136), None, "commit", "query"),               # beyond 128 features: exact_wide_scout_* behind the row sample
    ((128, 128, 136), None, "commit", "first_epoch"),
    ((128, 128, 136), None, "rows_decline", "query"),
    ((128, 128, 136), None, "rows_decline", "first_epoch"),
], ids=lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v))
def test_the_branches_at_the_other_shapes(shape, n, branch, mode):
    b = R.build(*shape)
    w, rows = b[branch]
    rows = rows if n is None else rows[:n]
    wide = shape[2] > 128
    p = Pair(shape, w, None if mode == "query" else rows)
    d, plan, fc, _ = p.launch("query" if mode == "query" else "accumulate", rows)
    print(shape, len(rows), branch, mode, "need %.4f est %.4f est1 %.4f share %.4f" % (fc["need"], fc["est"], fc["est1"], share(d)))
    if branch == "commit":
        assert_commit(d, plan, fc, tiles_asked=not wide and len(rows) // 256 > 256, wide=wide)
    else:
        ASSERT[branch](d, plan, fc)
    if not wide:
        p.row_sample_against_float64(rows, fc, "%s %s %s:" % (shape, branch, mode))
    p.close()


# ------------------------------------------------------------------------------------------ the forecast and the plan
def test_the_sample_tiles_forecast_what_the_pass_then_plans():
    """Commit, one pass, resident: the sample is planned exactly as the pass is -- the same rows in the same tiles against the same
    centroids by the same kernels -- so the sampled tiles' lists in the pass are as long as they were in the sample."""
    b = R.build(*MAIN)
    w, rows = b["commit"]
    p = Pair(MAIN, w, rows)
    d, plan, fc, _ = p.launch("accumulate")
    assert_commit(d, plan, fc)
    blocks, groups, level2 = p.x.exact_tile_blocks()
    assert len(blocks) == 257 and d["passes"] == 1
    assert int(blocks.sum()) == d["run"]                      # what exact_list_totals_body summed into blocks_run
    assert (blocks <= 4 * groups).all() and (groups <= p.G).all()
    st = fc["st"]
    assert st == 2
    sampled = np.arange(128) * st
    print("sample: blocks %d groups %d level 2 %d; pass: blocks %d groups %d level 2 %d" % (
        fc["blocks_run"], fc["groups_run"], fc["level2"], blocks[sampled].sum(), groups[sampled].sum(), level2))
    assert int(groups[sampled].sum()) == fc["groups_run"]     # level 1 does not depend on whether level 2 runs
    if bool(fc["level2"]) == level2:
        assert int(blocks[sampled].sum()) == fc["blocks_run"]
    assert abs(fc["est"] - fc["blocks_run"] / (128 * p.G * 4)) < 1e-12 and abs(fc["est1"] - fc["groups_run"] / (128 * p.G)) < 1e-12
    p.close()


# ------------------------------------------------------------------------------------------ after a decline
def replay(script):
    from xpysom_dask_amd import _lib
    lib = _lib.load()
    flat = [float(v) for row in script for v in row]
    out = (C.c_double * (18 * len(script)))()
    assert lib.som_policy_replay(len(script), (C.c_double * len(flat))(*flat), out) == 0
    return np.array(list(out)).reshape(len(script), 18)


def test_after_a_decline_memory_cooldown_and_a_row_set_that_plans():
    """Resident, tiles_decline data, twelve searches on one handle with the codebook left alone (no merge: the device counts the
    same need every time), then queries, then a row set that plans.  The sequence of plans is what som_policy_replay makes of the
    device's own answers, and, spelled out (policy::PlanState):
      launch 0       FRESH: the tiles decline; one idle plan on the ladder; the need is remembered
      launches 1-8   MEMORY: the row sample declines (need >= 0.9 x the remembered one), no tiles asked, est = -1; the ladder stays
      launch 9       the memory is eight launches old: forgotten, the tiles are asked again and decline (PRICED: est >= 0.77); two
                     idle plans: a pause of two launches
      launches 10-11 the cooldown: no plan, nothing asked (need = -1)
    (The memory holds for eight launches and a decline from memory does not step the ladder, so the cooldown cannot come before
    the tenth launch.)"""
    b = R.build(*MAIN)
    w, rows = b["tiles_decline"]
    N = len(rows)
    p = Pair(MAIN, w, rows)
    script, seen = [], []
    for i in range(12):
        d, plan, fc, _ = p.launch("accumulate")
        seen.append((d, plan, fc))
        asked_tiles = fc["est"] >= 0.0
        script.append([1, i > 0, 1, N, 1, 1, 0, 0, 0, 1, 1, p.G * 4 / 256.0, 1, 1, 1, 0,
                       max(fc["need"], 0.0), fc["est"] if asked_tiles else -1.0, max(fc["est1"], 0.0),
                       1.0, 0.8, 0.1, 0.1, d["run"], d["total"], d["total"] // 4, 0, 0, 0])
    out = replay(script)
    declined = 0
    for i, (d, plan, fc) in enumerate(seen):
        o = out[i]
        got = [plan[k] for k in ("skip", "resort", "scout", "level2", "estimate", "sample_tiles")]
        assert got == [bool(v) for v in o[:6]], (i, plan, o)
        assert (fc["need"] >= 0.0) == bool(o[8]) and (fc["est"] >= 0.0) == bool(o[9]), (i, fc, o)
        assert d["declined"] == int(o[10] + o[11]), (i, d, o)
        declined += d["declined"]
        assert d["run"] == d["total"] and not plan["skip"], (i, d)
    need0 = seen[0][2]["need"]
    assert_tiles_decline(*seen[0])
    for i in range(1, 9):
        d, plan, fc = seen[i]
        assert fc["need"] >= 0.9 * need0 and fc["need"] <= 0.9 and fc["est"] == -1.0 and d["declined"] == 1, (i, fc)
    d, plan, fc = seen[9]
    assert fc["est"] >= 0.77 and d["declined"] == 1, fc     # PRICED
    for i in (10, 11):
        d, plan, fc = seen[i]
        assert not plan["skip"] and not plan["estimate"] and fc["need"] == -1.0 and fc["est"] == -1.0 and d["declined"] == 0, (i, plan, fc)
    assert declined == 10 and p.x.exact_forecast()["scout_declined"] == 10
    assert [int(v) for v in out[9][12:15]] == [2, 2, 4] and [int(v) for v in out[11][12:15]] == [0, 2, 4]
    # the other searches on the same rows after the declines
    a1, a2 = p.f.bmu_top2(rows)
    b1, b2 = p.x.bmu_top2(rows)
    assert np.array_equal(a1, b1) and np.array_equal(a2, b2)
    qf, qx = p.f.quantization_error(rows), p.x.quantization_error(rows)
    assert abs(qf - qx) <= 1e-6 * qf, (qf, qx)
    # a row set that plans, on the SAME handle: PRICED, and the tiles forecast a share far below (0.8 - 0.03 ratio) / 1.05
    wc, xc = b["commit"]
    p.load(wc, xc)
    d, plan, fc, _ = p.launch("accumulate")
    ratio = fc["full_total"] / fc["full_screen"] if fc["full_screen"] > 0 else float("nan")
    print("after the declines: need %.4f est %.4f share %.4f full_total / full_screen %.3f" % (fc["need"], fc["est"], share(d), ratio))
    assert 0.0 <= fc["need"] < 0.9 * need0 and 0.0 < fc["est"] < 0.5, fc
    assert plan["skip"] and plan["scout"] and share(d) < 0.6 and d["declined"] == 0 and d["scouted"] == 1, (plan, d)
    p.close()


# ------------------------------------------------------------------------------------------ several passes
@pytest.mark.parametrize("mode", ["query", "first_epoch"])
@pytest.mark.parametrize("branch", ["commit", "tiles_decline"])
def test_several_passes(monkeypatch, branch, mode):
    """128 x 128 x 128, 147 000 rows in two passes (288 tiles, then 287 with a partial one); the samples only ask pass 0.  A decline
    leaves pass 1 without a plan as well; a commit plans both."""
    monkeypatch.setenv("SOM_EXACT_PASS_ROWS", "73728")
    shape = (128, 128, 128)
    b = R.build(*shape)
    w, rows = b[branch]
    p = Pair(shape, w, None if mode == "query" else rows)
    d, plan, fc, _ = p.launch("query" if mode == "query" else "accumulate", rows)
    print(branch, mode, "two passes: need %.4f est %.4f st %d share %.4f" % (fc["need"], fc["est"], fc["st"], share(d)))
    assert d["passes"] == 2 and fc["st"] == 2 and fc["n_st"] == 128
    ASSERT[branch](d, plan, fc)
    blocks, groups, _ = p.x.exact_tile_blocks() if branch == "commit" else (np.zeros(0), None, None)
    if branch == "commit":
        assert len(blocks) == 287 and 0 < blocks.sum() < d["run"]      # the LAST pass ran under a plan, and so did the first
        assert d["total"] == (288 + 287) * p.G * 4
    else:
        assert d["run"] == d["total"] == (288 + 287) * p.G * 4
    p.row_sample_against_float64(rows, fc, "%s %s two passes:" % (branch, mode))
    p.close()


def test_one_pass_of_574_tiles_samples_every_fourth():
    shape = (128, 128, 128)
    b = R.build(*shape)
    w, rows = b["commit"]
    p = Pair(shape, w)
    d, plan, fc, _ = p.launch("query", rows)
    assert_commit(d, plan, fc)
    assert d["passes"] == 1 and fc["st"] == 4 and fc["n_st"] == 128
    blocks, groups, level2 = p.x.exact_tile_blocks()
    assert len(blocks) == 575 and int(blocks.sum()) == d["run"]
    sampled = np.arange(128) * 4
    assert int(groups[sampled].sum()) == fc["groups_run"]
    if bool(fc["level2"]) == level2:
        assert int(blocks[sampled].sum()) == fc["blocks_run"]
    p.close()


# ------------------------------------------------------------------------------------------ queries remember
def test_queries_remember_a_plan_that_paid_and_ask_again_after_a_decline():
    b = R.build(*MAIN)
    w, rows = b["commit"]
    p = Pair(MAIN, w)
    d, plan, fc, _ = p.launch("query", rows)
    assert_commit(d, plan, fc)
    assert share(d) < 0.5
    # the last transient share is below 0.5: the next query plans without an estimate
    d, plan, fc, _ = p.launch("query", rows)
    assert plan["skip"] and plan["scout"] and not plan["estimate"] and not plan["sample_tiles"], plan
    assert fc["need"] == -1.0 and fc["est"] == -1.0 and d["scouted"] == 1 and d["transient"] == 1 and share(d) < 0.5
    p.close()
    w, rows = b["tiles_decline"]
    p = Pair(MAIN, w)
    d, plan, fc, _ = p.launch("query", rows)
    assert_tiles_decline(d, plan, fc)
    # a declined one asks again (and here declines from MEMORY: the same rows need what they needed)
    d2, plan2, fc2, _ = p.launch("query", rows)
    assert fc2["need"] >= 0.9 * fc["need"] and fc2["rows"] == 128 and fc2["est"] == -1.0, (fc, fc2)
    assert not plan2["skip"] and d2["declined"] == 1 and d2["run"] == d2["total"]
    p.close()


# ------------------------------------------------------------------------------------------ twice the same bits
def test_twice_the_same_bits():
    b = R.build(*MAIN)
    w, rows = b["commit"]
    got = []
    for _ in range(2):
        p = Pair(MAIN, w)
        d, plan, fc, ids = p.launch("query", rows)
        assert_commit(d, plan, fc)
        got.append((ids, fc, d["run"]))
        p.close()
    assert np.array_equal(got[0][0], got[1][0])
    for k in ("need", "est", "est1", "blocks_run", "groups_run"):
        assert got[0][1][k] == got[1][1][k], k
