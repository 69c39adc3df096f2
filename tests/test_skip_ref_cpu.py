"""The float64 model of block skipping (tests/skip_ref.py) on the case table tests/test_gpu_skip_bound.py runs: the inputs have
teeth.  No GPU: som_patch_order is host arithmetic.

For every case: the true model keeps the BMU block of every adversarial row and skips at least half of all (row, group)
pairs; every applicable mutant of the model -- a radius that leaves the moved unit out, centroids of the codebook before the
move, a seed under that codebook, a sub-block filed under its neighbour's slot, the tail of a partial group ignored -- drops
the BMU block of at least one adversarial row (the collinear rows: a radius shrunk by eps / 8); the float64 BMU of every
adversarial moved_units row wins by a factor of 100 or more in squared distance."""
import numpy as np
import pytest

from tests import skip_ref as R

CASES = R.CASES
IDS = [c["id"] for c in CASES]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_model_keeps_every_bmu_block_and_the_mutants_do_not(c):
    b = R.build(c)
    levels = R.levels_of(c)
    keep1, keep2 = R.plan(b, None, levels)
    ok = R.bmu_block_kept(b, keep1, keep2)
    assert ok.all(), "the true model drops the BMU block of rows %s" % np.flatnonzero(~ok)[:8]
    s1, s2 = R.shares(b, keep1, keep2)
    print("%s: the model keeps %.3f of the (row, group) pairs, %.3f of the (row, 16-unit block) pairs" % (c["id"], s1, s2))
    assert s1 <= 0.5, "the true model skips only %.3f of the (row, group) pairs" % (1.0 - s1)
    adv = b["adv"]
    assert len(adv) >= 8
    for m in R.MUTANTS:
        if not R.applicable(b, m, levels):
            continue
        k1, k2 = R.plan(b, m, levels)
        dropped = ~R.bmu_block_kept(b, k1, k2)[adv]
        assert dropped.any(), "mutant %r drops no adversarial row's BMU block: the case cannot tell it from the true bound" % m
        print("   mutant %-10s drops the BMU block of %d of %d adversarial rows" % (m, int(dropped.sum()), len(adv)))
    if c["kind"] == "moved_units":
        assert b["margin"][adv].min() >= 100.0, b["margin"][adv].min()
        # the BMU of an adversarial row is a moved unit, its last unit is not the unit it picks now
        assert np.isin(b["bmu"][adv], b["moved"]).all() and (b["last"][adv] != b["bmu"][adv]).all()


def test_the_table_covers_the_layouts_the_issue_names():
    """Partial last groups with cnt in 1..15 and in 17..63, strips and 4 x 4 squares, one and two levels, the positions 0, 15, 16,
    47, 63 and the last position of a partial group."""
    cnts, layouts, levels = set(), set(), set()
    for c in CASES:
        b = R.build(c)
        K = c["X"] * c["Y"]
        cnts.add(K % 64)
        layouts.add(c["X"] % 8 == 0 and c["Y"] % 8 == 0 and c["env"].get("SOM_EXACT_SUB44") != "0")
        levels.add(R.levels_of(c))
        if c["kind"] == "moved_units":
            inv = np.empty(K, np.int64)
            inv[b["perm"]] = np.arange(K)
            pos = set((inv[b["moved"]] & 63).tolist())
            assert set(R.POSITIONS) <= pos, pos
            if K % 64:
                assert int(inv[b["moved"][-1]]) == K - 1
    assert any(1 <= v <= 15 for v in cnts) and any(17 <= v <= 63 for v in cnts) and 0 in cnts
    assert layouts == {True, False} and levels == {1, 2}


def test_slot_arithmetic_is_a_bijection_onto_the_level_2_table():
    for K in (64, 210, 256, 525, 561, 4096, 4608):
        G = R.n_groups(K)
        slots = [R.slot_of(g, b) for g in range(G) for b in range(4)]
        assert len(set(slots)) == 4 * G and max(slots) < R.n_slots(K, 1)
        seen = np.concatenate([R.block_positions(K, 1, s) for s in range(R.n_slots(K, 1))])
        assert np.array_equal(np.sort(seen), np.arange(K))
        for g in range(G):
            grp = np.concatenate([R.block_positions(K, 1, R.slot_of(g, b)) for b in range(4)])
            assert np.array_equal(grp, R.block_positions(K, 0, g))


@pytest.mark.parametrize("eps", R.COLLINEAR_EPS)
def test_collinear_slack_and_the_share_the_float64_reference_decides(eps):
    """The ideal test keeps k's group with a relative slack of eps delta / (r + delta) -- about eps / 20 --, and the float64
    reference decides (margin above the float32 window) at least 90 % of the COLLINEAR rows for exactly the eps listed in
    COLLINEAR_F64_EPS (every filler row is decided at every eps: they do not count towards the cap)."""
    c = [c for c in CASES if c["kind"] == "collinear" and c["eps"] == eps][0]
    b = R.build(c)
    slack = R.collinear_slack(b)
    print("eps 2^%d: slack of the ideal test %.3g .. %.3g" % (int(np.log2(eps)), slack.min(), slack.max()))
    assert (slack > 0).all() and slack.max() < eps / 10.0 and slack.min() > eps / 40.0
    a = b["adv"]
    # (the adversarial rows' BMU is k, a sheet unit; their last unit -- the helper -- is the runner-up)
    assert np.isin(b["bmu"][a], b["moved"]).all()
    left_out = R.undecided(b)
    print("eps 2^%d: %.3f of the rows are left out of the float64 check (%d of the %d collinear rows among them)" % (
        int(np.log2(eps)), left_out.mean(), int(left_out[a].sum()), len(a)))
    assert not left_out[np.setdiff1d(np.arange(len(left_out)), a)].any()
    assert (left_out[a].mean() <= R.COLLINEAR_F64_CAP) == (eps in R.COLLINEAR_F64_EPS), left_out[a].mean()
