"""The exact mode's block-skipping POLICY (csrc/exact_policy.hpp) without a GPU: pure functions of measured costs, reached through
the library's test hook som_policy_eval (include/somhip_test.h).  What is pinned: each decision's direction in its cost terms, its
behaviour before anything is measured, and the benchmark's own recorded numbers (profiles/r05_*: epoch 1 of the schedule is
committed at a forecast of 0.58, a random codebook's 1.0 is declined; level 2 pays late in the schedule and not on the smooth map
after the first merge)."""
import ctypes as C

import pytest

from xpysom_dask_amd import _lib

NAMES = ("full_total", "full_screen", "plan_total", "plan_over", "plan_over_scout", "blk_ms", "l2_ms_group", "l2_ratio", "sort_ms")
BPR = 1024 * 4 / 256.0            # 16-unit blocks per row at 256 x 256 units: 1024 groups x 4 / 256-row tiles


def ev(which, costs, *args):
    lib = _lib.load()
    c = dict(full_total=0.0, full_screen=0.0, plan_total=0.0, plan_over=0.0, plan_over_scout=0.0, blk_ms=0.0, l2_ms_group=0.0, l2_ratio=1.0, sort_ms=0.0)
    c.update(costs)
    ca = (C.c_double * 9)(*[c[k] for k in NAMES])
    aa = (C.c_double * 4)(*(list(args) + [0.0] * (4 - len(args))))
    out = C.c_int32(-1)
    assert lib.som_policy_eval(which, ca, aa, C.byref(out)) == 0
    return bool(out.value)


# the benchmark's own measurements (per row of a 1 Mi-row launch, ms): profiles/r05_* schedule traces
FULL = dict(full_total=14.6 / 2 ** 20, full_screen=13.2 / 2 ** 20)
PLANNED = dict(FULL, plan_total=1.3 / 2 ** 20, plan_over=1.05 / 2 ** 20, plan_over_scout=3.0 / 2 ** 20, blk_ms=1.0e-6, l2_ms_group=0.8e-6, l2_ratio=0.5, sort_ms=0.6 / 2 ** 20)


def test_commit_a_scouted_plan():
    assert not ev(0, {}, 1.0, BPR) and not ev(0, {}, 0.81, BPR) and ev(0, {}, 0.8, BPR) and ev(0, {}, 0.02, BPR)   # nothing priced: 0.8
    assert ev(0, FULL, 0.58, BPR)                            # epoch 1 of the schedule: committed (it costs what the scan costs)
    assert not ev(0, FULL, 1.0, BPR) and not ev(0, FULL, 0.9, BPR)
    assert ev(0, PLANNED, 0.04, BPR) and not ev(0, PLANNED, 0.95, BPR)
    # monotone in the forecast, in the block time and in the overhead
    shares = [s / 100.0 for s in range(0, 101)]
    got = [ev(0, PLANNED, s, BPR) for s in shares]
    assert got == sorted(got, reverse=True) and got[0] and not got[-1]
    assert ev(0, PLANNED, 0.5, BPR) and not ev(0, dict(PLANNED, blk_ms=2.0e-6), 0.5, BPR)
    assert not ev(0, dict(PLANNED, plan_over_scout=14.0 / 2 ** 20), 0.04, BPR)


def test_level_two():
    # from a sample: the smooth map after the first merge (0.7491 -> 0.7238 of the blocks) does not pay, the late map (0.25 -> 0.07) does
    assert not ev(1, FULL, 0.7238, 0.7491, BPR) and ev(1, FULL, 0.07, 0.25, BPR)
    assert ev(1, {}, 0.5, 0.7, BPR) and not ev(1, {}, 0.69, 0.7, BPR)            # nothing priced: a ratio below 0.85
    assert ev(1, FULL, 0.0, 0.0, BPR)                                            # no sample of level 1: on
    # measured: (1 - ratio) * 4 * block time against its own time per kept group
    assert ev(2, PLANNED, 0.01, 0.02) and not ev(2, dict(PLANNED, l2_ratio=0.9), 0.01, 0.02)
    assert not ev(2, dict(PLANNED, l2_ms_group=3.0e-6), 0.01, 0.02)
    assert ev(2, {}, 0.02, 0.2) and not ev(2, {}, 0.19, 0.2)                     # before both are measured: round 4's rule


def test_sort_paid_idle_plans_and_the_scout():
    assert ev(3, PLANNED, 0.04, 0.02, BPR, 8) and not ev(3, PLANNED, 0.0201, 0.02, BPR, 8)
    assert ev(3, PLANNED, 0.0215, 0.02, BPR, 64) and not ev(3, PLANNED, 0.0215, 0.02, BPR, 1)   # the epochs the order will serve count
    assert ev(3, {}, 0.1, 0.09, BPR, 8) and not ev(3, {}, 0.1, 0.095, BPR, 8)                   # unmeasured: the share fell by 7 %
    assert not ev(4, PLANNED, 0.02) and not ev(4, dict(PLANNED, plan_total=20.0 / 2 ** 20), 0.3)   # few blocks run: never idle
    assert ev(4, dict(PLANNED, plan_total=14.5 / 2 ** 20), 0.9) and not ev(4, dict(PLANNED, plan_total=10.0 / 2 ** 20), 0.9)
    assert ev(4, {}, 0.98) and not ev(4, {}, 0.96)
    assert not ev(5, PLANNED, 0.2, 0.9, BPR)                                      # too few wins
    assert ev(5, PLANNED, 0.6, 0.5, BPR) and not ev(5, PLANNED, 0.6, 0.03, BPR)   # ... and halving the screen must pay for it
    assert not ev(6, {}, 30000, 65536, 128) and ev(6, {}, 40000, 65536, 128) and not ev(6, {}, 1e6, 4096, 32)


def test_unknown_decision_is_refused():
    lib = _lib.load()
    out = C.c_int32(0)
    ca, aa = (C.c_double * 9)(), (C.c_double * 4)()
    assert lib.som_policy_eval(99, ca, aa, C.byref(out)) != 0
    assert lib.som_policy_eval(0, None, aa, C.byref(out)) != 0


# ---- the plan's STATE from launch to launch (policy::PlanState) through som_policy_replay --------------------------------------------
# The expected sequences below are written out from the rules the library documents (csrc/exact_policy.hpp), launch by launch.
N_ROWS = 2 ** 20
OUT = ("skip", "resort", "scout", "level2", "estimate", "sample_tiles", "refine", "time_phases", "asked_rows", "asked_tiles",
       "rows_declined", "tiles_declined")


def L(**kw):
    """One launch of a script: facts, sample answers, outcome.  Default: resident rows with last BMUs on a 256 x 256 map, default
    mode, no scout; a plan that runs a tenth of the blocks (level 1 alone: a fifth) in 1 ms."""
    d = dict(resident=1, have_last=1, rows=1, n=N_ROWS, can_skip=1, scout_ok=0, wide=0, wide_can=0, wide_scout_ok=0, l2_fits=1, lo=1,
             bpr=BPR, mode=1, refine_on=1, sub_blocks=1, res_every=0, f=0.5, est=-1.0, est1=0.0,
             t_total=1.0, t_screen=0.5, t_l2=0.05, t_sort=0.1, share=0.1, l1_share=0.2, pairs_row=1.0, pairs_out_row=1.0, win_share=0.0)
    assert set(kw) <= set(d), set(kw) - set(d)
    d.update(kw)
    return d


def replay(script):
    lib = _lib.load()
    flat = []
    for d in script:
        total = d["n"] * d["bpr"]                            # 16-unit blocks of the launch
        flat += [d["resident"], d["have_last"], d["rows"], d["n"], d["can_skip"], d["scout_ok"], d["wide"], d["wide_can"], d["wide_scout_ok"],
                 d["l2_fits"], d["lo"], d["bpr"], d["mode"], d["refine_on"], d["sub_blocks"], d["res_every"], d["f"], d["est"], d["est1"],
                 d["t_total"], d["t_screen"], d["t_l2"], d["t_sort"], round(d["share"] * total), total, round(d["l1_share"] * total / 4),
                 round(d["pairs_row"] * d["n"]), round(d["pairs_out_row"] * d["n"]), round(d["win_share"] * d["n"])]
    n_in, n_out = 29, 18
    assert len(flat) == n_in * len(script)
    out = (C.c_double * (n_out * len(script)))()
    assert lib.som_policy_replay(len(script), (C.c_double * len(flat))(*flat), out) == 0
    res = []
    for i in range(len(script)):
        o = [int(v) for v in out[n_out * i:n_out * (i + 1)]]
        r = dict(zip(OUT, o[:12]))
        r["res_pause"], r["tr_pause"] = tuple(o[12:15]), tuple(o[15:18])   # (cooldown, idle, pause)
        res.append(r)
    return res


def col(res, key):
    return [r[key] for r in res]


IDLE = dict(share=1.0, l1_share=1.0)         # a plan that kept every block: idle
SCOUTED = dict(have_last=0, scout_ok=1)      # rows without last BMUs: the scout plans, the samples are asked first


def test_pause_ladder_doubles_up_to_sixteen():
    # plan, plan, 2 without, plan, 4 without, plan, 8 without, plan, 16 without, plan, 16 without
    want = [1, 1] + [0] * 2 + [1] + [0] * 4 + [1] + [0] * 8 + [1] + [0] * 16 + [1] + [0] * 16 + [1]
    res = replay([L(**IDLE) for _ in want])
    assert col(res, "skip") == want
    assert res[1]["res_pause"] == (2, 2, 4) and res[4]["res_pause"] == (4, 3, 8) and res[-1]["res_pause"] == (16, 7, 16)
    assert all(r["tr_pause"] == (0, 0, 2) for r in res)


def test_a_paying_plan_resets_the_ladder():
    script = [L(**IDLE), L(**IDLE), L(**IDLE), L(**IDLE), L(share=0.1), L(**IDLE), L(**IDLE), L(**IDLE), L(**IDLE), L(**IDLE)]
    res = replay(script)
    assert col(res, "skip") == [1, 1, 0, 0, 1, 1, 1, 0, 0, 1]      # ... "two idle plans, then 2" again, not 4
    assert res[4]["res_pause"] == (0, 0, 2) and res[6]["res_pause"] == (2, 2, 4)


def test_a_plan_the_sample_tiles_decline_counts_as_idle():
    # (a lower f each time: at 0.9 of the declined f or more the row sample would answer for the tiles)
    script = [L(f=0.5, est=1.0, est1=1.0, **SCOUTED), L(f=0.4, est=1.0, est1=1.0, **SCOUTED), L(**SCOUTED), L(**SCOUTED),
              L(f=0.3, est=1.0, est1=1.0, **SCOUTED)]
    res = replay(script)
    assert col(res, "skip") == [0, 0, 0, 0, 0]
    assert col(res, "asked_tiles") == [1, 1, 0, 0, 1] and col(res, "tiles_declined") == [1, 1, 0, 0, 1]
    assert col(res, "asked_rows") == [1, 1, 0, 0, 1]               # (a paused launch asks nothing)
    assert [r["res_pause"] for r in res] == [(0, 1, 2), (2, 2, 4), (1, 2, 4), (0, 2, 4), (4, 3, 8)]


def test_resident_and_transient_ladders_do_not_touch():
    R, T = L(**IDLE), L(resident=0, rows=7, n=65536, f=0.5, **dict(IDLE, **SCOUTED))
    res = replay([R, T, R, T, T, R, R, T])
    assert col(res, "skip") == [1, 1, 1, 1, 0, 0, 0, 0]
    assert [r["res_pause"] for r in res] == [(0, 1, 2), (0, 1, 2), (2, 2, 4), (2, 2, 4), (2, 2, 4), (1, 2, 4), (0, 2, 4), (0, 2, 4)]
    assert [r["tr_pause"] for r in res] == [(0, 0, 2), (0, 1, 2), (0, 1, 2), (2, 2, 4), (1, 2, 4), (1, 2, 4), (1, 2, 4), (0, 2, 4)]


@pytest.mark.parametrize("mode", [2, 3])
def test_forced_modes_never_pause(mode):
    res = replay([L(mode=mode, **IDLE) for _ in range(8)])
    assert col(res, "skip") == [1] * 8 and all(r["res_pause"] == (0, 0, 2) for r in res)


def sorts(res):
    return [i + 1 for i, r in enumerate(res) if r["resort"]]     # launches, counted from 1


def test_fresh_rows_sort():
    res = replay([L(), L(), L(rows=2), L(rows=2), L(rows=2, n=N_ROWS // 2), L(rows=2, n=N_ROWS // 2),
                  L(rows=2, n=N_ROWS // 2, est=-1.0, **SCOUTED), L(rows=2, n=N_ROWS // 2)])
    assert col(res, "resort") == [1, 0, 1, 0, 1, 0, 1, 0]          # never sorted; new X; new N; no last BMUs


def test_resort_while_a_quarter_of_the_blocks_run_then_every_eighth_epoch():
    res = replay([L(share=0.3, l1_share=0.4), L(share=0.25, l1_share=0.4), L(share=0.1)] + [L() for _ in range(10)])
    assert sorts(res) == [1, 2, 3, 11]                             # last share >= 0.25: sort; then 8 planned epochs after the last one


def test_an_unpaid_sort_doubles_the_interval_up_to_64_and_a_paid_one_resets_it():
    res = replay([L() for _ in range(190)])                        # the same share before and after every sort: none pays
    assert sorts(res) == [1, 9, 25, 57, 121, 185]                  # 8, 16, 32, 64, 64
    script = [L() for _ in range(60)]
    script[24] = L(share=0.02, l1_share=0.04)                      # the sort at launch 25 (interval 16 by then) takes 0.1 -> 0.02: paid
    for i in range(25, 60):
        script[i] = L(share=0.02, l1_share=0.04)
    assert sorts(replay(script)) == [1, 9, 25, 33, 49]             # ... back to 8; the next one is unpaid again: 16


def test_a_sort_is_judged_only_between_like_epochs():
    script = [L() for _ in range(34)]
    script[8] = L(sub_blocks=0)                                    # the sort at launch 9 runs without level 2, the epoch before ran with it
    assert sorts(replay(script)) == [1, 9, 17, 33]                 # not judged: still 8; launch 17's is (unpaid): 16
    # last share >= 0.25: sorted in any case, never judged
    res = replay([L(share=0.3, l1_share=0.4) for _ in range(12)] + [L() for _ in range(10)])
    assert sorts(res) == list(range(1, 14)) + [21]


def test_res_every_overrides_the_schedule():
    res = replay([L(res_every=3, share=0.3, l1_share=0.4) for _ in range(10)])
    assert sorts(res) == [1, 4, 7, 10]


NO_PAY = dict(share=0.19, l1_share=0.2)      # level 2 drops a twentieth of level 1's blocks at an eighth of a block's time per group: no


def test_level_two_is_on_until_measured_then_probed_after_four_epochs_without():
    res = replay([L(**NO_PAY) for _ in range(12)])
    assert col(res, "level2") == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    assert col(replay([L() for _ in range(6)]), "level2") == [1] * 6          # where it pays it stays


def test_level_two_is_probed_at_once_when_level_ones_share_moves_by_half():
    assert col(replay([L(**NO_PAY), L(share=0.3, l1_share=0.31), L(share=0.3, l1_share=0.31)]), "level2") == [1, 0, 1]
    assert col(replay([L(**NO_PAY), L(share=0.12, l1_share=0.13), L(share=0.12, l1_share=0.13)]), "level2") == [1, 0, 1]
    assert col(replay([L(**NO_PAY), L(share=0.28, l1_share=0.29), L(share=0.28, l1_share=0.29)]), "level2") == [1, 0, 0]


def test_level_two_is_not_probed_while_level_one_keeps_nearly_everything():
    res = replay([L(share=0.94, l1_share=0.95, t_total=0.6) for _ in range(12)])
    assert col(res, "skip") == [1] * 12 and col(res, "level2") == [1] + [0] * 11


def test_a_fresh_resident_row_set_starts_level_two_over():
    assert col(replay([L(**NO_PAY), L(**NO_PAY), L(rows=2, **NO_PAY), L(rows=2, **NO_PAY)]), "level2") == [1, 0, 1, 0]


def test_row_sample_declines_above_nine_tenths():
    res = replay([L(f=0.91, **SCOUTED), L(f=0.9, **SCOUTED)])
    assert col(res, "asked_rows") == [1, 1] and col(res, "rows_declined") == [1, 0] and col(res, "skip") == [0, 1]
    assert col(res, "asked_tiles") == [0, 0]                       # (est < 0: passes too short for sample tiles)
    assert res[0]["res_pause"] == (0, 0, 2)                        # nearly free: not an idle plan


def test_row_sample_remembers_a_tile_decline_for_eight_launches():
    script = [L(f=0.5, est=1.0, est1=1.0, **SCOUTED)] + [L(f=0.46, est=1.0, est1=1.0, **SCOUTED) for _ in range(9)]
    res = replay(script)
    assert col(res, "asked_tiles") == [1] + [0] * 8 + [1]
    assert col(res, "rows_declined") == [0] + [1] * 8 + [0]
    assert [r["res_pause"] for r in res[:9]] == [(0, 1, 2)] * 9    # the remembered answers are not idle plans
    # below 0.9 of the declined f the tiles are asked again at once
    res = replay([L(f=0.5, est=1.0, est1=1.0, **SCOUTED), L(f=0.44, est=0.1, est1=0.2, **SCOUTED)])
    assert col(res, "asked_tiles") == [1, 1] and col(res, "skip") == [0, 1]


def test_refinement_from_three_pairs_a_row():
    res = replay([L(pairs_row=3.0), L(pairs_row=2.99), L(pairs_row=5.0), L(pairs_row=5.0, lo=0), L(refine_on=0)])
    assert col(res, "refine") == [0, 1, 0, 0, 0]
    assert col(replay([L(mode=2, pairs_row=0.0), L(mode=3, pairs_row=0.0)]), "refine") == [1, 1]


def test_replay_refuses_null_arguments():
    lib = _lib.load()
    assert lib.som_policy_replay(1, None, (C.c_double * 18)()) != 0
    assert lib.som_policy_replay(-1, (C.c_double * 29)(), (C.c_double * 18)()) != 0
