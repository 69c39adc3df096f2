// precision 'exact', block skipping: the POLICY -- what a launch decides from the measured costs of the handle's own earlier
// launches, and the STATE those decisions move from launch to launch (PlanState: the pause ladder, the re-sort schedule, the
// level-2 probe, the memory of a declined estimate).  Pure host arithmetic (no HIP, no handle): the host code (exact_host.hpp)
// feeds it the facts of a launch and acts on the LaunchPlan it gets back; som_policy_eval and som_policy_replay
// (include/somhip_test.h) expose it to the CPU test suite (tests/test_policy_cpu.py).
//
// All costs are in milliseconds PER ROW of the launch they were measured on (so that launches of different sizes compare),
// except blk_ms (per 16-unit block run) and l2_ms_group (per (tile, group) pair level 1 kept).  0 = not measured yet.
#pragma once
#include <algorithm>
#include <cstdint>

namespace somhip {
namespace policy {

struct Costs {
    double full_total = 0.0;       // BMU search of the last launch WITHOUT a plan
    double full_screen = 0.0;      //   ... of which its screen
    double plan_total = 0.0;       // BMU search of the last launch under a plan
    double plan_over = 0.0;        //   ... less its screen (plan, lists, select, refine, re-score): launches without the scout
    double plan_over_scout = 0.0;  //   ... launches with the scout (+ nearest centroid, sort, gather, pick)
    double blk_ms = 0.0;           // screen ms per 16-unit block run under a plan
    double l2_ms_group = 0.0;      // level-2 ms per (tile, group) pair level 1 kept, when it last ran
    double l2_ratio = 1.0;         // blocks after level 2 / blocks after level 1, when it last ran
    double sort_ms = 0.0;          // sort + gather
};

constexpr int TILES_PER_GROUP = 4;   // 16-unit blocks of a 64-unit group

// the screen time per block a forecast works with: measured under a plan, else derived from a full scan (5 % for the list walk)
inline double block_ms(const Costs& c, double blocks_per_row) {
    return c.blk_ms > 0.0 ? c.blk_ms : c.full_screen > 0.0 ? 1.05 * c.full_screen / blocks_per_row : 0.0;
}
// what a scouted launch spends outside its screen: measured, else a full scan's own non-screen part + a fifth of its screen
inline double scouted_overhead(const Costs& c) {
    return c.plan_over_scout > 0.0 ? c.plan_over_scout : c.full_total > 0.0 ? (c.full_total - c.full_screen) + 0.2 * c.full_screen : 0.0;
}

// COMMIT a scouted plan whose sample tiles forecast `share` of the blocks?  Priced: share x blocks x block time + overhead must
// stay 3 % under the last launch without a plan.  Not priced yet (no full scan on record): declined above 0.8 of the blocks.
inline bool commit_scouted_plan(const Costs& c, double share, double blocks_per_row) {
    const double blk = block_ms(c, blocks_per_row), over = scouted_overhead(c);
    if (blk > 0.0 && over > 0.0 && c.full_total > 0.0) return share * blocks_per_row * blk + over < 0.97 * c.full_total;
    return !(share > 0.8);
}

// LEVEL 2 from a sample that ran both levels (share after level 2, after level 1): it removes (1 - ratio) of a kept group's
// four blocks at its measured -- else: a sixth of the group's screen -- cost per kept group.  Nothing priced: below a ratio of 0.85.
inline bool level2_from_sample(const Costs& c, double share, double share1, double blocks_per_row) {
    if (!(share1 > 0.0)) return true;
    const double ratio = share / share1, blk = block_ms(c, blocks_per_row);
    const double l2c = c.l2_ms_group > 0.0 ? c.l2_ms_group : blk > 0.0 ? TILES_PER_GROUP * blk / 6.0 : 0.0;
    if (l2c > 0.0 && blk > 0.0) return (1.0 - ratio) * TILES_PER_GROUP * blk > l2c;
    return ratio < 0.85;
}
// ... and from the launch that just ran it (both measured); before that: round 4's fitted rule on the two shares
inline bool level2_pays(const Costs& c, double share, double share1) {
    if (c.l2_ms_group > 0.0 && c.blk_ms > 0.0) return (1.0 - c.l2_ratio) * TILES_PER_GROUP * c.blk_ms > c.l2_ms_group;
    return 1.5 * (share1 - share) > 0.1 * share1 + 0.006;
}

// did a SORT pay?  The blocks it saved against the stale order's share, at the measured screen time per block, over the epochs
// the order will serve, against the measured sort + gather (before those are measured: the share fell by 7 % or more)
inline bool sort_paid(const Costs& c, double share_stale, double share_fresh, double blocks_per_row, int epochs_served) {
    if (c.blk_ms > 0.0 && c.sort_ms > 0.0) return (share_stale - share_fresh) * blocks_per_row * c.blk_ms * (double)epochs_served > c.sort_ms;
    return share_fresh <= 0.93 * share_stale;
}

// an IDLE plan: it ran more than half of the blocks and cost what the last launch without a plan cost (with no such launch on
// record: it kept more than 0.97 of the blocks).  With most blocks proven empty a slow launch is somebody else's kernels on the card.
inline bool plan_idle(const Costs& c, double share) {
    return share > 0.5 && (c.full_total > 0.0 ? c.plan_total >= 0.97 * c.full_total : share > 0.97);
}

// does the scout GO ON beside last epoch's BMUs?  Its picks beat them by a tenth of the squared distance on a quarter of the rows
// AND halving the screen would still pay for it: (last share) x (screen time per block) / 2 against what a scouted launch spends
// beyond an unscouted one outside its screen (before that is measured: a tenth of a full screen)
inline bool scout_continues(const Costs& c, double win_share, double share_last, double blocks_per_row) {
    if (!(win_share >= 0.25)) return false;
    const double blk = c.blk_ms > 0.0 ? c.blk_ms : c.full_screen > 0.0 ? c.full_screen / blocks_per_row : 0.0;
    const double sc = (c.plan_over_scout > 0.0 && c.plan_over > 0.0) ? c.plan_over_scout - c.plan_over : 0.1 * c.full_screen;
    return blk > 0.0 && sc > 0.0 && 0.5 * share_last * blocks_per_row * blk > sc;
}

// is a row set large enough for the scout's fixed part (some thirty small launches, a quarter of a millisecond) to pay?
inline bool rows_worth_a_scout(double n_rows, double units, double features) { return n_rows * units * features >= 3.0e11; }


// ---- the plan's STATE from launch to launch ---------------------------------------------------------------------------------------

// Default mode: two launches in a row whose plans were idle -- rows without structure -- are followed by two launches without a
// plan (the plan costs 4-8 % of a full scan), the next idle plan by four, then eight, sixteen; a plan that pays resets the ladder.
struct Pause {
    int cooldown = 0;   // launches still to run without a plan
    int idle = 0;       // idle plans in a row
    int pause = 2;      // launches the next pause lasts (doubles while the plans stay idle)
    bool take_cooldown() { if (cooldown <= 0) return false; --cooldown; return true; }
    void plan_idle() { if (++idle >= 2) { cooldown = pause; pause = std::min(2 * pause, 16); } }   // (or declined by the sample tiles)
    void plan_paid() { idle = 0; pause = 2; }
};

// The facts of one launch, gathered by the host.  The user and test switches (SOM_EXACT_SKIP, _REFINE, _SUBBLOCKS, _RESORT) stay
// with the handle and come in here.
struct LaunchFacts {
    bool resident = false;          // the engine's resident rows (else: query rows, a streamed chunk)
    bool have_last = false;         // ... with last epoch's BMUs
    const void* rows = nullptr;     // the row set: the resident order is valid for (rows, n_rows)
    long n_rows = 0;
    bool can_skip = false, scout_ok = false;                      // up to 128 features: a plan / the scout is possible
    bool wide = false, wide_can = false, wide_scout_ok = false;   // beyond 128 features
    bool l2_fits_lds = false;       // level 2's list of kept groups fits in LDS
    bool have_lo_image = false;     // the units' second half image exists (the refinement pass reads it)
    double blocks_per_row = 0.0;    // 16-unit blocks of the whole map per row of a 256-row tile
    int skip_mode = 1;
    bool refine_on = true, sub_blocks = true;
    int res_every = 0;
};

// What a launch does.  The host may only take away from it (an allocation refused: cancel(), refine = false).
struct LaunchPlan {
    bool skip = false;          // plan and skip blocks
    bool resort = false;        // (re-)sort the rows
    bool scout = false;         // pseudo last BMUs from the scout
    bool level2 = false;        // the plan's second level (16-unit sub-blocks)
    bool estimate = false;      // ask the row sample before committing to the plan
    bool sample_tiles = false;  // ... and then the sample tiles
    bool refine = false;        // the refinement pass
    bool time_phases = true;    // time screen, level 2, sort + gather (the launch as a whole: always)
    // no plan after all: every block runs, unsorted (level2 is left as decided: nothing reads it without a plan)
    void cancel() { skip = resort = scout = estimate = sample_tiles = refine = false; time_phases = true; }
    // the rows' second half image is new: the order is rebuilt in this launch, so that the gather fills it
    void force_sort() { resort = true; time_phases = true; }
};

// What a launch measured and counted, summed over its passes.
struct LaunchOutcome {
    double t_total = 0.0, t_screen = 0.0, t_l2 = 0.0, t_sort = 0.0;   // ms
    bool screen_timed = false, l2_timed = false, sort_timed = false;
    int64_t blocks_run = 0, blocks_total = 0;   // 16-unit blocks of the screens
    int64_t groups_run = 0;                     // (tile, group) pairs level 1 kept
    int64_t pairs_in = 0, pairs_out = 0;        // candidate (row, group) pairs selected / kept by the refinement
    int64_t scout_wins = 0;                     // rows whose scout pick beat their last BMU by a tenth of the squared distance
};

// What end() made of a launch under a plan, for the SOM_DEBUG line (the values as they stood when the parent printed them).
struct LaunchReport {
    bool planned = false;
    double share = 0.0, l1_share = 0.0, pairs_per_row = 0.0, win_share = 0.0;
    bool level2_paid = false;                        // (the verdict BEFORE this launch's own)
    int epochs_since_sort = 0, next_forced_sort = 0;
    int64_t planned_epochs = 0;
};

class PlanState {
public:
    struct Stats {   // som_exact_resident_stats, som_exact_scout_stats, som_exact_refine_stats
        int64_t planned = 0, resorts = 0;          // resident epochs under a plan; sorts of the resident rows
        int64_t scouted = 0, tr_planned = 0;       // launches that ran the scout; transient launches under a plan
        int64_t scout_declined = 0;                // launches whose estimate said: nothing to skip, no plan
        int64_t pairs_refined_in = 0, pairs_refined_out = 0;
    };
    const Costs& costs() const { return costs_; }
    const Stats& stats() const { return stats_; }
    const Pause& pause(bool resident) const { return pause_[resident ? 0 : 1]; }
    // executed share of the last launch under a plan of this kind (what the screen sizes its codebook parts by)
    double share_last(bool resident) const { return resident ? res_share_last : tr_share_last; }
    // the resident order no longer holds: new rows, new passes, new sorted copies
    void order_lost() { res_valid = false; }
    bool order_valid() const { return res_valid; }   // (the top-2 launch leaves a resident order alone: exact_top2_host.hpp)

    // BEGIN A LAUNCH: does it plan at all, re-sort, scout, run level 2, ask the samples, refine; which phases it times.
    LaunchPlan begin(const LaunchFacts& f) {
        LaunchPlan p;
        // A plan needs, per row, SOME unit whose distance bounds the distance to the BMU: last epoch's BMU (resident rows from
        // their second epoch on) or a pseudo last BMU from the scout.  Beyond 128 features: resident rows with last BMUs, or the scout.
        const bool wide_skip = f.wide_can && (f.have_last || f.wide_scout_ok);
        p.skip = (f.can_skip && (f.have_last || f.scout_ok)) || wide_skip;
        if (p.skip && f.skip_mode == 1 && pause_[f.resident ? 0 : 1].take_cooldown()) p.skip = false;
        // the resident sorted pass: (re-)sort when there is none for these rows, when asked to (res_every = n: every n-th
        // planned epoch), or when the order has gone stale: while a quarter of the blocks or more still run a sort costs a few
        // percent of the screen it sharpens (the early epochs of a schedule, where rows still travel across the map); later
        // every eighth planned epoch, and a sort that did not pay (the share it left is within 7 % of the stale order's, level 2 on
        // or off in both: the schedule, not the order, moves the share) doubles that interval, up to 64; one that paid resets it.
        // (Measured, tools/resid_probe.py + bound_probe.py: past a schedule's first epochs an order three epochs old runs the same
        // blocks as a fresh one; a trigger on the share's growth fired on the schedule's own late growth, where sorting buys nothing.)
        // A stale order costs speed, never correctness: the plan tests every row of a tile where it sits.
        // A transient row set is sorted by the scout every time (there is nothing to keep).
        if (p.skip) {
            const bool fresh = !f.resident || !f.have_last || !res_valid || res_rows != f.rows || res_n != f.n_rows;
            if (fresh) p.resort = true;
            else if (f.res_every > 0) p.resort = res_since >= f.res_every;
            else p.resort = res_share_last >= 0.25 || res_since >= res_forced;
            // the scout: always where there is no last BMU; with one, in the epochs that sort anyway because much of the map still
            // runs -- there the bound from the current codebook's own centroids is the better one (tools/ucent_probe.py: 0.78 against
            // 0.95 of the blocks in a schedule's second epoch, 0.28 against 0.52 in its third), and the plan takes the better of the
            // two units row by row
            // ... and goes on, sorting the rows by its keys, while its picks still beat last epoch's BMUs by a tenth of the squared
            // distance or more on a quarter of the rows (counted in the plan's prologue) AND halving the screen would still pay for
            // it: (last share) x (measured screen time per block) / 2 against what a scouted launch spends beyond an unscouted one
            // outside its screen (measured; before that: a tenth of a full screen)
            const bool scout_on_wins = f.scout_ok && f.have_last && !fresh && scout_continues(costs_, scout_win_share, res_share_last, f.blocks_per_row);
            if (scout_on_wins) p.resort = true;
            p.scout = f.scout_ok && (!f.have_last || (p.resort && (fresh || res_share_last >= 0.25 || scout_on_wins)));
            if (f.wide) p.scout = f.wide_scout_ok && !f.have_last;    // (beyond 128 features: only where there is no last BMU)
            // level 2 of the plan (the groups' 16-unit sub-blocks) where it pays.  Whether it does is MEASURED each time it runs
            // (both levels' shares come back with the pass's counters): it costs about a tenth of level 1's share of a full scan
            // (four centroids per kept group), it saves the blocks it drops -- on the smooth maps of a schedule's first epochs
            // and on the compact patches of its middle it drops next to nothing, late, when the patches have spread out, more
            // than half.  While it does not pay it is probed again every fourth planned epoch, or at once when level 1's share
            // has moved by half since the last probe.
            bool probe = l1_share_probe < 0.0 || l2_wait <= 0 || l1_share_last > 1.5 * l1_share_probe || l1_share_last < l1_share_probe / 1.5;
            // (a new row set starts like a new engine: level 2 is taken to pay until it has been measured on these rows)
            if (fresh && f.resident) { l2_pays = true; l1_share_probe = -1.0; }
            if (l1_share_last > 0.9 && l1_share_probe >= 0.0 && !l2_pays) probe = false;   // (nothing for four times the centroids to find)
            p.level2 = !f.wide && f.sub_blocks && (l2_pays || probe || f.skip_mode >= 2 || !f.resident) && f.l2_fits_lds;
        }
        // (the forecast from samples: where the scout plans and there is no good recent plan of the same kind to go by;
        //  beyond 128 features: the row sample only, no sample tiles)
        p.estimate = p.skip && p.scout && f.skip_mode == 1 && (f.resident || tr_share_last >= 0.5);
        p.sample_tiles = p.estimate && !f.wide;
        // the refinement pass (bmu_exact.hpp) where it pays: it costs about a third of the float32 re-score of the pairs it is
        // given (it is bound by the same gather of rows) and leaves one to one and a half pairs a row, at two small launches more:
        // worth it from three candidate pairs a row on (the last planned epoch's count) -- the smooth maps of a schedule's middle
        p.refine = p.skip && f.refine_on && f.have_lo_image && (pairs_per_row_last >= 3.0 || f.skip_mode >= 2);
        // the phases under a plan -- screen, level 2, sort + gather -- are timed in the first planned launches, in every launch
        // that sorts or scouts, and every fourth one after that
        p.time_phases = !p.skip || since >= 3 || costs_.blk_ms == 0.0 || p.resort || p.scout;
        return p;
    }

    // THE ROW SAMPLE RETURNED: a sampled row needs `f` of the groups.  A tile needs at least what its rows need: where a row alone
    // needs more than 0.9 of the groups -- a random codebook, rows without structure -- the launch runs without the scout, the
    // sort and the plan.  Returns whether it declined.
    bool rows_sampled(double f, LaunchPlan& p) {
        // (... or about as much as when the sample tiles last said no, up to eight launches ago: the same answer without asking them)
        if (scout_f_age < 8) scout_f_age += 1; else scout_f_declined = 0.0;
        scout_f_now = f;
        if (!(f > 0.9 || (scout_f_declined > 0.0 && f >= 0.9 * scout_f_declined))) return false;
        // (nearly free: not counted as an idle plan, asked again at the next launch)
        p.cancel(); stats_.scout_declined += 1;
        return true;
    }

    // THE SAMPLE TILES RETURNED: they would run `share` of their blocks (`share1` after level 1 alone).  Commit the scouted plan,
    // and with level 2?  Returns whether it declined.
    bool tiles_sampled(double share, double share1, const LaunchFacts& f, LaunchPlan& p) {
        const bool decline = !commit_scouted_plan(costs_, share, f.blocks_per_row);
        if (p.level2 && share1 > 0.0 && f.skip_mode == 1) p.level2 = level2_from_sample(costs_, share, share1, f.blocks_per_row);
        if (decline) { scout_f_declined = scout_f_now; scout_f_age = 0; } else scout_f_declined = 0.0;
        if (decline) {
            p.cancel(); stats_.scout_declined += 1;
            if (f.resident) res_valid = false;       // (the order was rebuilt, the sorted copies were not)
            // (a declined plan counts as an idle one: rows without structure are asked less and less often)
            pause_[f.resident ? 0 : 1].plan_idle();
        }
        return decline;
    }

    // END OF THE LAUNCH: what it cost, per row; what its plan ran; what that says about the next one.
    LaunchReport end(const LaunchFacts& f, const LaunchPlan& p, const LaunchOutcome& o) {
        LaunchReport r;
        const long N = f.n_rows;
        if (N > 0 && o.t_total > 0.0) {
            if (!p.skip) {
                costs_.full_total = o.t_total / (double)N;
                if (o.screen_timed && o.t_screen > 0.0) costs_.full_screen = o.t_screen / (double)N;
            } else {
                costs_.plan_total = o.t_total / (double)N;
                if (o.screen_timed && o.t_screen > 0.0) {
                    (p.scout ? costs_.plan_over_scout : costs_.plan_over) = (o.t_total - o.t_screen) / (double)N;
                    if (o.blocks_run > 0) costs_.blk_ms = o.t_screen / (double)o.blocks_run;
                    since = 0;
                } else {
                    since += 1;
                }
                if (o.sort_timed && o.t_sort > 0.0) costs_.sort_ms = o.t_sort / (double)N;
            }
        }
        if (!p.skip || o.blocks_total <= 0) return r;
        const double share = (double)o.blocks_run / (double)o.blocks_total;
        const double l1_share = (double)o.groups_run * TILES_PER_GROUP / (double)o.blocks_total;
        if (p.scout) stats_.scouted += 1;
        if (f.resident) scout_win_share = (p.scout && f.have_last) ? (double)o.scout_wins / (double)std::max<long>(N, 1) : 0.0;
        pairs_per_row_last = (double)o.pairs_in / (double)std::max<long>(N, 1);
        if (p.refine) { stats_.pairs_refined_in += o.pairs_in; stats_.pairs_refined_out += o.pairs_out; }
        if (p.level2 && o.l2_timed && o.t_l2 > 0.0 && o.groups_run > 0) {
            costs_.l2_ms_group = o.t_l2 / (double)o.groups_run;
            costs_.l2_ratio = l1_share > 0.0 ? share / l1_share : 1.0;
        }
        // an IDLE plan: the launch cost what the last launch without a plan cost (per row; with no such launch on record: it
        // kept more than 0.97 of the blocks) and ran more than half of the blocks (plan_idle above)
        const bool idle = plan_idle(costs_, share);
        Pause& pause = pause_[f.resident ? 0 : 1];
        r.planned = true; r.share = share; r.l1_share = l1_share; r.pairs_per_row = pairs_per_row_last;
        if (!f.resident) {
            stats_.tr_planned += 1;
            tr_share_last = share;
            if (f.skip_mode == 1) { if (idle) pause.plan_idle(); else pause.plan_paid(); }
            return r;
        }
        stats_.planned += 1;
        if (p.resort) {
            // a sort that did not pay doubles the wait before the next one, up to 64 epochs; one that paid resets it to eight.  Paid:
            // the blocks it saved against the stale order's share, at the measured screen time per block, over the epochs the order
            // will serve, outweigh the measured sort + gather (before those are measured: the share fell by 7 % or more)
            if (res_valid && res_share_last < 0.25 && res_l2_last == p.level2) {
                const bool paid = sort_paid(costs_, res_share_last, share, f.blocks_per_row, res_forced);
                res_forced = paid ? 8 : std::min(2 * res_forced, 64);
            }
            stats_.resorts += 1; res_since = 0; res_valid = true; res_rows = f.rows; res_n = f.n_rows;
        }
        res_since += 1;
        res_share_last = share; res_l2_last = p.level2;
        l1_share_last = l1_share;
        r.win_share = scout_win_share; r.level2_paid = l2_pays; r.epochs_since_sort = res_since; r.next_forced_sort = res_forced; r.planned_epochs = stats_.planned;
        if (p.level2) {
            // level 2 pays where the blocks it removes from a kept group -- (1 - ratio) of four, at the measured screen time per block
            // -- cost more than its own measured time per kept group (before both are measured: round 4's fitted rule)
            l2_pays = level2_pays(costs_, share, l1_share_last);
            l1_share_probe = l1_share_last;
            l2_wait = 4;
        } else {
            l2_wait -= 1;
        }
        if (f.skip_mode == 1) { if (idle) pause.plan_idle(); else pause.plan_paid(); }
        return r;
    }

private:
    Costs costs_;
    int since = 99;                   // planned launches since the phases were last timed
    Pause pause_[2];                  // [0] the resident rows, [1] transient row sets
    Stats stats_;
    // the resident sorted pass
    const void* res_rows = nullptr; long res_n = -1;   // the rows it was sorted from
    bool res_valid = false;
    int res_since = 0;                // planned epochs since the last sort
    int res_forced = 8;               // planned epochs after which the rows are sorted in any case (doubles after a forced sort that did not pay)
    double res_share_last = 1.0;      // executed share of the last planned epoch
    bool res_l2_last = false;         // ... whether level 2 ran in it (shares compare like with like)
    double pairs_per_row_last = 0.0;  // candidate (row, group) pairs per row of the last planned epoch
    double scout_f_now = 0.0, scout_f_declined = 0.0; int scout_f_age = 0;   // the sampled rows' need now / when the sample tiles last declined a plan
    double scout_win_share = 0.0;     // rows of the last launch whose scout pick beat their last BMU by a tenth of the squared distance
    double tr_share_last = 1.0;       // executed share of the last transient launch under a plan
    // level 2 of the plan runs where it pays (l2_pays: measured whenever it runs), is probed again after l2_wait epochs or
    // when level 1's share has moved by half since the last probe
    double l1_share_last = 1.0, l1_share_probe = -1.0;
    bool l2_pays = true;
    int l2_wait = 0;
};

}  // namespace policy
}  // namespace somhip
