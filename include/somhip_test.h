/* somhip_test.h -- entry points of libsomhip.so that exist for the test suite and the measurement tools only.
 * Not part of the drop-in boundary (include/somhip.h): nothing a caller of the hot path needs, nothing whose behaviour is
 * promised from one build to the next. */
#ifndef SOMHIP_TEST_H
#define SOMHIP_TEST_H

#include "somhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the canary's TEST HOOK (som_set_verify, include/somhip.h): zeroes the operand images the kernels read (bit 0: the 16-bit
 * image, bit 1: the float32 image) without marking them stale, as a lost staging copy would (tests/test_gpu_verify.py). */
int som_debug_corrupt_operands(som_handle* h, int32_t which);

/* read-only: a 64-bit FNV-1a hash of one of the codebook's operand buffers as it stands on the device right now (nothing is
 * refreshed first).  which: 0 the 16-bit stage image, 1 its second half (exact mode), 2 the float32 stage image, 3 |w|^2 in the
 * image order, 4 the screen's norms, 5 the {max |w|^2, max rounding error^2} pair, 6 the exact plan's centroids, radii, |c|^2 and
 * maxima of both levels, 7 the codebook in the image order.  A buffer the handle does not hold hashes as the empty string.
 * tests/test_gpu_exact_merge_prep.py compares the fused merge's operands with the separate kernels' through it. */
int som_debug_operand_crc(som_handle* h, int32_t which, uint64_t* out);

/* read-only: the exact plan's block geometry of one level as it stands on the device right now -- centroids C_out
 * [n_slots][input_len], radii r_out [n_slots] (a slot without units: -1) and |c|^2 csq_out [n_slots].  level 0: the 64-unit groups
 * of the patch order (som_patch_order; beyond 128 features the only level), slot g = group g; level 1: their 16-unit sub-blocks,
 * slot 16 (g >> 2) + 4 (g & 3) + b = sub-block b of group g.  Launches nothing, refreshes nothing, changes no state: the buffers
 * describe the codebook of the last planned launch or fused merge -- a zero return says the buffers exist, NOT that they are
 * current: after som_set_weights and before the next planned launch they are the old codebook's.  *n_slots_out is written first; each of the three arrays may be
 * NULL.  Returns non-zero when the handle holds no centroids (no launch has planned yet) or has no such level.
 * tests/test_gpu_skip_bound.py compares them with a float64 computation from som_get_weights. */
int som_debug_exact_centroids(som_handle* h, int32_t level, float* C_out, float* r_out, float* csq_out, int32_t* n_slots_out);

/* measurement hook: ONE v_mfma_f32_16x16x32 (_f16 when is_f16, else _bf16) on the caller's operands -- a [16][32] and
 * b [32][16] as 16-bit patterns, c and d [16][16] float32, row-major.  tests/test_gpu_exact.py uses it to measure the
 * rounding error the exact mode's bound charges per MFMA (the hardware's internal summation is not documented). */
int som_debug_mfma16(som_handle* h, const uint16_t* a_host, const uint16_t* b_host, const float* c_host, float* d_host,
                     int32_t is_f16);

/* Three small kernels of the exact mode's epoch on caller-supplied HOST arrays, copied to device buffers of the call's own and
 * back (tests/test_gpu_radix_sort_hook.py, tests/test_gpu_select2_tiles_hook.py compare them with NumPy models).  Each call
 * checks on the host that its input cannot lead the kernel out of those buffers, and launches nothing when it could.
 *
 * The stable radix sort of (keys, row index) pairs by the low `bits` bits of the keys (radix_sort_rows, csrc/update.hpp: the
 * sort by unit takes it on large maps): keys [n] -> keys_out [n], vals_out [n] = the items' indices in sorted order.
 * 1 <= n < 2^31, 1 <= bits <= 31; key bits from `bits` rounded up to a multiple of 8 on must be zero for a sorted result. */
int som_debug_radix_sort(som_handle* h, const int32_t* keys, int64_t n, int32_t bits, int32_t* keys_out, int32_t* vals_out);

/* exact_select2_kernel (csrc/bmu_exact.hpp): plist [n_groups][stride] row ids and rmin [n_groups][stride], gcount [n_groups] the
 * lists' lengths, thr2 [n_rows].  Group g's list is compacted IN PLACE, in list order, to the entries i < gcount[g] with
 * rmin[g][i] <= thr2[plist[g][i]]; gcount[g] becomes their number and *kept_total the sum over the groups.  What lies behind
 * a list's survivors is not specified. */
int som_debug_exact_select2(som_handle* h, int32_t* plist, const uint32_t* rmin, int64_t stride, int32_t* gcount, const uint32_t* thr2,
                            int32_t n_groups, int64_t n_rows, int32_t* kept_total);

/* exact_tiles_kernel (csrc/bmu_exact.hpp) on a grid of `blocks` workgroups: the lists' entries from gstart (NULL: zeros) to gcount
 * cut into tiles of up to 128, group by group: tile_tab [table_entries][4] = {group, group * stride + first entry, entries, 0}.
 * tile_tab and out3 = {n_tiles, overflow, pairs} go to the device as the caller filled them and come back as the kernel left
 * them (it writes overflow only to raise it; with more than `capacity` pairs it writes no tile); gstart_out (NULL: none)
 * likewise, and takes the lists' lengths.  Refused where the tiles would not fit in table_entries. */
int som_debug_exact_tiles(som_handle* h, const int32_t* gcount, const int32_t* gstart, int32_t n_groups, int64_t stride, int64_t capacity,
                          int32_t blocks, int64_t table_entries, int32_t* tile_tab, int32_t* out3, int32_t* gstart_out);

/* bytes of device memory the engines of this process hold right now (every handle's buffers, scratch included): a closed
 * handle gives back all it took (tests/test_gpu_exact.py).  Returns non-zero for a NULL argument. */
int som_debug_device_bytes(int64_t* out);

/* precision EXACT, quantization_error: rows whose BMU the screen + re-score searched so far, and how many of them the
 * tie-window test sent on to the float32 SQRT kernel (som_quantization_error*, include/somhip.h). */
int som_debug_qe_stats(som_handle* h, int64_t* rows, int64_t* rows_sqrt);

/* precision EXACT, planned epochs over the resident rows: how many of them took the sorted rows' last-BMU positions from
 * the epoch before (stored by its exact_finalize_kernel) instead of gathering them with exact_lastpos_kernel. */
int som_debug_exact_chain_stats(som_handle* h, int64_t* carried_epochs);

/* precision EXACT, the candidate selection of the screen passes so far: passes whose listed screen selected in its own launch
 * (the select tail of csrc/bmu_bf16_k16.hpp), passes that launched exact_select_kernel behind their screen, and the tiles
 * of the former whose list was cut into parts and which the last part to arrive selected (tests/test_gpu_exact_select_fused.py). */
int som_debug_exact_select_stats(som_handle* h, int64_t* fused_passes, int64_t* launched_passes, int64_t* ticket_tiles);

/* precision EXACT up to 128 features, the plans of the screen passes so far (exact_skip_plan, csrc/exact_host.hpp): plans that
 * ran levels 1 and 2 and the lists in ONE launch (exact_plan_fused_kernel, csrc/exact_skip.hpp), and plans that ran them as
 * launches of their own -- every plan without level 2, with a scout, of a pass of few tiles, every plan whose level 2 the policy
 * timed, and all of them under SOM_EXACT_FUSE_PLAN=0 (tests/test_gpu_exact_plan_fused.py). */
int som_debug_exact_plan_stats(som_handle* h, int64_t* fused_launches, int64_t* split_launches);

/* precision EXACT up to 128 features, the plans of the screen passes so far by the form of their test: plans whose kernels took
 * the row threshold P into the extra MFMA step and tested a sign (the default), and plans that compared every accumulator with P
 * (SOM_EXACT_PLAN_FOLD=0) -- fused or split alike (tests/test_gpu_exact_plan_fold.py). */
int som_debug_exact_plan_fold_stats(som_handle* h, int64_t* folded, int64_t* compared);

/* The folded plan's split of a threshold (plan_fold_scale, plan_split_threshold, csrc/exact_skip.hpp) on caller-supplied numbers --
 * the host side of the __host__ __device__ functions the plan kernels call, NO device needed (tests/test_plan_fold_cpu.py).
 *   bf16: 0 = IEEE half operands, else bfloat16.  Per item i: the level's scale c from s_bmag[i] (= S'Bm'), then P[i] split:
 *   out4[4 i ..] = {c, p1, p2, p3}, c (p1 + p2 + p3) >= P[i].  Returns non-zero for a NULL argument or a negative count. */
int som_debug_plan_split(int32_t bf16, int64_t n, const float* P, const float* s_bmag, float* out4);

/* The transform's band arithmetic (band_entry_with, band_tile_range, band_union, csrc/update.hpp) on a caller-supplied table --
 * the host side of the __host__ __device__ functions the kernels call, NO device needed (tests/test_transform_bands_cpu.py).
 *   H [rows][nseg * segw] float32, row-major; wg_rows: 64 or 128, the rows of H a workgroup of the GEMM owns.
 *   tiles_out [ceil(rows / 32)][nseg][2] = {tlo, thi}: the columns, in segment coordinates, in which a wave issues the 32-row
 *     tile's MFMA steps (rounded outwards to the skipping granularity; {0, 0}: none).
 *   wg_out [ceil(rows / wg_rows)][3] = {lo, hi, chunks}: the workgroup stages columns [lo, lo + 32 chunks) of every segment, those
 *     from hi on as zeros.
 * Returns non-zero for a NULL or non-positive argument. */
int som_debug_band_walk(const float* H, int32_t rows, int32_t nseg, int32_t segw, int32_t wg_rows, int32_t* tiles_out,
                        int32_t* wg_out);

/* read-only: the neighbourhood tables of the last build and the band ranges recorded with them, as they stand on the device
 * (csrc/update.hpp, "ranges").  info4 = {the bands are on, nt = segments, range entries per buffer, the buffer the last build
 * filled}; entries_out [entries][2] = {segw - first nonzero column, last nonzero column + 1} per 32-row tile and segment -- stage 1
 * entry t * ceil(Y / 32) + tile, then stage 2 entry nt * ceil(Y / 32) + tile * nt + t; P1_out [nt][Y][Y], P2_out [X][nt * X].  Each
 * array may be NULL.  Without bands the entries are whatever the buffer holds (zeros).  tests/test_gpu_transform_bands.py compares
 * the entries with the tables' own nonzeros. */
int som_debug_band_tables(som_handle* h, int32_t* info4, int32_t* entries_out, float* P1_out, float* P2_out);

/* The same arithmetic for a TOROIDAL table, whose segments are cut at band_wrap_mid(segw) into a low piece [0, mid) and a high
 * piece [mid, segw) with a range each (csrc/update.hpp) -- NO device needed (tests/test_torus_bands_cpu.py).  Arguments as above;
 *   tiles_out [ceil(rows / 32)][nseg][2 pieces][2] = {tlo, thi} in segment coordinates per piece, low first;
 *   wg_out [ceil(rows / wg_rows)][2 pieces][3] = {lo, hi, chunks}: the workgroup stages [lo, lo + 32 chunks) of the low piece of
 *     every segment, then of the high piece, each piece's columns from its hi on as zeros (the low lo is a multiple of 32, the
 *     high lo of 8 and never below the cut). */
int som_debug_band_walk_wrap(const float* H, int32_t rows, int32_t nseg, int32_t segw, int32_t wg_rows, int32_t* tiles_out,
                             int32_t* wg_out);

/* som_debug_band_tables for a TOROIDAL handle (which that call refuses, as this one refuses the others): info4 as there, with
 * range entries counted per piece; entries_out [entries][2] with entry 2 e + piece where a rectangular handle has entry e -- the
 * same {segw - first nonzero column, last nonzero column + 1} pair in segment coordinates, over the nonzeros of the piece alone
 * (low: columns below band_wrap_mid(side) = ((side / 2 + 4) / 8) * 8; high: the rest).  tests/test_gpu_torus.py. */
int som_debug_band_tables_wrap(som_handle* h, int32_t* info4, int32_t* entries_out, float* P1_out, float* P2_out);

/* precision EXACT: the plan of the last BMU launch as it ran (policy::LaunchPlan, csrc/exact_policy.hpp):
 *   out8 = [0] skip  [1] resort  [2] scout  [3] level 2  [4] estimate  [5] sample_tiles  [6] refine  [7] time_phases */
int som_debug_exact_last_plan(som_handle* h, int32_t* out8);

/* precision EXACT, read-only: what the last BMU launch learned from its samples before it committed to a plan (the default
 * switches' forecast: launch_bmu_exact, exact_sample_tiles, csrc/exact_host.hpp) -- plain numbers the host stored where it
 * computed them; nothing is launched.
 *   out12 = [0] need: the share of the groups a sampled row needs (-1: the row sample was not asked)  [1] rows sampled
 *           [2] est, [3] est1: the share of their blocks the sample tiles would run after both levels / after level 1
 *           [4] n_st: sample tiles  [5] st: their stride in tiles of the pass   ([2..5]: -1 where the tiles were not asked)
 *           [6] blocks_run, [7] groups_run: the sample's raw counters (-1: not asked)
 *           [8] scout_declined: launches of this handle so far whose estimate declined the plan (policy::PlanState::stats())
 *           [9] the sample was planned with level 2 (-1: not asked)
 *           [10] full_total, [11] full_screen: the policy's costs of the last launch WITHOUT a plan as they stand now (ms per row;
 *           0: none on record) -- to be printed, never asserted on
 * tests/test_gpu_default_plan.py compares them with a float64 model (tests/scout_ref.py). */
int som_debug_exact_forecast(som_handle* h, double* out12);

/* precision EXACT up to 128 features, read-only: the tiles' lists of the LAST PASS of the last BMU launch as its screen walked
 * them -- blocks_out[t] the 16-unit blocks on tile t's list (tcnt), groups_out[t] the groups level 1 kept (the two numbers
 * exact_list_totals_body sums into the pass's blocks_run and groups_run).  info2 = {tiles of that pass (0: it ran without a plan),
 * its plan ran level 2}; written first, and alone when n_tiles == 0 or both arrays are NULL.  Returns non-zero where n_tiles
 * exceeds the pass's tiles. */
int som_debug_exact_tile_blocks(som_handle* h, int32_t* blocks_out, int32_t* groups_out, int64_t n_tiles, int32_t* info2);

/* diagnostic builds only (-DSOM_STAMPS, tools/stamps.py builds one on demand): out_host == NULL attaches a buffer of n_pairs
 * (shader-clock ticks, 100 MHz ticks) pairs, one per workgroup of the next BMU launches (n_pairs == 0 detaches);
 * out_host != NULL reads n_pairs pairs back.  The product build refuses both. */
int som_debug_stamps(som_handle* h, int64_t n_pairs, uint64_t* out_host);

/* The exact mode's POLICY (csrc/exact_policy.hpp: commit a scouted plan, level 2, did a sort pay, is a plan idle, does the
 * scout go on, is a row set worth a scout) on caller-supplied numbers -- pure host arithmetic, NO device needed: the seam the
 * CPU suite tests the decisions through (tests/test_policy_cpu.py).
 *   costs[9] = {full_total, full_screen, plan_total, plan_over, plan_over_scout, blk_ms, l2_ms_group, l2_ratio, sort_ms}
 *              (ms per row; blk_ms per 16-unit block; l2_ms_group per kept (tile, group) pair; 0 = not measured yet)
 *   which: 0 commit_scouted_plan(share, blocks_per_row)   1 level2_from_sample(share, share1, blocks_per_row)
 *          2 level2_pays(share, share1)                   3 sort_paid(share_stale, share_fresh, blocks_per_row, epochs_served)
 *          4 plan_idle(share)                             5 scout_continues(win_share, share_last, blocks_per_row)
 *          6 rows_worth_a_scout(rows, units, features)
 *   *out = 0 / 1; returns non-zero for an unknown `which` or a NULL argument. */
int som_policy_eval(int32_t which, const double* costs, const double* args, int32_t* out);

/* The policy's STATE MACHINE (csrc/exact_policy.hpp, policy::PlanState) on a caller-supplied script of launches -- pure host
 * arithmetic, NO device needed.  A fresh PlanState is driven as launch_bmu_exact drives it: begin; the row sample and the
 * sample tiles where the plan asks for them; end (tests/test_policy_cpu.py).
 *   script[n_launches][SOM_POLICY_REPLAY_IN], per launch:
 *     the facts    [0] resident  [1] last BMUs valid  [2] row set (an id)  [3] rows  [4] can_skip  [5] scout_ok  [6] wide
 *                  [7] wide_can  [8] wide_scout_ok  [9] level 2's list fits in LDS  [10] the lo image exists  [11] blocks_per_row
 *                  [12] skip_mode  [13] refine_on  [14] sub_blocks  [15] res_every
 *     the samples  [16] the row sample's f   [17] the sample tiles' share after both levels (< 0: the pass is too short for
 *                  sample tiles)   [18] ... after level 1
 *     the outcome  [19..22] ms: launch, screen, level 2, sort + gather (each phase counts as timed where the plan times it)
 *                  [23] blocks run  [24] blocks in all  [25] (tile, group) pairs level 1 kept  [26] pairs selected
 *                  [27] pairs the refinement kept  [28] rows the scout won   (without a plan every block runs, whatever [23] says)
 *   out[n_launches][SOM_POLICY_REPLAY_OUT], per launch:
 *     the plan as it ran  [0] skip  [1] resort  [2] scout  [3] level 2  [4] estimate  [5] sample_tiles  [6] refine  [7] time_phases
 *     [8] the row sample was asked  [9] the sample tiles were asked  [10] the row sample declined  [11] the sample tiles declined
 *     the pauses after the launch  [12..14] resident: cooldown, idle, pause  [15..17] transient
 *   returns non-zero for a NULL argument or a negative count. */
#define SOM_POLICY_REPLAY_IN 29
#define SOM_POLICY_REPLAY_OUT 18
int som_policy_replay(int32_t n_launches, const double* script, double* out);

/* The codebook operands' STATE (csrc/codebook_operands.hpp, operands::State: which of |w|^2, the patch-order copy, the float32
 * image and its order, the 16-bit image with its norms, the plan's centroids are current) on a caller-supplied script of events
 * -- pure host code, NO device needed.  A fresh State (everything stale) is moved as the host code moves the handle's
 * (tests/test_operands_cpu.py).
 *   config[6] = {half, exact, patch order, cosine, resident (exact, <= 128 features), a float32 stage image exists}
 *   script[n_events][SOM_OPERANDS_REPLAY_IN] = {event, request, flag}
 *     event   0 codebook replaced   1 plain merge   2 half-fused merge   3 exact fused merge (flag: it wrote the centroids)
 *             4 a request (flag: the caller may defer the 16-bit image to its launch), decided and committed
 *             5 the pending 16-bit image is taken (by the planned launch, or flushed)
 *             6 a captured graph replayed (its request)   7 the canary's |w|^2
 *     request 0 the configured search   1 a float32 kernel in the units' own order   2 the exact screen's patch-order operands
 *   out[n_events][SOM_OPERANDS_REPLAY_OUT], per event:
 *     the rebuilds the decision listed (events 4 and 7; else 0)
 *             [0] |w|^2  [1] permute  [2] float32 image  [3] ... in patch order  [4] 16-bit image  [5] ... its norms step skipped
 *             [6] ... its image kernel deferred  [7] ... which also sets the centroid levels' maxima (cm)
 *     [8] a pending image was flushed (event 4) or taken (event 5)  [9] ... with cm
 *     the accessors afterwards  [10] the float32 image is in patch order  [11] an image is pending  [12] the centroids are fresh
 *             [13] the patch-order copy is in step with the codebook
 *   returns non-zero for a NULL argument, a negative count, an inconsistent config, an unknown event or request, or an event the
 *   config has no path for (2 without a plain half mode, 3 and a deferring request without the resident exact path, 6 in exact mode). */
#define SOM_OPERANDS_REPLAY_IN 3
#define SOM_OPERANDS_REPLAY_OUT 14
int som_operands_replay(const int32_t* config, int32_t n_events, const int32_t* script, int32_t* out);

/* The ROW SETS' size rule (csrc/row_set.hpp, rowset::sizes: what the resident rows, the query scratch and a pinned-chunk slot
 * allocate for n rows) on caller-supplied numbers -- pure host arithmetic, NO device needed (tests/test_row_sets_cpu.py).
 *   kind: 0 resident  1 query scratch  2 pinned-chunk slot;  dp: the feature stride of the 16-bit row image
 *   flags: bit 0 precision is f32 (no 16-bit image)  bit 1 exact (|x|^2 holds the rows' errors in a second half)
 *          bit 2 the configured search reads |x|^2  bit 3 cosine on the tiled 16-bit path (|x|^2 as scratch)
 *   out5 = {cap, X, xsq, Xb, ids}: the rows the derived buffers hold, then elements per buffer (0: the set holds no such buffer;
 *          a buffer that exists holds at least one element).  Returns non-zero for a NULL or out-of-range argument. */
int som_debug_row_set_sizes(int32_t kind, int64_t n, int32_t input_len, int32_t dp, int32_t flags, int64_t* out5);

/* The SORT BY UNIT's rule (csrc/unit_sort.hpp, unitsort::sizes and unitsort::counting: what a sort scratch of capacity rows_cap
 * allocates on a map of K units, and which sort n rows then take) on caller-supplied numbers -- pure host arithmetic, NO device
 * needed (tests/test_unit_sort_cpu.py).  counting_on: the handle's SOM_COUNTING_SORT switch.
 *   out6 = {skey, srow, radix scratch, counting table (elements; 0: no table), cs_blocks, 1 if n rows take the counting sort else 0}.
 *   Returns non-zero for a NULL out6, negative rows or K < 1. */
int som_debug_unit_sort_sizes(int64_t rows_cap, int32_t K, int32_t counting_on, int64_t n, int64_t* out6);
/* The sorts by unit the handle ran since som_create, by kind (segment sums of resident rows and streamed chunks, the per-unit
 * queries): the path the rule above PREDICTS, observed.  Counted where the host launches a sort: a replayed graph's are not. */
int som_debug_unit_sort_stats(som_handle* h, int64_t* counting, int64_t* radix);

/* The EXACT MODE'S SCRATCH rule (csrc/exact_scratch.hpp) on caller-supplied numbers -- pure host arithmetic, NO device and no
 * handle needed (tests/test_exact_scratch_cpu.py).
 *   geometry8 = {K, input_len, dp, stage_bytes, wide (0 | 1), item_slots, SOM_EXACT_PASS_ROWS (0: none), SOM_EXACT_PAIRS (0: none)}
 *   out[0 .. 16): the stride ladder for `rows` rows -- first_stride without a cap, then next_stride of each -- zero from its end on
 *   out[16 .. 75): one BLOCK at the ladder's first stride;  out[75 .. 134): one BLOCK at first_stride(rows, stride_cap).
 * A BLOCK is 59 values, counts in elements of each buffer's own type:
 *   [0]  pass:   stride, pairs, max_tiles, too_large, gmin, gflags, rowcnt, rowarg, seed, plist, fb_list, tile_tab, ctr
 *   [13] centroid levels of the geometry (1 beyond 128 features, else 2)
 *   [14] level 0, [23] level 1 (zeros where there is none): n_slots, n_cstages, n_img_stages, Cc, rg, csq, cmax2, Cst, Cst_plain
 *   [32] a sorted pass of `rows` rows: cap, order, Xb_s, Xl_s, Xf_s, xsq_s, xerr_s, seed_s, sU_s, lastpos_s
 *   [42] plan:   stride, tiles, sk_keys, sk_keys2, sk_vals, sk_tmp, scout_g, tq, need, need2, glist, gcnt, tlist, tcnt, tile_counts,
 *                tile_ticket, items
 * Returns non-zero for a NULL argument, rows < 1, a negative stride_cap, K < 1 or input_len < 1. */
int som_debug_exact_scratch_sizes(const int64_t* geometry8, int64_t rows, int64_t stride_cap, int64_t* out);
/* ... and what the handle's four owners HOLD now, read-only (nothing is launched or allocated): out[0 .. 59) one BLOCK in the order
 * above -- capacities in elements, 0 for a buffer that is not held; levels 0 while no centroid set is held; the sorted pass is the
 * resident rows' --, out[59 .. 69) the transient rows' sorted pass, out[69 .. 77) the geometry8 the handle sizes by,
 * out[77 .. 79) the float32 fallback's dense rows and ids (fbX, fb_ids). */
int som_debug_exact_scratch_held(som_handle* h, int64_t* out);

/* The ROW MOMENTS' launch geometry (csrc/moments.hpp) for n_rows rows of input_len features -- pure host arithmetic, NO device
 * needed (tests/moments_ref.py mirrors the chunk length into its bound; tests/test_gpu_moments.py takes its boundary shapes from it).
 *   out6 = {SOM_MOMENTS_CHUNK_ROWS: rows per float32 chain of the Gram kernel, 32 x 32 tiles with a-block <= b-block, row splits,
 *           chunks in one round of the row split, workgroups of the sums kernel, SOM_MOMENTS_MAX_FEATURES}
 *   Returns non-zero for a NULL out6, negative rows or input_len < 1. */
#define SOM_MOMENTS_CHUNK_ROWS 256
int som_debug_moments_plan(int64_t n_rows, int32_t input_len, int64_t* out6);

/* The DENSITY scan's launch geometry (csrc/density.hpp, density_plan) for n_rows rows on a map of K units -- pure host arithmetic, NO
 * device needed.  slots: workgroups of the scan the chip holds at once; forced_slabs > 0: the slab count SOM_DENSITY_SLABS asks
 * for (read only under SOM_TEST_HOOKS=1), 0: none.  A workgroup owns one tile of 128 units and a slab of consecutive 128-row tiles:
 *   unit tiles = ceil(K / 128), row tiles = ceil(n_rows / 128),
 *   slabs asked for = clamp(forced_slabs or ceil(slots / unit tiles), 1, row tiles), row tiles per slab = ceil(row tiles / slabs
 *   asked for), slabs = ceil(row tiles / row tiles per slab) -- the slabs that hold a row tile; the grid is unit tiles * slabs.
 *   out4 = {unit tiles, row tiles, slabs, row tiles per slab}
 *   Returns non-zero for a NULL out4, n_rows < 1 or > 2^31-1, K < 1, slots < 1 or forced_slabs < 0. */
int som_debug_density_plan(int64_t n_rows, int32_t K, int64_t slots, int32_t forced_slabs, int64_t* out4);

/* The TOP-K scan's launch geometry (csrc/topk.hpp, topk_plan) for a pass of n_rows rows on a map of K units -- pure host arithmetic,
 * NO device needed.  slots: workgroups of the scan the chip holds at once; forced_parts > 0: the part count SOM_TOPK_PARTS asks for
 * (read only under SOM_TEST_HOOKS=1), 0: none.  A workgroup owns one tile of 128 rows and one part of the codebook's 128-unit stages:
 *   row tiles = ceil(n_rows / 128), stages = ceil(K / 128),
 *   parts asked for = clamp(forced_parts or ceil(slots / row tiles), 1, stages), stages per part = ceil(stages / parts asked for),
 *   parts = ceil(stages / stages per part) -- the parts that hold a stage; the grid is row tiles x parts.
 *   out4 = {row tiles, stages, parts, stages per part}
 *   Returns non-zero for a NULL out4, n_rows < 1 or > 2^31-1, K < 1, slots < 1 or forced_parts < 0. */
int som_debug_topk_plan(int64_t n_rows, int32_t K, int64_t slots, int32_t forced_parts, int64_t* out4);

#ifdef __cplusplus
}
#endif
#endif
