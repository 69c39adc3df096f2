// THE EXACT MODE'S SCRATCH: the pass scratch (group minima, row masks, the groups' row lists, the re-score tiles), the plan's
// per-tile words, lists and work queue, the two centroid levels and the sorted passes.  This header owns HOW LARGE those buffers
// are and how a pass shrinks when the device refuses one: one rule, pure host arithmetic (no HIP, no handle), in the manner of
// row_set.hpp and unit_sort.hpp.  somhip.hip's PassScratch, PlanScratch, CentroidSet and SortedRows allocate what the rule says
// (exact_host.hpp: their reserve); som_debug_exact_scratch_sizes exposes it to the CPU suite (tests/test_exact_scratch_cpu.py),
// som_debug_exact_scratch_held what a handle holds.  Counts are ELEMENTS of each buffer's own type; an allocation of none is one
// of one element (DevBuf::alloc), which the rule says too.
#pragma once

#include <algorithm>
#include <cstddef>
#include "unit_sort.hpp"

namespace somhip {

// the tiling constants the sizes depend on, beside the rule (the kernels' headers include this one)
constexpr int K16_T = 4;              // resident screen (bmu_bf16_k16.hpp): 16-unit tiles per stage
constexpr int K16_STAGE_UNITS = 16 * K16_T;
constexpr int WD_T = 2;               // wide screen (bmu_bf16_wide.hpp): 16-unit tiles per stage
constexpr int WD_STAGE_UNITS = 16 * WD_T;
constexpr int EX_GROUP = 64;          // units per group = one stage of the float32 stage image = one stage of the screen
constexpr int EX_PAIRS = 64;          // least capacity of a pass in (row, group) pairs per row ON AVERAGE
constexpr int EX_TR = 128;            // rows per re-score tile (4 waves x 32 rows against one 64-unit group)
constexpr int SK_TILE = 256;          // rows per plan / screen workgroup tile (exact_skip.hpp: the resident screen's workgroup)
constexpr int EX_PASS_COUNTERS = 11;  // ints of PassCounters (bmu_exact.hpp), the tail of the pass's counter block
constexpr size_t EX_CTR_TAIL_INTS = EX_PASS_COUNTERS + 16;   // ... and the 64 bytes a whole-line fill of the block may run over

namespace exscratch {

// everything the sizes depend on.  item_slots: the resident workgroup slots of a chip at eight workgroups a CU (the listed
// screen's work queue is cut for at most that many); pass_rows_override, pairs_hook: SOM_EXACT_PASS_ROWS, SOM_EXACT_PAIRS (0: none)
struct Geometry { long K; int D, dp, stage_bytes; bool wide; int item_slots; long pass_rows_override, pairs_hook; };

inline long cdiv(long a, long b) { return (a + b - 1) / b; }
inline long round_up(long a, long b) { return cdiv(a, b) * b; }
inline size_t some(long a) { return (size_t)(a > 0 ? a : 1); }
inline long groups(const Geometry& g) { return cdiv(g.K, EX_GROUP); }

// rows of one screen pass: the group-minimum matrix of a pass (and, as large again, the groups' row lists) stays within
// 4 GiB -- address space rather than traffic: both are written and read only where a row is near its minimum.  1 Mi rows
// of a 256 x 256 map, or a 250 000-row shard of a 512 x 512 one, are ONE pass (measured against passes of a quarter of
// that: -2.3 % / -3.5 % per epoch: fewer, larger launches and one counter read-back instead of four).
inline long pass_rows(const Geometry& g) {
    long rows = (4L << 30) / (4 * groups(g));
    if (g.pass_rows_override > 0) rows = g.pass_rows_override;   // SOM_EXACT_PASS_ROWS: tests walk several passes on small data
    rows = rows / 1024 * 1024;                                   // (a multiple of every screen kernel's workgroup tile)
    return rows < 1024 ? 1024 : rows;
}

// THE STRIDE LADDER.  The first attempt for `rows` rows: as large a pass as the 4 GiB rule allows (stride_cap > 0: and no larger
// than what the device had memory for before).  Where the device refuses it (other handles, other processes on the card): passes
// of half the rows, and half again, down to 1 024 -- smaller passes cost a few percent, a refused allocation costs the run.
// next_stride == 0: nothing smaller to try.
inline long first_stride(const Geometry& g, long rows, long stride_cap) {
    const long stride = round_up(std::min(rows, pass_rows(g)), 256);
    return stride_cap > 0 ? std::min(stride, stride_cap) : stride;
}
inline long next_stride(long stride) { return stride <= 1024 ? 0 : std::max(1024L, round_up(stride / 2, 256)); }

// THE PASS SCRATCH for passes of `stride` rows.  pairs: capacity of a pass in (row, group) pairs per row on average: a quarter of
// the groups -- past that the float32 kernel over all of them costs about what the re-score would
struct PassSizes {
    long stride = 0, pairs = 0, max_tiles = 0;
    bool too_large = false;           // stride * pairs > 2^31 - 1: the lists' entries are ints
    size_t gmin = 0, gflags = 0, rowcnt = 0, rowarg = 0, seed = 0, plist = 0, fb_list = 0, tile_tab = 0, ctr = 0;
};
inline PassSizes pass(const Geometry& g, long stride) {
    const long n_groups = groups(g);
    PassSizes z;
    z.stride = stride;
    z.pairs = std::max<long>(EX_PAIRS, std::min<long>(n_groups / 4, 512));
    if (g.pairs_hook > 0) z.pairs = g.pairs_hook;
    z.too_large = stride * z.pairs > 0x7fffffffL;
    z.gmin = some(n_groups * stride);
    z.gflags = some(n_groups * (stride / 64));
    z.rowcnt = z.rowarg = z.seed = z.fb_list = some(stride);
    z.plist = some(n_groups * stride);                           // every group: room for the whole pass
    z.max_tiles = cdiv(stride * z.pairs, EX_TR) + n_groups;
    z.tile_tab = some(z.max_tiles);
    z.ctr = (size_t)3 * n_groups + EX_CTR_TAIL_INTS;             // [n_groups gcount][n_groups gstart of round 2][PassCounters]
    return z;
}

// THE PLAN'S CENTROIDS.  level 0: the 64-unit groups; level 1: their 16-unit sub-blocks, sixteen slots per four groups and
// 4 * ncs stages (need2 is addressed [tile][4 * ncs]: exact_lists_kernel).  The centroid image's own stages hold 64 centroids each
// up to 128 features, 32 on the wide kernel's tiling -- where n_cstages stays the number of 64-group WORDS of the need bitmaps
inline int levels(const Geometry& g) { return g.wide ? 1 : 2; }
struct CentroidSizes {
    int n_slots = 0, n_cstages = 0, n_img_stages = 0;
    size_t Cc = 0, rg = 0, csq = 0, cmax2 = 0, Cst = 0, Cst_plain = 0;   // (Cst_plain, the scout's copy: level 0 only)
};
inline CentroidSizes centroids(const Geometry& g, int level) {
    CentroidSizes z;
    if (level < 0 || level >= levels(g)) return z;
    const long n_groups = groups(g);
    const int ncs = (int)cdiv(n_groups, K16_STAGE_UNITS);
    z.n_slots = level == 0 ? (int)n_groups : (int)cdiv(n_groups, 4) * 16;
    z.n_cstages = level == 0 ? ncs : 4 * ncs;
    z.n_img_stages = g.wide ? (int)cdiv(n_groups, WD_STAGE_UNITS) : z.n_cstages;
    z.Cc = some((long)z.n_slots * g.D);
    z.rg = z.csq = some(z.n_slots);
    z.cmax2 = 2;
    z.Cst = some((long)z.n_img_stages * g.stage_bytes);
    if (level == 0) z.Cst_plain = z.Cst;
    return z;
}

// A SORTED PASS of `rows` positions (each pass padded to the tile).  Xl_s, the rows' second half image, is allocated by the first
// launch that refines (SortedRows::reserve_second_half), from the same cap
struct SortedSizes { long cap = 0; size_t order = 0, Xb_s = 0, Xl_s = 0, Xf_s = 0, xsq_s = 0, xerr_s = 0, seed_s = 0, sU_s = 0, lastpos_s = 0; };
inline SortedSizes sorted(const Geometry& g, long rows) {
    SortedSizes z;
    z.cap = round_up(rows, SK_TILE);
    z.order = z.xsq_s = z.xerr_s = z.seed_s = z.sU_s = z.lastpos_s = some(z.cap);
    z.Xb_s = z.Xl_s = some(z.cap * g.dp);
    z.Xf_s = some(z.cap * g.D);
    return z;
}

// THE PLAN'S per-pass buffers for passes of `stride` rows: the sort's keys, the scout's groups, the tiles' need words, lists and
// counts, and the listed screen's work queue -- its items (exact_list_totals_body, exact_skip.hpp) are within 5 tiles + 4 slots
// of them; + the queue's two words and their padding
struct PlanSizes {
    long stride = 0, tiles = 0;
    int item_slots = 0;               // (the geometry's: what the queue is sized for)
    size_t sk_keys = 0, sk_keys2 = 0, sk_vals = 0, sk_tmp = 0, scout_g = 0, tq = 0;   // (tq: the wide plan only)
    size_t need = 0, need2 = 0, glist = 0, gcnt = 0, tlist = 0, tcnt = 0, tile_counts = 0, tile_ticket = 0, items = 0;
};
inline PlanSizes plan(const Geometry& g, long stride) {
    const long n_groups = groups(g);
    PlanSizes z;
    z.stride = stride;
    z.tiles = stride / SK_TILE;
    z.item_slots = g.item_slots;
    z.sk_keys = z.sk_keys2 = z.sk_vals = z.scout_g = some(stride);
    if (g.wide) z.tq = some(stride);
    z.need = some(z.tiles * centroids(g, 0).n_cstages);
    z.need2 = some(z.tiles * centroids(g, 1).n_cstages);         // (beyond 128 features: no level 2, one element)
    z.glist = some(z.tiles * n_groups);
    z.gcnt = z.tile_counts = z.tcnt = z.tile_ticket = some(z.tiles);
    z.tlist = some(z.tiles * n_groups * K16_T);
    z.items = (size_t)(5 * z.tiles + 4 * g.item_slots + 16);
    z.sk_tmp = unitsort::radix_scratch_ints(stride);
    return z;
}

}  // namespace exscratch
}  // namespace somhip
