// libsomhip.so -- C ABI over the gfx950 kernels (include/somhip.h).
// Host side only orchestrates: buffers, launch geometry checks, the per-epoch kernel
// sequence on one HIP stream, hipEvent timing.  No compute happens on the host and
// there is no CPU fallback: every path either launches the HIP kernels or fails.
#include <hip/hip_runtime.h>

#include <cstring>

#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/somhip.h"
#include "../../include/somhip_test.h"
#include "bmu_bf16_k16.hpp"
#include "bmu_bf16_tiled.hpp"
#include "bmu_bf16_wide.hpp"
#include "bmu_exact.hpp"
#include "exact_skip.hpp"
#include "exact_policy.hpp"
#include "codebook_operands.hpp"
#include "row_set.hpp"
#include "exact_skip_wide.hpp"
#include "bmu_f32.hpp"
#include "bmu_f32_res.hpp"
#include "bmu_f32_tiled.hpp"
#include "bmu_masked_f32.hpp"
#include "bmu_pairwise.hpp"
#include "update.hpp"
#include "diag.hpp"
#include "monitor.hpp"
#include "project.hpp"
#include "impute.hpp"
#include "moments.hpp"
#include "density.hpp"
#include "topk.hpp"

using namespace somhip;

namespace {

thread_local std::string g_create_error;

// Environment switches.  Five are for users (SOM_VERIFY, SOM_DEBUG, SOM_EXACT_SKIP, SOM_EXACT_TOP2, SOM_GRAPH).  Everything
// else -- A/B switches of kernel variants, forced pass sizes, refused allocations -- belongs to the tests and the tools and is
// read ONLY when SOM_TEST_HOOKS=1 is set (tests/conftest.py sets it): a stray variable in a user's environment changes nothing.
const char* dev_env(const char* name) {
    static const bool on = [] { const char* v = std::getenv("SOM_TEST_HOOKS"); return v != nullptr && std::atoi(v) != 0; }();
    return on ? std::getenv(name) : nullptr;
}

struct EventPair { hipEvent_t a, b; int kernel; };

}  // namespace

// RCCL, bound at run time (dlopen): the library has no link-time dependency on it, and in a process that also
// runs torch the SAME copy torch loaded is used.  Only what the one exchange step of the path needs.
struct som_nccl_id { char internal[128]; };
struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(som_nccl_id*) = nullptr;
    int (*CommInitRank)(void**, int, som_nccl_id, int) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
static RcclApi g_rccl;
static std::string g_rccl_error;

// Device memory the engine owns: one allocation of `cap` elements, freed by its owner's destructor (move-only; alloc and
// reserve free what is held BEFORE they allocate, so a grown buffer never holds twice its memory).  The bytes held by every live
// DevBuf of the process are counted (som_debug_device_bytes: the suite checks that a handle gives back what it took).
static std::atomic<int64_t> g_dev_bytes{0};
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;          // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() {
        if (p) { (void)hipFree(p); g_dev_bytes -= (int64_t)(cap * sizeof(T)); }
        p = nullptr; cap = 0;
    }
    int alloc(som_handle* h, size_t n);   // (defined with the handle: capture refusal, graph staleness, error message)
    int reserve(som_handle* h, size_t n, size_t round = 1) { return n <= cap ? 0 : alloc(h, (n + round - 1) / round * round); }
    operator T*() const { return p; }
};

// what a search, a segment sum or the canary reads of a row set, by value: nobody downstream asks the handle which set it was
struct Rows {
    const float* X; long N; const float* xsq; const float* xerr; const __bf16* Xb; const float* xmax2; int* out; int* out2;
    const float* wgt; bool resident; bool ids_valid;
};

// The sort by unit (unit_sort.hpp) and its buffers: the one owner.  The handle holds three -- the resident rows' and the streamed
// chunks' (SegScratch), the query scratch's (RowSet::Diag).  reserve and sort_rows_by_unit take it whole; neither
// synchronises: a caller whose earlier launches may still read the buffers does that before it lets them grow.
struct UnitSort {
    DevBuf<int> skey, srow;      // [cap] the sorted (unit, row) pairs
    DevBuf<int> tmp;             // radix_sort_rows' scratch
    DevBuf<int> cs_table;        // counting sort (small maps): [K][blocks of 1 024 rows] counts, then [K] totals
    long cs_blocks = 0;          // ... the blocks the table was sized for (0: no table)
    long cap = 0;                // rows the buffers serve
};

// One row set (row_set.hpp) and everything derived from its rows: the one owner of these buffers.  The handle holds three --
// `res` the resident training rows, `q` the query scratch (also the pageable streamed chunks), Slot::rows the pinned chunks.
struct RowSet {
    rowset::Kind kind = rowset::Kind::Query;
    const float* X = nullptr;    // the float32 rows: X_owned, or the caller's device rows (som_set_data_device, the *_device queries)
    DevBuf<float> X_owned;
    long N = 0, cap = 0;         // rows in it now; rows its derived buffers hold
    DevBuf<float> xsq;           // |x|^2 in NumPy's order; exact mode: twice cap, see xerr()
    DevBuf<__bf16> Xb;           // the 16-bit operand image
    DevBuf<int> bmu, bmu2;       // the ids a search writes (bmu2: the query set's second-best units)
    // per-row sample weights: float32, finite, >= 0; nullptr = every row counts 1 (update.hpp, runsum_kernel<.., WEIGHTED>: level 0 only)
    const float* wgt = nullptr;  // wgt_owned, or the caller's device array (som_set_sample_weights_device)
    DevBuf<float> wgt_owned;
    float* xmax2 = nullptr;      // max_n |x~_n|^2: this set's float of som_handle::xmax2 ([0] resident, [1] every transient set)
    bool err_half = false;       // precision 'exact'
    bool ids_valid = false;      // bmu holds the ids of a completed BMU pass over THESE rows (resident set only: a transient set's never outlive the call)
    // map diagnostics (diag.hpp; the query set only): the rows' distances to their BMUs, the rows sorted by BMU, the segment starts
    // and the per-unit results.  Grown with the set's `cap` (diag_reserve), so nothing is allocated once a size has been seen.
    struct Diag {
        DevBuf<float> dist;                      // [cap] d_n
        UnitSort sort;                           // the rows sorted by unit (grown with `cap` by the first per-unit query: diag_reserve_stats)
        DevBuf<int> start;                       // [K] first sorted position of every unit that has rows, else -1
        DevBuf<long long> count;                 // [K]
        DevBuf<double> sums;                     // [2 K] sum | sum of squares
        DevBuf<float> max;                       // [K]
        // label and value maps (project.hpp): the host entry points' labels and values beside the rows, the [K][C] results
        DevBuf<int> labels;                      // [cap]
        DevBuf<float> values;                    // [cap][C]
        DevBuf<long long> pcount;                // [K][C]
        DevBuf<double> psums;                    // [2][K][C] sum | sum of squares
    } diag;
    bool resident() const { return kind == rowset::Kind::Resident; }
    // precision 'exact': the rows' measured operand rounding errors (bmu_exact.hpp) live in the second half of xsq.  The only place that knows.
    float* xerr() const { return err_half && xsq.p != nullptr ? xsq.p + cap : nullptr; }
    Rows view() const { return Rows{X, N, xsq, xerr(), Xb, xmax2, bmu, bmu2, wgt, resident(), ids_valid}; }
};

// THE EXACT MODE'S SCRATCH (exact_scratch.hpp: how large; exact_host.hpp: reserve, one overload each): four owners.  Each holds its buffers
// and the numbers that say what they were sized for; reserve allocates what the rule's sizes struct says, in a fixed order, and a
// refusal part of the way releases the WHOLE group before the error goes back: nothing half allocated is ever held or used.
// (a pass's screen, select, refinement and re-score; the float32 fallback's dense rows, grown on demand)
struct PassScratch {
    DevBuf<uint32_t> gmin;               // [n_groups][stride] group minima of the chunk being screened (sparse: see gflags)
    DevBuf<unsigned long long> gflags;   // [stride / 64][n_groups] which rows' minima the screen stored
    DevBuf<int> rowcnt;                  // [stride] candidate groups of every row of the last pass (som_exact_last_counts)
    DevBuf<int> rowarg;                  // [stride] the group round 1 scored for the row (-1: none)
    DevBuf<float> seed;                  // [stride] exact_seed_kernel: the cap on the screen's keep threshold
    DevBuf<int> plist;                   // [n_groups][stride] rows bucketed by candidate group
    DevBuf<int> fb_list;                 // [stride] the rows the pass hands to the float32 kernel
    DevBuf<int4> tile_tab;               // [max_tiles] re-score tiles: (group, first list entry, rows)
    DevBuf<int> ctr;                     // [n_groups gcount][n_groups gstart of round 2][PassCounters] (bmu_exact.hpp; zeroed per pass; PassCtr names the parts)
    DevBuf<float> fbX; DevBuf<int> fb_ids;   // fallback rows, dense, for the float32 kernel, and its ids (exact_fallback_rows grows them)
    long stride = 0, pairs = 64, max_tiles = 0;   // rows per group line (0: nothing held); (row, group) pairs per row on average; [tile_tab]
    void release() { *this = PassScratch{}; }
};
// (a pass's plan: the sort's keys, the scout's groups, the tiles' need words, lists and counts, the listed screen's work queue)
struct PlanScratch {
    DevBuf<int> sk_keys, sk_keys2, sk_vals, sk_tmp;   // [stride] the sort's keys and values; radix_sort_rows' scratch
    DevBuf<int> scout_g;              // [stride] nearest group centroid of every row of the pass
    DevBuf<float> tq;                 // [stride] wide plan: the float32 score of every sorted row's last BMU under the current codebook
    DevBuf<unsigned long long> need, need2;
    DevBuf<int> glist, gcnt;          // per tile: (group << 4 | sub-block mask) items: what the select kernel walks
    DevBuf<int2> tile_counts;
    DevBuf<int> tlist, tcnt;          // per tile: the same blocks as a dense list of 16-unit tiles: what the screen walks
    DevBuf<int> tile_ticket;          // per tile: arrivals of its parts in the listed screen's select tail (zeroed by the lists kernels)
    DevBuf<int2> items;               // the listed screen's work queue: [0] = (items, counter), from [8] on (tile, part | parts << 16)
    long stride = 0; int item_slots = 0;   // rows per pass the buffers hold; resident workgroups the queue was sized for
    void release() { *this = PlanScratch{}; }
};
// (the centroid sets of the plan: [0] the 64-unit groups, [1] their 16-unit sub-blocks -- exact_centroid_kernel's slot order)
struct CentroidSet {
    struct Level { DevBuf<float> Cc, rg, csq, cmax2; DevBuf<char> Cst;
                   DevBuf<char> Cst_plain;      // level 0 only: the scout's copy (plain initial accumulators)
                   int n_slots = 0, n_cstages = 0, n_img_stages = 0; } lv[2];
    bool ready = false;               // every level of the geometry is allocated
    void release() { *this = CentroidSet{}; }
};
// THE SORTED PASS: rows in the order of their (pseudo) last BMU's patch (position -> row: `order`), with sorted copies of the half
// image, its second half, the float32 rows and the norms.  The handle holds two: the RESIDENT rows' (all passes; valid for one row
// set, re-sorted when the order has gone stale -- policy::PlanState --, not every epoch) and ONE pass of a TRANSIENT row set
// (query rows, streamed chunks: sorted by the scout of exact_skip.hpp, used once).
struct SortedRows {
    bool resident = false;        // the resident rows' pass (fixed at construction): replacing its buffers loses the resident order
    long cap = 0;                 // positions the buffers hold (each pass padded to the tile)
    DevBuf<int> order;
    DevBuf<__bf16> Xb_s;
    DevBuf<__bf16> Xl_s;          // ... the rows' second half image (the refinement pass): reserve_second_half, when it first engages
    bool xl_filled = false;       //     ... and written by a gather since
    DevBuf<float> Xf_s, xsq_s, xerr_s, seed_s, sU_s;
    DevBuf<int> lastpos_s;        // position (patch order) of every sorted row's (pseudo) last BMU
    // lastpos_s[p] == inv[bmu[order[p]]] for every position of the resident rows: the last epoch's finalize stored them
    // pass by pass and no row fell back.  Taken (and cleared) by the next resident launch; cleared by whatever else writes
    // the resident ids or replaces these buffers (launch_bmu_exact, exact_pass)
    bool lastpos_valid = false;
    explicit SortedRows(bool resident_rows = false) : resident(resident_rows) {}
    void release() { *this = SortedRows{resident}; }
};

struct som_handle {
    som_config cfg{};
    void* comm = nullptr;        // ncclComm_t of som_comm_init (NULL: single GPU, or the host does the all-reduce)
    int comm_world = 1;
    hipStream_t comm_stream = nullptr;   // the blockwise all-reduce runs here, under the transform of the next block
    hipEvent_t ev_block = nullptr, ev_comm = nullptr;
    int X = 0, Y = 0, K = 0, D = 0, D1p = 0;
    // missing values (som_config.missing == SOM_MISSING_NAN): a NaN feature is "not observed".  The search is
    // bmu_masked_f32_kernel, level 0 of the run sum keeps a count per feature, the merge divides per (unit, feature).
    // UD: the features of an update row -- D, or masked 2 * D, [sums | per-feature counts] -- with the count in column UD;
    // D1p = round_up(UD + 1, 4).  Everything between level 0 and the merge sees UD features and nothing else.
    bool masked = false;
    int UD = 0;
    int ks32 = 0;            // bf16, 16x16x32 shape: ceil(D/32)
    bool tiled = false;      // bf16, input_len > 128: two-sided tiling (bmu_bf16_tiled.hpp)
    bool f16 = false;        // precision f16: _Float16 operands instead of __bf16 (the same kernels, som_common.hpp)
    bool exact = false;      // precision 'exact': MFMA screen + float32 re-score of the candidates (bmu_exact.hpp)
    // exact mode: the operand images in PATCH ORDER (som_common.hpp; ex_perm[position] = unit, ex_inv[unit] = position) -- prepared
    // from a permuted copy of the codebook (the float32 kernels proper -- fallback rows, top-2, analysis calls -- want the
    // float32 image in the units' own order and rebuild it: operands::Request::F32Units)
    bool ex_patch = false;
    bool ex_sub44 = false;                              // ... with every group an 8 x 8 patch in 4 x 4 blocks (patch_order)
    DevBuf<int> ex_perm;
    DevBuf<int> ex_inv;
    DevBuf<float> Wp;        // [K][D] codebook in patch order
    DevBuf<float> wsq_p;     // [K]   its |w|^2 (the float32 kernel's own values, permuted)
    struct ExactScratch {
        PassScratch pass;                 // the buffers: four owners (above), sized by exact_scratch.hpp
        PlanScratch pbuf;
        CentroidSet cen;
        SortedRows srt[2] = {SortedRows{true}, SortedRows{false}};   // [0] the resident rows, [1] one pass of a transient row set
        long stride_cap = 0;              // rows per pass the device had memory for (0: no allocation was ever refused)
        PassCounters* pass_host = nullptr;   // pinned: the pass's counter tail, read back once per pass
        hipEvent_t fb_ready = nullptr;       // recorded behind the counter's copy
        struct Switches {                 // between kernel sequences (A/B; read once in som_create: read_env)
            bool seed_on = true;              // SOM_EXACT_SEED=0: no seed
            int two_round = -1;               // SOM_EXACT_TWO_ROUND=0|1 forces the one- / two-round re-score (default: two rounds beyond 128 features)
            int skip_mode = 1;                // SOM_EXACT_SKIP: 0 off, 1 on for maps of >= 4096 units (default), 2 on for every map of >= 2 groups (tests), 3: plan, keep everything
            bool sub_blocks = true;           // SOM_EXACT_SUBBLOCKS=0: the plan stops at the groups
            bool chain = true;                // SOM_EXACT_CHAIN=0: the planned epoch's small launches as separate kernels and fills
            int res_every = 0;                // SOM_EXACT_RESORT=n: re-sort every n-th planned epoch (0: when the order has gone stale)
            bool refine_on = true;            // SOM_EXACT_REFINE=0: no refinement pass
            int grid_mult = 2;                // persistent re-score / refinement kernels: workgroups per resident slot (SOM_EXACT_GRID_MULT)
            bool scout_on = true;             // SOM_EXACT_SCOUT=0: no scout (exact_skip.hpp: pseudo last BMUs for rows that have none, or whose last BMUs say little)
            bool fuse_select = true;          // SOM_EXACT_FUSE_SELECT=0: exact_select_kernel in a launch of its own, not the listed screen's select tail (bmu_bf16_k16.hpp)
            bool fuse_plan = true;            // SOM_EXACT_FUSE_PLAN=0: a pass's plan always as three launches, not exact_plan_fused_kernel's one where the launch allows it
            bool plan_fold = true;            // SOM_EXACT_PLAN_FOLD=0: the plan kernels compare against P as before instead of folding it into the extra MFMA step
            bool item_queue = true;           // SOM_EXACT_QUEUE=0: one workgroup per tile (and part) instead of the work queue
            int item_len_pct = 125;           // ... =<pct >= 25>: an item's length in per cent of the mean list
        } sw;
        struct Hooks {                    // the tests' (SOM_TEST_HOOKS=1): SOM_EXACT_PASS_ROWS, _DEBUG_REFUSE_ABOVE, _PAIRS, _DEBUG_REFUSE_SKIP, _PLAN_PARTS
            long pass_rows_override = 0, refuse_above = 0, pairs = 0; bool refuse_skip = false; int plan_parts = 0;
        } hook;
        void read_env() {
            if (const char* e = dev_env("SOM_EXACT_PASS_ROWS")) hook.pass_rows_override = std::atol(e);
            if (const char* e = dev_env("SOM_EXACT_DEBUG_REFUSE_ABOVE")) hook.refuse_above = std::atol(e);
            if (const char* e = dev_env("SOM_EXACT_PAIRS")) hook.pairs = std::max(1L, std::atol(e));
            hook.refuse_skip = dev_env("SOM_EXACT_DEBUG_REFUSE_SKIP") != nullptr;
            if (const char* e = dev_env("SOM_EXACT_TWO_ROUND")) sw.two_round = std::atoi(e) != 0 ? 1 : 0;
            if (const char* e = dev_env("SOM_EXACT_SEED")) sw.seed_on = std::atoi(e) != 0;
            if (const char* e = std::getenv("SOM_EXACT_SKIP")) sw.skip_mode = std::atoi(e);
            if (const char* e = dev_env("SOM_EXACT_SUBBLOCKS")) sw.sub_blocks = std::atoi(e) != 0;
            if (const char* e = dev_env("SOM_EXACT_REFINE")) sw.refine_on = std::atoi(e) != 0;
            if (const char* e = dev_env("SOM_EXACT_QUEUE")) { sw.item_queue = std::atoi(e) != 0; if (std::atoi(e) >= 25) sw.item_len_pct = std::atoi(e); }
            if (const char* e = dev_env("SOM_EXACT_SCOUT")) sw.scout_on = std::atoi(e) != 0;
            if (const char* e = dev_env("SOM_EXACT_GRID_MULT")) sw.grid_mult = std::max(1, std::atoi(e));
            if (const char* e = dev_env("SOM_EXACT_RESORT")) sw.res_every = std::max(0, std::atoi(e));
            if (const char* e = dev_env("SOM_EXACT_CHAIN")) sw.chain = std::atoi(e) != 0;
            if (const char* e = dev_env("SOM_EXACT_FUSE_SELECT")) sw.fuse_select = std::atoi(e) != 0;
            if (const char* e = dev_env("SOM_EXACT_FUSE_PLAN")) sw.fuse_plan = std::atoi(e) != 0;
            if (const char* e = dev_env("SOM_EXACT_PLAN_FOLD")) sw.plan_fold = std::atoi(e) != 0;
            if (const char* e = dev_env("SOM_EXACT_PLAN_PARTS")) hook.plan_parts = std::max(0, std::atoi(e));
        }
        struct Stats {                    // what the som_exact_*_stats / som_debug_exact_*_stats entries return
            int64_t rows_total = 0, rows_fallback = 0, chunks = 0;   // som_exact_stats
            int64_t blocks_run = 0, blocks_total = 0;                // som_exact_skip_stats: (256-row tile, 16-unit block) blocks of the screens
            int64_t lastpos_carried_epochs = 0;   // planned resident epochs that skipped exact_lastpos_kernel (som_debug_exact_chain_stats)
            int64_t sel_fused_passes = 0, sel_launched_passes = 0, sel_ticket_tiles = 0;   // som_debug_exact_select_stats
            int64_t plan_fused_launches = 0, plan_split_launches = 0, plan_folded = 0, plan_compared = 0;   // som_debug_exact_plan_stats, _plan_fold_stats
        } stats;
        bool seed_live = false; int screen_slots = 0;   // this pass's screen reads the seed; the listed screen's last grid (what the next plan cuts its lists for)
        // what a launch decides -- plan at all, re-sort, scout, level 2, refine -- and the state those decisions move from
        // launch to launch (pause ladder, re-sort schedule, level-2 probe, measured costs): exact_policy.hpp
        policy::PlanState plan;
        policy::LaunchPlan lp;            // ... of the launch in flight (launch_bmu_exact)
        double share_forecast = 1.0;      // executed share expected of the launch about to run (the screen sizes its codebook parts by it)
        // what the last launch learned from its samples, as plain numbers (-1: not asked), and the geometry of its last planned
        // pass up to 128 features (read-only test accessors: som_debug_exact_forecast, som_debug_exact_tile_blocks)
        struct Forecast {
            double need = -1.0, rows = 0.0;                           // the row sample: share of the groups a row needs; rows sampled
            double est = -1.0, est1 = -1.0, n_st = -1.0, st = -1.0;   // the sample tiles: shares after both levels / level 1; tiles; stride
            double blocks_run = -1.0, groups_run = -1.0;              // ... their raw counters
            double level2 = -1.0;                                     // ... planned with level 2?
        } fc;
        long last_plan_tiles = 0;         // tiles of the last pass of the last launch, where it ran under a plan (else 0)
        bool last_plan_l2 = false;        // ... whether that pass's plan ran level 2
        // MEASURED COSTS (hipEvents on the handle's stream; per ROW, in ms, so that launches of different sizes compare): what the
        // policy decides from -- is a plan worth its launches, does level 2 pay, did a sort pay, is the plan idle.  The launch as
        // a whole is timed every time (two records); its phases under a plan -- screen, level 2, sort + gather -- in the first
        // planned launches, in every launch that sorts, and every fourth one after that (a record costs a few microseconds of
        // stream bubble: eight of them a launch would be 2 % of a 1.8 ms epoch).
        struct Cost {                     // (the numbers themselves and what is decided from them: policy::Costs, exact_policy.hpp)
            hipEvent_t ev[8] = {};            // [0] launch / pass start, [1, 2] screen, [3, 4] level 2, [5, 6] sort + gather, [7] pass end
            bool have = false;
        } cost;
    } ex;
    int n_kchunks = 0;       // tiled: 64-feature chunks
    int n_ublocks = 0;       // tiled: unit blocks of tl_bn
    bool tl_big = false;     // tiled: 256 x 256 workgroup tiles (8 waves) instead of 128 x 128
    bool wide = false;       // bf16, 128 < input_len <= 800, big maps: samples resident in registers (bmu_bf16_wide.hpp)
    int tl_bm = 128, tl_bn = 128, tl_xtile = 0, tl_wfrag = 0, tl_wtile = 0;
    int dp = 0;              // feature stride of the bf16 row image
    int stage_bytes = 0;     // bytes of one codebook stage image
    int stage_units = 0;     // units per stage
    int nt = 1;              // neighbourhood terms
    bool swapped = false;    // mexican_hat + compact_support, rectangular: row stage, mask, column stage (update.hpp)
    bool torus = false;      // toroidal topology: wrapped offsets in the tables, two band ranges per tile and segment (update.hpp)
    int norm_p = 2;          // exponent of the norm_p distances
    double norm_pr = 0.0;    // ... when it is not an integer (0: norm_p)
    hipStream_t stream = nullptr;
    bool own_stream = false;

    DevBuf<float> W, wsq, SC, T, ACC, P1, P2;
    DevBuf<float> Ud;        // the count column after stage 1 of the transform, dense [nt][X][Y]
    DevBuf<char> Wst;
    DevBuf<char> Wst_lo;     // exact mode, input_len <= 128: the units' second half image (the refinement pass, bmu_exact.hpp)
    DevBuf<char> Wfst;       // f32 parity mode, input_len <= 128: float32 stage image (bmu_f32_res.hpp)
    int fr_kg = 0, fr_stages = 0;
    DevBuf<char> Wfimg;      // f32 parity mode, input_len > 128: float32 tile image (bmu_f32_tiled.hpp)
    DevBuf<char> ftX;        //   sample tile image of the rows being scanned (scratch, grown on demand)
    int ft_kchunks = 0, ft_ublocks = 0;
    int n_stages = 0;
    // which of the operands derived from W are current (rebuilt lazily: refresh_codebook_operands): codebook_operands.hpp
    operands::State ops;

    RowSet res{rowset::Kind::Resident};   // the resident training rows (som_set_data*), their sample weights (som_set_sample_weights*)
    // precision 'exact': the update-side work that does not depend on the BMUs (the zeroed segment sums, the neighbourhood
    // tables) is queued BEFORE the pass's counter read-back, so the GPU has it to do while the host wakes up
    struct EarlyUpdate { bool armed = false, done = false; double sigma = 0, eta = 0; int neigh_f64 = 0; } early;
    DevBuf<unsigned long long> best64;   // bf16 path: per-row (value bits | unit) merged across codebook parts
    int n_cus = 0;
    // BMU-ordered view of a row set + the partial lists of the segment sum's upper levels (update.hpp)
    struct SegScratch {
        UnitSort sort;                           // (its cap: the rows this scratch serves)
        DevBuf<int> kA, kB;                      // keys of the level-1 / level-2 lists (ping-pong from there on)
        DevBuf<float> vA, vB;                    // their vectors [entries][D1p]
    };
    SegScratch seg;                              // resident rows
    DevBuf<float> xmax2;     // [0] resident rows, [1] every transient row set: max_n |x~_n|^2 (RowSet::xmax2)
    DevBuf<float> wn;        // |w~_k|^2 per unit
    DevBuf<float> wmax2;

    RowSet q;                // the rows of a query (som_bmu*, som_quantization_error*, ...) or of a pageable streamed chunk
    DevBuf<double> qX64;     // som_bmu_f64: float64 query rows
    DevBuf<double> dsum;
    // precision 'exact', value-only quantization BMUs (run_quantization_bmu): the rows whose screen pick a tie of the sqrt'd
    // distance could overturn, gathered for the float32 SQRT kernel, and how many rows went each way (som_debug_qe_stats)
    DevBuf<int> qe_list, qe_ids, qe_cnt; DevBuf<float> qe_X, qe_xsq;
    int64_t qe_rows = 0, qe_rows_sqrt = 0;
    // precision 'exact', top-2 (exact_top2_host.hpp): the screen's per-part minima, the unit round 2 leaves out, the rows the
    // float32 top-2 kernel answers (gathered), and how many rows went each way (som_exact_top2_stats)
    struct Top2Scratch {
        bool on = true;                   // SOM_EXACT_TOP2=0: the float32 top-2 kernel for every row
        DevBuf<float> m;                  // [2 x codebook parts][rows of the pass, padded]: (minimum, second minimum) of every part
        DevBuf<int> excl;                 // [rows of the pass] position of round 1's winner
        DevBuf<float> X, xsq;
        DevBuf<int> ids1, ids2;
        int64_t rows = 0, rows_f32 = 0;
    } t2;
    // streamed epochs (rows that do not stay resident): per-chunk sort scratch, grown on demand
    SegScratch st_seg;
    bool streaming = false;
    // double-buffered device staging for chunks that arrive in pinned host memory
    struct Slot {
        RowSet rows{rowset::Kind::Slot};         // (its sample weights, som_stream_rows_weighted: allocated on first use)
        hipEvent_t copied = nullptr, consumed = nullptr;
        bool used = false;
    } slot[2];
    hipStream_t copy_stream = nullptr;
    int slot_idx = 0;

    // whole-epoch hipGraph (som_epoch_accumulate on resident rows), opt-in with SOM_GRAPH=1: captured on the
    // second epoch over the same buffers, replayed afterwards; any (re)allocation or new row set makes it
    // stale.  Off by default: measured on ROCm 7.2 the replay is no faster than the eager launches
    // (6x6x4 map, 150 rows: 49.5 us vs 41.2 us per epoch; 64x64x32, 100k rows: 0.366 vs 0.356 ms).
    bool use_graph = false;
    bool capturing = false;
    hipGraphExec_t gexec = nullptr;
    unsigned long alloc_gen = 0, gexec_gen = 0;
    const void* gexec_rows = nullptr;
    long gexec_n = -1;
    int graph_warm = 0;
    DevBuf<NeighParams> np_dev;   // read by the captured neigh_tables_kernel
    DevBuf<int2> bands;      // nonzero column ranges of the neighbourhood tables per 32-row tile: two buffers (update.hpp, "ranges")
    bool use_bands = true;
    int band_sel = 0;        // the buffer the last build of the tables filled; the next build fills the other one
    int lm_rows = 0;         // SOM_LM_ROWS: rows of H per leftmul workgroup, 64 or 128 (0: launch_leftmul's own choice)

    // canary (som_set_verify / SOM_VERIFY=n): n strided rows of every BMU launch re-scored by the float32 kernel
    int verify_rows = 0;
    bool verifying = false;
    DevBuf<int> vf_rows, vf_picks, vf_best, vf_bad;
    DevBuf<float> vf_X;
    int vf_cap = 0;
    int64_t verify_launches = 0, verify_rows_checked = 0;
    bool fuse_merge_prep = true; // SOM_FUSE_MERGE=0: separate merge and operand-preparation launches (A/B)
    bool counting_sort = true;   // SOM_COUNTING_SORT=0: the radix sort on small maps too (A/B)
    int64_t sorts_counting = 0, sorts_radix = 0;   // sorts by unit of each kind since som_create (som_debug_unit_sort_stats)
    // read once in som_create (experiments / A-B runs): forced part counts, launch-geometry printing
    int env_bf16_parts = 0;
    int env_f32_parts = 0;   // SOM_F32_PARTS: the float32 resident kernel's part count (clamped to [1, fr_stages])
    bool debug = false;
    // per kernel function: the dynamic-LDS attribute is set and the occupancy queried once, not per launch
    struct KernelSlots { const void* fn; size_t lds; int per_cu; };
    std::vector<KernelSlots> kernel_slots;
    int staged_blocks_done = -1; // som_epoch_accumulate_begin / _block: next block expected, -1 = none pending
    // training monitor (monitor.hpp; som_monitor): everything here is allocated when it is switched on and freed when it is
    // switched off -- `prev`, last measured epoch's ids of the resident rows, beside the row set but not of rowset::sizes
    struct Monitor {
        bool on = false;
        DevBuf<int> prev;                        // [res.N] the ids the last som_epoch_measure_rows saw
        bool prev_valid = false;                 // ... of THESE resident rows (som_set_data* clears it)
        DevBuf<MonitorRowPartial> rpart;         // [4096] one per workgroup of the row kernel
        DevBuf<MonitorShiftPartial> spart;       // [2048] ... of the shift kernel
        DevBuf<som_epoch_metrics_t> m;           // the metrics of the epoch in flight
        som_epoch_metrics_t* m_host = nullptr;   // pinned: som_epoch_metrics' one read-back
    } mon;
    // row moments and the row gather (moments.hpp; som_row_moments*, som_gather_rows_device): the one owner of their scratch, grown
    // on demand and freed with the handle.  Size rule, for n rows of D features (moments_plan): X n * D and w n floats (the host
    // entry's staged rows and weights), pivot D floats, spart mom_sum_grid(n) * (D + 1) and sums D + 1 doubles, gpart
    // mom_splits(n, D) * mom_tiles(D) * 1024 and gram D * D doubles (only where the Gram matrix is asked for); the gather: idx k
    // int64 and rows k * D floats
    struct MomentsScratch {
        DevBuf<float> X, w, pivot;
        DevBuf<double> spart, sums, gpart, gram;
        DevBuf<long long> idx;
        DevBuf<float> rows;
    } mom;
    // data density per unit (density.hpp; som_unit_density*): the one owner of its scratch, grown on demand and freed with the handle.
    // Size rule: pivot D floats, Wc K * D floats (the centred codebook), wsq K floats, counts 8 * K (the largest radius count).  The
    // rows' |x'|^2 go into the query set's xsq, which a query of n rows always holds (row_set.hpp).
    struct DensityScratch {
        DevBuf<float> pivot, Wc, wsq;
        DevBuf<unsigned long long> counts;
    } den;
    // the k nearest units (topk.hpp; som_bmu_topk*, som_unit_rank_counts*): the one owner of its scratch, grown on demand and freed with
    // the handle.  Size rule, for a pass of P <= TOPK_PASS_ROWS rows cut into `parts` codebook parts: the lists ids / score / dist
    // P * TOPK_MAX each (score and dist only once a call has asked for them), the partial lists part_sc / part_id parts * P * TOPK_MAX
    // each, counts TOPK_MAX * K.
    struct TopkScratch {
        DevBuf<int> ids, part_id;
        DevBuf<float> score, dist, part_sc;
        DevBuf<unsigned long long> counts;
    } topk;
    bool searched = false;       // the resident ids are those of a search since the last som_epoch_merge
    bool async_copies = false;   // SOM_ASYNC_COPIES=1: round 1's original copy path (fresh_process_stress.py)
    int prof = 0;            // som_profile_enable: 0 off, 1 every kernel family, 2 the BMU family only
    std::vector<EventPair> pending, pool;
    double ms[SOM_K_COUNT] = {0};
    int64_t launches[SOM_K_COUNT] = {0};

    std::string err;
};

namespace {

int fail(som_handle* h, const std::string& msg) {
    if (h) h->err = msg; else g_create_error = msg;
    return 1;
}
int fail_hip(som_handle* h, const char* what, hipError_t e) {
    return fail(h, std::string(what) + ": " + hipGetErrorString(e));
}

// Every entry point runs on the handle's device and leaves the calling thread's current device as it found
// it (the host process shares this HIP runtime with torch, whose current device must not move under it).
struct DeviceGuard {
    int prev = -1;
    bool moved = false;
    explicit DeviceGuard(const som_handle* h) {
        if (!h) return;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != h->cfg.device) { (void)hipSetDevice(h->cfg.device); moved = true; }
    }
    ~DeviceGuard() { if (moved && prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

#define HIPCHK(h, call)                                              \
    do {                                                             \
        hipError_t e_ = (call);                                      \
        if (e_ != hipSuccess) return fail_hip((h), #call, e_);       \
    } while (0)

}  // namespace

template <typename T>
int DevBuf<T>::alloc(som_handle* h, size_t n) {
    reset();
    if (n == 0) n = 1;
    if (h->capturing) return fail(h, "allocation during graph capture");
    if (hipError_t e = hipMalloc((void**)&p, n * sizeof(T)); e != hipSuccess) { p = nullptr; return fail_hip(h, "hipMalloc", e); }
    ++h->alloc_gen;                                   // device pointers baked into a captured graph may be stale
    cap = n;
    g_dev_bytes += (int64_t)(n * sizeof(T));
    return 0;
}

namespace {

// Host -> device copy of caller-owned (usually pageable) memory.  Blocking on purpose: the runtime stages
// pageable sources through its own pinned buffers; the copy is complete before anything that reads `dst` is
// launched, and the stream is drained first, so nothing of ours still touches dst.
// SOM_ASYNC_COPIES=1 restores round 1's original form (hipMemcpyAsync on the engine's stream, no host wait)
// for tools/fresh_process_stress.py, which exists to confirm or kill the hypothesis that that form produced the
// one wrong-BMU event on record.
int h2d_blocking(som_handle* h, void* dst, const void* src, size_t bytes) {
    if (h->async_copies) {
        HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
        return 0;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
}
// ... and results back to caller-owned memory, the same way: drain the stream, then a blocking copy.
int d2h_blocking(som_handle* h, void* dst, const void* src, size_t bytes) {
    if (h->async_copies) {
        HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return 0;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
}

// Workgroups of `fn` (threads per workgroup, dynamic LDS bytes) one CU holds at once; the first call per
// (function, LDS size) raises the function's dynamic-LDS limit and asks the runtime, later calls read the cache.
int kernel_per_cu(som_handle* h, const void* fn, int threads, size_t lds, int* per_cu) {
    for (const auto& k : h->kernel_slots)
        if (k.fn == fn && k.lds == lds) { *per_cu = k.per_cu; return 0; }
    HIPCHK(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int n = 0;
    HIPCHK(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, threads, lds));
    h->kernel_slots.push_back({fn, lds, n > 0 ? n : 1});
    *per_cu = n > 0 ? n : 1;
    return 0;
}

// resident workgroup slots of a kernel on the chip (per_cu: kernel_per_cu's answer)
inline long resident_slots(const som_handle* h, int per_cu) { return (long)per_cu * (h->n_cus > 0 ? h->n_cus : 256); }

inline long cdiv(long a, long b) { return (a + b - 1) / b; }
inline long round_up(long a, long b) { return cdiv(a, b) * b; }
constexpr float HALF_MAX = 65504.0f;   // largest finite _Float16
using rowset::ROW_PAD;

// ---- profiling: event pairs recorded around kernel families, resolved lazily ---------------
struct Timed {
    som_handle* h; int kernel; EventPair ep{}; bool on;
    Timed(som_handle* h_, int k) : h(h_), kernel(k), on(h_->prof == 1 || (h_->prof == 2 && (k == SOM_K_BMU || k == SOM_K_SCREEN))) {
        if (!on) return;
        if (!h->pool.empty()) { ep = h->pool.back(); h->pool.pop_back(); }
        else { (void)hipEventCreate(&ep.a); (void)hipEventCreate(&ep.b); }
        ep.kernel = kernel;
        (void)hipEventRecord(ep.a, h->stream);
    }
    ~Timed() {
        if (!on) return;
        (void)hipEventRecord(ep.b, h->stream);
        h->pending.push_back(ep);
    }
};

int resolve_profile(som_handle* h) {
    if (h->pending.empty()) return 0;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (auto& ep : h->pending) {
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, ep.a, ep.b));
        h->ms[ep.kernel] += ms;
        h->launches[ep.kernel] += 1;
        h->pool.push_back(ep);
    }
    h->pending.clear();
    return 0;
}

// ---- codebook-derived operands (w_sq cache, xpysom.py:529-537; bf16 / f16 stage image) -----
// The 'bf16' and 'f16' paths are templates on the operand type's tag E (Bf16 or F16, som_common.hpp); SOM_HALF picks
// the instance from the handle.  (The exact mode has one operand type, ExactEl -- bmu_exact.hpp -- and no such template.)
#define SOM_HALF(h, fn, ...) ((h)->f16 ? fn<F16>(__VA_ARGS__) : fn<Bf16>(__VA_ARGS__))
// ... and these call f with the handle's feature count as a std::integral_constant, so that f names the instance it wants:
// ks32 32-feature steps up to 128 features, n_kchunks 64-feature chunks beyond (the wide kernel).  A count without an
// instance fails with `none`.
template <class F>
int for_ks32(som_handle* h, const char* none, F&& f) {
    switch (h->ks32) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    }
    return fail(h, none);
}
template <class F>
int for_kchunks(som_handle* h, const char* none, F&& f) {
    switch (h->n_kchunks) {
#define SOM_KCHUNKS_CASE(k) case k: return f(std::integral_constant<int, k>{});
    SOM_KCHUNKS_CASE(5) SOM_KCHUNKS_CASE(6) SOM_KCHUNKS_CASE(7) SOM_KCHUNKS_CASE(8) SOM_KCHUNKS_CASE(9) SOM_KCHUNKS_CASE(10) SOM_KCHUNKS_CASE(11)
    SOM_KCHUNKS_CASE(12) SOM_KCHUNKS_CASE(13) SOM_KCHUNKS_CASE(14) SOM_KCHUNKS_CASE(15) SOM_KCHUNKS_CASE(16) SOM_KCHUNKS_CASE(17) SOM_KCHUNKS_CASE(18)
    SOM_KCHUNKS_CASE(19) SOM_KCHUNKS_CASE(20) SOM_KCHUNKS_CASE(21) SOM_KCHUNKS_CASE(22) SOM_KCHUNKS_CASE(23) SOM_KCHUNKS_CASE(24) SOM_KCHUNKS_CASE(25)
#undef SOM_KCHUNKS_CASE
    }
    return fail(h, none);
}

// the exact mode's 16-bit stage image up to 128 features (cm: with the centroid levels' maxima -- the fused merge wrote the
// centroids).  It is due whenever the codebook has changed; a planned launch writes it in one grid with its centroid images
// (exact_prep_images_kernel), which only launch_bmu_exact can know: its caller lets the refresh leave this one kernel pending
// (operands::State), and the launch -- or, should it not get there, the next refresh -- pays it
int launch_prep_w_exact(som_handle* h, bool cm) {
    const float* Wex = h->ex_patch ? h->Wp : h->W;
    float* cm1 = cm ? (float*)h->ex.cen.lv[0].cmax2 : nullptr;
    float* cm2 = cm ? (float*)h->ex.cen.lv[1].cmax2 : nullptr;
    const dim3 tgrid((unsigned)cdiv((long)h->n_stages * K16_T, 4)), block(256);
    switch (h->ks32) {
#define SOM_PREPX_CASE(k) case k: prep_w_exact_k16_kernel<k, ExactEl><<<tgrid, block, 0, h->stream>>>(Wex, h->K, h->D, h->Wst, h->n_stages, h->wmax2, h->wmax2 + 1, h->Wst_lo, cm1, cm2); break;
    SOM_PREPX_CASE(1) SOM_PREPX_CASE(2) SOM_PREPX_CASE(3) SOM_PREPX_CASE(4)
#undef SOM_PREPX_CASE
    default: return fail(h, "the resident half-precision kernel supports input_len <= 128");
    }
    return 0;
}
int flush_prep_w(som_handle* h) {
    bool cm = false;
    if (!h->ops.take_pending_image(&cm)) return 0;
    if (int rc = launch_prep_w_exact(h, cm)) return rc;
    HIPCHK(h, hipGetLastError());
    return 0;
}

// the exact mode's 16-bit operand images of the codebook, in patch order where the handle has one (the screen's image from the
// permuted codebook: refresh_codebook_operands wrote it)
// (r: the refresh's decision -- up to 128 features it skips the norms step behind a fused merge and may leave the image kernel pending)
int prep_codebook_exact(som_handle* h, const operands::Rebuilds& r) {
    const float* Wex = h->ex_patch ? h->Wp : h->W;
    const float* qex = h->ex_patch ? h->wsq_p : h->wsq;
    const dim3 block(256);
    if (h->wide) {
        // beyond 128 features: the float32 kernel's own |w|^2 as the norm term (euclidean) or none (cosine:
        // unit-length units, max |w| = 1), the units scaled by a power of two, their rounding errors measured
        const float* unit = h->cfg.distance == SOM_DIST_COSINE ? qex : nullptr;
        if (unit) {
            HIPCHK(h, hipMemsetAsync(h->wn, 0, (size_t)h->K * sizeof(float), h->stream));
            HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)h->wmax2, 0x3F800000, 1, h->stream));
        } else {
            HIPCHK(h, hipMemsetAsync(h->wmax2, 0, sizeof(float), h->stream));
            exact_copy_wsq_kernel<<<dim3((unsigned)cdiv(h->K, 1024)), dim3(1024), 0, h->stream>>>(qex, h->K, h->wn, h->wmax2);
        }
        long total = (long)h->n_stages * WD_T * h->n_kchunks * 64;
        prep_w_bf16_wide_kernel<ExactEl><<<dim3((unsigned)cdiv(total, 256)), block, 0, h->stream>>>(
            Wex, h->K, h->D, h->n_kchunks, h->Wst, h->n_stages, unit, h->wmax2);
        HIPCHK(h, hipMemsetAsync(h->wmax2 + 1, 0, sizeof(float), h->stream));
        exact_werr_kernel<ExactEl><<<dim3((unsigned)cdiv(h->K, 4 * EX_WERR_UNITS)), block, 0, h->stream>>>(Wex, h->K, h->D, h->wmax2, h->wmax2 + 1, unit);
        return 0;
    }
    // up to 128 features: the float32 kernel's own |w|^2 (refreshed just before) and its maximum first: the units go in scaled by
    // ex_scale(max |w|^2); then the scaled stage image and the units' rounding errors in one pass
    // (after a fused merge both are there already, and the pair was zeroed in front of it: exact_merge_prep_kernel)
    if (!r.skip_norms) {
        HIPCHK(h, hipMemsetAsync(h->wmax2, 0, 2 * sizeof(float), h->stream));     // [0]: max |w|^2, [1]: max_k |w^_k - w~_k|^2
        exact_copy_wsq_kernel<<<dim3((unsigned)cdiv(h->K, 1024)), dim3(1024), 0, h->stream>>>(qex, h->K, h->wn, h->wmax2);
    }
    // (r.cm: centroids the fused merge wrote: their levels' maxima are due now that max |w|^2 is final)
    if (h->ks32 < 1 || h->ks32 > 4) return fail(h, "the resident half-precision kernel supports input_len <= 128");
    if (r.deferred) return 0;
    return launch_prep_w_exact(h, r.cm);
}

// precisions 'bf16' and 'f16': the 16-bit operand images of the codebook -- stage / tile image, |w~|^2 per unit and its maximum
template <class E>
int prep_codebook_half(som_handle* h) {
    const float* unit = h->cfg.distance == SOM_DIST_COSINE ? h->wsq : nullptr;
    const dim3 block(256);
    if (h->tiled) {
        if (h->wide) {
            long total = (long)h->n_stages * WD_T * h->n_kchunks * 64;
            prep_w_bf16_wide_kernel<E><<<dim3((unsigned)cdiv(total, 256)), block, 0, h->stream>>>(
                h->W, h->K, h->D, h->n_kchunks, h->Wst, h->n_stages, unit);
        } else {
            long total = (long)h->n_ublocks * h->n_kchunks * (h->tl_bn / 16) * TL_KS * 64;
            prep_tiles_bf16_kernel<E><<<dim3((unsigned)cdiv(total, 256)), block, 0, h->stream>>>(
                h->W, h->K, h->D, h->n_kchunks, h->n_ublocks, h->tl_bn, h->tl_wtile, -1.0f, unit, h->Wst);
        }
        HIPCHK(h, hipMemsetAsync(h->wmax2, 0, sizeof(float), h->stream));
        rownorm_bf16_kernel<E><<<dim3((unsigned)cdiv(h->K, 4)), block, 0, h->stream>>>(
            h->W, h->K, h->D, unit, unit != nullptr, h->wn, h->wmax2);
        return 0;
    }
    const long total = (long)h->n_stages * K16_T * h->ks32 * 64;
    const dim3 grid((unsigned)cdiv(total, 256));
    const float* sc = nullptr;
    switch (h->ks32) {
    case 1: prep_w_bf16_k16_kernel<1, E><<<grid, block, 0, h->stream>>>(h->W, h->K, h->D, h->Wst, h->n_stages, unit, sc); break;
    case 2: prep_w_bf16_k16_kernel<2, E><<<grid, block, 0, h->stream>>>(h->W, h->K, h->D, h->Wst, h->n_stages, unit, sc); break;
    case 3: prep_w_bf16_k16_kernel<3, E><<<grid, block, 0, h->stream>>>(h->W, h->K, h->D, h->Wst, h->n_stages, unit, sc); break;
    case 4: prep_w_bf16_k16_kernel<4, E><<<grid, block, 0, h->stream>>>(h->W, h->K, h->D, h->Wst, h->n_stages, unit, sc); break;
    default: return fail(h, "the resident half-precision kernel supports input_len <= 128");
    }
    HIPCHK(h, hipMemsetAsync(h->wmax2, 0, sizeof(float), h->stream));
    prep_wnorm_kernel<E><<<dim3((unsigned)cdiv(h->K, 256)), block, 0, h->stream>>>(h->W, h->K, h->D, h->wn, h->wmax2, unit);
    return 0;
}

// |w|^2 in NumPy's order (the parity kernels' own; with a patch order also permuted into wsq_p)
void launch_codebook_wsq(som_handle* h) {
    row_sq_f32_kernel<<<dim3((unsigned)cdiv(h->K, 256)), dim3(256), 0, h->stream>>>(h->W, h->K, h->D, h->wsq, h->wsq_p, h->ex_inv);
}

// the operands `rq`'s reader needs, rebuilt where they are stale: decide, launch what the decision lists, commit
// (may_defer: operands::State::decide)
int refresh_codebook_operands(som_handle* h, operands::Request rq, bool may_defer = false) {
    const operands::Rebuilds r = h->ops.decide(rq, may_defer);
    // (an image a BMU launch left pending and did not get to: whoever reads the operands next pays it)
    if (r.flush) {
        if (int rc = launch_prep_w_exact(h, r.flush_cm)) return rc;
        HIPCHK(h, hipGetLastError());
    }
    if (r.any()) {
        Timed t(h, SOM_K_PREP);
        if (r.wsq) launch_codebook_wsq(h);
        if (r.permute) {
            const long total = (long)h->K * ((h->D & 3) == 0 ? h->D / 4 : h->D);
            exact_permute_kernel<<<dim3((unsigned)cdiv(total, 256)), dim3(256), 0, h->stream>>>(h->W, h->wsq, h->K, h->D, h->ex_perm, h->Wp,
                                                                                               h->wsq_p);
        }
        if (r.f32) {
            const float* Wsrc = r.f32_patch ? h->Wp : h->W;
            const float* qsrc = r.f32_patch ? h->wsq_p : h->wsq;
            if (h->Wfimg) {
                long total = (long)h->ft_ublocks * h->ft_kchunks * (4 * 4 * 64 + 128);
                prep_tiles_f32_kernel<<<dim3((unsigned)cdiv(total, 256)), dim3(256), 0, h->stream>>>(
                    Wsrc, h->K, h->D, h->ft_kchunks, h->ft_ublocks, FT_WTILE, qsrc, h->Wfimg);
            }
            if (h->Wfst) {
                long total = (long)h->fr_stages * ((long)FR_UT * h->fr_kg * 64 + 64);
                prep_w_f32_res_kernel<<<dim3((unsigned)cdiv(total, 256)), dim3(256), 0, h->stream>>>(
                    Wsrc, qsrc, h->K, h->D, h->fr_kg, h->Wfst, h->fr_stages);
            }
        }
        if (r.half) if (int rc = h->exact ? prep_codebook_exact(h, r) : SOM_HALF(h, prep_codebook_half, h)) return rc;
        HIPCHK(h, hipGetLastError());
    }
    h->ops.commit(r);
    return 0;
}

// ---- BMU launches ----------------------------------------------------------------------------
int choose_parts(som_handle* h, long blocks, long slots, int max_parts_hint);

template <int MODE, int KG, bool TOP2 = false>
int launch_bmu_f32_res_kg(som_handle* h, const float* X, long N, const float* xsq, int* out, int* out2 = nullptr) {
    auto kern = bmu_f32_res_kernel<MODE, KG, TOP2>;
    size_t lds = 2 * (size_t)fr_stage_bytes(KG);
    int per_cu = 1;
    if (int rc = kernel_per_cu(h, (const void*)kern, 256, lds, &per_cu)) return rc;
    long grid = cdiv(N, FR_WG_SAMPLES);
    if (grid <= 0 || grid > 0x7fffffffL) return fail(h, "bmu_f32: row count out of range");
    int parts = 1;
    if (!TOP2) {
        const long slots = resident_slots(h, per_cu);
        parts = choose_parts(h, grid, slots, h->fr_stages);
        if (h->env_f32_parts > 0) parts = h->env_f32_parts;   // (tests: the single-part and the merged paths at any size)
        if (parts > h->fr_stages) parts = h->fr_stages;
        if (h->debug)
            std::fprintf(stderr, "[somhip] bmu_f32_res: blocks=%ld per_cu=%d slots=%ld parts=%d stages=%d\n", grid, per_cu,
                         slots, parts, h->fr_stages);
    }
    if (parts == 1) {
        kern<<<dim3((unsigned)grid), dim3(256), lds, h->stream>>>(X, N, h->D, xsq, h->Wfst, h->fr_stages, h->K, out, out2,
                                                                 nullptr);
    } else {
        if (int rc = h->best64.reserve(h, (size_t)N, 1024)) return rc;
        HIPCHK(h, hipMemsetAsync(h->best64, 0xFF, (size_t)N * sizeof(unsigned long long), h->stream));
        kern<<<dim3((unsigned)grid, (unsigned)parts), dim3(256), lds, h->stream>>>(X, N, h->D, xsq, h->Wfst, h->fr_stages,
                                                                                  h->K, out, out2, h->best64);
        bmu_finalize_kernel<<<dim3((unsigned)cdiv(N, 256)), dim3(256), 0, h->stream>>>(h->best64, N, h->K, out);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

template <int MODE, bool TOP2>
int launch_bmu_f32_tiled(som_handle* h, const float* X, long N, const float* xsq, int* out, int* out2) {
    const long n_blocks = cdiv(N, FT_BM);
    if (n_blocks <= 0 || n_blocks > 0x7fffffffL) return fail(h, "bmu_f32: row count out of range");
    if (int rc = h->ftX.reserve(h, (size_t)n_blocks * h->ft_kchunks * FT_TILE)) return rc;
    long total = n_blocks * h->ft_kchunks * (4 * 4 * 64);
    prep_tiles_f32_kernel<<<dim3((unsigned)cdiv(total, 256)), dim3(256), 0, h->stream>>>(
        X, N, h->D, h->ft_kchunks, n_blocks, FT_TILE, nullptr, h->ftX);
    size_t lds = 2 * (size_t)FT_STAGE;
    { int pc; if (int rc = kernel_per_cu(h, (const void*)bmu_f32_tiled_kernel<MODE, TOP2>, 256, lds, &pc)) return rc; }
    bmu_f32_tiled_kernel<MODE, TOP2><<<dim3((unsigned)n_blocks), dim3(256), lds, h->stream>>>(
        h->ftX, N, xsq, h->Wfimg, h->ft_ublocks, h->ft_kchunks, h->K, out, out2);
    HIPCHK(h, hipGetLastError());
    return 0;
}

template <int MODE>
int launch_bmu_f32_any(som_handle* h, const float* X, long N, const float* xsq, int* out) {
    if (h->Wfimg) return launch_bmu_f32_tiled<MODE, false>(h, X, N, xsq, out, nullptr);   // input_len > 128
    switch (h->fr_kg) {
    case 1: return launch_bmu_f32_res_kg<MODE, 1>(h, X, N, xsq, out);
    case 2: return launch_bmu_f32_res_kg<MODE, 2>(h, X, N, xsq, out);
    case 4: return launch_bmu_f32_res_kg<MODE, 4>(h, X, N, xsq, out);
    case 8: return launch_bmu_f32_res_kg<MODE, 8>(h, X, N, xsq, out);
    case 16: return launch_bmu_f32_res_kg<MODE, 16>(h, X, N, xsq, out);
    }
    return fail(h, "bmu_f32: bad k-group count");
}

// missing values: the masked search (bmu_masked_f32.hpp) reads the rows and the codebook as they are -- no operand image, no |w|^2
int launch_bmu_masked(som_handle* h, const float* X, long N, int* out) {
    const long grid = cdiv(N, F32_SB);
    if (grid <= 0 || grid > 0x7fffffffL) return fail(h, "bmu_masked_f32: row count out of range");
    bmu_masked_f32_kernel<<<dim3((unsigned)grid), dim3(256), MSK_LDS_BYTES, h->stream>>>(X, N, h->D, (int)round_up(h->D, F32_KC), h->W,
                                                                                        h->K, out);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// best AND second-best unit under the sqrt'd Euclidean distance (topographic error)
int launch_bmu_top2(som_handle* h, const float* X, long N, const float* xsq, int* out, int* out2) {
    constexpr int M = SCORE_EUCLID_SQRT;
    if (h->Wfimg) return launch_bmu_f32_tiled<M, true>(h, X, N, xsq, out, out2);
    switch (h->fr_kg) {
    case 1: return launch_bmu_f32_res_kg<M, 1, true>(h, X, N, xsq, out, out2);
    case 2: return launch_bmu_f32_res_kg<M, 2, true>(h, X, N, xsq, out, out2);
    case 4: return launch_bmu_f32_res_kg<M, 4, true>(h, X, N, xsq, out, out2);
    case 8: return launch_bmu_f32_res_kg<M, 8, true>(h, X, N, xsq, out, out2);
    case 16: return launch_bmu_f32_res_kg<M, 16, true>(h, X, N, xsq, out, out2);
    }
    return fail(h, "bmu_f32: bad k-group count");
}

// Number of codebook parts the scan is split into: fill whole rounds of the resident workgroup
// slots (large inputs) or spread a short scan over the chip (few rows: winner / small data).
int choose_parts(som_handle* h, long blocks, long slots, int max_parts_hint) {
    (void)h;
    int parts = 1;
    if (blocks < slots) {
        // fewer workgroups than resident slots: split the scan so about two slots' worth of workgroups
        // exist -- co-resident workgroups share a CU's MFMA pipe, so finer pieces balance the CUs
        // (measured: batch 65 536 at 256x256x128 bf16 +5 %, configs[1] f32 +15 % over one exact round)
        parts = (int)cdiv(2 * slots, blocks);
        // a handful of query rows: spread the scan itself (one or two workgroups' worth of rows -- winner() of a few
        // samples, the exact mode's fallback rows -- over up to 256 pieces: every CU streams a slice of the codebook)
        const int cap = blocks <= 2 ? 256 : 32;
        if (parts > cap) parts = cap;
    } else {
        double best_eff = 0.0;
        for (int p = 1; p <= 4; ++p) {
            long wgs = blocks * p;
            double eff = (double)wgs / (double)(cdiv(wgs, slots) * slots);
            if (eff > best_eff + 0.02) { best_eff = eff; parts = p; }
        }
    }
    if (parts > max_parts_hint) parts = max_parts_hint;
    if (parts < 1) parts = 1;
    return parts;
}

template <int KS32, class E>
int launch_bmu_bf16_k16(som_handle* h, const __bf16* Xb, long N, int* out) {
    size_t lds = 2 * (size_t)k16_stage_bytes(KS32);
    int per_cu = 1;
    if (int rc = kernel_per_cu(h, (const void*)bmu_bf16_k16_kernel<KS32, E>, 64 * K16_NW, lds, &per_cu)) return rc;
    long blocks = cdiv(N, K16_WG_SAMPLES);
    if (blocks <= 0 || blocks > 0x7fffffffL) return fail(h, "bmu_bf16: row count out of range");
    // split the codebook scan into `parts` so the grid fills whole rounds of resident workgroups
    const long slots = resident_slots(h, per_cu);
    int parts = choose_parts(h, blocks, slots, h->n_stages);
    if (h->env_bf16_parts > 0) parts = h->env_bf16_parts;   // experiments
    if (h->debug)
        std::fprintf(stderr, "[somhip] bmu_bf16_k16: blocks=%ld per_cu=%d cus=%d slots=%ld parts=%d stages=%d\n", blocks,
                     per_cu, h->n_cus, slots, parts, h->n_stages);
    // (best64[0..N) was reset by prep_wsqh_kernel, launch_bmu_bf16)
    bmu_bf16_k16_kernel<KS32, E><<<dim3((unsigned)blocks, (unsigned)parts), dim3(64 * K16_NW), lds, h->stream>>>(
        Xb, N, h->Wst, h->n_stages, h->K, h->best64);
    bmu_finalize_kernel<<<dim3((unsigned)cdiv(N, 256)), dim3(256), 0, h->stream>>>(h->best64, N, h->K, out);
    HIPCHK(h, hipGetLastError());
    return 0;
}

template <int WS, int NWR, int NWC, class E>
int launch_bmu_bf16_tiled_cfg(som_handle* h, const __bf16* Ximg, long N, int* out) {
    using C = TileCfg<WS, NWR, NWC>;
    auto kern = bmu_bf16_tiled_kernel<WS, NWR, NWC, E>;
    size_t lds = (size_t)C::LDS_BYTES;
    int per_cu = 1;
    if (int rc = kernel_per_cu(h, (const void*)kern, 64 * C::WAVES, lds, &per_cu)) return rc;
    long blocks = cdiv(N, C::BM);
    if (blocks <= 0 || blocks > 0x7fffffffL) return fail(h, "bmu_bf16: row count out of range");
    const long slots = resident_slots(h, per_cu);
    int parts = choose_parts(h, blocks, slots, h->n_ublocks);
    // with many unit blocks, 8 parts let one XCD's resident workgroups share sample tiles through its L2
    if (h->n_ublocks >= 64 && blocks * 8 >= slots) parts = 8;
    if (h->env_bf16_parts > 0) parts = h->env_bf16_parts;
    if (parts > h->n_ublocks) parts = h->n_ublocks;
    if (int rc = h->best64.reserve(h, (size_t)N, 1024)) return rc;
    HIPCHK(h, hipMemsetAsync(h->best64, 0xFF, (size_t)N * sizeof(unsigned long long), h->stream));
    const long grid = round_up(blocks, 8) * parts;
    if (grid > 0x7fffffffL) return fail(h, "bmu_bf16: grid too large");
    kern<<<dim3((unsigned)grid), dim3(64 * C::WAVES), lds, h->stream>>>(
        (const char*)Ximg, N, h->Wst, h->n_ublocks, h->n_kchunks, h->K, h->best64, (int)blocks, parts);
    bmu_finalize_kernel<<<dim3((unsigned)cdiv(N, 256)), dim3(256), 0, h->stream>>>(h->best64, N, h->K, out);
    HIPCHK(h, hipGetLastError());
    return 0;
}

template <int KS32, class E>
int launch_bmu_bf16_wide(som_handle* h, const __bf16* Ximg, const float* xmax2, long N, int* out) {
    auto kern = bmu_bf16_wide_kernel<KS32, E>;
    const size_t lds = (size_t)WD_SLOTS * wd_stage_bytes(KS32);
    int per_cu = 1;
    if (int rc = kernel_per_cu(h, (const void*)kern, 64 * WD_NW, lds, &per_cu)) return rc;
    const long blocks = cdiv(N, WD_WG_SAMPLES);
    if (blocks <= 0 || blocks > 0x7fffffffL) return fail(h, "bmu_bf16: row count out of range");
    const long slots = resident_slots(h, per_cu);
    // parts: whole rounds of the resident slots (every round scans one part in step: one L2 miss per XCD and stage)
    int parts = 1;
    if (blocks < slots) {
        parts = (int)std::min<long>(cdiv(slots, blocks), 64);
    } else {
        double best_eff = 0.0;
        for (int p = 1; p <= 8; ++p) {
            const long wgs = blocks * p;
            const double eff = (double)wgs / (double)(cdiv(wgs, slots) * slots);
            if (eff > best_eff + 0.01) { best_eff = eff; parts = p; }
        }
    }
    if (h->env_bf16_parts > 0) parts = h->env_bf16_parts;
    if (parts > h->n_stages) parts = h->n_stages;
    if (int rc = h->best64.reserve(h, (size_t)N, 1024)) return rc;
    const long units = (long)h->n_stages * h->stage_units;
    prep_wsqh_kernel<<<dim3((unsigned)cdiv(std::max(units, N), 256)), dim3(256), 0, h->stream>>>(
        h->wn, h->K, h->wmax2, xmax2, h->Wst, h->n_stages, h->stage_bytes, h->stage_units, h->best64, N);
    if (h->debug)
        std::fprintf(stderr, "[somhip] bmu_bf16_wide: blocks=%ld per_cu=%d slots=%ld parts=%d stages=%d\n", blocks, per_cu, slots,
                     parts, h->n_stages);
    bmu_bf16_wide_kernel<KS32, E><<<dim3((unsigned)blocks, (unsigned)parts), dim3(64 * WD_NW), lds, h->stream>>>(
        (const char*)Ximg, N, h->Wst, h->n_stages, h->best64);
    bmu_finalize_kernel<<<dim3((unsigned)cdiv(N, 256)), dim3(256), 0, h->stream>>>(h->best64, N, h->K, out);
    HIPCHK(h, hipGetLastError());
    return 0;
}

template <class E>
int launch_bmu_bf16_tiled(som_handle* h, const __bf16* Ximg, const float* xmax2, long N, int* out) {
    if (h->wide)
        return for_kchunks(h, "bmu_bf16_wide: no instance for this input_len",
                           [&](auto k) { return launch_bmu_bf16_wide<decltype(k)::value, E>(h, Ximg, xmax2, N, out); });
    long cin = (long)h->n_ublocks * h->n_kchunks * h->tl_bn;
    prep_tiles_cin_kernel<<<dim3((unsigned)cdiv(cin, 256)), dim3(256), 0, h->stream>>>(
        h->wn, h->K, h->wmax2, xmax2, h->n_kchunks, h->n_ublocks, h->tl_bn, h->tl_wfrag, h->tl_wtile, h->Wst);
    if (h->tl_big) return launch_bmu_bf16_tiled_cfg<8, 2, 4, E>(h, Ximg, N, out);
    return launch_bmu_bf16_tiled_cfg<4, 2, 2, E>(h, Ximg, N, out);
}

template <class E>
int launch_bmu_half(som_handle* h, const __bf16* Xb, const float* xmax2, long N, int* out) {
    if (h->tiled) return launch_bmu_bf16_tiled<E>(h, Xb, xmax2, N, out);
    // the stage image's initial accumulators depend on the row set through B = xmax * wmax; the same launch
    // resets the per-row merge keys of the 16x16x32 kernel
    long units = (long)h->n_stages * h->stage_units;
    if (int rc = h->best64.reserve(h, (size_t)N, 1024)) return rc;
    prep_wsqh_kernel<<<dim3((unsigned)cdiv(std::max(units, N), 256)), dim3(256), 0, h->stream>>>(
        h->wn, h->K, h->wmax2, xmax2, h->Wst, h->n_stages, h->stage_bytes, h->stage_units, h->best64, N);
    return for_ks32(h, "bf16 precision supports input_len <= 128",
                    [&](auto k) { return launch_bmu_bf16_k16<decltype(k)::value, E>(h, Xb, N, out); });
}

int launch_bmu_bf16(som_handle* h, const Rows& r) {
    return SOM_HALF(h, launch_bmu_half, h, r.Xb, r.xmax2, r.N, r.out);
}

// the exact mode's rows -> half operand image, max |x|^2 and the rows' measured rounding errors.  The set's xsq holds the rows'
// |x|^2 in NumPy's order (the caller's row_sq); its second half takes the errors (RowSet::xerr)
int prep_rows_exact(som_handle* h, RowSet& s) {
    const float* X = s.X; const long N = s.N, Np = round_up(N, ROW_PAD);
    __bf16* Xb = s.Xb; float* xmax2 = s.xmax2; float* xsq_scratch = s.xsq; float* xerr = s.xerr();
    HIPCHK(h, hipMemsetAsync(xmax2, 0, sizeof(float), h->stream));
    if (!xerr && N > 0) return fail(h, "exact: no row norms");
    if (h->tiled) {
        // beyond 128 features: the tile image; cosine: the rows go in at unit length
        const bool unit = h->cfg.distance == SOM_DIST_COSINE;
        const float* usq = unit ? xsq_scratch : nullptr;
        if (unit) HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)xmax2, 0x3F800000, 1, h->stream));   // unit-length rows: max |x| = 1
        else if (N > 0) exact_max_kernel<<<dim3((unsigned)std::min<long>(cdiv(N, 256), 512)), dim3(256), 0, h->stream>>>(xsq_scratch, N, xmax2);
        const long n_blocks = Np / h->tl_bm;
        const long total = n_blocks * h->n_kchunks * (h->tl_bm / 16) * TL_KS * 64;
        prep_tiles_bf16_kernel<ExactEl><<<dim3((unsigned)cdiv(total, 256)), dim3(256), 0, h->stream>>>(
            X, N, h->D, h->n_kchunks, n_blocks, h->tl_bm, h->tl_xtile, 1.0f, usq, (char*)Xb, xmax2);
        if (N > 0) exact_rowerr_kernel<ExactEl><<<dim3((unsigned)cdiv(N, 4)), dim3(256), 0, h->stream>>>(X, N, h->D, usq, xmax2, xerr);
        HIPCHK(h, hipGetLastError());
        return 0;
    }
    // up to 128 features: max |x|^2 from the rows' float32 norms, then the rows scaled by ex_scale of it
    if (N > 0) exact_max_kernel<<<dim3((unsigned)std::min<long>(cdiv(N, 256), 512)), dim3(256), 0, h->stream>>>(xsq_scratch, N, xmax2);
    prep_x_bf16_kernel<ExactEl><<<dim3((unsigned)cdiv(Np, 4)), dim3(256), 0, h->stream>>>(X, N, h->D, h->dp, Np, Xb, nullptr, 0, xmax2, xerr);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// precisions 'bf16' and 'f16': rows -> 16-bit operand image (+ max |x~|^2 for the offset B).  Cosine: the rows go in at unit
// length -- the argmin does not depend on |x|, and B = max|x~| max|w~| then resolves every row alike (a short row next to
// long ones would otherwise be compared at B's absolute precision).  The set's xsq is scratch here: N floats, cosine + tiled only.
template <class E>
int prep_rows_half(som_handle* h, RowSet& s) {
    const float* X = s.X; const long N = s.N, Np = round_up(N, ROW_PAD);
    __bf16* Xb = s.Xb; float* xmax2 = s.xmax2; float* xsq_scratch = s.xsq;
    const bool unit = h->cfg.distance == SOM_DIST_COSINE;
    HIPCHK(h, hipMemsetAsync(xmax2, 0, sizeof(float), h->stream));
    if (h->tiled) {
        const float* usq = nullptr;
        if (unit && N > 0) {
            if (!xsq_scratch) return fail(h, "prep_rows_half: no row-norm scratch");
            row_sq_f32_kernel<<<dim3((unsigned)cdiv(N, 256)), dim3(256), 0, h->stream>>>(X, N, h->D, xsq_scratch);
            usq = xsq_scratch;
        }
        long n_blocks = Np / h->tl_bm;
        long total = n_blocks * h->n_kchunks * (h->tl_bm / 16) * TL_KS * 64;
        prep_tiles_bf16_kernel<E><<<dim3((unsigned)cdiv(total, 256)), dim3(256), 0, h->stream>>>(
            X, N, h->D, h->n_kchunks, n_blocks, h->tl_bm, h->tl_xtile, 1.0f, usq, (char*)Xb);
        if (N > 0)
            rownorm_bf16_kernel<E><<<dim3((unsigned)cdiv(N, 4)), dim3(256), 0, h->stream>>>(X, N, h->D, usq, 0, nullptr, xmax2);
        HIPCHK(h, hipGetLastError());
        return 0;
    }
    prep_x_bf16_kernel<E><<<dim3((unsigned)cdiv(Np, 4)), dim3(256), 0, h->stream>>>(X, N, h->D, h->dp, Np, Xb, xmax2, unit ? 1 : 0);
    HIPCHK(h, hipGetLastError());
    return 0;
}

bool needs_xsq(const som_handle* h) {
    if (h->exact) return true;                          // |x_n| scales the row's error bound (bmu_exact.hpp)
    return h->cfg.precision == SOM_PREC_F32 &&
           (h->cfg.distance == SOM_DIST_EUCLIDEAN_NO_OPT || h->cfg.distance == SOM_DIST_COSINE);
}

int row_sq(som_handle* h, const float* X, long N, float* out) {
    if (N == 0) return 0;
    row_sq_f32_kernel<<<dim3((unsigned)cdiv(N, 256)), dim3(256), 0, h->stream>>>(X, N, h->D, out);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// what a search reads besides the set's float32 rows: |x|^2 where the caller wants it, the 16-bit operand image (with max |x~|^2
// and, exact mode, the rows' measured errors) unless the precision is f32.  The one place that prepares a row set.
int prepare(som_handle* h, RowSet& s, bool want_xsq) {
    if (s.N == 0) return 0;
    if (want_xsq) if (int rc = row_sq(h, s.X, s.N, s.xsq)) return rc;
    if (h->cfg.precision == SOM_PREC_F32) return 0;
    return h->exact ? prep_rows_exact(h, s) : SOM_HALF(h, prep_rows_half, h, s);
}

// precision 'bf16' or 'f16': 16-bit operands and no float32 re-score (as opposed to 'exact', whose screen reads them too)
inline bool is_half1(const som_handle* h) { return h->cfg.precision == SOM_PREC_BF16 || h->cfg.precision == SOM_PREC_F16; }

template <class E>
int merge_prep_half(som_handle* h) {
    HIPCHK(h, hipMemsetAsync(h->wmax2, 0, sizeof(float), h->stream));
    if (h->wide) {
        merge_prep_wide_kernel<E><<<dim3((unsigned)(h->n_stages * WD_T)), dim3(256), 0, h->stream>>>(
            h->W, h->ACC, h->K, h->D, h->D1p, h->n_kchunks, h->Wst, h->wn, h->wmax2, h->cfg.distance == SOM_DIST_COSINE);
        return 0;
    }
    const long n_tiles = (long)h->n_stages * K16_T;
    const dim3 grid((unsigned)cdiv(n_tiles, MP_TILES));
    switch (h->ks32) {
    case 1: merge_prep_k16_kernel<1, E><<<grid, dim3(64), 0, h->stream>>>(h->W, h->ACC, h->K, h->D, h->D1p, h->Wst, h->wn, h->wmax2, n_tiles); break;
    case 2: merge_prep_k16_kernel<2, E><<<grid, dim3(128), 0, h->stream>>>(h->W, h->ACC, h->K, h->D, h->D1p, h->Wst, h->wn, h->wmax2, n_tiles); break;
    case 3: merge_prep_k16_kernel<3, E><<<grid, dim3(192), 0, h->stream>>>(h->W, h->ACC, h->K, h->D, h->D1p, h->Wst, h->wn, h->wmax2, n_tiles); break;
    case 4: merge_prep_k16_kernel<4, E><<<grid, dim3(256), 0, h->stream>>>(h->W, h->ACC, h->K, h->D, h->D1p, h->Wst, h->wn, h->wmax2, n_tiles); break;
    default: return fail(h, "the resident half-precision kernel supports input_len <= 128");
    }
    return 0;
}

int launch_bmu_pairwise(som_handle* h, const float* X, long N, int p, bool even, int* out) {
    const double pr = h->norm_pr;                        // (a real exponent: the generic form, whatever `even` says)
    if (pr != 0.0) even = false;
    size_t w_bytes = (size_t)PW_UNITS * h->D * sizeof(float);
    size_t x_bytes = (size_t)PW_SAMPLES * (h->D + 1) * sizeof(float);
    int x_in_lds = w_bytes + x_bytes <= 150 * 1024;
    size_t lds = w_bytes + (x_in_lds ? x_bytes : 0);
    if (lds > 150 * 1024) return fail(h, "pairwise distance: input_len too large for the LDS unit tile");
    long grid = cdiv(N, PW_SAMPLES);
    if (grid <= 0 || grid > 0x7fffffffL) return fail(h, "bmu_pairwise: row count out of range");
    if (even) {
        { int pc; if (int rc = kernel_per_cu(h, (const void*)bmu_pairwise_kernel<PW_EVEN>, PW_SAMPLES, lds, &pc)) return rc; }
        bmu_pairwise_kernel<PW_EVEN><<<dim3((unsigned)grid), dim3(PW_SAMPLES), lds, h->stream>>>(X, N, h->D, h->W, h->K, p, x_in_lds, out);
    } else {
        { int pc; if (int rc = kernel_per_cu(h, (const void*)bmu_pairwise_kernel<PW_GENERIC>, PW_SAMPLES, lds, &pc)) return rc; }
        bmu_pairwise_kernel<PW_GENERIC><<<dim3((unsigned)grid), dim3(PW_SAMPLES), lds, h->stream>>>(X, N, h->D, h->W, h->K, p, x_in_lds, out, pr);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ---- the sort by unit (unit_sort.hpp: the rule; update.hpp: the kernels) ----------------------------------------------------
// The stable radix sort of update.hpp: (keys_in, row index) -> (keys_out, vals_out), `bits` key bits, 8 a pass.  scratch: two
// pairs of n ints + the 256 x blocks table (radix_scratch_ints).  keys_in is left intact.
int radix_sort_rows(som_handle* h, const int* keys_in, long n, int bits, int* keys_out, int* vals_out, int* scratch) {
    if (n <= 0) return 0;
    const int B = (int)cdiv(n, RS_BLOCK);
    int* ka = scratch; int* va = scratch + n; int* kb = scratch + 2 * n; int* vb = scratch + 3 * n;
    int* table = scratch + 4 * n;
    int* tot = table + 256L * B;
    const int passes = std::max(1, (int)cdiv(bits, 8));
    const int* kin = keys_in; const int* vin = nullptr;
    for (int p = 0; p < passes; ++p) {
        const bool last = p == passes - 1;
        int* ko = last ? keys_out : (p & 1) ? kb : ka;
        int* vo = last ? vals_out : (p & 1) ? vb : va;
        rs_hist_kernel<<<dim3((unsigned)B), dim3(256), 0, h->stream>>>(kin, n, 8 * p, B, table);
        rs_scan_kernel<<<dim3(64), dim3(256), 0, h->stream>>>(table, B, tot);
        rs_scatter_kernel<<<dim3((unsigned)B), dim3(256), 0, h->stream>>>(kin, vin, n, 8 * p, B, table, tot, ko, vo);
        kin = ko; vin = vo;
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

// the buffers for up to `rows` rows, as unitsort::sizes says: they only grow (free first, then allocate)
int reserve(som_handle* h, UnitSort& u, long rows) {
    if (rows <= u.cap) return 0;
    u.skey.reset(); u.srow.reset(); u.tmp.reset(); u.cs_table.reset(); u.cs_blocks = 0; u.cap = 0;
    if (rows > 0x7fffffffL) return fail(h, "more than 2^31-1 rows per GPU in one row set");   // (the sort holds row indices as ints)
    const unitsort::Sizes z = unitsort::sizes(rows, h->K, h->counting_sort);
    if (int rc = u.skey.alloc(h, z.skey)) return rc;
    if (int rc = u.srow.alloc(h, z.srow)) return rc;
    if (int rc = u.tmp.alloc(h, z.scratch)) return rc;
    if (z.table) if (int rc = u.cs_table.alloc(h, z.table)) return rc;
    u.cs_blocks = z.cs_blocks;
    u.cap = rows;
    return 0;
}

// (skey, srow) = the N rows sorted by their unit `bmu`, rows ascending inside a unit (stable): the counting sort where
// unitsort::counting says so -- the table is held, the rows fit it and fill two blocks --, else the radix sort
int sort_rows_by_unit(som_handle* h, UnitSort& u, const int* bmu, long N) {
    if (N <= 0) return 0;
    const int bits = unitsort::key_bits(h->K);
    if (!unitsort::counting(u.cs_blocks, N)) {
        h->sorts_radix += 1;
        return radix_sort_rows(h, bmu, N, bits, u.skey, u.srow, u.tmp);
    }
    // few units: a stable counting sort in three launches (same order as the radix sort: unit, then row)
    const int B = (int)cdiv(N, CS_BLOCK);
    int* tot = u.cs_table + (long)B * h->K;             // (the totals behind THESE rows' blocks, not behind the table's)
    const size_t lds = (size_t)h->K * sizeof(int);
    cs_hist_kernel<<<dim3((unsigned)B), dim3(256), lds, h->stream>>>(bmu, N, h->K, B, u.cs_table);
    cs_scan_kernel<<<dim3((unsigned)cdiv(h->K, 4)), dim3(256), 0, h->stream>>>(u.cs_table, h->K, B, tot);
    cs_scatter_kernel<<<dim3((unsigned)B), dim3(CS_BLOCK), lds, h->stream>>>(bmu, N, h->K, B, bits, u.cs_table, tot, u.skey, u.srow);
    HIPCHK(h, hipGetLastError());
    h->sorts_counting += 1;
    return 0;
}

#include "exact_host.hpp"   // launch_bmu_exact and everything it drives (precision 'exact'): same translation unit

// ---- canary: re-score a strided sample of a BMU launch's rows with the float32 kernel (bmu_exact.hpp) -------------
int verify_bmu_launch(som_handle* h, const Rows& r) {
    const int n = (int)std::min<long>(h->verify_rows, r.N);
    if (n <= 0 || h->cfg.distance > SOM_DIST_COSINE) return 0;     // (the VALU distances have one precision: nothing to cross-check)
    if (h->capturing) return fail(h, "SOM_VERIFY reads a flag back per launch: not capturable");
    if (n > h->vf_cap) {
        h->vf_rows.reset(); h->vf_picks.reset(); h->vf_best.reset(); h->vf_X.reset(); h->vf_cap = 0;
        if (int rc = h->vf_rows.alloc(h, (size_t)n)) return rc;
        if (int rc = h->vf_picks.alloc(h, (size_t)n)) return rc;
        if (int rc = h->vf_best.alloc(h, (size_t)n)) return rc;
        if (int rc = h->vf_X.alloc(h, (size_t)n * h->D)) return rc;
        if (!h->vf_bad) if (int rc = h->vf_bad.alloc(h, 4)) return rc;
        h->vf_cap = n;
    }
    verify_pick_rows_kernel<<<dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream>>>(r.N, n, r.out, h->vf_rows, h->vf_picks);
    exact_gather_rows_kernel<<<dim3((unsigned)cdiv((long)n * h->D, 256)), dim3(256), 0, h->stream>>>(r.X, h->vf_rows, n, h->D, h->vf_X);
    HIPCHK(h, hipMemsetAsync(h->vf_bad, 0, 4 * sizeof(int), h->stream));
    if (const operands::Rebuilds rb = h->ops.decide_wsq(); rb.wsq) {
        launch_codebook_wsq(h);
        h->ops.commit(rb);
    }
    const dim3 grid((unsigned)n), block(256);
    const size_t lds = (size_t)h->D * sizeof(float);
    if (lds > 60 * 1024) return fail(h, "SOM_VERIFY: input_len too large for the canary's row buffer");
    switch (h->cfg.distance) {
    case SOM_DIST_EUCLIDEAN: verify_best_kernel<SCORE_EUCLID_PART><<<grid, block, lds, h->stream>>>(h->vf_X, h->D, h->W, h->wsq, h->K, h->vf_best); break;
    case SOM_DIST_EUCLIDEAN_NO_OPT: verify_best_kernel<SCORE_EUCLID_SQ><<<grid, block, lds, h->stream>>>(h->vf_X, h->D, h->W, h->wsq, h->K, h->vf_best); break;
    default: verify_best_kernel<SCORE_COSINE><<<grid, block, lds, h->stream>>>(h->vf_X, h->D, h->W, h->wsq, h->K, h->vf_best); break;
    }
    // the mode's bound on the score gap: 0 = the float32 pick itself (f32, exact); half operands: 4 ub |x||w| (two
    // units, two operands each) with a margin
    float tol = 0.0f;
    const int prec = h->cfg.precision;
    const bool cosine = h->cfg.distance == SOM_DIST_COSINE;
    if (prec == SOM_PREC_BF16) tol = 8.0f / 256.0f;
    else if (prec == SOM_PREC_F16) tol = 8.0f / 2048.0f;
    if (cosine && tol > 0.0f) tol *= 0.5f;                         // (unit-length operands: |x||w| = 1)
    verify_picks_kernel<<<dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream>>>(
        h->vf_X, n, h->D, h->W, h->wsq, h->wmax2 ? h->wmax2 : h->wsq, h->vf_rows, h->vf_picks, h->vf_best, cosine ? 1 : 0, tol, h->vf_bad);
    HIPCHK(h, hipGetLastError());
    int bad[4] = {0, 0, 0, 0};
    if (int rc2 = d2h_blocking(h, bad, h->vf_bad, sizeof(bad))) return rc2;
    h->verify_launches += 1; h->verify_rows_checked += n;
    if (bad[0] > 0) {
        char msg[256];
        std::snprintf(msg, sizeof(msg), "SOM_VERIFY: %d of %d re-scored rows carry a pick outside the precision mode's bound "
                      "(e.g. row %d: unit %d, the float32 kernel says %d)", bad[0], n, bad[1], bad[2], bad[3]);
        return fail(h, msg);
    }
    return 0;
}

// BMU of a row set's device rows with the configured activation distance (xpysom.py:410-417)
int run_activation_bmu_launch(som_handle* h, const Rows& r) {
    if (h->masked) {                                     // missing values: one kernel, no codebook operands to refresh
        Timed t(h, SOM_K_BMU);
        return launch_bmu_masked(h, r.X, r.N, r.out);
    }
    // (exact mode up to 128 features: the launch writes the codebook's 16-bit image itself, in one grid with its plan's centroid images)
    if (int rc = refresh_codebook_operands(h, operands::Request::Search, h->exact && h->ex.sw.chain)) return rc;
    Timed t(h, SOM_K_BMU);
    if (h->exact) return launch_bmu_exact(h, r);
    if (h->cfg.precision != SOM_PREC_F32) return launch_bmu_bf16(h, r);
    switch (h->cfg.distance) {
    case SOM_DIST_EUCLIDEAN: return launch_bmu_f32_any<SCORE_EUCLID_PART>(h, r.X, r.N, r.xsq, r.out);
    case SOM_DIST_EUCLIDEAN_NO_OPT: return launch_bmu_f32_any<SCORE_EUCLID_SQ>(h, r.X, r.N, r.xsq, r.out);
    case SOM_DIST_COSINE: return launch_bmu_f32_any<SCORE_COSINE>(h, r.X, r.N, r.xsq, r.out);
    case SOM_DIST_MANHATTAN: return launch_bmu_pairwise(h, r.X, r.N, 1, false, r.out);
    case SOM_DIST_NORM_P_NO_OPT: return launch_bmu_pairwise(h, r.X, r.N, h->norm_p, false, r.out);
    case SOM_DIST_NORM_P: return launch_bmu_pairwise(h, r.X, r.N, h->norm_p, h->norm_p % 2 == 0, r.out);
    }
    return fail(h, "unknown distance id");
}

int run_activation_bmu(som_handle* h, const Rows& r) {
    if (r.N == 0) return 0;
    if (int rc = run_activation_bmu_launch(h, r)) return rc;
    if (r.resident) h->res.ids_valid = true;              // (the next epoch's exact screen seeds its thresholds from these ids)
    if (h->verify_rows > 0 && !h->verifying) return verify_bmu_launch(h, r);
    return 0;
}

// `s`'s buffers for n rows, by the size rule of row_set.hpp: a transient set only grows (free first, then allocate), the resident set is
// rebuilt, cap == N, for every row set the handle adopts.  with_rows: host rows will be staged through the set's own float32 buffer
int reserve(som_handle* h, RowSet& s, long n, bool with_rows) {
    const rowset::Sizes z = rowset::sizes(s.kind, n, h->D, h->dp, rowset::Flags{h->cfg.precision == SOM_PREC_F32, h->exact, needs_xsq(h),
                                                                                h->cfg.distance == SOM_DIST_COSINE && h->tiled});
    if (with_rows) if (int rc = s.resident() ? s.X_owned.alloc(h, z.X) : s.X_owned.reserve(h, z.X)) return rc;
    if (!s.resident() && n <= s.cap) return 0;
    s.bmu.reset(); s.bmu2.reset(); s.xsq.reset(); s.Xb.reset(); s.cap = 0;
    if (s.kind == rowset::Kind::Slot) s.wgt_owned.reset();
    if (int rc = s.bmu.alloc(h, z.ids)) return rc;
    if (s.kind == rowset::Kind::Query) if (int rc = s.bmu2.alloc(h, z.ids)) return rc;
    if (z.xsq) if (int rc = s.xsq.alloc(h, z.xsq)) return rc;
    if (z.Xb) if (int rc = s.Xb.alloc(h, z.Xb)) return rc;
    s.cap = z.cap;
    return 0;
}

// ---- update path: segment sum + separable neighbourhood transform --------------------------
// SC[b] += sum of the rows whose BMU is b (and their count): sort by BMU, chunked register sums
// scratch for the segment sum of up to `rows` rows (sort buffers + the partial lists of levels 1 and 2;
// level 3 reuses level 1's, and so on)
int seg_reserve(som_handle* h, som_handle::SegScratch& sg, long rows) {
    if (rows <= sg.sort.cap) return 0;
    sg.kA.reset(); sg.vA.reset(); sg.kB.reset(); sg.vB.reset();
    const int nw = seg_waves_per_block(h->D1p);
    const long n1 = seg_next_entries(rows, SEG_CHUNK, nw), n2 = seg_next_entries(n1, SEG_CHUNK_UP, nw);
    int rc = reserve(h, sg.sort, rows);
    if (!rc) rc = sg.kA.alloc(h, (size_t)n1);
    if (!rc) rc = sg.vA.alloc(h, (size_t)n1 * h->D1p);
    if (!rc) rc = sg.kB.alloc(h, (size_t)n2);
    if (!rc) rc = sg.vB.alloc(h, (size_t)n2 * h->D1p);
    if (rc) sg = som_handle::SegScratch{};               // (refused part of the way: nothing half allocated is used, the next call tries again)
    return rc;
}

// one level of the run sum over n entries; returns the number of workgroups it used
template <bool LEVEL0>
long launch_runsum(som_handle* h, const float* X, const int* keys, const int* srow, const float* vin, long n,
                   int accumulate, int* kout, float* vout, const float* wgt = nullptr) {
    const int nw = seg_waves_per_block(h->D1p);
    const int chunk = LEVEL0 ? SEG_CHUNK : seg_chunk_up(n, nw);
    const long blocks = cdiv(n, (long)nw * chunk);
    const dim3 grid((unsigned)blocks), block(64 * nw);
    const size_t lds = nw > 1 ? (size_t)2 * nw * (h->D1p + 1) * sizeof(float) : 0;
    if constexpr (LEVEL0) {
        if (h->masked) {                                 // missing values: the masked instances of level 0, with or without weights
            const bool v2 = (h->D & 1) == 0;
#define SOM_RUNSUM_MASKED(V, WG) runsum_kernel<true, V, WG, true><<<grid, block, lds, h->stream>>>(X, keys, srow, vin, n, chunk, h->D, h->D1p, accumulate, h->SC, h->SC + (size_t)h->K * h->D1p, kout, vout, wgt)
            if (wgt != nullptr) { if (v2) SOM_RUNSUM_MASKED(true, true); else SOM_RUNSUM_MASKED(false, true); }
            else { if (v2) SOM_RUNSUM_MASKED(true, false); else SOM_RUNSUM_MASKED(false, false); }
#undef SOM_RUNSUM_MASKED
            return blocks;
        }
        if (wgt != nullptr) {                            // sample weights: the weighted instances of level 0
            if ((h->D & 1) == 0)
                runsum_kernel<true, true, true><<<grid, block, lds, h->stream>>>(X, keys, srow, vin, n, chunk, h->D, h->D1p, accumulate, h->SC, h->SC + (size_t)h->K * h->D1p, kout, vout, wgt);
            else
                runsum_kernel<true, false, true><<<grid, block, lds, h->stream>>>(X, keys, srow, vin, n, chunk, h->D, h->D1p, accumulate, h->SC, h->SC + (size_t)h->K * h->D1p, kout, vout, wgt);
            return blocks;
        }
    }
    // (UD: D, or -- the upper levels of a masked handle -- the 2 * D features of its lists)
    if ((h->UD & 1) == 0)
        runsum_kernel<LEVEL0, true><<<grid, block, lds, h->stream>>>(X, keys, srow, vin, n, chunk, h->UD, h->D1p, accumulate, h->SC, h->SC + (size_t)h->K * h->D1p, kout, vout);
    else
        runsum_kernel<LEVEL0, false><<<grid, block, lds, h->stream>>>(X, keys, srow, vin, n, chunk, h->UD, h->D1p, accumulate, h->SC, h->SC + (size_t)h->K * h->D1p, kout, vout);
    return blocks;
}

// SC[b] += sum of the rows whose BMU is b (and their count): sort by BMU, then the levels of update.hpp's
// run sum (rows -> partial lists) until one workgroup holds the whole list.  zero_first: SC starts from zero and
// every unit is written once (plain stores); otherwise the chunk's sums are added to what SC holds.
// r.wgt != nullptr: the sample weights of these N rows (device, indexed like X's rows): SC[b] = sum of w_n x_n, count = sum of w_n.
int segsum_rows(som_handle* h, const Rows& r, som_handle::SegScratch& sg, bool zero_first) {
    const float* X = r.X; const int* bmu = r.out; const long N = r.N;
    Timed t(h, SOM_K_SEGSUM);
    if (zero_first && !(h->early.done && r.resident))   // (exact mode: already zeroed before the pass's read-back)
        HIPCHK(h, hipMemsetAsync(h->SC, 0, (size_t)h->K * (h->D1p + 1) * sizeof(float), h->stream));
    if (N > 0) {
        if (N > sg.sort.cap) return fail(h, "segment sum: scratch smaller than the row set");
        if (int rc = sort_rows_by_unit(h, sg.sort, bmu, N)) return rc;
        const int acc = zero_first ? 0 : 1;
        long blocks = launch_runsum<true>(h, X, sg.sort.skey, sg.sort.srow, nullptr, N, acc, sg.kA, sg.vA, r.wgt);
        int *kin = sg.kA, *kout = sg.kB;
        float *vin = sg.vA, *vout = sg.vB;
        while (blocks > 1) {                             // 2 * blocks entries are waiting in (kin, vin)
            blocks = launch_runsum<false>(h, nullptr, kin, nullptr, vin, 2 * blocks, acc, kout, vout);
            std::swap(kin, kout);
            std::swap(vin, vout);
        }
        HIPCHK(h, hipGetLastError());
    }
    return 0;
}

int run_transform(som_handle* h, double sigma, double eta, int neigh_f64);

NeighParams make_neigh_params(const som_handle* h, double sigma, double eta, int neigh_f64) {
    NeighParams p{};
    p.sigma = sigma; p.eta = eta;
    p.d = 2.0 * (h->cfg.std_coeff * h->cfg.std_coeff) * (sigma * sigma);
    p.kind = h->cfg.neighborhood; p.compact = h->cfg.compact_support; p.wide = neigh_f64 ? 1 : 0;
    // the reference's triangle is float64 whatever sigma's type (int64 - |...| + sigma, neighborhoods.py:121-122)
    if (p.kind == SOM_NEIGH_TRIANGLE) p.wide = 1;
    p.X = h->X; p.Y = h->Y; p.nt = h->nt;
    p.hex = h->cfg.topology == SOM_TOPO_HEXAGONAL && h->cfg.neighborhood != SOM_NEIGH_BUBBLE;
    p.ncls = !p.hex ? 1 : h->cfg.compact_support ? 4 : 3;
    p.base_nt = h->nt / p.ncls;
    p.swapped = h->swapped ? 1 : 0;
    p.torus = h->torus ? 1 : 0;
    return p;
}

int run_update(som_handle* h, double sigma, double eta, int neigh_f64) {
    if (int rc = segsum_rows(h, h->res.view(), h->seg, true)) return rc;
    return run_transform(h, sigma, eta, neigh_f64);
}

// [num|den] = sum_t (Px_t (x) Py_t) [S|c]
// the factor tables of this epoch's neighbourhood, and (in the same launch) their nonzero bands: the kernel fills one
// of the two range buffers and zeroes the other, and the buffers change roles from build to build.  A captured launch
// reads the role from np_dev, where som_epoch_accumulate puts the next one before every replay.
int build_tables(som_handle* h, double sigma, double eta, int neigh_f64, hipStream_t st) {
    NeighParams p = make_neigh_params(h, sigma, eta, neigh_f64);
    if (!h->capturing) h->band_sel ^= 1;
    p.rsel = h->band_sel;
    // (late epochs: most of Px, Py is exact zeros; SOM_NO_BANDS=1 records nothing and walks everything)
    neigh_tables_kernel<<<dim3((unsigned)neigh_tables_grid(h->X, h->Y, h->nt, p.swapped)), dim3(NT_THREADS), 0, st>>>(
        p, h->capturing ? (const NeighParams*)h->np_dev : nullptr, h->P1, h->P2, h->use_bands ? (int2*)h->bands : nullptr);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// the ranges of the tables' last build from entry `first` on (update.hpp: band_entry_stage1 / band_entry_stage2)
BandRanges band_ranges_from(const som_handle* h, long first) {
    BandRanges br{};
    if (!h->use_bands || h->swapped) return br;
    const int pieces = h->torus ? 2 : 1;                 // toroidal: an entry per piece of a segment (update.hpp, band_wrap_mid)
    br.base = (const int2*)h->bands + first * pieces;
    br.p_dev = h->capturing ? (const NeighParams*)h->np_dev : nullptr;
    br.stride = band_entries(h->X, h->Y, h->nt) * pieces;
    br.sel = h->band_sel;
    return br;
}

// OUT = H * M over C columns (rows of M / OUT ld floats apart): 128-wide MFMA tiles, and a VALU kernel for a last
// tile of <= LM_NARROW columns.  row_blocks: the 128-row blocks of H.
// A toroidal handle's ranges come in pairs (update.hpp, band_wrap_mid): its MFMA tiles go to leftmul_wrap_f32_kernel, and
// its narrow last tile walks everything (the VALU kernel knows one range per tile; skipped columns add exact zeros, so
// the result is the same, and no map of the flagship kind -- input_len a multiple of 128 -- has a narrow tile).
void launch_leftmul(som_handle* h, const float* H, int Ro, int Ri, const float* M, long mstride, float* OUT, long ostride,
                    long C, long ld, int row_blocks, int batch, const BandRanges& ranges, int nseg, int segw, long ldo = 0) {
    if (ldo == 0) ldo = ld;                              // rows of OUT as far apart as rows of M unless told otherwise
    long wide = cdiv(C, LM_BN);
    const long rem = C - (C / LM_BN) * LM_BN;
    if (rem > 0 && rem <= LM_NARROW) {
        --wide;
        const dim3 g(1, (unsigned)row_blocks, (unsigned)batch), b(256);
        const BandRanges nr = h->torus ? BandRanges{} : ranges;
        if (rem <= 4) leftmul_narrow_f32_kernel<2><<<g, b, 0, h->stream>>>(H, Ro, Ri, M, mstride, OUT, ostride, C, ld, ldo, C - rem, nr, nseg, segw);
        else leftmul_narrow_f32_kernel<4><<<g, b, 0, h->stream>>>(H, Ro, Ri, M, mstride, OUT, ostride, C, ld, ldo, C - rem, nr, nseg, segw);
    }
    if (wide <= 0) return;
    // 64-row tiles where 128-row ones would be half empty (64 x 64 x 32: transform 34.6 -> 26.6 us), and wherever the
    // launch walks bands: a 64-row workgroup stages the union of two 32-row tiles' ranges, not of four, so staging and
    // barriers shrink with the band as the MFMAs do (256 x 256 x 128, sigma 1.2: 21 us a launch against 25; on dense
    // tables the two were measured neutral at that shape, 49 us both).  Without ranges: the 128-row tile as before.
    const bool rows64 = h->lm_rows == 64 || (h->lm_rows == 0 && (Ro <= 64 || ranges.base != nullptr));
    if (h->torus && ranges.base != nullptr) {
        if (rows64)
            leftmul_wrap_f32_kernel<64><<<dim3((unsigned)wide, (unsigned)cdiv(Ro, 64), (unsigned)batch), dim3(256), 0, h->stream>>>(
                H, Ro, Ri, M, mstride, OUT, ostride, C, ld, ldo, ranges, nseg, segw);
        else
            leftmul_wrap_f32_kernel<128><<<dim3((unsigned)wide, (unsigned)row_blocks, (unsigned)batch), dim3(256), 0, h->stream>>>(
                H, Ro, Ri, M, mstride, OUT, ostride, C, ld, ldo, ranges, nseg, segw);
    } else if (rows64)
        leftmul_f32_kernel<64><<<dim3((unsigned)wide, (unsigned)cdiv(Ro, 64), (unsigned)batch), dim3(256), 0, h->stream>>>(
            H, Ro, Ri, M, mstride, OUT, ostride, C, ld, ldo, ranges, nseg, segw);
    else
        leftmul_f32_kernel<128><<<dim3((unsigned)wide, (unsigned)row_blocks, (unsigned)batch), dim3(256), 0, h->stream>>>(
            H, Ro, Ri, M, mstride, OUT, ostride, C, ld, ldo, ranges, nseg, segw);
}

// tables + stage 1: T_t[a] = Py_t (Y x Y) * SC[a] (Y x D), batched
// over the X map rows; the count column goes its own way: U_t = C Py_t^T (X x Y, update.hpp)
int run_transform_stage1(som_handle* h, double sigma, double eta, int neigh_f64) {
    // (built on this stream: handing them to a side stream under the BMU kernel was measured -- the two event
    //  waits cost more than the 7 us kernel, epoch 1.058 vs 1.035 ms at 65 536 rows)
    if (!h->early.done)                                  // (exact mode: built before the pass's read-back)
        if (int rc = build_tables(h, sigma, eta, neigh_f64, h->stream)) return rc;
    const int nyb = (int)cdiv(h->Y, LM_BM);
    const long slab = (long)h->Y * h->D1p;
    if (h->swapped) {
        // mexican_hat + compact_support, rectangular (X == Y): the row stage first, V_t = Fx_t (X x X) * SC (X x Y*D1p),
        // laid out T[i][t][b][:] (rows of term t: T + t*slab, nt*slab apart); then the reference's second mask,
        // m2(i, b), on terms 0 and 1 and its complement on term 3 (update.hpp, neigh_factor); the column stage follows in run_transform_stage2
        const int nxb = (int)cdiv(h->X, LM_BM);
        for (int t1 = 0; t1 < h->nt; ++t1)
            launch_leftmul(h, h->P1 + (long)t1 * h->X * h->X, h->X, h->X, h->SC, 0, h->T + (long)t1 * slab, 0, slab, slab, nxb,
                           1, BandRanges{}, 1, h->X, (long)h->nt * slab);
        const NeighParams p = make_neigh_params(h, sigma, eta, neigh_f64);
        const long total = (long)h->X * h->nt * slab;
        mask_rows_kernel<<<dim3((unsigned)cdiv(total, 256)), dim3(256), 0, h->stream>>>(
            p, h->capturing ? (const NeighParams*)h->np_dev : nullptr, h->T, h->D1p);
        HIPCHK(h, hipGetLastError());
        return 0;
    }
    for (int t1 = 0; t1 < h->nt; ++t1)
        launch_leftmul(h, h->P1 + (long)t1 * h->Y * h->Y, h->Y, h->Y, h->SC, slab, h->T + (long)t1 * h->X * slab, slab,
                       h->UD, h->D1p, nyb, h->X, band_ranges_from(h, band_entry_stage1(t1, 0, h->Y)), 1, h->Y);
    // U_t[a][j] = sum_b C[a][b] Py_t[j][b] from the dense counts; stage 2 reads it densely (Ud) when it batches over
    // the map columns, or finds it where stage 1 would have put it, T_t[a][j][D], when it runs over whole rows
    const bool per_column = h->UD % LM_BN == 0;
    strided_gemm_f32_kernel<<<dim3((unsigned)cdiv(h->Y, SG_T), (unsigned)cdiv(h->X, SG_T), (unsigned)h->nt), dim3(256), 0, h->stream>>>(
        h->SC + (size_t)h->K * h->D1p, h->Y, 1, h->P1, 1, h->Y, per_column ? h->Ud : h->T + h->UD, per_column ? h->Y : slab,
        per_column ? 1 : h->D1p, h->X, h->Y, h->Y, 0, (long)h->Y * h->Y, per_column ? (long)h->K : (long)h->X * slab);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// stage 2 for the map-row blocks [b0, b1) of LM_BM rows: ACC = [Px_0 | Px_1 ...] (X x nt*X) * T (nt*X x Y*D1p).
// input_len a multiple of the 128-column tile: batched over the Y map columns, one exact tile set per (j, features)
// -- 256 x 2 workgroups at 256 x 256 x 128, one round of the resident slots, where 132-float rows cut into 128-wide
// tiles made 264 x 2 -- and the count column through the strided kernel.  Otherwise: over the whole Y*D1p-wide rows.
int run_transform_stage2(som_handle* h, int b0, int b1) {
    const int nyb = (int)cdiv(h->Y, LM_BM), nxb = (int)cdiv(h->X, LM_BM);
    if (b0 < 0 || b1 > nxb || b0 >= b1) return fail(h, "transform: map-row block out of range");
    const long slab = (long)h->Y * h->D1p;
    const long i0 = (long)b0 * LM_BM;
    const int rows = (int)std::min<long>((long)b1 * LM_BM, h->X) - (int)i0;
    if (h->swapped) {
        // the column stage, batched over the block's map rows: ACC[i] = [Gy_0 | Gy_1 ...] (Y x nt*Y) * T[i] (nt*Y x D1p)
        launch_leftmul(h, h->P2, h->Y, h->nt * h->Y, h->T + i0 * h->nt * slab, (long)h->nt * slab, h->ACC + i0 * slab, slab,
                       h->D1p, h->D1p, nyb, rows, BandRanges{}, 1, h->nt * h->Y);
        HIPCHK(h, hipGetLastError());
        return 0;
    }
    const float* H = h->P2 + i0 * h->nt * h->X;
    const BandRanges ranges = band_ranges_from(h, band_entry_stage2((int)i0, 0, h->Y, h->nt));   // the block's first 32-row tile
    if (h->UD % LM_BN == 0) {
        launch_leftmul(h, H, rows, h->nt * h->X, h->T, h->D1p, h->ACC + i0 * slab, h->D1p, h->UD, slab, b1 - b0, h->Y, ranges,
                       h->nt, h->X);
        // den[i][j] = sum_k [Px_0 | Px_1 ...][i][k] U[k][j], U = [U_0; U_1; ...] dense (stage 1)
        strided_gemm_f32_kernel<<<dim3((unsigned)cdiv(h->Y, SG_T), (unsigned)cdiv(rows, SG_T), 1), dim3(256), 0, h->stream>>>(
            H, (long)h->nt * h->X, 1, h->Ud, h->Y, 1, h->ACC + i0 * slab + h->UD, slab, h->D1p, rows, h->Y, h->nt * h->X, 0, 0, 0);
    } else {
        launch_leftmul(h, H, rows, h->nt * h->X, h->T, 0, h->ACC + i0 * slab, 0, slab, slab, b1 - b0, 1, ranges, h->nt, h->X);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

int run_transform(som_handle* h, double sigma, double eta, int neigh_f64) {
    Timed t(h, SOM_K_KRON);
    if (int rc = run_transform_stage1(h, sigma, eta, neigh_f64)) return rc;
    return run_transform_stage2(h, 0, (int)cdiv(h->X, LM_BM));
}

// `s` takes the n rows at x, without weights: host rows staged through its own buffer, or the caller's device rows read where they are
int take_rows(som_handle* h, RowSet& s, const void* x, long n, bool host) {
    s.X = nullptr; s.N = 0; s.wgt = nullptr;
    if (int rc = reserve(h, s, n, host)) return rc;
    if (host && n > 0) if (int rc = h2d_blocking(h, s.X_owned, x, (size_t)n * h->D * sizeof(float))) return rc;
    s.X = host ? (const float*)s.X_owned : (const float*)x; s.N = n;
    return 0;
}
int query_rows(som_handle* h, const float* x_host, const void* x_dev, long n) {
    return take_rows(h, h->q, x_host ? (const void*)x_host : x_dev, n, x_host != nullptr);
}

#include "exact_top2_host.hpp"   // launch_top2_exact (precision 'exact', top-2): same translation unit

template <int MODE>
int launch_dist_matrix(som_handle* h, long N, float* out) {
    const int Dp = (int)round_up(h->D, F32_KC);
    size_t lds = (size_t)(F32_UB * (F32_KC + 1) + F32_UB + F32_SB * (F32_KC + 1)) * sizeof(float);
    dim3 grid((unsigned)cdiv(N, F32_SB), (unsigned)cdiv(h->K, F32_UB));
    dist_matrix_f32_kernel<MODE><<<grid, dim3(256), lds, h->stream>>>(h->q.X, N, h->D, Dp, h->W, h->wsq, h->K, h->q.xsq, out);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// the density scan (density.hpp) over the query set's rows: its geometry from the kernel's resident slots (density_plan)
template <int R>
int launch_unit_density(som_handle* h, const RowSet& q, int forced_slabs, const DensityRadii& rad, int n_radii) {
    auto& g = h->den;
    int per_cu = 1;
    if (int rc = kernel_per_cu(h, (const void*)unit_density_f32_kernel<R>, 256, DEN_LDS_BYTES, &per_cu)) return rc;
    const DensityPlan p = density_plan(q.N, h->K, resident_slots(h, per_cu), forced_slabs);
    if (p.unit_tiles * p.slabs > 0x7fffffffL) return fail(h, "unit density: the grid exceeds 2^31-1 workgroups");
    unit_density_f32_kernel<R><<<dim3((unsigned)(p.unit_tiles * p.slabs)), dim3(256), DEN_LDS_BYTES, h->stream>>>(
        q.X, q.N, h->D, (int)round_up(h->D, F32_KC), g.pivot, q.xsq, g.Wc, g.wsq, h->K, (int)p.unit_tiles, p.row_tiles, p.per, rad, n_radii,
        g.counts);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// the k nearest units (topk.hpp) of the pass's rows X[N][D] (xsq: their |x|^2, read unless the score is the Euclidean part): the scan
// over `parts` codebook parts into the partial lists, the merge into g.ids (and g.score where the caller wants the scores).  Its
// geometry from the kernel's resident slots.
template <int MODE, int KK>
int launch_topk(som_handle* h, const float* X, long N, const float* xsq, int k, int forced_parts, bool want_score) {
    auto& g = h->topk;
    int per_cu = 1;
    if (int rc = kernel_per_cu(h, (const void*)bmu_topk_f32_kernel<MODE, KK>, 256, TOPK_LDS_BYTES, &per_cu)) return rc;
    const TopkPlan p = topk_plan(N, h->K, resident_slots(h, per_cu), forced_parts);
    if (p.parts > 65535) return fail(h, "top-k: more than 65535 codebook parts");
    if (int rc = g.part_sc.reserve(h, (size_t)p.parts * N * TOPK_MAX)) return rc;
    if (int rc = g.part_id.reserve(h, (size_t)p.parts * N * TOPK_MAX)) return rc;
    bmu_topk_f32_kernel<MODE, KK><<<dim3((unsigned)p.row_tiles, (unsigned)p.parts), dim3(256), TOPK_LDS_BYTES, h->stream>>>(
        X, N, h->D, (int)round_up(h->D, F32_KC), h->W, h->wsq, h->K, xsq, (int)p.stages, (int)p.per, g.part_sc, g.part_id);
    topk_merge_kernel<KK><<<dim3((unsigned)cdiv(N, 256)), dim3(256), 0, h->stream>>>(g.part_sc, g.part_id, N, (int)p.parts, k, g.ids, want_score ? (float*)g.score : nullptr);
    HIPCHK(h, hipGetLastError());
    return 0;
}
template <int MODE>
int launch_topk_mode(som_handle* h, const float* X, long N, const float* xsq, int k, int forced_parts, bool want_score) {
    return k <= 4 ? launch_topk<MODE, 4>(h, X, N, xsq, k, forced_parts, want_score) : launch_topk<MODE, 8>(h, X, N, xsq, k, forced_parts, want_score);
}
}  // namespace

// ==============================================================================================
// the exact mode's patch order (som_common.hpp): position -> unit.  Host arithmetic only (som_patch_order exports it).
// Where both sides are multiples of 8 every group is a whole 8 x 8 patch, held in FOUR-BY-FOUR blocks (ex_rank44, bmu_f32.hpp):
// the 16-unit sub-blocks the plan tests (exact_skip.hpp) are then 4 x 4 squares of the map -- at the end of the benchmark's
// schedule a third fewer of them must run than of 2 x 8 strips (tools/bound_probe.py) -- and the re-score kernels decide equal
// scores by rank.  Elsewhere the units of a group ascend.
static bool patch_order_blocks(int X, int Y) { return X % 8 == 0 && Y % 8 == 0; }
static void patch_order(int X, int Y, std::vector<int>& perm, bool blocks = true) {
    const long K = (long)X * Y;
    perm.clear(); perm.reserve((size_t)K);
    for (int x0 = 0; x0 < X; x0 += 8)
        for (int y = 0; y < Y; ++y)
            for (int x = x0; x < std::min(x0 + 8, X); ++x) perm.push_back(x * Y + y);
    for (long g = 0; g < K; g += EX_GROUP) std::sort(perm.begin() + g, perm.begin() + std::min<long>(g + EX_GROUP, K));
    if (!blocks || !patch_order_blocks(X, Y)) return;
    int sorted[EX_GROUP];
    for (long g = 0; g < K; g += EX_GROUP) {
        for (int i = 0; i < EX_GROUP; ++i) sorted[i] = perm[g + i];
        for (int w = 0; w < EX_GROUP; ++w)
            perm[g + w] = sorted[8 * (4 * ((w >> 5) & 1) + ((w >> 2) & 3)) + 4 * ((w >> 4) & 1) + (w & 3)];
    }
}

extern "C" {

#ifndef SOM_SRC_HASH
#define SOM_SRC_HASH "unversioned-build"
#endif
// ends in the hash of the sources this binary was built from (xpysom_dask_amd/build.py checks it against the tree)
const char* som_version(void) { return "somhip 0.2 (gfx950) somhip-src:" SOM_SRC_HASH; }

int som_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* som_last_error(const som_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int som_create(const som_config* cfg, som_handle** out) {
    if (!out) return fail(nullptr, "som_create: out is NULL");
    *out = nullptr;
    if (!cfg) return fail(nullptr, "som_create: cfg is NULL");
    if (cfg->x < 1 || cfg->y < 1 || cfg->input_len < 1) return fail(nullptr, "som_create: x, y, input_len must be >= 1");
    if ((long)cfg->x * cfg->y > (1L << 30)) return fail(nullptr, "som_create: map too large");
    if (cfg->distance < 0 || cfg->distance > SOM_DIST_NORM_P_NO_OPT) return fail(nullptr, "som_create: unknown distance id");
    if (cfg->norm_p < 0 || cfg->norm_p > PW_MAX_P) return fail(nullptr, "som_create: norm_p out of range (1..16)");
    if (cfg->norm_p_real != 0.0 && !(cfg->norm_p_real > 0.0 && cfg->norm_p_real <= 64.0))
        return fail(nullptr, "som_create: norm_p_real out of range (0 < p <= 64)");
    if (cfg->distance >= SOM_DIST_MANHATTAN && cfg->precision != SOM_PREC_F32 && cfg->precision != SOM_PREC_EXACT)
        return fail(nullptr, "som_create: manhattan / norm_p distances are float32 VALU kernels (precision f32)");
    if (cfg->neighborhood < 0 || cfg->neighborhood > SOM_NEIGH_TRIANGLE)
        return fail(nullptr, "som_create: unknown neighbourhood id");
    if (cfg->neighborhood == SOM_NEIGH_MEXICAN_HAT && cfg->compact_support && cfg->topology == SOM_TOPO_RECTANGULAR &&
        cfg->x != cfg->y)
        return fail(nullptr, "som_create: mexican_hat with compact_support needs a square map on the rectangular topology "
                             "(the reference's second mask on px does not broadcast otherwise, neighborhoods.py:70)");
    if (cfg->topology != SOM_TOPO_RECTANGULAR && cfg->topology != SOM_TOPO_HEXAGONAL && cfg->topology != SOM_TOPO_TOROIDAL)
        return fail(nullptr, "som_create: unknown topology id");
    if (cfg->topology == SOM_TOPO_TOROIDAL && cfg->neighborhood == SOM_NEIGH_MEXICAN_HAT && cfg->compact_support)
        return fail(nullptr, "som_create: mexican_hat with compact_support is not defined on the toroidal topology (the "
                             "rectangular form reproduces the reference's double mask; the torus has no reference)");
    if (cfg->topology == SOM_TOPO_HEXAGONAL && cfg->neighborhood == SOM_NEIGH_TRIANGLE)
        return fail(nullptr, "som_create: the hexagonal topology has no triangle neighbourhood (xpysom.py:271-279)");
    if (cfg->precision < SOM_PREC_F32 || cfg->precision > SOM_PREC_EXACT)
        return fail(nullptr, "som_create: unknown precision id");
    if (cfg->precision == SOM_PREC_RETIRED_2 || cfg->precision == SOM_PREC_RETIRED_4)
        return fail(nullptr, "som_create: the split-operand precisions (ids 2 and 4: 'bf16x3', 'f16x3') are retired -- "
                             "precision 'exact' returns float32's own BMUs, faster");
    if (cfg->precision != SOM_PREC_F32 && cfg->precision != SOM_PREC_EXACT) {
        if (cfg->distance == SOM_DIST_EUCLIDEAN_NO_OPT)
            return fail(nullptr, "som_create: bf16 precision implements 'euclidean' and 'cosine' "
                                 "('euclidean_no_opt' has the same argmin as 'euclidean')");
    }
    if (cfg->missing != SOM_MISSING_NONE && cfg->missing != SOM_MISSING_NAN) return fail(nullptr, "som_create: unknown missing-value mode");
    if (cfg->missing == SOM_MISSING_NAN) {
        if (cfg->distance != SOM_DIST_EUCLIDEAN)
            return fail(nullptr, "som_create: missing values (SOM_MISSING_NAN) are defined for the 'euclidean' activation distance only");
        if (cfg->precision == SOM_PREC_BF16 || cfg->precision == SOM_PREC_F16)
            return fail(nullptr, "som_create: missing values (SOM_MISSING_NAN) run the float32 masked kernel: precision 'exact' or "
                                 "'f32', not 'bf16' / 'f16'");
        if ((long)cfg->input_len > (1L << 20)) return fail(nullptr, "som_create: missing values: input_len too large");
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1) return fail(nullptr, "som_create: no HIP device available");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, "som_create: device ordinal out of range");

    som_handle* h = new som_handle();
    h->cfg = *cfg;
    h->masked = cfg->missing == SOM_MISSING_NAN;
    if (h->masked) h->cfg.precision = SOM_PREC_F32;      // no screen applies: the float32 masked kernel IS the exact mode
    else if (cfg->precision == SOM_PREC_EXACT) {
        // the screen + re-score scheme covers the euclidean distance up to 128 features; everywhere else the
        // float32 kernels ARE the exact mode
        // (<= 128 features: the resident screen, euclidean; 129 .. 800 features on maps of >= 4096 units: the wide
        //  screen, euclidean and cosine -- decided below, once the tiling is known)
        if ((cfg->distance == SOM_DIST_EUCLIDEAN && cfg->input_len <= 128) ||
            ((cfg->distance == SOM_DIST_EUCLIDEAN || cfg->distance == SOM_DIST_COSINE) && cfg->input_len > 128)) h->exact = true;
        else h->cfg.precision = SOM_PREC_F32;
    }
    cfg = &h->cfg;
    h->X = cfg->x; h->Y = cfg->y; h->K = cfg->x * cfg->y; h->D = cfg->input_len;
    h->UD = h->masked ? 2 * h->D : h->D;
    h->D1p = (int)round_up(h->UD + 1, 4);
    h->norm_p = cfg->norm_p > 0 ? cfg->norm_p : 2;
    if (cfg->norm_p_real != 0.0 && (cfg->distance == SOM_DIST_NORM_P || cfg->distance == SOM_DIST_NORM_P_NO_OPT)) h->norm_pr = cfg->norm_p_real;
    h->ks32 = (int)cdiv(h->D, 32);
    h->f16 = cfg->precision == SOM_PREC_F16 || h->exact;   // (the exact mode's screen: IEEE half)
    h->tiled = (cfg->precision == SOM_PREC_BF16 || cfg->precision == SOM_PREC_F16 || h->exact) && h->D > 128;
    if (h->tiled) {
        // 256 x 256 tiles need enough units to amortise them; SOM_BF16_TILE=128|256 overrides
        h->tl_big = h->K >= 4096;
        if (h->tl_big) {
            using C = TileCfg<8, 2, 4>;
            h->tl_bm = C::BM; h->tl_bn = C::BN; h->tl_xtile = C::XTILE; h->tl_wfrag = C::WFRAG; h->tl_wtile = C::WTILE;
        } else {
            using C = TileCfg<4, 2, 2>;
            h->tl_bm = C::BM; h->tl_bn = C::BN; h->tl_xtile = C::XTILE; h->tl_wfrag = C::WFRAG; h->tl_wtile = C::WTILE;
        }
        h->n_kchunks = (int)cdiv((long)h->D, TL_BK);
        h->n_ublocks = (int)cdiv(h->K, h->tl_bn);
    }
    h->wide = h->tiled && h->tl_big && h->n_kchunks <= 25;
    if (const char* e = dev_env("SOM_BF16_WIDE")) if (std::atoi(e) == 0) h->wide = false;   // A/B: the two-sided tiling
    if (h->exact && h->tiled && !h->wide) {              // no exact screen on the two-sided tiling: the float32 kernels serve
        h->exact = false; h->f16 = false; h->tiled = false;
        h->cfg.precision = SOM_PREC_F32;
    }
    for (RowSet* s : {&h->res, &h->q, &h->slot[0].rows, &h->slot[1].rows}) s->err_half = h->exact;
    h->ex_patch = h->exact && h->K >= 2 * EX_GROUP;      // (a map of one group has nothing to order)
    if (const char* e = dev_env("SOM_EXACT_PATCH")) if (std::atoi(e) == 0) h->ex_patch = false;   // A/B: groups = strips of a map row
    h->ops = operands::State(operands::Config{h->cfg.precision != SOM_PREC_F32, h->exact, h->ex_patch, h->cfg.distance == SOM_DIST_COSINE,
                                              h->exact && !h->tiled, h->D <= 128});
    h->dp = h->tiled ? TL_BK * h->n_kchunks : 32 * h->ks32;
    h->stage_bytes = h->wide ? wd_stage_bytes(h->n_kchunks) : k16_stage_bytes(h->ks32);
    h->stage_units = h->wide ? WD_STAGE_UNITS : K16_STAGE_UNITS;
    h->nt = cfg->neighborhood == SOM_NEIGH_MEXICAN_HAT ? (cfg->compact_support ? 4 : 2) : 1;
    h->swapped = cfg->neighborhood == SOM_NEIGH_MEXICAN_HAT && cfg->compact_support && cfg->topology == SOM_TOPO_RECTANGULAR;
    h->torus = cfg->topology == SOM_TOPO_TOROIDAL;
    // hexagonal: one copy of the terms per parity class of (unit row, BMU row) -- three classes by the x offset
    // difference (0, +0.5, -0.5); four with compact_support, whose mask compares ABSOLUTE x coordinates (update.hpp)
    if (cfg->topology == SOM_TOPO_HEXAGONAL && cfg->neighborhood != SOM_NEIGH_BUBBLE) h->nt *= cfg->compact_support ? 4 : 3;
    int rc = 0;
    auto bail = [&](int code) { g_create_error = h->err; som_destroy(h); return code; };
    DeviceGuard dev_guard(h);
    {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess || cur != cfg->device) return bail(fail(h, "hipSetDevice failed"));
    }
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess) h->n_cus = prop.multiProcessorCount;
    }
    if (cfg->stream) { h->stream = (hipStream_t)cfg->stream; }
    else {
        if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess)
            return bail(fail(h, "hipStreamCreate failed"));
        h->own_stream = true;
    }
    const size_t KD1 = (size_t)h->K * h->D1p;
    if ((rc = h->W.alloc(h, (size_t)h->K * h->D))) return bail(rc);
    if ((rc = h->wsq.alloc(h, (size_t)h->K))) return bail(rc);
    if (h->ex_patch) {
        if ((rc = h->Wp.alloc(h, (size_t)h->K * h->D))) return bail(rc);
        if ((rc = h->wsq_p.alloc(h, (size_t)h->K))) return bail(rc);
        if ((rc = h->ex_perm.alloc(h, (size_t)h->K))) return bail(rc);
        if ((rc = h->ex_inv.alloc(h, (size_t)h->K))) return bail(rc);
        // bands of 8 map rows, column by column: 64 consecutive positions = 8 columns of a band = an 8 x 8 patch (where
        // the sides are no multiples of 8 a group may straddle two bands or hold a narrower band's 64 / h columns: still
        // compact); then every group's units in ascending order (the first-minimum rule inside a re-score tile)
        std::vector<int> perm;
        bool blocks = true;
        if (const char* e = dev_env("SOM_EXACT_SUB44")) blocks = std::atoi(e) != 0;   // A/B: every group's units ascending (2 x 8 sub-blocks)
        h->ex_sub44 = blocks && patch_order_blocks(h->X, h->Y);
        patch_order(h->X, h->Y, perm, blocks);
        std::vector<int> inv((size_t)h->K);
        for (int p = 0; p < h->K; ++p) inv[(size_t)perm[(size_t)p]] = p;
        if (hipMemcpy(h->ex_perm, perm.data(), (size_t)h->K * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->ex_inv, inv.data(), (size_t)h->K * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
            return bail(fail(h, "hipMemcpy of the patch-order tables failed"));
    }
    if ((rc = h->SC.alloc(h, KD1 + (size_t)h->K))) return bail(rc);        // [K][D1p] sums|counts, then the counts densely [K]
    if ((rc = h->Ud.alloc(h, (size_t)h->nt * h->K))) return bail(rc);
    if ((rc = h->T.alloc(h, KD1 * h->nt))) return bail(rc);
    if ((rc = h->ACC.alloc(h, KD1))) return bail(rc);
    if ((rc = h->P1.alloc(h, (size_t)h->nt * h->Y * h->Y))) return bail(rc);
    if ((rc = h->P2.alloc(h, (size_t)h->X * h->nt * h->X))) return bail(rc);
    if ((rc = h->dsum.alloc(h, 1))) return bail(rc);
    {
        if ((rc = h->np_dev.alloc(h, 1))) return bail(rc);
        if (const char* e = std::getenv("SOM_GRAPH")) h->use_graph = std::atoi(e) != 0;
        if (const char* e = dev_env("SOM_BF16_PARTS")) h->env_bf16_parts = std::atoi(e);
        if (const char* e = dev_env("SOM_F32_PARTS")) h->env_f32_parts = std::atoi(e);
        h->debug = std::getenv("SOM_DEBUG") != nullptr;
        if (const char* e = std::getenv("SOM_VERIFY")) h->verify_rows = std::max(0, std::atoi(e));
        if (h->masked) h->verify_rows = 0;               // (the canary re-scores with the unmasked float32 kernel: not on these rows)
        h->ex.read_env();
        if (const char* e = std::getenv("SOM_EXACT_TOP2")) h->t2.on = std::atoi(e) != 0;
        if (const char* e = dev_env("SOM_ASYNC_COPIES")) h->async_copies = std::atoi(e) != 0;
        if (const char* e = dev_env("SOM_FUSE_MERGE")) h->fuse_merge_prep = std::atoi(e) != 0;
        if (const char* e = dev_env("SOM_COUNTING_SORT")) h->counting_sort = std::atoi(e) != 0;
        // the ranges are kept per 32-row tile of a table (update.hpp): a tile can have a zero column, and an MFMA step to
        // skip, as soon as the table has more columns than the tile has rows -- a map side above 32.  They cost no launch.
        h->use_bands = h->X > LM_TILE || h->Y > LM_TILE;
        if (const char* e = dev_env("SOM_NO_BANDS")) h->use_bands = std::atoi(e) == 0;
        if (const char* e = dev_env("SOM_LM_ROWS")) h->lm_rows = std::atoi(e) == 64 ? 64 : std::atoi(e) == 128 ? 128 : 0;
        const size_t nb = (size_t)2 * band_entries(h->X, h->Y, h->nt) * (h->torus ? 2 : 1);   // two buffers, both empty (toroidal: an entry per piece)
        if ((rc = h->bands.alloc(h, nb))) return bail(rc);
        if (hipMemsetAsync(h->bands, 0, nb * sizeof(int2), h->stream) != hipSuccess) return bail(fail(h, "hipMemsetAsync failed"));
    }
    // (T: stage 1 of the transform writes the feature columns and the count column only; the padding columns behind
    //  them are read by a whole-row stage 2 and end up in ACC's padding, which is all-reduced: keep them defined)
    if (hipMemsetAsync(h->W, 0, (size_t)h->K * h->D * sizeof(float), h->stream) != hipSuccess ||
        hipMemsetAsync(h->T, 0, KD1 * h->nt * sizeof(float), h->stream) != hipSuccess ||
        hipMemsetAsync(h->ACC, 0, KD1 * sizeof(float), h->stream) != hipSuccess)
        return bail(fail(h, "hipMemsetAsync failed"));
    // (a masked handle's search reads the codebook itself: no float32 operand image)
    if (h->D > 128 && !h->masked) {
        h->ft_kchunks = (int)cdiv(h->D, FT_BK);
        h->ft_ublocks = (int)cdiv(h->K, FT_BN);
        if ((rc = h->Wfimg.alloc(h, (size_t)h->ft_ublocks * h->ft_kchunks * FT_WTILE))) return bail(rc);
    }
    if (h->D <= 128 && !h->masked) {
        int kg = 1;
        while (kg * 8 < h->D) kg *= 2;                      // 8, 16, 32, 64 or 128 features per row image
        h->fr_kg = kg;
        h->fr_stages = (int)cdiv(h->K, FR_STAGE_UNITS);
        if ((rc = h->Wfst.alloc(h, (size_t)h->fr_stages * fr_stage_bytes(kg)))) return bail(rc);
    }
    if (h->cfg.precision != SOM_PREC_F32) {
        h->n_stages = (int)cdiv(h->K, h->stage_units);
        size_t bytes = (size_t)h->n_stages * h->stage_bytes;
        if (h->tiled && !h->wide) bytes = (size_t)h->n_ublocks * h->n_kchunks * h->tl_wtile;
        if ((rc = h->Wst.alloc(h, bytes))) return bail(rc);
        if (h->exact && !h->tiled) {
            if ((rc = h->Wst_lo.alloc(h, bytes))) return bail(rc);
            if (hipMemsetAsync(h->Wst_lo, 0, bytes, h->stream) != hipSuccess) return bail(fail(h, "hipMemsetAsync failed"));
        }
        if ((rc = h->xmax2.alloc(h, 2))) return bail(rc);
        h->res.xmax2 = h->xmax2;                         // (the one place that binds a row set to its float)
        h->q.xmax2 = h->slot[0].rows.xmax2 = h->slot[1].rows.xmax2 = h->xmax2 + 1;
        if ((rc = h->wn.alloc(h, (size_t)h->K))) return bail(rc);
        if ((rc = h->wmax2.alloc(h, 2))) return bail(rc);
        if (hipMemsetAsync(h->Wst, 0, bytes, h->stream) != hipSuccess) return bail(fail(h, "hipMemsetAsync failed"));
    }
    if (hipStreamSynchronize(h->stream) != hipSuccess) return bail(fail(h, "hipStreamSynchronize failed"));
    *out = h;
    return 0;
}

void som_destroy(som_handle* h) {
    if (!h) return;
    DeviceGuard dev_guard(h);
    (void)som_comm_destroy(h);
    if (h->comm_stream) (void)hipStreamDestroy(h->comm_stream);
    if (h->ev_block) (void)hipEventDestroy(h->ev_block);
    if (h->ev_comm) (void)hipEventDestroy(h->ev_comm);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->gexec) (void)hipGraphExecDestroy(h->gexec);
    for (auto& ep : h->pending) { (void)hipEventDestroy(ep.a); (void)hipEventDestroy(ep.b); }
    for (auto& ep : h->pool) { (void)hipEventDestroy(ep.a); (void)hipEventDestroy(ep.b); }
    if (h->ex.cost.have) for (auto& e : h->ex.cost.ev) (void)hipEventDestroy(e);
    if (h->ex.fb_ready) (void)hipEventDestroy(h->ex.fb_ready);
    for (auto& sl : h->slot) {
        if (sl.copied) (void)hipEventDestroy(sl.copied);
        if (sl.consumed) (void)hipEventDestroy(sl.consumed);
    }
    if (h->ex.pass_host) (void)hipHostFree(h->ex.pass_host);
    if (h->mon.m_host) (void)hipHostFree(h->mon.m_host);
    if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;                                            // (the device buffers free themselves, on the handle's device: dev_guard)
}

int som_set_weights(som_handle* h, const float* w_host) {
    DeviceGuard dev_guard(h);
    if (!h || !w_host) return fail(h, "som_set_weights: NULL argument");
    if (h->f16 && !h->exact && h->cfg.distance != SOM_DIST_COSINE) {   // (cosine rounds unit-length rows; exact scales)
        // every unit's own norm must fit IEEE half (NaN / infinite units are left to the kernels' NaN rules)
        for (long k = 0; k < h->K; ++k) {
            double q = 0.0;
            for (int d = 0; d < h->D; ++d) { const double v = w_host[k * h->D + d]; q += v * v; }
            if (q > (double)HALF_MAX * HALF_MAX && q <= 1.0e300)
                return fail(h, "som_set_weights: precision 'f16' needs units of norm <= 65504 (float16 range): scale the data, or use 'bf16' / 'f32'");
        }
    }
    if (int rc = h2d_blocking(h, h->W, w_host, (size_t)h->K * h->D * sizeof(float))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->ops.codebook_replaced();
    return 0;
}

int som_get_weights(som_handle* h, float* w_host) {
    DeviceGuard dev_guard(h);
    if (!h || !w_host) return fail(h, "som_get_weights: NULL argument");
    return d2h_blocking(h, w_host, h->W, (size_t)h->K * h->D * sizeof(float));
}

namespace { void drop_graph(som_handle* h); }

// no sample weights from here on; a captured epoch graph has the weighted or the unweighted instance of the segment sum baked in,
// so it goes, and its warm-up epoch runs again
static void clear_sample_weights(som_handle* h) {
    if (h->res.wgt == nullptr) return;
    h->res.wgt = nullptr;
    h->res.wgt_owned.reset();
    drop_graph(h);
    h->graph_warm = 0;
}

// the resident set takes n_rows rows at x: host rows through its own buffer, or the caller's device rows where they are
static int adopt_rows(som_handle* h, const std::string& who, const void* x, int64_t n_rows, bool host) {
    DeviceGuard dev_guard(h);
    if (!h || n_rows < 0 || (!x && n_rows > 0)) return fail(h, who + ": bad argument");
    RowSet& s = h->res;
    clear_sample_weights(h);                             // (weights belong to the rows they were set for)
    if (!host) s.X_owned.reset();
    s.ids_valid = false;
    h->mon.prev_valid = false;                           // (the monitor's last ids belong to the rows they were found for)
    h->searched = false;
    h->ex.plan.order_lost();                             // (the resident sorted pass belongs to the rows it was sorted from)
    h->ex.srt[0].lastpos_valid = false;
    h->seg = som_handle::SegScratch{};
    if (n_rows > 0x7fffffffL) return fail(h, "som_set_data: more than 2^31-1 rows per GPU");
    if (int rc = take_rows(h, s, x, n_rows, host)) return rc;
    if (n_rows > 0)
        if (int rc = seg_reserve(h, h->seg, n_rows)) return rc;
    if (int rc = prepare(h, s, needs_xsq(h))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->f16 && !h->exact && n_rows > 0) {             // IEEE half tops out at 65504: refuse rows that do not fit
        float m2 = 0.0f;
        if (int rc = d2h_blocking(h, &m2, s.xmax2, sizeof(float))) return rc;
        if (!(m2 <= HALF_MAX * HALF_MAX))
            return fail(h, "som_set_data: precision 'f16' needs rows of norm <= 65504 (float16 range): scale the data, or use 'bf16' / 'f32'");
    }
    if (h->exact && n_rows > 0) {
        // the exact mode's pass scratch and, where block skipping can engage, the resident sorted pass's buffers: allocated with
        // the rows, not inside the first epochs (gigabytes of fresh device memory can take a driver tens to hundreds of
        // milliseconds).  A refusal here is not an error: launch_bmu_exact asks again and settles it (smaller passes, no plan).
        bool ok = exact_reserve(h, n_rows) == 0;
        if (ok && exact_skip_wanted(h) && !h->wide)
            ok = exact_skip_reserve(h, h->ex.srt[0], n_rows, h->ex.pass.stride) == 0;
        if (!ok) { (void)hipGetLastError(); h->err.clear(); }
    }
    return 0;
}

int som_set_data(som_handle* h, const float* x_host, int64_t n_rows) { return adopt_rows(h, "som_set_data", x_host, n_rows, true); }
int som_set_data_device(som_handle* h, const void* x_dev, int64_t n_rows) { return adopt_rows(h, "som_set_data_device", x_dev, n_rows, false); }

// Order the engine behind whoever produced device rows handed to som_set_data_device: a
// __cuda_array_interface__ `stream` value (1 = legacy default stream, 2 = per-thread default stream, else a
// hipStream_t), or -- has_stream == 0, the producer named none -- the whole device.
int som_sync_producer(som_handle* h, uint64_t stream, int32_t has_stream) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    if (!has_stream) { HIPCHK(h, hipDeviceSynchronize()); return 0; }
    hipStream_t st = stream == 1 ? (hipStream_t)0 : stream == 2 ? hipStreamPerThread : (hipStream_t)(uintptr_t)stream;
    HIPCHK(h, hipStreamSynchronize(st));
    return 0;
}

// Device rows the caller owns, copied back to host memory (analysis calls on data that lives in HBM).
int som_copy_to_host(som_handle* h, const void* x_dev, uint64_t bytes, void* dst_host) {
    DeviceGuard dev_guard(h);
    if (!h || (bytes > 0 && (!x_dev || !dst_host))) return fail(h, "som_copy_to_host: bad argument");
    if (bytes == 0) return 0;
    return d2h_blocking(h, dst_host, x_dev, (size_t)bytes);
}

namespace {

int epoch_accumulate_eager(som_handle* h, double sigma, double eta, int neigh_f64) {
    h->early = som_handle::EarlyUpdate();
    h->early.armed = h->exact && !h->capturing && h->res.N > 0;
    h->early.sigma = sigma; h->early.eta = eta; h->early.neigh_f64 = neigh_f64;
    int rc = run_activation_bmu(h, h->res.view());
    if (rc == 0) rc = run_update(h, sigma, eta, neigh_f64);
    h->early = som_handle::EarlyUpdate();
    return rc;
}

// ---- training monitor (monitor.hpp): eager launches on the handle's stream, never inside a captured graph -----
// the row metrics of `r` under its own ids: the partials, then their sum into the metrics struct (add: onto a streamed epoch's
// running sums).  prev: the id buffer to refresh, and with have_prev to compare with (nullptr: a streamed chunk, or no rows).
int monitor_launch_rows(som_handle* h, const Rows& r, int* prev, bool have_prev, bool add) {
    auto& mon = h->mon;
    const int grid = (int)monitor_rows_grid(r.N);
    if (grid > 0) {
        const dim3 g((unsigned)grid), b(256);
        const int hp = have_prev ? 1 : 0;
        if (h->masked) {
            if (r.wgt) monitor_rows_kernel<true, true><<<g, b, 0, h->stream>>>(r.X, r.out, h->W, r.wgt, prev, hp, r.N, h->D, mon.rpart);
            else monitor_rows_kernel<true, false><<<g, b, 0, h->stream>>>(r.X, r.out, h->W, nullptr, prev, hp, r.N, h->D, mon.rpart);
        } else {
            if (r.wgt) monitor_rows_kernel<false, true><<<g, b, 0, h->stream>>>(r.X, r.out, h->W, r.wgt, prev, hp, r.N, h->D, mon.rpart);
            else monitor_rows_kernel<false, false><<<g, b, 0, h->stream>>>(r.X, r.out, h->W, nullptr, prev, hp, r.N, h->D, mon.rpart);
        }
        HIPCHK(h, hipGetLastError());
    }
    monitor_rows_reduce_kernel<<<dim3(1), dim3(MON_REDUCE_THREADS), 0, h->stream>>>(mon.rpart, grid, add ? 1 : 0,
                                                                                  have_prev ? 1 : 0, mon.m);
    HIPCHK(h, hipGetLastError());
    return 0;
}

void monitor_free(som_handle* h) {
    auto& mon = h->mon;
    mon.on = false;
    mon.prev_valid = false;
    mon.prev.reset(); mon.rpart.reset(); mon.spart.reset(); mon.m.reset();
    if (mon.m_host) (void)hipHostFree(mon.m_host);
    mon.m_host = nullptr;
}

void drop_graph(som_handle* h) {
    if (h->gexec) (void)hipGraphExecDestroy(h->gexec);
    h->gexec = nullptr;
}

// Capture one epoch (codebook prep, BMU, sort, segment sum, tables, transform) into a hipGraph.
// Every launch parameter except sigma / eta / the neighbourhood dtype is a function of the handle's
// buffers and row count, which the caller has checked are unchanged; those three travel through np_dev.
// Returns 0 with h->gexec set, or 0 with h->use_graph cleared (the eager path then runs as before).
int capture_epoch_graph(som_handle* h) {
    drop_graph(h);
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeRelaxed) != hipSuccess) {
        (void)hipGetLastError();
        h->use_graph = false;
        return 0;
    }
    h->capturing = true;
    h->ops.codebook_replaced();                         // the replayed epoch always rebuilds the operands its BMU kernel needs
    const std::string saved_err = h->err;
    int rc = epoch_accumulate_eager(h, 1.0, 1.0, 1);
    h->capturing = false;
    hipError_t e = hipStreamEndCapture(h->stream, &graph);
    if (rc == 0 && e == hipSuccess && graph != nullptr) e = hipGraphInstantiate(&h->gexec, graph, nullptr, nullptr, 0);
    if (graph) (void)hipGraphDestroy(graph);
    if (rc != 0 || e != hipSuccess || h->gexec == nullptr) {
        (void)hipGetLastError();
        h->gexec = nullptr;
        h->use_graph = false;                           // this handle stays on the eager path
        h->err = saved_err;
        h->ops.codebook_replaced();
        if (h->debug) std::fprintf(stderr, "[somhip] epoch graph capture failed; eager launches\n");
        return 0;
    }
    h->gexec_gen = h->alloc_gen;
    h->gexec_rows = h->res.X;
    h->gexec_n = h->res.N;
    return 0;
}

}  // namespace

int som_epoch_accumulate(som_handle* h, double sigma, double eta, int neigh_f64) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    const RowSet& res = h->res;
    if (!res.X && res.N > 0) return fail(h, "som_epoch_accumulate: no resident data (call som_set_data)");
    h->searched = true;
    // launch-bound maps (many short kernels per epoch) replay a captured graph; profiling needs the
    // per-kernel events of the eager path
    if (h->use_graph && !h->prof && res.N > 0 && !h->exact) {
        const bool same = h->gexec && h->gexec_gen == h->alloc_gen && h->gexec_rows == res.X && h->gexec_n == res.N;
        if (!same) {
            if (h->graph_warm == 0 || h->gexec_rows != res.X || h->gexec_n != res.N) {
                // first epoch over these rows runs eagerly: it sizes every scratch buffer
                drop_graph(h);
                h->gexec_rows = res.X; h->gexec_n = res.N; h->graph_warm = 1;
                return epoch_accumulate_eager(h, sigma, eta, neigh_f64);
            }
            if (int rc = capture_epoch_graph(h)) return rc;
        }
        if (h->gexec) {
            NeighParams p = make_neigh_params(h, sigma, eta, neigh_f64);
            h->band_sel ^= 1;                           // the replayed build of the tables fills the other range buffer
            p.rsel = h->band_sel;
            store_params_kernel<<<dim3(1), dim3(64), 0, h->stream>>>(p, (NeighParams*)h->np_dev);
            HIPCHK(h, hipGraphLaunch(h->gexec, h->stream));
            h->ops.graph_replayed(operands::Request::Search);   // (the captured epoch's own refresh: run_activation_bmu_launch)
            return 0;
        }
    }
    return epoch_accumulate_eager(h, sigma, eta, neigh_f64);
}

// the same accumulator through the update as the reference states it (update.hpp, faithful_update_f32_kernel)
int som_epoch_accumulate_faithful(som_handle* h, double sigma, double eta, int neigh_f64) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    const Rows r = h->res.view();
    if (!r.X && r.N > 0) return fail(h, "som_epoch_accumulate_faithful: no resident data (call som_set_data)");
    if (h->swapped) return fail(h, "som_epoch_accumulate_faithful: mexican_hat with compact_support on the rectangular "
                                   "topology is not a sum of row factor x column factor terms");
    if (h->masked) return fail(h, "som_epoch_accumulate_faithful: the handle was created with SOM_MISSING_NAN; the faithful form is "
                                  "the cross-check of the update without missing values");
    if (r.wgt) return fail(h, "som_epoch_accumulate_faithful: sample weights are set; the faithful form is the cross-check of the "
                               "unweighted update (clear them with som_set_sample_weights(h, NULL, 0))");
    h->searched = true;
    if (int rc = run_activation_bmu(h, r)) return rc;
    Timed t(h, SOM_K_KRON);
    if (int rc = build_tables(h, sigma, eta, neigh_f64, h->stream)) return rc;
    HIPCHK(h, hipMemsetAsync(h->ACC, 0, (size_t)h->K * h->D1p * sizeof(float), h->stream));
    const dim3 grid((unsigned)cdiv(h->D, LM_BN), (unsigned)cdiv(h->K, LM_BM));
    faithful_update_f32_kernel<<<grid, dim3(256), 0, h->stream>>>(r.X, r.out, r.N, h->D, h->D1p, h->X, h->Y, h->nt, h->P1,
                                                              h->P2, h->ACC);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int som_epoch_accumulate_forced(som_handle* h, const int32_t* bmu_host, double sigma, double eta, int neigh_f64) {
    DeviceGuard dev_guard(h);
    if (!h || (!bmu_host && h->res.N > 0)) return fail(h, "som_epoch_accumulate_forced: bad argument");
    for (long i = 0; i < h->res.N; ++i)
        if (bmu_host[i] < 0 || bmu_host[i] >= h->K) return fail(h, "som_epoch_accumulate_forced: id out of range");
    h->ex.srt[0].lastpos_valid = false;                  // (ids from outside: the sorted rows' carried positions are not theirs)
    h->searched = true;                                  // (... and the monitor measures the rows against them)
    if (h->res.N > 0)
        if (int rc = h2d_blocking(h, h->res.bmu, bmu_host, (size_t)h->res.N * sizeof(int))) return rc;
    return run_update(h, sigma, eta, neigh_f64);
}

// ---- per-row sample weights (include/somhip.h) ------------------------------------------------
// index of the first weight that is not finite or is negative, -1 = none
static int64_t first_bad_weight(const float* w, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!(std::isfinite(w[i]) && w[i] >= 0.0f)) return i;
    return -1;
}
static int fail_bad_weight(som_handle* h, const char* who, const float* w, int64_t i) {
    char msg[160];
    std::snprintf(msg, sizeof(msg), "%s: weight %lld is %g: sample weights must be finite and >= 0", who, (long long)i, (double)w[i]);
    return fail(h, msg);
}

int som_set_sample_weights(som_handle* h, const float* w_host, int64_t n_rows) {
    DeviceGuard dev_guard(h);
    if (!h || n_rows < 0) return fail(h, "som_set_sample_weights: bad argument");
    if (!w_host || n_rows == 0) { clear_sample_weights(h); return 0; }
    if (n_rows != h->res.N) return fail(h, "som_set_sample_weights: one weight per resident row (set the rows first: som_set_data)");
    if (const int64_t bad = first_bad_weight(w_host, n_rows); bad >= 0) return fail_bad_weight(h, "som_set_sample_weights", w_host, bad);
    clear_sample_weights(h);
    if (int rc = h->res.wgt_owned.alloc(h, (size_t)n_rows)) return rc;
    if (int rc = h2d_blocking(h, h->res.wgt_owned, w_host, (size_t)n_rows * sizeof(float))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->res.wgt = h->res.wgt_owned;
    drop_graph(h);
    h->graph_warm = 0;
    return 0;
}

int som_set_sample_weights_device(som_handle* h, const void* w_dev, int64_t n_rows) {
    DeviceGuard dev_guard(h);
    if (!h || n_rows < 0) return fail(h, "som_set_sample_weights_device: bad argument");
    if (!w_dev || n_rows == 0) { clear_sample_weights(h); return 0; }
    if (n_rows != h->res.N) return fail(h, "som_set_sample_weights_device: one weight per resident row (set the rows first: som_set_data)");
    clear_sample_weights(h);
    h->res.wgt = (const float*)w_dev;
    drop_graph(h);
    h->graph_warm = 0;
    return 0;
}

// ---- streamed epoch: rows pass through HBM chunk by chunk (out-of-core data) ------------------
int som_stream_begin(som_handle* h) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    if (int rc = refresh_codebook_operands(h, operands::Request::Search)) return rc;
    HIPCHK(h, hipMemsetAsync(h->SC, 0, (size_t)h->K * (h->D1p + 1) * sizeof(float), h->stream));
    if (h->mon.on) {                                     // the epoch's running row sums start at zero, `changed` unknown
        monitor_rows_reduce_kernel<<<dim3(1), dim3(MON_REDUCE_THREADS), 0, h->stream>>>(h->mon.rpart, 0, 0, 0, h->mon.m);
        HIPCHK(h, hipGetLastError());
    }
    h->streaming = true;
    return 0;
}

static bool is_pinned_host(const void* p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeHost;
}

// one streamed chunk; w_host != nullptr: with its sample weights (checked by the caller)
static int stream_rows(som_handle* h, const float* x_host, const float* w_host, int64_t n_rows) {
    if (!h->streaming) return fail(h, "som_stream_rows: call som_stream_begin first");
    if (n_rows == 0) return 0;
    if (n_rows > 0x7fffffffL) return fail(h, "som_stream_rows: more than 2^31-1 rows in one chunk");
    const bool pinned = is_pinned_host(x_host);
    if (n_rows > h->st_seg.sort.cap) {
        HIPCHK(h, hipStreamSynchronize(h->stream));       // earlier chunks' kernels still read the old scratch
        if (int rc = seg_reserve(h, h->st_seg, round_up(n_rows, 1024))) return rc;
    }
    // how the bytes arrive: a slot's on the copy stream, the search behind an event; pageable ones staged by the runtime, synchronous
    som_handle::Slot* const sl = pinned ? &h->slot[h->slot_idx] : nullptr;
    RowSet& s = pinned ? sl->rows : h->q;
    if (pinned) {
        // Pinned chunk: copy on a second stream into one of two device slots, so the transfer of
        // chunk i+1 runs under the kernels of chunk i.  The caller may reuse the buffer of call i
        // once call i+1 has returned (its copy is waited for here).
        if (!h->copy_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
        som_handle::Slot& prev = h->slot[h->slot_idx ^ 1];
        if (prev.used) HIPCHK(h, hipEventSynchronize(prev.copied));
        h->slot_idx ^= 1;
        if (!sl->copied) {
            HIPCHK(h, hipEventCreateWithFlags(&sl->copied, hipEventDisableTiming));
            HIPCHK(h, hipEventCreateWithFlags(&sl->consumed, hipEventDisableTiming));
        }
        if (sl->used) HIPCHK(h, hipEventSynchronize(sl->consumed));   // the kernels that read this slot are done: it may grow, and be written
        if (int rc = reserve(h, s, n_rows, true)) return rc;
        if (w_host) {                                    // the weights travel with the rows, on the copy stream, into the slot
            if (int rc = s.wgt_owned.reserve(h, (size_t)s.cap)) return rc;
            HIPCHK(h, hipMemcpyAsync(s.wgt_owned, w_host, (size_t)n_rows * sizeof(float), hipMemcpyHostToDevice, h->copy_stream));
        }
        HIPCHK(h, hipMemcpyAsync(s.X_owned, x_host, (size_t)n_rows * h->D * sizeof(float), hipMemcpyHostToDevice, h->copy_stream));
        HIPCHK(h, hipEventRecord(sl->copied, h->copy_stream));
        HIPCHK(h, hipStreamWaitEvent(h->stream, sl->copied, 0));
        s.X = s.X_owned; s.N = n_rows;
    } else {
        if (int rc = take_rows(h, s, x_host, n_rows, true)) return rc;
        if (w_host) {                                    // (the stream is drained: nothing reads the old weights)
            if (int rc = s.wgt_owned.reserve(h, (size_t)n_rows, 1024)) return rc;
            if (int rc = h2d_blocking(h, s.wgt_owned, w_host, (size_t)n_rows * sizeof(float))) return rc;
        }
    }
    s.wgt = w_host ? (const float*)s.wgt_owned : nullptr;
    // the one tail: prepare, search, segment sum
    if (int rc = prepare(h, s, needs_xsq(h))) return rc;
    const Rows r = s.view();
    if (int rc = run_activation_bmu(h, r)) return rc;
    if (int rc = segsum_rows(h, r, h->st_seg, false)) return rc;
    // the monitor reads the chunk where it lies, behind its search and before the slot is given back
    if (h->mon.on)
        if (int rc = monitor_launch_rows(h, r, nullptr, false, true)) return rc;
    // a slot is free again behind this event; a pageable chunk's buffer -- the caller's and ours -- on return
    if (!pinned) { HIPCHK(h, hipStreamSynchronize(h->stream)); return 0; }
    HIPCHK(h, hipEventRecord(sl->consumed, h->stream));
    sl->used = true;
    return 0;
}

int som_stream_rows(som_handle* h, const float* x_host, int64_t n_rows) {
    DeviceGuard dev_guard(h);
    if (!h || n_rows < 0 || (n_rows > 0 && !x_host)) return fail(h, "som_stream_rows: bad argument");
    return stream_rows(h, x_host, nullptr, n_rows);
}

int som_stream_rows_weighted(som_handle* h, const float* x_host, const float* w_host, int64_t n_rows) {
    DeviceGuard dev_guard(h);
    if (!h || n_rows < 0 || (n_rows > 0 && (!x_host || !w_host))) return fail(h, "som_stream_rows_weighted: bad argument");
    if (const int64_t bad = first_bad_weight(w_host, n_rows); bad >= 0) return fail_bad_weight(h, "som_stream_rows_weighted", w_host, bad);
    return stream_rows(h, x_host, w_host, n_rows);
}

int som_pinned_alloc(uint64_t bytes, void** out) {
    if (!out) return 1;
    *out = nullptr;
    if (hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return 1; }
    return 0;
}

int som_pinned_free(void* p) {
    if (p && hipHostFree(p) != hipSuccess) { (void)hipGetLastError(); return 1; }
    return 0;
}

int som_stream_end(som_handle* h, double sigma, double eta, int neigh_f64) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    if (!h->streaming) return fail(h, "som_stream_end: call som_stream_begin first");
    h->streaming = false;
    return run_transform(h, sigma, eta, neigh_f64);
}

int som_epoch_merge(som_handle* h) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    h->searched = false;
    Timed t(h, SOM_K_MERGE);
    if (h->masked) {                                     // missing values: a denominator per unit and feature (update.hpp)
        const long total = (long)h->K * h->D;
        merge_masked_kernel<<<dim3((unsigned)cdiv(total, 256)), dim3(256), 0, h->stream>>>(h->W, h->ACC, h->K, h->D, h->D1p);
        HIPCHK(h, hipGetLastError());
        h->ops.merged_plain();
        return 0;
    }
    // the exact mode up to 128 features (euclidean): the merge also writes the patch-order copy, |w|^2 and its maximum, the
    // float32 stage image and the plan's centroids -- everything of the next epoch's operands that does not wait for the
    // maximum (exact_merge_prep_kernel); the 16-bit images follow at the head of the BMU launch (they stay owed)
    if (h->fuse_merge_prep && h->exact && !h->tiled) {
        const int n_groups = (int)cdiv(h->K, EX_GROUP);
        const bool cen = h->ex.cen.ready;
        HIPCHK(h, hipMemsetAsync(h->wmax2, 0, 2 * sizeof(float), h->stream));     // [0]: max |w|^2, [1]: max_k |w^_k - w~_k|^2
        const MergePrepOut o{h->W, h->ex_patch ? (float*)h->Wp : nullptr, h->ex_patch ? (const int*)h->ex_perm : nullptr,
                             h->wsq, h->ex_patch ? (float*)h->wsq_p : nullptr, h->wn, h->wmax2, h->Wfst, h->fr_kg};
        CentroidLevel l1{nullptr, nullptr, nullptr, nullptr, 0}, l2 = l1;
        if (cen) {
            auto& c0 = h->ex.cen.lv[0];
            auto& c1 = h->ex.cen.lv[1];
            l1 = CentroidLevel{c0.Cc, c0.rg, c0.csq, c0.cmax2, c0.n_slots};
            l2 = CentroidLevel{c1.Cc, c1.rg, c1.csq, c1.cmax2, c1.n_slots};
        }
        const unsigned grid = (unsigned)(cen ? cdiv(n_groups, 4) * 4 : n_groups);
        exact_merge_prep_kernel<<<dim3(grid), dim3(512), 0, h->stream>>>(h->ACC, h->K, h->D, h->D1p, n_groups, o, l1, l2);
        HIPCHK(h, hipGetLastError());
        h->ops.merged_exact_fused(cen);
        return 0;
    }
    // the half-precision paths whose operand image is a stage image (resident kernel, euclidean; wide kernel,
    // euclidean and cosine): the merge also writes the next epoch's 16-bit operands
    if (h->fuse_merge_prep && ((is_half1(h) && !h->tiled && h->cfg.distance == SOM_DIST_EUCLIDEAN) ||
                               (h->wide && !h->exact && h->n_kchunks <= 4 * WD_MP_ITERS))) {
        if (int rc = SOM_HALF(h, merge_prep_half, h)) return rc;
        HIPCHK(h, hipGetLastError());
        h->ops.merged_half_fused();                      // the stage image and |w~|^2 are already the new codebook's
        return 0;
    }
    long total = (long)h->K * h->D;
    // (exact mode in patch order: a copy that was in step with the codebook stays in step -- the merge writes both)
    const bool keep_wp = h->ops.patch_copy_in_step();
    merge_kernel<<<dim3((unsigned)cdiv(total, 256)), dim3(256), 0, h->stream>>>(h->W, h->ACC, h->K, h->D, h->D1p,
                                                                                keep_wp ? h->Wp : nullptr, h->ex_inv);
    HIPCHK(h, hipGetLastError());
    h->ops.merged_plain();
    return 0;
}

int som_epoch_accumulate_begin(som_handle* h, double sigma, double eta, int neigh_f64);
int som_epoch_accumulate_block(som_handle* h, int32_t block, int64_t* offset, int64_t* n_floats);

// ---- the exchange step inside the library: RCCL all-reduce of the fused accumulator over xGMI ----------------
namespace {
int rccl_load(const char* path) {
    if (g_rccl.lib) return 0;
    // an explicit path means that library and no other; NULL: a copy some other component of the process already
    // loaded (torch's), else the system's
    const char* search[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
    const char* only[] = {path};
    const char* const* cands = path ? only : search;
    const int n_cands = path ? 1 : 3;
    void* lib = nullptr;
    for (int i = 0; i < n_cands && !lib; ++i) lib = dlopen(cands[i], RTLD_NOW | RTLD_NOLOAD);
    std::string why;
    for (int i = 0; i < n_cands && !lib; ++i) {
        lib = dlopen(cands[i], RTLD_NOW | RTLD_LOCAL);
        if (!lib) { const char* e = dlerror(); why = e ? e : ""; }   // dlerror() clears the message: read it once
    }
    if (!lib) { g_rccl_error = std::string("librccl not found: ") + why; return 1; }
    RcclApi a;
    a.lib = lib;
    a.GetUniqueId = (int (*)(som_nccl_id*))dlsym(lib, "ncclGetUniqueId");
    a.CommInitRank = (int (*)(void**, int, som_nccl_id, int))dlsym(lib, "ncclCommInitRank");
    a.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(lib, "ncclAllReduce");
    a.CommDestroy = (int (*)(void*))dlsym(lib, "ncclCommDestroy");
    a.GetErrorString = (const char* (*)(int))dlsym(lib, "ncclGetErrorString");
    if (!a.GetUniqueId || !a.CommInitRank || !a.AllReduce || !a.CommDestroy) { g_rccl_error = "librccl: symbols missing"; return 1; }
    g_rccl = a;
    return 0;
}
int fail_rccl(som_handle* h, const char* what, int code) {
    return fail(h, std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(code) : "RCCL error"));
}
constexpr int NCCL_FLOAT32 = 7, NCCL_SUM = 0;           // rccl.h: ncclFloat32, ncclSum

int comm_allreduce(som_handle* h, long offset, long n_floats, hipStream_t st) {
    int rc = g_rccl.AllReduce(h->ACC + offset, h->ACC + offset, (size_t)n_floats, NCCL_FLOAT32, NCCL_SUM, h->comm, st);
    if (rc != 0) return fail_rccl(h, "ncclAllReduce", rc);
    return 0;
}
}  // namespace

int som_comm_load(const char* librccl_path) {
    if (rccl_load(librccl_path)) { g_create_error = g_rccl_error; return 1; }
    return 0;
}

int som_comm_unique_id(void* id_out) {
    if (!id_out) return 1;
    if (rccl_load(nullptr)) { g_create_error = g_rccl_error; return 1; }
    som_nccl_id id;
    int rc = g_rccl.GetUniqueId(&id);
    if (rc != 0) { g_create_error = "ncclGetUniqueId failed"; return 1; }
    std::memcpy(id_out, id.internal, sizeof(id.internal));
    return 0;
}

int som_comm_init(som_handle* h, int32_t world, int32_t rank, const void* id_bytes) {
    DeviceGuard dev_guard(h);
    if (!h || !id_bytes || world < 1 || rank < 0 || rank >= world) return fail(h, "som_comm_init: bad argument");
    if (h->comm) return fail(h, "som_comm_init: this handle already has a communicator");
    if (rccl_load(nullptr)) return fail(h, g_rccl_error);
    som_nccl_id id;
    std::memcpy(id.internal, id_bytes, sizeof(id.internal));
    int rc = g_rccl.CommInitRank(&h->comm, world, id, rank);
    if (rc != 0) { h->comm = nullptr; return fail_rccl(h, "ncclCommInitRank", rc); }
    h->comm_world = world;
    if (!h->comm_stream) {
        HIPCHK(h, hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));
        HIPCHK(h, hipEventCreateWithFlags(&h->ev_block, hipEventDisableTiming));
        HIPCHK(h, hipEventCreateWithFlags(&h->ev_comm, hipEventDisableTiming));
    }
    return 0;
}

int som_comm_destroy(som_handle* h) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    if (h->comm) {
        (void)hipStreamSynchronize(h->stream);
        if (h->comm_stream) (void)hipStreamSynchronize(h->comm_stream);
        (void)g_rccl.CommDestroy(h->comm);
        h->comm = nullptr;
        h->comm_world = 1;
    }
    return 0;
}

int som_epoch_allreduce(som_handle* h) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    if (!h->comm) return 0;                             // one GPU: the local sums are the global ones
    return comm_allreduce(h, 0, (long)h->K * h->D1p, h->stream);
}

// accumulate (+ all-reduce, when som_comm_init gave this handle a communicator) + merge.  With more than one
// 128-row block of the map the collective runs block by block on a second stream, each block's all-reduce under
// the next block's transform; one block: one all-reduce on the handle's own stream.
int som_epoch(som_handle* h, double sigma, double eta, int neigh_f64) {
    if (!h) return 1;
    const int nb = (int)cdiv(h->X, LM_BM);
    if (!h->comm || nb < 2) {
        if (int rc = som_epoch_accumulate(h, sigma, eta, neigh_f64)) return rc;
        if (int rc = som_epoch_allreduce(h)) return rc;
        return som_epoch_merge(h);
    }
    DeviceGuard dev_guard(h);
    if (int rc = som_epoch_accumulate_begin(h, sigma, eta, neigh_f64)) return rc;
    for (int b = 0; b < nb; ++b) {
        int64_t off = 0, n = 0;
        if (int rc = som_epoch_accumulate_block(h, b, &off, &n)) return rc;
        HIPCHK(h, hipEventRecord(h->ev_block, h->stream));
        HIPCHK(h, hipStreamWaitEvent(h->comm_stream, h->ev_block, 0));
        if (int rc = comm_allreduce(h, off, n, h->comm_stream)) return rc;
    }
    HIPCHK(h, hipEventRecord(h->ev_comm, h->comm_stream));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_comm, 0));
    return som_epoch_merge(h);
}

// ---- the epoch in stages: finished map-row blocks of the accumulator can be all-reduced while the next are computed
int som_epoch_accumulate_begin(som_handle* h, double sigma, double eta, int neigh_f64) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    const Rows r = h->res.view();
    if (!r.X && r.N > 0) return fail(h, "som_epoch_accumulate_begin: no resident data (call som_set_data)");
    h->searched = true;
    if (int rc = run_activation_bmu(h, r)) return rc;
    if (int rc = segsum_rows(h, r, h->seg, true)) return rc;
    Timed t(h, SOM_K_KRON);
    if (int rc = run_transform_stage1(h, sigma, eta, neigh_f64)) return rc;
    h->staged_blocks_done = 0;
    return 0;
}

int som_epoch_block_count(som_handle* h, int32_t* n_blocks) {
    if (!h || !n_blocks) return fail(h, "som_epoch_block_count: NULL argument");
    *n_blocks = (int32_t)cdiv(h->X, LM_BM);
    return 0;
}

int som_epoch_accumulate_block(som_handle* h, int32_t block, int64_t* offset, int64_t* n_floats) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    if (h->staged_blocks_done < 0 || block != h->staged_blocks_done)
        return fail(h, "som_epoch_accumulate_block: blocks go in order, after som_epoch_accumulate_begin");
    {
        Timed t(h, SOM_K_KRON);
        if (int rc = run_transform_stage2(h, block, block + 1)) return rc;
    }
    const long slab = (long)h->Y * h->D1p, i0 = (long)block * LM_BM;
    const long rows = std::min<long>(i0 + LM_BM, h->X) - i0;
    if (offset) *offset = i0 * slab;
    if (n_floats) *n_floats = rows * slab;
    h->staged_blocks_done = block + 1 == (int)cdiv(h->X, LM_BM) ? -1 : block + 1;
    return 0;
}

int som_accum_device_ptr(som_handle* h, void** dev_ptr, int64_t* n_floats) {
    if (!h || !dev_ptr || !n_floats) return fail(h, "som_accum_device_ptr: NULL argument");
    *dev_ptr = h->ACC;
    *n_floats = (int64_t)h->K * h->D1p;
    return 0;
}

int som_get_stream(som_handle* h, void** stream_out) {
    if (!h || !stream_out) return fail(h, "som_get_stream: NULL argument");
    *stream_out = (void*)h->stream;
    return 0;
}

int som_epoch_fetch(som_handle* h, float* num, float* den, int32_t* bmu) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    if (h->masked) return fail(h, "som_epoch_fetch: the handle was created with SOM_MISSING_NAN, its denominator is [K][input_len]: "
                                  "call som_epoch_fetch_masked");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (num || den) {
        std::vector<float> acc((size_t)h->K * h->D1p);
        HIPCHK(h, hipMemcpy(acc.data(), h->ACC, acc.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (long k = 0; k < h->K; ++k) {
            if (num) std::memcpy(num + k * h->D, acc.data() + k * h->D1p, (size_t)h->D * sizeof(float));
            if (den) den[k] = acc[k * h->D1p + h->D];
        }
    }
    if (bmu && h->res.N > 0) HIPCHK(h, hipMemcpy(bmu, h->res.bmu, (size_t)h->res.N * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

int som_epoch_fetch_masked(som_handle* h, float* num, float* den, int32_t* bmu) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    if (!h->masked) return fail(h, "som_epoch_fetch_masked: the handle was not created with SOM_MISSING_NAN: call som_epoch_fetch");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (num || den) {
        std::vector<float> acc((size_t)h->K * h->D1p);
        HIPCHK(h, hipMemcpy(acc.data(), h->ACC, acc.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (long k = 0; k < h->K; ++k) {
            if (num) std::memcpy(num + k * h->D, acc.data() + k * h->D1p, (size_t)h->D * sizeof(float));
            if (den) std::memcpy(den + k * h->D, acc.data() + k * h->D1p + h->D, (size_t)h->D * sizeof(float));
        }
    }
    if (bmu && h->res.N > 0) HIPCHK(h, hipMemcpy(bmu, h->res.bmu, (size_t)h->res.N * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

// ---- training monitor (include/somhip.h; csrc/monitor.hpp) -----------------------------------------------------
int som_monitor(som_handle* h, int32_t on) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    auto& mon = h->mon;
    if (!on) {
        if (mon.on) HIPCHK(h, hipStreamSynchronize(h->stream));   // (its launches may still be reading what goes)
        monitor_free(h);
        return 0;
    }
    if (mon.on) return 0;
    int rc = mon.rpart.alloc(h, (size_t)monitor_rows_grid(0x7fffffffL));
    if (rc == 0) rc = mon.spart.alloc(h, (size_t)monitor_shift_grid((long)h->K * h->D));
    if (rc == 0) rc = mon.m.alloc(h, 1);
    if (rc == 0 && h->res.N > 0) rc = mon.prev.alloc(h, (size_t)h->res.N);
    if (rc == 0 && hipHostMalloc((void**)&mon.m_host, sizeof(som_epoch_metrics_t), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        mon.m_host = nullptr;
        rc = fail(h, "som_monitor: no pinned host memory for the metrics");
    }
    if (rc == 0) {
        hipError_t e = hipMemsetAsync(mon.m, 0, sizeof(som_epoch_metrics_t), h->stream);
        if (e != hipSuccess) rc = fail_hip(h, "som_monitor: hipMemsetAsync", e);
    }
    if (rc != 0) { const std::string why = h->err; monitor_free(h); h->err = why; return rc; }
    mon.on = true;
    mon.prev_valid = false;
    return 0;
}

int som_epoch_measure_rows(som_handle* h) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    auto& mon = h->mon;
    if (!mon.on) return fail(h, "som_epoch_measure_rows: the monitor is off (call som_monitor(h, 1))");
    if (!h->searched) return fail(h, "som_epoch_measure_rows: no search over the resident rows since the last som_epoch_merge "
                                     "(call a som_epoch_accumulate* form first)");
    const Rows r = h->res.view();
    if (r.N > 0 && (size_t)r.N > mon.prev.cap) {         // rows adopted after som_monitor: the ids' copy grows with them
        if (int rc = mon.prev.alloc(h, (size_t)r.N)) return rc;
        mon.prev_valid = false;
    }
    if (int rc = monitor_launch_rows(h, r, mon.prev, mon.prev_valid, false)) return rc;
    mon.prev_valid = true;
    return 0;
}

int som_epoch_measure_shift(som_handle* h) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    auto& mon = h->mon;
    if (!mon.on) return fail(h, "som_epoch_measure_shift: the monitor is off (call som_monitor(h, 1))");
    if (h->staged_blocks_done >= 0)
        return fail(h, "som_epoch_measure_shift: staged blocks are outstanding: the accumulator is final after the last "
                       "som_epoch_accumulate_block");
    if (h->streaming) return fail(h, "som_epoch_measure_shift: a streamed epoch is open: call som_stream_end first");
    const int grid = (int)monitor_shift_grid((long)h->K * h->D);
    if (h->masked) monitor_shift_kernel<true><<<dim3((unsigned)grid), dim3(256), 0, h->stream>>>(h->ACC, h->W, h->K, h->D, h->D1p, mon.spart);
    else monitor_shift_kernel<false><<<dim3((unsigned)grid), dim3(256), 0, h->stream>>>(h->ACC, h->W, h->K, h->D, h->D1p, mon.spart);
    HIPCHK(h, hipGetLastError());
    monitor_shift_reduce_kernel<<<dim3(1), dim3(MON_REDUCE_THREADS), 0, h->stream>>>(mon.spart, grid, mon.m);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int som_epoch_metrics(som_handle* h, som_epoch_metrics_t* out) {
    DeviceGuard dev_guard(h);
    if (!h || !out) return fail(h, "som_epoch_metrics: NULL argument");
    auto& mon = h->mon;
    if (!mon.on) return fail(h, "som_epoch_metrics: the monitor is off (call som_monitor(h, 1))");
    HIPCHK(h, hipMemcpyAsync(mon.m_host, mon.m, sizeof(som_epoch_metrics_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *out = *mon.m_host;
    return 0;
}

namespace {
// BMU under the full Euclidean distance for quantization / quantization_error (xpysom.py:632-645, 699-707)
// of the n_rows rows in the query scratch.  f32 precision: the reference's sqrt'd distance, bit for bit.
// bf16 / f16 precision with the 'euclidean' activation distance: the same argmin through the configured
// MFMA path (the squared distance is monotone in it); the caller evaluates the distance itself exactly.
// value_only (quantization_error): in EXACT precision with the 'euclidean' activation distance the screen + re-score serve
// first.  Their pick is float32's argmin of the squared distance's unit part, which is NOT always float32's pick under the
// sqrt'd distance: where |x|^2 is large against the distances (un-centred data) the radicand rounds, or clamps to 0, so that
// units at different distances tie under the sqrt and the lowest id wins.  exact_qe_window_kernel keeps the rows whose pick
// no such tie can overturn; the others go through the float32 SQRT kernel, so the ids are float32's bit for bit.
int run_quantization_bmu(som_handle* h, bool value_only = false) {
    RowSet& q = h->q; const float* X = q.X; const long n_rows = q.N;
    // missing values: the sqrt is monotone, the masked search's first minimum IS the row's unit (include/somhip.h)
    if (h->masked) return run_activation_bmu(h, q.view());
    if (h->cfg.precision != SOM_PREC_F32 && h->cfg.distance == SOM_DIST_EUCLIDEAN && (!h->exact || value_only)) {
        if (int rc = prepare(h, q, h->exact)) return rc;
        if (int rc = run_activation_bmu(h, q.view())) return rc;
        if (!h->exact) return 0;
        if (int rc = h->qe_list.reserve(h, (size_t)n_rows, 1024)) return rc;
        if (int rc = h->qe_cnt.reserve(h, 1, 1)) return rc;
        if (int rc = refresh_codebook_operands(h, operands::Request::F32Units)) return rc;       // (|w|^2; the float32 image in the units' order)
        HIPCHK(h, hipMemsetAsync(h->qe_cnt, 0, sizeof(int), h->stream));
        exact_qe_window_kernel<<<dim3((unsigned)cdiv(n_rows, 256)), dim3(256), 0, h->stream>>>(
            X, n_rows, h->D, h->W, h->wsq, q.xsq, q.bmu, h->qe_list, h->qe_cnt);
        HIPCHK(h, hipGetLastError());
        int n_sq = 0;
        if (int rc = d2h_blocking(h, &n_sq, h->qe_cnt, sizeof(int))) return rc;
        if (n_sq < 0 || n_sq > n_rows) return fail(h, "quantization: tie-window counter out of range");
        h->qe_rows += n_rows; h->qe_rows_sqrt += n_sq;
        if (n_sq == 0) return 0;
        if (int rc = h->qe_X.reserve(h, (size_t)n_sq * h->D, (size_t)1024 * h->D)) return rc;
        if (int rc = h->qe_xsq.reserve(h, (size_t)n_sq, 1024)) return rc;
        if (int rc = h->qe_ids.reserve(h, (size_t)n_sq, 1024)) return rc;
        exact_gather_rows_kernel<<<dim3((unsigned)cdiv((long)n_sq * h->D, 256)), dim3(256), 0, h->stream>>>(X, h->qe_list, n_sq, h->D, h->qe_X);
        row_sq_f32_kernel<<<dim3((unsigned)cdiv(n_sq, 256)), dim3(256), 0, h->stream>>>(h->qe_X, n_sq, h->D, h->qe_xsq);
        {
            Timed t(h, SOM_K_BMU);
            if (int rc = launch_bmu_f32_any<SCORE_EUCLID_SQRT>(h, h->qe_X, n_sq, h->qe_xsq, h->qe_ids)) return rc;
        }
        exact_scatter_ids_kernel<<<dim3((unsigned)cdiv(n_sq, 256)), dim3(256), 0, h->stream>>>(h->qe_ids, h->qe_list, n_sq, q.bmu);
        HIPCHK(h, hipGetLastError());
        return 0;
    }
    if (int rc = refresh_codebook_operands(h, operands::Request::F32Units)) return rc;
    if (int rc = row_sq(h, X, n_rows, q.xsq)) return rc;
    Timed t(h, SOM_K_BMU);
    return launch_bmu_f32_any<SCORE_EUCLID_SQRT>(h, X, n_rows, q.xsq, q.bmu);
}

// best and second-best unit of the query set's rows under the sqrt'd Euclidean distance into its bmu / bmu2: the exact mode's screen
// + two re-score rounds where they serve (exact_top2_fast), else -- and for every row they cannot settle -- the float32 kernel
int run_top2(som_handle* h) {
    RowSet& q = h->q;
    if (exact_top2_fast(h)) {
        if (int rc = prepare(h, q, true)) return rc;
        if (int rc = refresh_codebook_operands(h, operands::Request::ExactScreen)) return rc;
        Timed t(h, SOM_K_BMU);
        return launch_top2_exact(h, q.view());
    }
    if (int rc = refresh_codebook_operands(h, operands::Request::F32Units)) return rc;
    if (int rc = row_sq(h, q.X, q.N, q.xsq)) return rc;
    h->t2.rows += q.N; h->t2.rows_f32 += q.N;
    Timed t(h, SOM_K_BMU);
    return launch_bmu_top2(h, q.X, q.N, q.xsq, q.bmu, q.bmu2);
}

// ---- the queries: the host and the device entry point of a pair (x_host or x_dev is NULL; `who` names it in the messages) share
// their argument checks and everything after "the rows are on the device" (query_rows) ----
int query_bmu(som_handle* h, const std::string& who, const float* x_host, const void* x_dev, int64_t n_rows, int32_t mode, int32_t* ids_out) {
    DeviceGuard dev_guard(h);
    if (!h || n_rows < 0 || (n_rows > 0 && ((!x_host && !x_dev) || !ids_out))) return fail(h, who + ": bad argument");
    if (mode != SOM_BMU_ACTIVATION && mode != SOM_BMU_QUANTIZATION) return fail(h, who + ": unknown mode");
    if (n_rows == 0) return 0;
    if (x_dev && n_rows > 0x7fffffffL) return fail(h, who + ": more than 2^31-1 rows in one call");
    if (int rc = query_rows(h, x_host, x_dev, n_rows)) return rc;
    if (mode == SOM_BMU_ACTIVATION) if (int rc = prepare(h, h->q, needs_xsq(h))) return rc;
    if (int rc = mode == SOM_BMU_QUANTIZATION ? run_quantization_bmu(h) : run_activation_bmu(h, h->q.view())) return rc;
    return d2h_blocking(h, ids_out, h->q.bmu, (size_t)n_rows * sizeof(int));
}
// ... the pair to the host (one unit: it is named twice -- include/somhip.h)
int query_top2(som_handle* h, const std::string& who, const float* x_host, const void* x_dev, int64_t n_rows, int32_t* ids1_out, int32_t* ids2_out) {
    DeviceGuard dev_guard(h);
    if (!h || n_rows < 0 || (n_rows > 0 && ((!x_host && !x_dev) || !ids1_out || !ids2_out))) return fail(h, who + ": bad argument");
    if (n_rows == 0) return 0;
    if (x_dev && n_rows > 0x7fffffffL) return fail(h, who + ": more than 2^31-1 rows in one call");
    if (h->masked) return fail(h, who + ": the top-2 search is not defined on a handle created with SOM_MISSING_NAN");
    if (int rc = query_rows(h, x_host, x_dev, n_rows)) return rc;
    if (int rc = run_top2(h)) return rc;
    const size_t bytes = (size_t)n_rows * sizeof(int);
    if (int rc = d2h_blocking(h, ids1_out, h->q.bmu, bytes)) return rc;
    if (h->K == 1) { std::memcpy(ids2_out, ids1_out, bytes); return 0; }
    return d2h_blocking(h, ids2_out, h->q.bmu2, bytes);
}
int query_quantization_error(som_handle* h, const std::string& who, const float* x_host, const void* x_dev, int64_t n_rows, double* qe_out) {
    DeviceGuard dev_guard(h);
    if (!h || !qe_out || n_rows < 0 || (n_rows > 0 && !x_host && !x_dev)) return fail(h, who + ": bad argument");
    if (n_rows == 0) { *qe_out = NAN; return 0; }     // numpy: mean of an empty array
    if (x_dev && n_rows > 0x7fffffffL) return fail(h, who + ": more than 2^31-1 rows in one call");
    if (int rc = query_rows(h, x_host, x_dev, n_rows)) return rc;
    if (int rc = run_quantization_bmu(h, true)) return rc;
    HIPCHK(h, hipMemsetAsync(h->dsum, 0, sizeof(double), h->stream));
    const dim3 qe_grid((unsigned)std::min<long>(cdiv(n_rows, 4), 4096));
    if (h->masked) qe_masked_kernel<<<qe_grid, dim3(256), 0, h->stream>>>(h->q.X, h->q.bmu, h->W, n_rows, h->D, h->dsum);
    else qe_kernel<<<qe_grid, dim3(256), 0, h->stream>>>(h->q.X, h->q.bmu, h->W, n_rows, h->D, h->dsum);
    HIPCHK(h, hipGetLastError());
    double s = 0.0;
    if (int rc = d2h_blocking(h, &s, h->dsum, sizeof(double))) return rc;
    *qe_out = s / (double)n_rows;
    return 0;
}

// ---- map diagnostics (diag.hpp): every row's distance to its BMU, and the per-unit statistics of those distances ----
// the query set's rows are on the device: their units into q.bmu -- quantization_error's own search, so in EXACT precision
// the screen and its tie window serve it -- and q.diag.dist[n] = the float32 qe_kernel would add for row n
int run_bmu_distances(som_handle* h) {
    RowSet& q = h->q;
    if (int rc = q.diag.dist.reserve(h, (size_t)q.cap)) return rc;
    if (int rc = run_quantization_bmu(h, true)) return rc;
    const dim3 grid((unsigned)std::min<long>(cdiv(q.N, 4), 4096));      // (qe_kernel's geometry)
    if (h->masked) bmu_dist_kernel<true><<<grid, dim3(256), 0, h->stream>>>(q.X, q.bmu, h->W, q.N, h->D, q.diag.dist);
    else bmu_dist_kernel<false><<<grid, dim3(256), 0, h->stream>>>(q.X, q.bmu, h->W, q.N, h->D, q.diag.dist);
    HIPCHK(h, hipGetLastError());
    return 0;
}
// the sort's buffers for the rows `s` holds (its cap: they grow with it), the per-unit buffers once
int diag_reserve_stats(som_handle* h, RowSet& s) {
    auto& g = s.diag;
    if (int rc = g.start.reserve(h, (size_t)h->K)) return rc;
    if (int rc = g.count.reserve(h, (size_t)h->K)) return rc;
    if (int rc = g.sums.reserve(h, 2 * (size_t)h->K)) return rc;
    if (int rc = g.max.reserve(h, (size_t)h->K)) return rc;
    return reserve(h, g.sort, s.cap);
}
// the set's rows sorted by unit (diag.sort) and every unit's first sorted position (diag.start; -1: the unit has no rows)
int sort_rows_with_heads(som_handle* h, RowSet& s) {
    auto& g = s.diag;
    if (int rc = sort_rows_by_unit(h, g.sort, s.bmu, s.N)) return rc;
    HIPCHK(h, hipMemsetAsync(g.start, 0xff, (size_t)h->K * sizeof(int), h->stream));
    unit_heads_kernel<<<dim3((unsigned)cdiv(s.N, 256)), dim3(256), 0, h->stream>>>(g.sort.skey, s.N, h->K, g.start);
    HIPCHK(h, hipGetLastError());
    return 0;
}
int query_bmu_distances(som_handle* h, const std::string& who, const float* x_host, const void* x_dev, int64_t n_rows, int32_t* ids_out,
                        float* dist_out) {
    DeviceGuard dev_guard(h);
    if (!h || n_rows < 0 || (n_rows > 0 && ((!x_host && !x_dev) || (!ids_out && !dist_out)))) return fail(h, who + ": bad argument");
    if (n_rows == 0) return 0;
    if (x_dev && n_rows > 0x7fffffffL) return fail(h, who + ": more than 2^31-1 rows in one call");
    if (int rc = query_rows(h, x_host, x_dev, n_rows)) return rc;
    if (int rc = run_bmu_distances(h)) return rc;
    if (ids_out) if (int rc = d2h_blocking(h, ids_out, h->q.bmu, (size_t)n_rows * sizeof(int))) return rc;
    if (dist_out) if (int rc = d2h_blocking(h, dist_out, h->q.diag.dist, (size_t)n_rows * sizeof(float))) return rc;
    return 0;
}
int query_unit_stats(som_handle* h, const std::string& who, const float* x_host, const void* x_dev, int64_t n_rows, int64_t* count,
                     double* sum, double* sumsq, float* max) {
    DeviceGuard dev_guard(h);
    if (!h || !count || !sum || !sumsq || !max || n_rows < 0 || (n_rows > 0 && !x_host && !x_dev)) return fail(h, who + ": bad argument");
    const size_t K = (size_t)h->K;
    if (n_rows == 0) {
        std::memset(count, 0, K * sizeof(int64_t)); std::memset(sum, 0, K * sizeof(double));
        std::memset(sumsq, 0, K * sizeof(double)); std::memset(max, 0, K * sizeof(float));
        return 0;
    }
    if (x_dev && n_rows > 0x7fffffffL) return fail(h, who + ": more than 2^31-1 rows in one call");
    if (int rc = query_rows(h, x_host, x_dev, n_rows)) return rc;
    RowSet& q = h->q; auto& g = q.diag;
    if (int rc = diag_reserve_stats(h, q)) return rc;
    if (int rc = run_bmu_distances(h)) return rc;
    {
        Timed t(h, SOM_K_SEGSUM);                                       // (the sort by unit and the reduction over its segments)
        if (int rc = sort_rows_with_heads(h, q)) return rc;
        unit_stats_kernel<<<dim3((unsigned)cdiv(h->K, 4)), dim3(256), 0, h->stream>>>(g.start, g.sort.skey, g.sort.srow, g.dist, q.N, h->K, g.count,
                                                                                     g.sums, g.sums + K, g.max);
        HIPCHK(h, hipGetLastError());
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "the per-unit counts are copied out as int64_t");
    if (int rc = d2h_blocking(h, count, g.count, K * sizeof(int64_t))) return rc;
    if (int rc = d2h_blocking(h, sum, g.sums, K * sizeof(double))) return rc;
    if (int rc = d2h_blocking(h, sumsq, g.sums + K, K * sizeof(double))) return rc;
    return d2h_blocking(h, max, g.max, K * sizeof(float));
}

// ---- label and value maps (project.hpp): what the rows a unit wins under the ACTIVATION search carry ----
// the checks the four entry points share; `what` names the column count in the messages
int project_check(som_handle* h, const std::string& who, const char* what, bool null_arg, int64_t n_rows, int32_t C) {
    if (!h || null_arg || n_rows < 0) return fail(h, who + ": bad argument");
    if (C < 1 || C > 4096) return fail(h, who + ": " + what + " must be between 1 and 4096");
    if ((int64_t)h->K * C > (1L << 26)) return fail(h, who + ": x * y * " + what + " exceeds 2^26 (analysis call: fewer columns at a time)");
    if (n_rows > 0x7fffffffL) return fail(h, who + ": more than 2^31-1 rows in one call");
    return 0;
}
// the query set's rows are on the device: their units under the configured distance (som_bmu ACTIVATION's own steps), the rows
// sorted by unit and every segment's start -- in diag_reserve_stats's buffers, which som_unit_stats* shares
int project_segments(som_handle* h) {
    RowSet& q = h->q;
    if (int rc = diag_reserve_stats(h, q)) return rc;
    if (int rc = prepare(h, q, needs_xsq(h))) return rc;
    if (int rc = run_activation_bmu(h, q.view())) return rc;
    Timed t(h, SOM_K_SEGSUM);                                           // (the sort by unit; the caller's reduction joins it)
    return sort_rows_with_heads(h, q);
}
int query_unit_label_counts(som_handle* h, const std::string& who, const float* x_host, const void* x_dev, const void* labels,
                            int64_t n_rows, int32_t n_classes, int64_t* counts) {
    DeviceGuard dev_guard(h);
    if (int rc = project_check(h, who, "n_classes", !counts || (n_rows > 0 && ((!x_host && !x_dev) || !labels)), n_rows, n_classes)) return rc;
    const size_t KC = (size_t)h->K * n_classes;
    if (n_rows == 0) { std::memset(counts, 0, KC * sizeof(int64_t)); return 0; }
    if (int rc = query_rows(h, x_host, x_dev, n_rows)) return rc;
    RowSet& q = h->q; auto& g = q.diag;
    if (int rc = g.pcount.reserve(h, KC)) return rc;
    const int* lab = (const int*)labels;
    if (x_host) {
        if (int rc = g.labels.reserve(h, (size_t)q.cap)) return rc;
        if (int rc = h2d_blocking(h, g.labels, labels, (size_t)n_rows * sizeof(int))) return rc;
        lab = g.labels;
    }
    if (int rc = project_segments(h)) return rc;
    {
        Timed t(h, SOM_K_SEGSUM);
        unit_label_counts_kernel<<<dim3((unsigned)cdiv(h->K, 4)), dim3(256), 0, h->stream>>>(g.start, g.sort.skey, g.sort.srow, lab, q.N, h->K,
                                                                                            n_classes, g.pcount);
        HIPCHK(h, hipGetLastError());
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "the per-unit counts are copied out as int64_t");
    return d2h_blocking(h, counts, g.pcount, KC * sizeof(int64_t));
}
int query_unit_value_sums(som_handle* h, const std::string& who, const float* x_host, const void* x_dev, const void* values,
                          int64_t n_rows, int32_t n_cols, int64_t* count, double* sum, double* sumsq) {
    DeviceGuard dev_guard(h);
    if (int rc = project_check(h, who, "n_cols", !count || !sum || !sumsq || (n_rows > 0 && ((!x_host && !x_dev) || !values)), n_rows, n_cols)) return rc;
    const size_t KC = (size_t)h->K * n_cols;
    if (n_rows == 0) {
        std::memset(count, 0, KC * sizeof(int64_t)); std::memset(sum, 0, KC * sizeof(double)); std::memset(sumsq, 0, KC * sizeof(double));
        return 0;
    }
    if (int rc = query_rows(h, x_host, x_dev, n_rows)) return rc;
    RowSet& q = h->q; auto& g = q.diag;
    if (int rc = g.pcount.reserve(h, KC)) return rc;
    if (int rc = g.psums.reserve(h, 2 * KC)) return rc;
    const float* val = (const float*)values;
    if (x_host) {
        if (int rc = g.values.reserve(h, (size_t)q.cap * n_cols)) return rc;
        if (int rc = h2d_blocking(h, g.values, values, (size_t)n_rows * n_cols * sizeof(float))) return rc;
        val = g.values;
    }
    if (int rc = project_segments(h)) return rc;
    {
        Timed t(h, SOM_K_SEGSUM);
        unit_value_sums_kernel<<<dim3((unsigned)cdiv(h->K, 4)), dim3(256), 0, h->stream>>>(g.start, g.sort.skey, g.sort.srow, val, q.N, h->K, n_cols,
                                                                                          g.pcount, g.psums, g.psums + KC);
        HIPCHK(h, hipGetLastError());
    }
    if (int rc = d2h_blocking(h, count, g.pcount, KC * sizeof(int64_t))) return rc;
    if (int rc = d2h_blocking(h, sum, g.psums, KC * sizeof(double))) return rc;
    return d2h_blocking(h, sumsq, g.psums + KC, KC * sizeof(double));
}

// ---- data density per unit (density.hpp): how many rows lie within each radius of every unit's weight vector ----
int query_density(som_handle* h, const std::string& who, const float* x_host, const void* x_dev, int64_t n_rows, const float* pivot,
                  const float* radii, int32_t n_radii, int64_t* counts) {
    DeviceGuard dev_guard(h);
    if (!h || !radii || !counts || n_rows < 0 || (n_rows > 0 && !x_host && !x_dev)) return fail(h, who + ": bad argument");
    if (n_radii < 1 || n_radii > DEN_MAX_RADII) return fail(h, who + ": n_radii must be between 1 and " + std::to_string(DEN_MAX_RADII));
    if (h->masked) return fail(h, who + ": not defined on a handle created with SOM_MISSING_NAN: a distance over a row's observed "
                                        "features has no common scale across rows");
    DensityRadii rad;
    for (int j = 0; j < DEN_MAX_RADII; ++j) rad.r2[j] = NAN;                // (a spare radius of the instance counts nothing)
    for (int j = 0; j < n_radii; ++j) {
        const float r2 = (float)((double)radii[j] * (double)radii[j]);
        if (!(radii[j] >= 0.0f) || !std::isfinite(r2)) return fail(h, who + ": radius " + std::to_string(j) + " must be >= 0 with a finite float32 square");
        rad.r2[j] = r2;
    }
    const size_t K = (size_t)h->K, RK = (size_t)n_radii * K;
    if (n_rows == 0) { std::memset(counts, 0, RK * sizeof(int64_t)); return 0; }
    if (n_rows > 0x7fffffffL) return fail(h, who + ": more than 2^31-1 rows in one call");
    if (int rc = query_rows(h, x_host, x_dev, n_rows)) return rc;
    if (int rc = refresh_codebook_operands(h, operands::Request::F32Units)) return rc;
    RowSet& q = h->q; auto& g = h->den;
    const int D = h->D;
    if (int rc = g.pivot.reserve(h, (size_t)D)) return rc;
    if (int rc = g.Wc.reserve(h, K * D)) return rc;
    if (int rc = g.wsq.reserve(h, K)) return rc;
    if (int rc = g.counts.reserve(h, (size_t)DEN_MAX_RADII * K)) return rc;
    if (pivot) { if (int rc = h2d_blocking(h, g.pivot, pivot, (size_t)D * sizeof(float))) return rc; }
    else HIPCHK(h, hipMemsetAsync(g.pivot, 0, (size_t)D * sizeof(float), h->stream));
    density_center_units_kernel<<<dim3((unsigned)cdiv(h->K, 4)), dim3(256), 0, h->stream>>>(h->W, g.pivot, h->K, D, g.Wc, g.wsq);
    density_row_sq_kernel<<<dim3((unsigned)std::min<long>(cdiv(q.N, 4), 4096)), dim3(256), 0, h->stream>>>(q.X, g.pivot, q.N, D, q.xsq);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemsetAsync(g.counts, 0, RK * sizeof(unsigned long long), h->stream));
    int forced = 0;
    if (const char* e = dev_env("SOM_DENSITY_SLABS")) forced = std::max(0, std::atoi(e));
    {
        Timed t(h, SOM_K_BMU);
        int rc;
        if (n_radii == 1) rc = launch_unit_density<1>(h, q, forced, rad, n_radii);
        else if (n_radii == 2) rc = launch_unit_density<2>(h, q, forced, rad, n_radii);
        else if (n_radii <= 4) rc = launch_unit_density<4>(h, q, forced, rad, n_radii);
        else rc = launch_unit_density<8>(h, q, forced, rad, n_radii);
        if (rc) return rc;
    }
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the per-unit counts are copied out as int64_t");
    return d2h_blocking(h, counts, g.counts, RK * sizeof(int64_t));
}

// ---- the k nearest units of every row (topk.hpp): ranked lists with scores and distances, and the per-unit rank counts ----
// the checks the four entry points share
int topk_check(som_handle* h, const std::string& who, bool null_arg, int64_t n_rows, int32_t k) {
    if (!h || null_arg || n_rows < 0) return fail(h, who + ": bad argument");
    if (k < 1 || k > TOPK_MAX) return fail(h, who + ": k must be between 1 and SOM_TOPK_MAX = " + std::to_string(TOPK_MAX));
    if (k > h->K) return fail(h, who + ": k = " + std::to_string(k) + " exceeds the map's " + std::to_string(h->K) + " units");
    if (h->masked) return fail(h, who + ": the top-k search is not defined on a handle created with SOM_MISSING_NAN");
    if (h->cfg.distance > SOM_DIST_COSINE)
        return fail(h, who + ": only the GEMM-form distances (euclidean, euclidean_no_opt, cosine)");
    if (n_rows > 0x7fffffffL) return fail(h, who + ": more than 2^31-1 rows in one call");
    // (the scan forms its staging offsets, a row of a tile times input_len, with a 24-bit multiply: topk.hpp)
    if (h->D >= (1 << 24)) return fail(h, who + ": input_len must be below 2^24");
    return 0;
}
// the rows are on the device (query_rows): rows [r0, r0 + P) of the query set into the lists g.ids (and g.score, g.dist)
int run_topk_pass(som_handle* h, long r0, long P, int k, bool want_score, bool want_dist, int forced_parts) {
    RowSet& q = h->q; auto& g = h->topk;
    const float* X = q.X + r0 * (long)h->D;
    const float* xsq = q.xsq + r0;
    {
        Timed t(h, SOM_K_BMU);
        int rc;
        if (h->cfg.distance == SOM_DIST_EUCLIDEAN) rc = launch_topk_mode<SCORE_EUCLID_PART>(h, X, P, xsq, k, forced_parts, want_score);
        else if (h->cfg.distance == SOM_DIST_EUCLIDEAN_NO_OPT) rc = launch_topk_mode<SCORE_EUCLID_SQ>(h, X, P, xsq, k, forced_parts, want_score);
        else rc = launch_topk_mode<SCORE_COSINE>(h, X, P, xsq, k, forced_parts, want_score);
        if (rc) return rc;
        if (want_dist) {
            const long slots = P * k;
            topk_dist_kernel<<<dim3((unsigned)std::min<long>(cdiv(slots, 4), 4096)), dim3(256), 0, h->stream>>>(X, g.ids, h->W, slots, k, h->D, g.dist);
            HIPCHK(h, hipGetLastError());
        }
    }
    return 0;
}
// what both queries do before their passes: the rows, the float32 codebook with |w|^2, the rows' |x|^2, the lists' scratch -- the
// scores' and the distances' only where the caller asked for them
int topk_begin(som_handle* h, const float* x_host, const void* x_dev, int64_t n_rows, bool want_score, bool want_dist, int* forced_parts) {
    if (int rc = query_rows(h, x_host, x_dev, n_rows)) return rc;
    if (int rc = refresh_codebook_operands(h, operands::Request::F32Units)) return rc;
    if (h->cfg.distance != SOM_DIST_EUCLIDEAN) if (int rc = row_sq(h, h->q.X, n_rows, h->q.xsq)) return rc;
    auto& g = h->topk;
    const size_t slots = (size_t)std::min<long>(n_rows, TOPK_PASS_ROWS) * TOPK_MAX;
    if (int rc = g.ids.reserve(h, slots)) return rc;
    if (want_score) if (int rc = g.score.reserve(h, slots)) return rc;
    if (want_dist) if (int rc = g.dist.reserve(h, slots)) return rc;
    *forced_parts = 0;
    if (const char* e = dev_env("SOM_TOPK_PARTS")) *forced_parts = std::max(0, std::atoi(e));
    return 0;
}
int query_topk(som_handle* h, const std::string& who, const float* x_host, const void* x_dev, int64_t n_rows, int32_t k, int32_t* ids_out,
               float* score_out, float* dist_out) {
    DeviceGuard dev_guard(h);
    if (int rc = topk_check(h, who, !ids_out || (n_rows > 0 && !x_host && !x_dev), n_rows, k)) return rc;
    if (n_rows == 0) return 0;
    int forced = 0;
    if (int rc = topk_begin(h, x_host, x_dev, n_rows, score_out != nullptr, dist_out != nullptr, &forced)) return rc;
    auto& g = h->topk;
    for (long r0 = 0; r0 < n_rows; r0 += TOPK_PASS_ROWS) {
        const long P = std::min<long>(TOPK_PASS_ROWS, n_rows - r0);
        if (int rc = run_topk_pass(h, r0, P, k, score_out != nullptr, dist_out != nullptr, forced)) return rc;
        const size_t slots = (size_t)P * k, o = (size_t)r0 * k;
        if (int rc = d2h_blocking(h, ids_out + o, g.ids, slots * sizeof(int))) return rc;
        if (score_out) if (int rc = d2h_blocking(h, score_out + o, g.score, slots * sizeof(float))) return rc;
        if (dist_out) if (int rc = d2h_blocking(h, dist_out + o, g.dist, slots * sizeof(float))) return rc;
    }
    return 0;
}
int query_rank_counts(som_handle* h, const std::string& who, const float* x_host, const void* x_dev, int64_t n_rows, int32_t k,
                      int64_t* counts) {
    DeviceGuard dev_guard(h);
    if (int rc = topk_check(h, who, !counts || (n_rows > 0 && !x_host && !x_dev), n_rows, k)) return rc;
    const size_t kK = (size_t)k * h->K;
    if (n_rows == 0) { std::memset(counts, 0, kK * sizeof(int64_t)); return 0; }
    int forced = 0;
    if (int rc = topk_begin(h, x_host, x_dev, n_rows, false, false, &forced)) return rc;
    auto& g = h->topk;
    if (int rc = g.counts.reserve(h, (size_t)TOPK_MAX * h->K)) return rc;
    HIPCHK(h, hipMemsetAsync(g.counts, 0, kK * sizeof(unsigned long long), h->stream));
    for (long r0 = 0; r0 < n_rows; r0 += TOPK_PASS_ROWS) {
        const long P = std::min<long>(TOPK_PASS_ROWS, n_rows - r0);
        if (int rc = run_topk_pass(h, r0, P, k, false, false, forced)) return rc;
        Timed t(h, SOM_K_BMU);
        unit_rank_counts_kernel<<<dim3((unsigned)cdiv(P * k, 256)), dim3(256), 0, h->stream>>>(g.ids, P * k, k, h->K, g.counts);
        HIPCHK(h, hipGetLastError());
    }
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the rank counts are copied out as int64_t");
    return d2h_blocking(h, counts, g.counts, kK * sizeof(int64_t));
}

// ---- missing values: the completed rows (impute.hpp) ----
// out[n][d] = X[n][d] where observed, W[ids[n]][d] where NaN, on the handle's stream; out == X fills in place.  16 bytes a lane
// where input_len and the three addresses as they ARE allow it (a caller's view may start at any float), else a float a lane.
// The grid is bounded as qe_grid is; the kernel strides over its tiles of rows.
int launch_impute(som_handle* h, const float* X, const int* ids, long N, float* out) {
    const bool vec = h->D % 4 == 0 && (((uintptr_t)X | (uintptr_t)out | (uintptr_t)h->W.p) & 15) == 0;
    const long tiles = cdiv(N, impute_tile_rows(vec ? h->D / 4 : h->D));
    const dim3 grid((unsigned)std::min<long>(tiles, 4096));
    Timed t(h, SOM_K_FILL);
    if (vec) impute_rows_kernel<4><<<grid, dim3(256), 0, h->stream>>>(X, ids, h->W, N, h->D, out);
    else impute_rows_kernel<1><<<grid, dim3(256), 0, h->stream>>>(X, ids, h->W, N, h->D, out);
    HIPCHK(h, hipGetLastError());
    return 0;
}
int query_impute(som_handle* h, const std::string& who, const float* x_host, const void* x_dev, int64_t n_rows, float* out_host,
                 void* out_dev, int32_t* ids_out) {
    DeviceGuard dev_guard(h);
    if (!h) return fail(h, who + ": NULL handle");
    if (!h->masked) return fail(h, who + ": the handle was not created with SOM_MISSING_NAN: there is nothing to fill");
    if (n_rows < 0) return fail(h, who + ": n_rows < 0");
    if (n_rows == 0) return 0;
    if (!x_host && !x_dev) return fail(h, who + ": the rows are NULL");
    if (!out_host && !out_dev) return fail(h, who + ": out is NULL");
    if (x_dev && n_rows > 0x7fffffffL) return fail(h, who + ": more than 2^31-1 rows in one call");
    const size_t bytes = (size_t)n_rows * h->D * sizeof(float);
    {
        const uintptr_t a = x_host ? (uintptr_t)x_host : (uintptr_t)x_dev, b = out_host ? (uintptr_t)out_host : (uintptr_t)out_dev;
        if (a != b && a < b + bytes && b < a + bytes) return fail(h, who + ": the rows and out overlap without being the same array");
    }
    if (int rc = query_rows(h, x_host, x_dev, n_rows)) return rc;
    RowSet& q = h->q;
    if (int rc = prepare(h, q, needs_xsq(h))) return rc;                 // (som_bmu ACTIVATION's own steps: the same ids)
    if (int rc = run_activation_bmu(h, q.view())) return rc;
    // host rows: filled where they were staged, in place, and copied back; device rows: into the caller's array
    float* out = x_host ? q.X_owned.p : (float*)out_dev;
    if (int rc = launch_impute(h, q.X, q.bmu, n_rows, out)) return rc;
    if (x_host) if (int rc = d2h_blocking(h, out_host, out, bytes)) return rc;
    if (ids_out) return d2h_blocking(h, ids_out, q.bmu, (size_t)n_rows * sizeof(int));
    HIPCHK(h, hipStreamSynchronize(h->stream));                          // the fill is complete when the call returns
    return 0;
}
}  // namespace

int som_bmu(som_handle* h, const float* x_host, int64_t n_rows, int32_t mode, int32_t* ids_out) { return query_bmu(h, "som_bmu", x_host, nullptr, n_rows, mode, ids_out); }
int som_bmu_device(som_handle* h, const void* x_dev, int64_t n_rows, int32_t mode, int32_t* ids_out) { return query_bmu(h, "som_bmu_device", nullptr, x_dev, n_rows, mode, ids_out); }
int som_bmu_top2(som_handle* h, const float* x_host, int64_t n_rows, int32_t* ids1_out, int32_t* ids2_out) { return query_top2(h, "som_bmu_top2", x_host, nullptr, n_rows, ids1_out, ids2_out); }
int som_bmu_top2_device(som_handle* h, const void* x_dev, int64_t n_rows, int32_t* ids1_out, int32_t* ids2_out) { return query_top2(h, "som_bmu_top2_device", nullptr, x_dev, n_rows, ids1_out, ids2_out); }
int som_quantization_error(som_handle* h, const float* x_host, int64_t n_rows, double* qe_out) { return query_quantization_error(h, "som_quantization_error", x_host, nullptr, n_rows, qe_out); }
int som_quantization_error_device(som_handle* h, const void* x_dev, int64_t n_rows, double* qe_out) { return query_quantization_error(h, "som_quantization_error_device", nullptr, x_dev, n_rows, qe_out); }
int som_bmu_distances(som_handle* h, const float* x_host, int64_t n_rows, int32_t* ids_out, float* dist_out) { return query_bmu_distances(h, "som_bmu_distances", x_host, nullptr, n_rows, ids_out, dist_out); }
int som_bmu_distances_device(som_handle* h, const void* x_dev, int64_t n_rows, int32_t* ids_out, float* dist_out) { return query_bmu_distances(h, "som_bmu_distances_device", nullptr, x_dev, n_rows, ids_out, dist_out); }
int som_impute(som_handle* h, const float* x_host, int64_t n_rows, float* out_host, int32_t* ids_out) { return query_impute(h, "som_impute", x_host, nullptr, n_rows, out_host, nullptr, ids_out); }
int som_impute_device(som_handle* h, const void* x_dev, int64_t n_rows, void* out_dev, int32_t* ids_out) { return query_impute(h, "som_impute_device", nullptr, x_dev, n_rows, nullptr, out_dev, ids_out); }
int som_unit_stats(som_handle* h, const float* x_host, int64_t n_rows, int64_t* count, double* sum, double* sumsq, float* max) { return query_unit_stats(h, "som_unit_stats", x_host, nullptr, n_rows, count, sum, sumsq, max); }
int som_unit_stats_device(som_handle* h, const void* x_dev, int64_t n_rows, int64_t* count, double* sum, double* sumsq, float* max) { return query_unit_stats(h, "som_unit_stats_device", nullptr, x_dev, n_rows, count, sum, sumsq, max); }
int som_unit_label_counts(som_handle* h, const float* x_host, const int32_t* labels_host, int64_t n_rows, int32_t n_classes, int64_t* counts) { return query_unit_label_counts(h, "som_unit_label_counts", x_host, nullptr, labels_host, n_rows, n_classes, counts); }
int som_unit_label_counts_device(som_handle* h, const void* x_dev, const void* labels_dev, int64_t n_rows, int32_t n_classes, int64_t* counts) { return query_unit_label_counts(h, "som_unit_label_counts_device", nullptr, x_dev, labels_dev, n_rows, n_classes, counts); }
int som_unit_value_sums(som_handle* h, const float* x_host, const float* v_host, int64_t n_rows, int32_t n_cols, int64_t* count, double* sum, double* sumsq) { return query_unit_value_sums(h, "som_unit_value_sums", x_host, nullptr, v_host, n_rows, n_cols, count, sum, sumsq); }
int som_unit_value_sums_device(som_handle* h, const void* x_dev, const void* v_dev, int64_t n_rows, int32_t n_cols, int64_t* count, double* sum, double* sumsq) { return query_unit_value_sums(h, "som_unit_value_sums_device", nullptr, x_dev, v_dev, n_rows, n_cols, count, sum, sumsq); }
int som_unit_density(som_handle* h, const float* x_host, int64_t n_rows, const float* pivot, const float* radii, int32_t n_radii, int64_t* counts) { return query_density(h, "som_unit_density", x_host, nullptr, n_rows, pivot, radii, n_radii, counts); }
int som_unit_density_device(som_handle* h, const void* x_dev, int64_t n_rows, const float* pivot, const float* radii, int32_t n_radii, int64_t* counts) { return query_density(h, "som_unit_density_device", nullptr, x_dev, n_rows, pivot, radii, n_radii, counts); }
int som_bmu_topk(som_handle* h, const float* x_host, int64_t n_rows, int32_t k, int32_t* ids_out, float* score_out, float* dist_out) { return query_topk(h, "som_bmu_topk", x_host, nullptr, n_rows, k, ids_out, score_out, dist_out); }
int som_bmu_topk_device(som_handle* h, const void* x_dev, int64_t n_rows, int32_t k, int32_t* ids_out, float* score_out, float* dist_out) { return query_topk(h, "som_bmu_topk_device", nullptr, x_dev, n_rows, k, ids_out, score_out, dist_out); }
int som_unit_rank_counts(som_handle* h, const float* x_host, int64_t n_rows, int32_t k, int64_t* counts) { return query_rank_counts(h, "som_unit_rank_counts", x_host, nullptr, n_rows, k, counts); }
int som_unit_rank_counts_device(som_handle* h, const void* x_dev, int64_t n_rows, int32_t k, int64_t* counts) { return query_rank_counts(h, "som_unit_rank_counts_device", nullptr, x_dev, n_rows, k, counts); }

// ---- row moments and the row gather (moments.hpp): queries that touch nothing of the engine's row sets, weights, ids or plans ----
namespace {
int row_moments(som_handle* h, const std::string& who, const float* x_host, const void* x_dev, const void* w, int64_t n_rows,
                const float* pivot, double* wsum, double* s1, double* gram) {
    DeviceGuard dev_guard(h);
    if (!h) return fail(h, who + ": NULL handle");
    if (h->D > MOM_MAX_D)
        return fail(h, who + ": input_len " + std::to_string(h->D) + " exceeds SOM_MOMENTS_MAX_FEATURES (" + std::to_string(MOM_MAX_D) + ")");
    if (!wsum || !s1 || n_rows < 0 || (n_rows > 0 && !x_host && !x_dev)) return fail(h, who + ": bad argument");
    if (n_rows > 0x7fffffffL) return fail(h, who + ": more than 2^31-1 rows");
    const int D = h->D;
    if (x_host && w)
        if (const int64_t bad = first_bad_weight((const float*)w, n_rows); bad >= 0) return fail_bad_weight(h, who.c_str(), (const float*)w, bad);
    if (n_rows == 0) {
        *wsum = 0.0;
        std::memset(s1, 0, (size_t)D * sizeof(double));
        if (gram) std::memset(gram, 0, (size_t)D * D * sizeof(double));
        return 0;
    }
    auto& m = h->mom;
    const long N = n_rows;
    const float* X = (const float*)x_dev;
    const float* wd = (const float*)w;
    if (x_host) {
        if (int rc = m.X.reserve(h, (size_t)N * D)) return rc;
        if (int rc = h2d_blocking(h, m.X, x_host, (size_t)N * D * sizeof(float))) return rc;
        X = m.X;
        if (w) {
            if (int rc = m.w.reserve(h, (size_t)N)) return rc;
            if (int rc = h2d_blocking(h, m.w, w, (size_t)N * sizeof(float))) return rc;
            wd = m.w;
        }
    }
    if (int rc = m.pivot.reserve(h, (size_t)D)) return rc;
    if (pivot) { if (int rc = h2d_blocking(h, m.pivot, pivot, (size_t)D * sizeof(float))) return rc; }
    else HIPCHK(h, hipMemsetAsync(m.pivot, 0, (size_t)D * sizeof(float), h->stream));
    const long sg = mom_sum_grid(N);
    if (int rc = m.spart.reserve(h, (size_t)sg * (D + 1))) return rc;
    if (int rc = m.sums.reserve(h, (size_t)D + 1)) return rc;
    if (wd) moments_sums_kernel<true><<<dim3((unsigned)sg), dim3(256), 0, h->stream>>>(X, wd, m.pivot, N, D, m.spart);
    else moments_sums_kernel<false><<<dim3((unsigned)sg), dim3(256), 0, h->stream>>>(X, nullptr, m.pivot, N, D, m.spart);
    moments_sums_reduce_kernel<<<dim3((unsigned)cdiv(D + 1, 64)), dim3(64 * MOM_RED_WAVES), 0, h->stream>>>(m.spart, (int)sg, D, m.sums);
    HIPCHK(h, hipGetLastError());
    if (gram) {
        const long T = mom_tiles(D), S = mom_splits(N, D);
        if (int rc = m.gpart.reserve(h, (size_t)S * T * MOM_TILE)) return rc;
        if (int rc = m.gram.reserve(h, (size_t)D * D)) return rc;
        const dim3 grid((unsigned)mom_tile_groups(D), (unsigned)S);
        if (wd) moments_gram_kernel<true><<<grid, dim3(256), 0, h->stream>>>(X, wd, m.pivot, N, D, m.gpart);
        else moments_gram_kernel<false><<<grid, dim3(256), 0, h->stream>>>(X, nullptr, m.pivot, N, D, m.gpart);
        moments_gram_reduce_kernel<<<dim3((unsigned)T, 16), dim3(64 * MOM_RED_WAVES), 0, h->stream>>>(m.gpart, S, D, m.gram);
        HIPCHK(h, hipGetLastError());
    }
    if (int rc = d2h_blocking(h, s1, m.sums, (size_t)D * sizeof(double))) return rc;
    if (int rc = d2h_blocking(h, wsum, m.sums + D, sizeof(double))) return rc;
    if (gram) return d2h_blocking(h, gram, m.gram, (size_t)D * D * sizeof(double));
    return 0;
}
}  // namespace

int som_row_moments(som_handle* h, const float* x_host, const float* w_host, int64_t n_rows, const float* pivot, double* wsum, double* s1, double* gram) { return row_moments(h, "som_row_moments", x_host, nullptr, w_host, n_rows, pivot, wsum, s1, gram); }
int som_row_moments_device(som_handle* h, const void* x_dev, const void* w_dev, int64_t n_rows, const float* pivot, double* wsum, double* s1, double* gram) { return row_moments(h, "som_row_moments_device", nullptr, x_dev, w_dev, n_rows, pivot, wsum, s1, gram); }

int som_gather_rows_device(som_handle* h, const void* x_dev, int64_t n_rows, const int64_t* idx_host, int64_t k, float* out_host) {
    DeviceGuard dev_guard(h);
    if (!h || n_rows < 0 || k < 0 || (k > 0 && (!x_dev || !idx_host || !out_host))) return fail(h, "som_gather_rows_device: bad argument");
    if (k > 0x7fffffffL) return fail(h, "som_gather_rows_device: more than 2^31-1 rows asked for");
    for (int64_t i = 0; i < k; ++i)
        if (idx_host[i] < 0 || idx_host[i] >= n_rows)
            return fail(h, "som_gather_rows_device: index " + std::to_string(idx_host[i]) + " (entry " + std::to_string(i) + ") is outside the block of " + std::to_string(n_rows) + " rows");
    if (k == 0) return 0;
    auto& m = h->mom;
    static_assert(sizeof(long long) == sizeof(int64_t), "the indices are copied in as int64_t");
    if (int rc = m.idx.reserve(h, (size_t)k)) return rc;
    if (int rc = m.rows.reserve(h, (size_t)k * h->D)) return rc;
    if (int rc = h2d_blocking(h, m.idx, idx_host, (size_t)k * sizeof(int64_t))) return rc;
    const long g = std::min<long>(cdiv((long)k * h->D, 256), 4096);
    gather_rows_kernel<<<dim3((unsigned)g), dim3(256), 0, h->stream>>>((const float*)x_dev, m.idx, (long)k, h->D, m.rows);
    HIPCHK(h, hipGetLastError());
    return d2h_blocking(h, out_host, m.rows, (size_t)k * h->D * sizeof(float));
}

int som_debug_moments_plan(int64_t n_rows, int32_t input_len, int64_t* out6) {
    static_assert(MOM_R == SOM_MOMENTS_CHUNK_ROWS && MOM_MAX_D == SOM_MOMENTS_MAX_FEATURES, "the headers state the kernels' constants");
    if (!out6 || n_rows < 0 || input_len < 1) return 1;
    out6[0] = MOM_R; out6[1] = mom_tiles(input_len); out6[2] = mom_splits(n_rows, input_len); out6[3] = mom_split_cap(input_len);
    out6[4] = mom_sum_grid(n_rows); out6[5] = MOM_MAX_D;
    return 0;
}

int som_debug_density_plan(int64_t n_rows, int32_t K, int64_t slots, int32_t forced_slabs, int64_t* out4) {
    if (!out4 || n_rows < 1 || n_rows > 0x7fffffffL || K < 1 || slots < 1 || forced_slabs < 0) return 1;
    const DensityPlan p = density_plan(n_rows, K, slots, forced_slabs);
    out4[0] = p.unit_tiles; out4[1] = p.row_tiles; out4[2] = p.slabs; out4[3] = p.per;
    return 0;
}

int som_debug_topk_plan(int64_t n_rows, int32_t K, int64_t slots, int32_t forced_parts, int64_t* out4) {
    if (!out4 || n_rows < 1 || n_rows > 0x7fffffffL || K < 1 || slots < 1 || forced_parts < 0) return 1;
    const TopkPlan p = topk_plan(n_rows, K, slots, forced_parts);
    out4[0] = p.row_tiles; out4[1] = p.stages; out4[2] = p.parts; out4[3] = p.per;
    return 0;
}

int som_bmu_f64(som_handle* h, const double* x_host, int64_t n_rows, int32_t* ids_out) {
    DeviceGuard dev_guard(h);
    if (!h || n_rows < 0 || (n_rows > 0 && (!x_host || !ids_out))) return fail(h, "som_bmu_f64: bad argument");
    if (h->cfg.distance != SOM_DIST_EUCLIDEAN) return fail(h, "som_bmu_f64: the float64 query path serves the 'euclidean' activation distance");
    if (h->masked) return fail(h, "som_bmu_f64: not available on a handle created with SOM_MISSING_NAN (query with float32 rows)");
    if (n_rows == 0) return 0;
    const size_t w_bytes = (size_t)PW_UNITS * h->D * sizeof(float);
    if (w_bytes > 150 * 1024) return fail(h, "som_bmu_f64: input_len too large for the LDS unit tile");
    if (int rc = reserve(h, h->q, n_rows, true)) return rc;
    if (int rc = h->qX64.reserve(h, (size_t)n_rows * h->D, (size_t)1024 * h->D)) return rc;
    if (int rc = h2d_blocking(h, h->qX64, x_host, (size_t)n_rows * h->D * sizeof(double))) return rc;
    if (int rc = refresh_codebook_operands(h, operands::Request::F32Units)) return rc;       // |w|^2 in NumPy's float32 order
    {
        Timed t(h, SOM_K_BMU);
        bmu_f64_kernel<<<dim3((unsigned)cdiv(n_rows, PW_SAMPLES)), dim3(PW_SAMPLES), w_bytes, h->stream>>>(
            h->qX64, n_rows, h->D, h->W, h->wsq, h->K, h->q.bmu);
        HIPCHK(h, hipGetLastError());
    }
    return d2h_blocking(h, ids_out, h->q.bmu, (size_t)n_rows * sizeof(int));
}

int som_distance_matrix(som_handle* h, const float* x_host, int64_t n_rows, int32_t mode, float* dist_out) {
    DeviceGuard dev_guard(h);
    if (!h || n_rows < 0 || (n_rows > 0 && (!x_host || !dist_out))) return fail(h, "som_distance_matrix: bad argument");
    if (mode != SOM_BMU_ACTIVATION && mode != SOM_BMU_QUANTIZATION) return fail(h, "som_distance_matrix: unknown mode");
    if (h->masked) return fail(h, "som_distance_matrix: not available on a handle created with SOM_MISSING_NAN");
    if (mode == SOM_BMU_ACTIVATION && h->cfg.distance > SOM_DIST_COSINE)
        return fail(h, "som_distance_matrix: only the GEMM-form distances (euclidean, euclidean_no_opt, cosine)");
    if (n_rows == 0) return 0;
    if ((double)n_rows * h->K > 2.0e9) return fail(h, "som_distance_matrix: n_rows * K too large (analysis call, chunk it)");
    if (int rc = query_rows(h, x_host, nullptr, n_rows)) return rc;
    if (int rc = refresh_codebook_operands(h, operands::Request::F32Units)) return rc;
    if (int rc = row_sq(h, h->q.X, n_rows, h->q.xsq)) return rc;
    DevBuf<float> dm;
    if (int rc = dm.alloc(h, (size_t)n_rows * h->K)) return rc;
    int rc = 0;
    if (mode == SOM_BMU_QUANTIZATION) rc = launch_dist_matrix<SCORE_EUCLID_SQRT>(h, n_rows, dm);
    else if (h->cfg.distance == SOM_DIST_EUCLIDEAN) rc = launch_dist_matrix<SCORE_EUCLID_PART>(h, n_rows, dm);
    else if (h->cfg.distance == SOM_DIST_EUCLIDEAN_NO_OPT) rc = launch_dist_matrix<SCORE_EUCLID_SQ>(h, n_rows, dm);
    else rc = launch_dist_matrix<SCORE_COSINE>(h, n_rows, dm);
    if (rc) return rc;
    return d2h_blocking(h, dist_out, dm, (size_t)n_rows * h->K * sizeof(float));
}

int som_set_verify(som_handle* h, int32_t n_rows) {
    if (!h || n_rows < 0) return fail(h, "som_set_verify: bad argument");
    if (h->masked && n_rows > 0)
        return fail(h, "som_set_verify: the canary re-scores with the unmasked float32 kernel; not on a handle created with SOM_MISSING_NAN");
    h->verify_rows = n_rows;
    return 0;
}

int som_verify_stats(som_handle* h, int64_t* launches, int64_t* rows_checked) {
    if (!h) return 1;
    if (launches) *launches = h->verify_launches;
    if (rows_checked) *rows_checked = h->verify_rows_checked;
    return 0;
}

// TEST HOOK of the canary: overwrite the operand images the BMU kernels read (the 16-bit stage / tile image and the
// float32 stage image) with zeros WITHOUT marking them stale -- what a lost or torn staging copy would look like.
int som_debug_corrupt_operands(som_handle* h, int32_t which) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    // (every image, the float32 one in the order the next BMU launch wants: no rebuild there)
    if (int rc = refresh_codebook_operands(h, h->exact ? operands::Request::ExactScreen : operands::Request::F32Units)) return rc;
    if ((which & 1) && h->Wst) {
        size_t bytes = (size_t)h->n_stages * h->stage_bytes;
        if (h->tiled && !h->wide) bytes = (size_t)h->n_ublocks * h->n_kchunks * h->tl_wtile;
        HIPCHK(h, hipMemsetAsync(h->Wst, 0, bytes, h->stream));
    }
    if ((which & 2) && h->Wfst) HIPCHK(h, hipMemsetAsync(h->Wfst, 0, (size_t)h->fr_stages * fr_stage_bytes(h->fr_kg), h->stream));
    if ((which & 2) && h->Wfimg) HIPCHK(h, hipMemsetAsync(h->Wfimg, 0, (size_t)h->ft_ublocks * h->ft_kchunks * FT_WTILE, h->stream));
    return 0;
}

// TEST HOOK, read-only: a 64-bit FNV-1a hash of one of the codebook's operand buffers as it stands on the device (nothing is
// refreshed).  which: 0 Wst, 1 Wst_lo, 2 Wfst, 3 |w|^2 in the image order (wsq_p, or wsq without patch order), 4 wn, 5 the wmax2
// pair, 6 the plan's centroids, radii, |c|^2 and maxima (both levels), 7 the codebook in the image order (Wp, or W).  A buffer
// the handle does not hold hashes as the empty string.
int som_debug_operand_crc(som_handle* h, int32_t which, uint64_t* out) {
    DeviceGuard dev_guard(h);
    if (!h || !out) return 1;
    uint64_t hash = 0xcbf29ce484222325ull;
    std::vector<unsigned char> host;
    auto add = [&](const void* dev, size_t bytes) -> int {
        if (dev == nullptr || bytes == 0) return 0;
        host.resize(bytes);
        if (int rc = d2h_blocking(h, host.data(), dev, bytes)) return rc;
        for (size_t i = 0; i < bytes; ++i) { hash ^= host[i]; hash *= 0x100000001b3ull; }
        return 0;
    };
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const bool half = h->cfg.precision != SOM_PREC_F32;
    size_t st_bytes = (size_t)h->n_stages * h->stage_bytes;
    if (h->tiled && !h->wide) st_bytes = (size_t)h->n_ublocks * h->n_kchunks * h->tl_wtile;
    int rc = 0;
    switch (which) {
    case 0: rc = add(h->Wst, half ? st_bytes : 0); break;
    case 1: rc = add(h->Wst_lo, st_bytes); break;
    case 2:                                               // (a stage's fragments and its 64 norms: the rest of the last KiB is never written)
        for (int st = 0; h->Wfst && st < h->fr_stages && rc == 0; ++st)
            rc = add((const char*)h->Wfst + (size_t)st * fr_stage_bytes(h->fr_kg), (size_t)FR_UT * h->fr_kg * 1024 + 64 * sizeof(float));
        break;
    case 3: rc = add(h->ex_patch ? (const float*)h->wsq_p : (const float*)h->wsq, (size_t)h->K * sizeof(float)); break;
    case 4: rc = add(h->wn, half ? (size_t)h->K * sizeof(float) : 0); break;
    case 5: rc = add(h->wmax2, half ? 2 * sizeof(float) : 0); break;
    case 6:
        if (h->ex.cen.ready)
            for (int lv = 0; lv < (h->wide ? 1 : 2) && rc == 0; ++lv) {
                auto& c = h->ex.cen.lv[lv];
                if ((rc = add(c.Cc, (size_t)c.n_slots * h->D * sizeof(float)))) break;
                if ((rc = add(c.rg, (size_t)c.n_slots * sizeof(float)))) break;
                if ((rc = add(c.csq, (size_t)c.n_slots * sizeof(float)))) break;
                rc = add(c.cmax2, 2 * sizeof(float));
            }
        break;
    case 7: rc = add(h->ex_patch ? (const float*)h->Wp : (const float*)h->W, (size_t)h->K * h->D * sizeof(float)); break;
    default: return fail(h, "som_debug_operand_crc: unknown buffer");
    }
    if (rc) return rc;
    *out = hash;
    return 0;
}

// TEST HOOK, read-only: the exact plan's centroids, radii and |c|^2 of one level as they stand on the device (nothing is launched,
// nothing refreshed, no state changed).  level 0: the 64-unit groups (beyond 128 features the only level), level 1: the 16-unit
// sub-blocks in exact_centroids_kernel's slot order.  Any of the three outputs may be NULL; *n_slots_out is written first.
int som_debug_exact_centroids(som_handle* h, int32_t level, float* C_out, float* r_out, float* csq_out, int32_t* n_slots_out) {
    DeviceGuard dev_guard(h);
    if (!h || !n_slots_out) return fail(h, "som_debug_exact_centroids: NULL argument");
    if (!h->ex.cen.ready) return fail(h, "som_debug_exact_centroids: the handle holds no centroids (no launch has planned yet)");
    if (level < 0 || level >= (h->wide ? 1 : 2)) return fail(h, "som_debug_exact_centroids: no such level");
    const auto& c = h->ex.cen.lv[level];
    *n_slots_out = c.n_slots;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (C_out) if (int rc = d2h_blocking(h, C_out, c.Cc, (size_t)c.n_slots * h->D * sizeof(float))) return rc;
    if (r_out) if (int rc = d2h_blocking(h, r_out, c.rg, (size_t)c.n_slots * sizeof(float))) return rc;
    if (csq_out) if (int rc = d2h_blocking(h, csq_out, c.csq, (size_t)c.n_slots * sizeof(float))) return rc;
    return 0;
}

// TEST HOOK (no device needed): the exact mode's policy functions (csrc/exact_policy.hpp) on caller-supplied numbers.
// costs[9] = {full_total, full_screen, plan_total, plan_over, plan_over_scout, blk_ms, l2_ms_group, l2_ratio, sort_ms};
// which / args: 0 commit_scouted_plan(share, blocks_per_row) | 1 level2_from_sample(share, share1, blocks_per_row) |
// 2 level2_pays(share, share1) | 3 sort_paid(share_stale, share_fresh, blocks_per_row, epochs_served) | 4 plan_idle(share) |
// 5 scout_continues(win_share, share_last, blocks_per_row) | 6 rows_worth_a_scout(rows, units, features).  *out = 0 / 1.
int som_policy_eval(int32_t which, const double* costs, const double* args, int32_t* out) {
    if (!costs || !args || !out) return 1;
    policy::Costs c;
    c.full_total = costs[0]; c.full_screen = costs[1]; c.plan_total = costs[2]; c.plan_over = costs[3]; c.plan_over_scout = costs[4];
    c.blk_ms = costs[5]; c.l2_ms_group = costs[6]; c.l2_ratio = costs[7]; c.sort_ms = costs[8];
    switch (which) {
    case 0: *out = policy::commit_scouted_plan(c, args[0], args[1]); return 0;
    case 1: *out = policy::level2_from_sample(c, args[0], args[1], args[2]); return 0;
    case 2: *out = policy::level2_pays(c, args[0], args[1]); return 0;
    case 3: *out = policy::sort_paid(c, args[0], args[1], args[2], (int)args[3]); return 0;
    case 4: *out = policy::plan_idle(c, args[0]); return 0;
    case 5: *out = policy::scout_continues(c, args[0], args[1], args[2]); return 0;
    case 6: *out = policy::rows_worth_a_scout(args[0], args[1], args[2]); return 0;
    }
    return 1;
}

// TEST HOOK (no device needed): a script of launches through a fresh policy::PlanState, driven as launch_bmu_exact drives it
// (begin; the row sample and the sample tiles where the plan asks for them; end).  Layouts: include/somhip_test.h.
int som_policy_replay(int32_t n_launches, const double* script, double* out) {
    if (n_launches < 0 || !script || !out) return 1;
    policy::PlanState st;
    for (int32_t i = 0; i < n_launches; ++i) {
        const double* in = script + (size_t)i * SOM_POLICY_REPLAY_IN;
        double* o = out + (size_t)i * SOM_POLICY_REPLAY_OUT;
        policy::LaunchFacts f;
        f.resident = in[0] != 0.0; f.have_last = in[1] != 0.0; f.rows = (const void*)(uintptr_t)in[2]; f.n_rows = (long)in[3];
        f.can_skip = in[4] != 0.0; f.scout_ok = in[5] != 0.0; f.wide = in[6] != 0.0; f.wide_can = in[7] != 0.0; f.wide_scout_ok = in[8] != 0.0;
        f.l2_fits_lds = in[9] != 0.0; f.have_lo_image = in[10] != 0.0; f.blocks_per_row = in[11];
        f.skip_mode = (int)in[12]; f.refine_on = in[13] != 0.0; f.sub_blocks = in[14] != 0.0; f.res_every = (int)in[15];
        policy::LaunchPlan p = st.begin(f);
        const bool asked_rows = p.estimate;
        const bool row_no = asked_rows && st.rows_sampled(in[16], p);
        const bool asked_tiles = p.estimate && p.sample_tiles && in[17] >= 0.0;   // (in[17] < 0: a pass too short for sample tiles)
        const bool tile_no = asked_tiles && st.tiles_sampled(in[17], in[18], f, p);
        policy::LaunchOutcome oc;
        oc.t_total = in[19]; oc.t_screen = in[20]; oc.t_l2 = in[21]; oc.t_sort = in[22];
        oc.screen_timed = p.time_phases; oc.l2_timed = p.time_phases && p.skip && p.level2; oc.sort_timed = p.time_phases && p.skip && p.resort;
        oc.blocks_total = (int64_t)in[24];
        oc.blocks_run = p.skip ? (int64_t)in[23] : oc.blocks_total;            // (without a plan every block runs)
        oc.groups_run = p.skip ? (int64_t)in[25] : oc.blocks_total / policy::TILES_PER_GROUP;
        oc.pairs_in = (int64_t)in[26]; oc.pairs_out = p.refine ? (int64_t)in[27] : 0; oc.scout_wins = (p.skip && p.scout && f.have_last) ? (int64_t)in[28] : 0;
        st.end(f, p, oc);
        o[0] = p.skip; o[1] = p.resort; o[2] = p.scout; o[3] = p.level2; o[4] = p.estimate; o[5] = p.sample_tiles; o[6] = p.refine; o[7] = p.time_phases;
        o[8] = asked_rows; o[9] = asked_tiles; o[10] = row_no; o[11] = tile_no;
        for (int k = 0; k < 2; ++k) {
            const policy::Pause& ps = st.pause(k == 0);
            o[12 + 3 * k] = ps.cooldown; o[13 + 3 * k] = ps.idle; o[14 + 3 * k] = ps.pause;
        }
    }
    return 0;
}

// TEST HOOK (no device needed): a script of events through a fresh operands::State (csrc/codebook_operands.hpp), moved as the
// host code moves the handle's.  Layouts: include/somhip_test.h.
int som_operands_replay(const int32_t* config, int32_t n_events, const int32_t* script, int32_t* out) {
    if (!config || n_events < 0 || !script || !out) return 1;
    const operands::Config cfg{config[0] != 0, config[1] != 0, config[2] != 0, config[3] != 0, config[4] != 0, config[5] != 0};
    if (!cfg.valid()) return 1;
    operands::State st(cfg);
    for (int32_t i = 0; i < n_events; ++i) {
        const int32_t* in = script + (size_t)i * SOM_OPERANDS_REPLAY_IN;
        int32_t* o = out + (size_t)i * SOM_OPERANDS_REPLAY_OUT;
        if (in[1] < 0 || in[1] > 2) return 1;
        const operands::Request rq = in[1] == 0 ? operands::Request::Search : in[1] == 1 ? operands::Request::F32Units : operands::Request::ExactScreen;
        operands::Rebuilds r;
        switch (in[0]) {
        case 0: st.codebook_replaced(); break;
        case 1: st.merged_plain(); break;
        case 2: if (!cfg.half || cfg.exact) return 1; st.merged_half_fused(); break;
        case 3: if (!cfg.resident) return 1; st.merged_exact_fused(in[2] != 0); break;
        case 4: if (in[2] != 0 && !cfg.resident) return 1; r = st.decide(rq, in[2] != 0); st.commit(r); break;
        case 5: r.flush = st.take_pending_image(&r.flush_cm); break;
        case 6: if (cfg.exact) return 1; st.graph_replayed(rq); break;
        case 7: r = st.decide_wsq(); st.commit(r); break;
        default: return 1;
        }
        o[0] = r.wsq; o[1] = r.permute; o[2] = r.f32; o[3] = r.f32_patch; o[4] = r.half; o[5] = r.skip_norms; o[6] = r.deferred; o[7] = r.cm;
        o[8] = r.flush; o[9] = r.flush_cm;
        o[10] = st.f32_in_patch_order(); o[11] = st.image_pending(); o[12] = st.centroids_fresh(); o[13] = st.patch_copy_in_step();
    }
    return 0;
}

// TEST HOOK (no device needed): the row sets' size rule (csrc/row_set.hpp) on caller-supplied numbers.  Layout: include/somhip_test.h.
int som_debug_row_set_sizes(int32_t kind, int64_t n, int32_t input_len, int32_t dp, int32_t flags, int64_t* out5) {
    if (kind < 0 || kind > 2 || n < 0 || input_len < 1 || dp < 0 || !out5) return 1;
    const rowset::Sizes z = rowset::sizes((rowset::Kind)kind, (long)n, input_len, dp, {(flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) != 0});
    out5[0] = z.cap; out5[1] = (int64_t)z.X; out5[2] = (int64_t)z.xsq; out5[3] = (int64_t)z.Xb; out5[4] = (int64_t)z.ids;
    return 0;
}

int som_debug_unit_sort_sizes(int64_t rows_cap, int32_t K, int32_t counting_on, int64_t n, int64_t* out6) {
    if (rows_cap < 0 || n < 0 || K < 1 || !out6) return 1;
    const unitsort::Sizes z = unitsort::sizes((long)rows_cap, K, counting_on != 0);
    out6[0] = (int64_t)z.skey; out6[1] = (int64_t)z.srow; out6[2] = (int64_t)z.scratch; out6[3] = (int64_t)z.table;
    out6[4] = z.cs_blocks; out6[5] = unitsort::counting(z, (long)n) ? 1 : 0;
    return 0;
}

int som_debug_unit_sort_stats(som_handle* h, int64_t* counting, int64_t* radix) {
    if (!h || !counting || !radix) return fail(h, "som_debug_unit_sort_stats: NULL argument");
    *counting = h->sorts_counting;
    *radix = h->sorts_radix;
    return 0;
}

namespace {
// one block of som_debug_exact_scratch_sizes / _held (include/somhip_test.h has the order): 59 values
int64_t* put(int64_t* o, std::initializer_list<int64_t> v) { return std::copy(v.begin(), v.end(), o); }
int64_t* put_sorted(int64_t* o, const exscratch::SortedSizes& s) {
    return put(o, {s.cap, (int64_t)s.order, (int64_t)s.Xb_s, (int64_t)s.Xl_s, (int64_t)s.Xf_s, (int64_t)s.xsq_s, (int64_t)s.xerr_s, (int64_t)s.seed_s,
                   (int64_t)s.sU_s, (int64_t)s.lastpos_s});
}
int64_t* put_block(int64_t* o, const exscratch::PassSizes& p, int levels, const exscratch::CentroidSizes (&c)[2], const exscratch::SortedSizes& s,
                   const exscratch::PlanSizes& q) {
    o = put(o, {p.stride, p.pairs, p.max_tiles, p.too_large ? 1 : 0, (int64_t)p.gmin, (int64_t)p.gflags, (int64_t)p.rowcnt, (int64_t)p.rowarg,
                (int64_t)p.seed, (int64_t)p.plist, (int64_t)p.fb_list, (int64_t)p.tile_tab, (int64_t)p.ctr, levels});
    for (const auto& l : c)
        o = put(o, {l.n_slots, l.n_cstages, l.n_img_stages, (int64_t)l.Cc, (int64_t)l.rg, (int64_t)l.csq, (int64_t)l.cmax2, (int64_t)l.Cst, (int64_t)l.Cst_plain});
    o = put_sorted(o, s);
    return put(o, {q.stride, q.tiles, (int64_t)q.sk_keys, (int64_t)q.sk_keys2, (int64_t)q.sk_vals, (int64_t)q.sk_tmp, (int64_t)q.scout_g, (int64_t)q.tq,
                   (int64_t)q.need, (int64_t)q.need2, (int64_t)q.glist, (int64_t)q.gcnt, (int64_t)q.tlist, (int64_t)q.tcnt, (int64_t)q.tile_counts,
                   (int64_t)q.tile_ticket, (int64_t)q.items});
}
}  // namespace

int som_debug_exact_scratch_sizes(const int64_t* geometry8, int64_t rows, int64_t stride_cap, int64_t* out) {
    if (!geometry8 || !out || rows < 1 || stride_cap < 0 || geometry8[0] < 1 || geometry8[1] < 1) return 1;
    const int64_t* v = geometry8;
    const exscratch::Geometry g{(long)v[0], (int)v[1], (int)v[2], (int)v[3], v[4] != 0, (int)v[5], (long)v[6], (long)v[7]};
    int64_t* o = out;
    long stride = exscratch::first_stride(g, (long)rows, 0);
    for (int i = 0; i < 16; ++i, stride = stride > 0 ? exscratch::next_stride(stride) : 0) *o++ = stride;
    for (const long st : {exscratch::first_stride(g, (long)rows, 0), exscratch::first_stride(g, (long)rows, (long)stride_cap)})
        o = put_block(o, exscratch::pass(g, st), exscratch::levels(g), {exscratch::centroids(g, 0), exscratch::centroids(g, 1)},
                      exscratch::sorted(g, (long)rows), exscratch::plan(g, st));
    return 0;
}

int som_debug_exact_scratch_held(som_handle* h, int64_t* out) {
    if (!h || !out) return fail(h, "som_debug_exact_scratch_held: NULL argument");
    const auto& ex = h->ex;
    const PassScratch& p = ex.pass;
    const PlanScratch& q = ex.pbuf;
    const auto held = [](const SortedRows& s) {
        return exscratch::SortedSizes{s.cap, s.order.cap, s.Xb_s.cap, s.Xl_s.cap, s.Xf_s.cap, s.xsq_s.cap, s.xerr_s.cap, s.seed_s.cap, s.sU_s.cap, s.lastpos_s.cap};
    };
    exscratch::PassSizes hp;
    hp.stride = p.stride; hp.pairs = p.pairs; hp.max_tiles = p.max_tiles;
    hp.gmin = p.gmin.cap; hp.gflags = p.gflags.cap; hp.rowcnt = p.rowcnt.cap; hp.rowarg = p.rowarg.cap; hp.seed = p.seed.cap; hp.plist = p.plist.cap;
    hp.fb_list = p.fb_list.cap; hp.tile_tab = p.tile_tab.cap; hp.ctr = p.ctr.cap;
    exscratch::CentroidSizes hc[2];
    for (int lv = 0; lv < 2; ++lv) {
        const auto& c = ex.cen.lv[lv];
        hc[lv] = {c.n_slots, c.n_cstages, c.n_img_stages, c.Cc.cap, c.rg.cap, c.csq.cap, c.cmax2.cap, c.Cst.cap, c.Cst_plain.cap};
    }
    exscratch::PlanSizes hq;
    hq.stride = q.stride; hq.tiles = q.stride / SK_TILE; hq.item_slots = q.item_slots;
    hq.sk_keys = q.sk_keys.cap; hq.sk_keys2 = q.sk_keys2.cap; hq.sk_vals = q.sk_vals.cap; hq.sk_tmp = q.sk_tmp.cap; hq.scout_g = q.scout_g.cap; hq.tq = q.tq.cap;
    hq.need = q.need.cap; hq.need2 = q.need2.cap; hq.glist = q.glist.cap; hq.gcnt = q.gcnt.cap; hq.tlist = q.tlist.cap; hq.tcnt = q.tcnt.cap;
    hq.tile_counts = q.tile_counts.cap; hq.tile_ticket = q.tile_ticket.cap; hq.items = q.items.cap;
    const exscratch::Geometry g = exact_geometry(h);
    int64_t* o = put_block(out, hp, ex.cen.ready ? exscratch::levels(g) : 0, hc, held(ex.srt[0]), hq);
    o = put_sorted(o, held(ex.srt[1]));
    put(o, {g.K, g.D, g.dp, g.stage_bytes, g.wide ? 1 : 0, g.item_slots, g.pass_rows_override, g.pairs_hook, (int64_t)p.fbX.cap, (int64_t)p.fb_ids.cap});
    return 0;
}

int som_debug_mfma16(som_handle* h, const uint16_t* a_host, const uint16_t* b_host, const float* c_host, float* d_host,
                     int32_t is_f16) {
    DeviceGuard dev_guard(h);
    if (!h || !a_host || !b_host || !c_host || !d_host) return fail(h, "som_debug_mfma16: NULL argument");
    DevBuf<uint16_t> a, b;
    DevBuf<float> c, d;
    int rc = 0;
    if ((rc = a.alloc(h, 512)) || (rc = b.alloc(h, 512)) || (rc = c.alloc(h, 256)) || (rc = d.alloc(h, 256))) return rc;
    if (h2d_blocking(h, a, a_host, 1024) || h2d_blocking(h, b, b_host, 1024) || h2d_blocking(h, c, c_host, 1024)) return 1;
    if (is_f16) debug_mfma16_kernel<F16><<<dim3(1), dim3(64), 0, h->stream>>>(a, b, c, d);
    else debug_mfma16_kernel<Bf16><<<dim3(1), dim3(64), 0, h->stream>>>(a, b, c, d);
    return d2h_blocking(h, d_host, d, 1024);
}

int som_debug_radix_sort(som_handle* h, const int32_t* keys, int64_t n, int32_t bits, int32_t* keys_out, int32_t* vals_out) {
    DeviceGuard dev_guard(h);
    if (!h || !keys || !keys_out || !vals_out) return fail(h, "som_debug_radix_sort: NULL argument");
    if (n < 1 || n > 0x7fffffffL || bits < 1 || bits > 31) return fail(h, "som_debug_radix_sort: n or bits out of range");
    DevBuf<int> kin, ko, vo, tmp;
    int rc = 0;
    if ((rc = kin.alloc(h, (size_t)n)) || (rc = ko.alloc(h, (size_t)n)) || (rc = vo.alloc(h, (size_t)n)) ||
        (rc = tmp.alloc(h, radix_scratch_ints(n)))) return rc;
    if (h2d_blocking(h, kin, keys, (size_t)n * sizeof(int))) return 1;
    if ((rc = radix_sort_rows(h, kin, n, bits, ko, vo, tmp))) return rc;
    if (d2h_blocking(h, keys_out, ko, (size_t)n * sizeof(int))) return 1;
    return d2h_blocking(h, vals_out, vo, (size_t)n * sizeof(int));
}

int som_debug_exact_select2(som_handle* h, int32_t* plist, const uint32_t* rmin, int64_t stride, int32_t* gcount, const uint32_t* thr2,
                            int32_t n_groups, int64_t n_rows, int32_t* kept_total) {
    DeviceGuard dev_guard(h);
    if (!h || !plist || !rmin || !gcount || !thr2 || !kept_total) return fail(h, "som_debug_exact_select2: NULL argument");
    if (n_groups < 1 || stride < 1 || n_rows < 1 || (int64_t)n_groups * stride > 0x7fffffffL)
        return fail(h, "som_debug_exact_select2: size out of range");
    for (int g = 0; g < n_groups; ++g) {                      // (the kernel trusts its lists: nothing runs on one that leaves its buffers)
        if (gcount[g] > stride) return fail(h, "som_debug_exact_select2: a list longer than the stride");
        for (int i = 0; i < gcount[g]; ++i)
            if (plist[g * stride + i] < 0 || plist[g * stride + i] >= n_rows) return fail(h, "som_debug_exact_select2: a list entry is no row");
    }
    const size_t cells = (size_t)n_groups * (size_t)stride;
    DevBuf<int> dl, dc, dk;
    DevBuf<uint32_t> dm, dt;
    int rc = 0;
    if ((rc = dl.alloc(h, cells)) || (rc = dm.alloc(h, cells)) || (rc = dc.alloc(h, (size_t)n_groups)) || (rc = dt.alloc(h, (size_t)n_rows)) ||
        (rc = dk.alloc(h, 1))) return rc;
    const int zero = 0;
    if (h2d_blocking(h, dl, plist, cells * sizeof(int)) || h2d_blocking(h, dm, rmin, cells * sizeof(uint32_t)) ||
        h2d_blocking(h, dc, gcount, (size_t)n_groups * sizeof(int)) || h2d_blocking(h, dt, thr2, (size_t)n_rows * sizeof(uint32_t)) ||
        h2d_blocking(h, dk, &zero, sizeof(int))) return 1;
    exact_select2_kernel<<<dim3((unsigned)n_groups), dim3(256), 0, h->stream>>>(dl, dm, stride, dc, dt, dk);
    HIPCHK(h, hipGetLastError());
    if (d2h_blocking(h, plist, dl, cells * sizeof(int)) || d2h_blocking(h, gcount, dc, (size_t)n_groups * sizeof(int))) return 1;
    return d2h_blocking(h, kept_total, dk, sizeof(int));
}

int som_debug_exact_tiles(som_handle* h, const int32_t* gcount, const int32_t* gstart, int32_t n_groups, int64_t stride, int64_t capacity,
                          int32_t blocks, int64_t table_entries, int32_t* tile_tab, int32_t* out3, int32_t* gstart_out) {
    DeviceGuard dev_guard(h);
    if (!h || !gcount || !tile_tab || !out3) return fail(h, "som_debug_exact_tiles: NULL argument");
    if (n_groups < 1 || stride < 1 || blocks < 1 || blocks > 64 || table_entries < 1 || (int64_t)n_groups * stride > 0x7fffffffL)
        return fail(h, "som_debug_exact_tiles: size out of range");
    int64_t pairs = 0, tiles = 0;
    for (int g = 0; g < n_groups; ++g) {
        const int64_t c = (int64_t)gcount[g] - (gstart ? gstart[g] : 0);
        if (c < 0) return fail(h, "som_debug_exact_tiles: a list shorter than its start");
        pairs += c; tiles += (c + EX_TR - 1) / EX_TR;
    }
    if (pairs <= capacity && tiles > table_entries) return fail(h, "som_debug_exact_tiles: the table does not hold the tiles");
    DevBuf<int> dc, ds, dso, dout;
    DevBuf<int4> dtab;
    int rc = 0;
    if ((rc = dc.alloc(h, (size_t)n_groups)) || (rc = ds.alloc(h, (size_t)n_groups)) || (rc = dso.alloc(h, (size_t)n_groups)) ||
        (rc = dout.alloc(h, 3)) || (rc = dtab.alloc(h, (size_t)table_entries))) return rc;
    if (h2d_blocking(h, dc, gcount, (size_t)n_groups * sizeof(int)) || h2d_blocking(h, dout, out3, 3 * sizeof(int)) ||
        h2d_blocking(h, dtab, tile_tab, (size_t)table_entries * sizeof(int4))) return 1;
    if (gstart && h2d_blocking(h, ds, gstart, (size_t)n_groups * sizeof(int))) return 1;
    if (gstart_out && h2d_blocking(h, dso, gstart_out, (size_t)n_groups * sizeof(int))) return 1;
    exact_tiles_kernel<<<dim3((unsigned)blocks), dim3(1024), 0, h->stream>>>(dc, n_groups, stride, capacity, dtab, dout.p, dout.p + 1,
                                                                             gstart ? ds.p : nullptr, gstart_out ? dso.p : nullptr, dout.p + 2);
    HIPCHK(h, hipGetLastError());
    if (d2h_blocking(h, tile_tab, dtab, (size_t)table_entries * sizeof(int4)) || d2h_blocking(h, out3, dout, 3 * sizeof(int))) return 1;
    return gstart_out ? d2h_blocking(h, gstart_out, dso, (size_t)n_groups * sizeof(int)) : 0;
}

int som_debug_device_bytes(int64_t* out) {
    if (!out) return 1;
    *out = g_dev_bytes.load();
    return 0;
}

int som_debug_exact_chain_stats(som_handle* h, int64_t* carried_epochs) {
    if (!h || !carried_epochs) return fail(h, "som_debug_exact_chain_stats: NULL argument");
    *carried_epochs = h->ex.stats.lastpos_carried_epochs;
    return 0;
}

int som_debug_exact_select_stats(som_handle* h, int64_t* fused_passes, int64_t* launched_passes, int64_t* ticket_tiles) {
    if (!h || !fused_passes || !launched_passes || !ticket_tiles) return fail(h, "som_debug_exact_select_stats: NULL argument");
    *fused_passes = h->ex.stats.sel_fused_passes;
    *launched_passes = h->ex.stats.sel_launched_passes;
    *ticket_tiles = h->ex.stats.sel_ticket_tiles;
    return 0;
}

int som_debug_exact_plan_stats(som_handle* h, int64_t* fused_launches, int64_t* split_launches) {
    if (!h || !fused_launches || !split_launches) return fail(h, "som_debug_exact_plan_stats: NULL argument");
    *fused_launches = h->ex.stats.plan_fused_launches;
    *split_launches = h->ex.stats.plan_split_launches;
    return 0;
}

int som_debug_exact_plan_fold_stats(som_handle* h, int64_t* folded, int64_t* compared) {
    if (!h || !folded || !compared) return fail(h, "som_debug_exact_plan_fold_stats: NULL argument");
    *folded = h->ex.stats.plan_folded;
    *compared = h->ex.stats.plan_compared;
    return 0;
}

int som_debug_plan_split(int32_t bf16, int64_t n, const float* P, const float* s_bmag, float* out4) {
    if (n < 0 || (n > 0 && (!P || !s_bmag || !out4))) return 1;
    for (int64_t i = 0; i < n; ++i) {
        const float c = bf16 ? plan_fold_scale<Bf16>(s_bmag[i]) : plan_fold_scale<F16>(s_bmag[i]);
        const PlanParts pp = bf16 ? plan_split_threshold<Bf16>(P[i], c) : plan_split_threshold<F16>(P[i], c);
        out4[4 * i] = c; out4[4 * i + 1] = pp.p1; out4[4 * i + 2] = pp.p2; out4[4 * i + 3] = pp.p3;
    }
    return 0;
}

int som_debug_band_tables(som_handle* h, int32_t* info4, int32_t* entries_out, float* P1_out, float* P2_out) {
    DeviceGuard dev_guard(h);
    if (!h || !info4) return fail(h, "som_debug_band_tables: NULL argument");
    if (h->torus) return fail(h, "som_debug_band_tables: a toroidal handle keeps two ranges per tile and segment (som_debug_band_tables_wrap)");
    const long nb = band_entries(h->X, h->Y, h->nt);
    info4[0] = h->use_bands && !h->swapped; info4[1] = h->nt; info4[2] = (int32_t)nb; info4[3] = h->band_sel;
    if (entries_out)
        if (int rc = d2h_blocking(h, entries_out, (const int2*)h->bands + (long)h->band_sel * nb, (size_t)nb * sizeof(int2))) return rc;
    if (P1_out)
        if (int rc = d2h_blocking(h, P1_out, h->P1, (size_t)h->nt * h->Y * h->Y * sizeof(float))) return rc;
    if (P2_out)
        if (int rc = d2h_blocking(h, P2_out, h->P2, (size_t)h->X * h->nt * h->X * sizeof(float))) return rc;
    return 0;
}

int som_debug_band_walk(const float* H, int32_t rows, int32_t nseg, int32_t segw, int32_t wg_rows, int32_t* tiles_out,
                        int32_t* wg_out) {
    if (!H || !tiles_out || !wg_out || rows <= 0 || nseg <= 0 || segw <= 0 || (wg_rows != 64 && wg_rows != 128)) return 1;
    const int nt = band_tiles(rows), per_wg = wg_rows / LM_TILE;
    std::vector<int2> e((size_t)nt * nseg, make_int2(0, 0));
    for (int i = 0; i < rows; ++i)
        for (int sg = 0; sg < nseg; ++sg)
            for (int k = 0; k < segw; ++k)
                if (H[((size_t)i * nseg + sg) * segw + k] != 0.0f) {
                    int2& v = e[(size_t)(i / LM_TILE) * nseg + sg];
                    v = band_entry_with(v, k, segw);
                }
    for (size_t i = 0; i < e.size(); ++i) {
        int lo, hi;
        band_tile_range(e[i], segw, lo, hi);
        tiles_out[2 * i] = lo; tiles_out[2 * i + 1] = hi;
    }
    for (int w = 0; w * wg_rows < rows; ++w) {
        int lo, hi;
        band_union(e.data() + (size_t)w * per_wg * nseg, std::min(per_wg, band_tiles(rows - w * wg_rows)), nseg, segw, LM_BK, lo, hi);
        wg_out[3 * w] = lo; wg_out[3 * w + 1] = hi; wg_out[3 * w + 2] = (hi - lo + LM_BK - 1) / LM_BK;
    }
    return 0;
}

int som_debug_band_tables_wrap(som_handle* h, int32_t* info4, int32_t* entries_out, float* P1_out, float* P2_out) {
    DeviceGuard dev_guard(h);
    if (!h || !info4) return fail(h, "som_debug_band_tables_wrap: NULL argument");
    if (!h->torus) return fail(h, "som_debug_band_tables_wrap: not a toroidal handle (som_debug_band_tables)");
    const long nb = 2 * band_entries(h->X, h->Y, h->nt);
    info4[0] = h->use_bands; info4[1] = h->nt; info4[2] = (int32_t)nb; info4[3] = h->band_sel;
    if (entries_out)
        if (int rc = d2h_blocking(h, entries_out, (const int2*)h->bands + (long)h->band_sel * nb, (size_t)nb * sizeof(int2))) return rc;
    if (P1_out)
        if (int rc = d2h_blocking(h, P1_out, h->P1, (size_t)h->nt * h->Y * h->Y * sizeof(float))) return rc;
    if (P2_out)
        if (int rc = d2h_blocking(h, P2_out, h->P2, (size_t)h->X * h->nt * h->X * sizeof(float))) return rc;
    return 0;
}

int som_debug_band_walk_wrap(const float* H, int32_t rows, int32_t nseg, int32_t segw, int32_t wg_rows, int32_t* tiles_out,
                             int32_t* wg_out) {
    if (!H || !tiles_out || !wg_out || rows <= 0 || nseg <= 0 || segw <= 0 || (wg_rows != 64 && wg_rows != 128)) return 1;
    const int nt = band_tiles(rows), per_wg = wg_rows / LM_TILE;
    std::vector<int2> e((size_t)nt * nseg * 2, make_int2(0, 0));
    for (int i = 0; i < rows; ++i)
        for (int sg = 0; sg < nseg; ++sg)
            for (int k = 0; k < segw; ++k)
                if (H[((size_t)i * nseg + sg) * segw + k] != 0.0f) {
                    int2& v = e[((size_t)(i / LM_TILE) * nseg + sg) * 2 + band_wrap_piece(k, segw)];
                    v = band_entry_with(v, k, segw);
                }
    for (size_t i = 0; i < e.size(); ++i) {
        int lo, hi;
        band_tile_range(e[i], segw, lo, hi);
        tiles_out[2 * i] = lo; tiles_out[2 * i + 1] = hi;
    }
    for (int w = 0; w * wg_rows < rows; ++w)
        for (int piece = 0; piece < 2; ++piece) {
            int lo, hi;
            band_union(e.data() + (size_t)w * per_wg * nseg * 2 + piece, std::min(per_wg, band_tiles(rows - w * wg_rows)), nseg, segw,
                       piece ? LM_KG : LM_BK, lo, hi, 2);          // (as leftmul_f32_body rounds the two lower ends)
            int32_t* o = wg_out + (2 * w + piece) * 3;
            o[0] = lo; o[1] = hi; o[2] = (hi - lo + LM_BK - 1) / LM_BK;
        }
    return 0;
}

int som_debug_exact_last_plan(som_handle* h, int32_t* out8) {
    if (!h || !out8) return fail(h, "som_debug_exact_last_plan: NULL argument");
    const policy::LaunchPlan& p = h->ex.lp;
    out8[0] = p.skip; out8[1] = p.resort; out8[2] = p.scout; out8[3] = p.level2; out8[4] = p.estimate; out8[5] = p.sample_tiles;
    out8[6] = p.refine; out8[7] = p.time_phases;
    return 0;
}

// TEST HOOK, read-only: what the last launch_bmu_exact learned from its samples (plain numbers the host stored where it computed
// them: launch_bmu_exact, exact_sample_tiles) and the handle's running count of declined estimates.  Layout: include/somhip_test.h.
int som_debug_exact_forecast(som_handle* h, double* out12) {
    if (!h || !out12) return fail(h, "som_debug_exact_forecast: NULL argument");
    const auto& fc = h->ex.fc;
    out12[0] = fc.need; out12[1] = fc.rows; out12[2] = fc.est; out12[3] = fc.est1; out12[4] = fc.n_st; out12[5] = fc.st;
    out12[6] = fc.blocks_run; out12[7] = fc.groups_run; out12[8] = (double)h->ex.plan.stats().scout_declined; out12[9] = fc.level2;
    out12[10] = h->ex.plan.costs().full_total; out12[11] = h->ex.plan.costs().full_screen;
    return 0;
}

// TEST HOOK, read-only: the lengths of the tiles' lists as the screen of the last pass of the last launch walked them -- tcnt (16-unit
// blocks) and tile_counts (groups level 1 kept), the numbers exact_list_totals_body sums into the pass's counters.  Nothing is
// launched, no state changed.  Layout: include/somhip_test.h.
int som_debug_exact_tile_blocks(som_handle* h, int32_t* blocks_out, int32_t* groups_out, int64_t n_tiles, int32_t* info2) {
    DeviceGuard dev_guard(h);
    if (!h || !info2 || n_tiles < 0) return fail(h, "som_debug_exact_tile_blocks: bad argument");
    const auto& ex = h->ex;
    info2[0] = (int32_t)ex.last_plan_tiles; info2[1] = ex.last_plan_l2 ? 1 : 0;
    if (n_tiles == 0 || (!blocks_out && !groups_out)) return 0;
    if (ex.last_plan_tiles <= 0) return fail(h, "som_debug_exact_tile_blocks: the last launch ran no planned pass (up to 128 features)");
    if (n_tiles > ex.last_plan_tiles || n_tiles * SK_TILE > ex.pbuf.stride) return fail(h, "som_debug_exact_tile_blocks: the last planned pass had fewer tiles");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (blocks_out) if (int rc = d2h_blocking(h, blocks_out, ex.pbuf.tcnt, (size_t)n_tiles * sizeof(int32_t))) return rc;
    if (groups_out) {
        std::vector<int2> tc((size_t)n_tiles);
        if (int rc = d2h_blocking(h, tc.data(), ex.pbuf.tile_counts, (size_t)n_tiles * sizeof(int2))) return rc;
        for (int64_t t = 0; t < n_tiles; ++t) groups_out[t] = tc[(size_t)t].y;
    }
    return 0;
}

int som_debug_qe_stats(som_handle* h, int64_t* rows, int64_t* rows_sqrt) {
    if (!h || !rows || !rows_sqrt) return fail(h, "som_debug_qe_stats: NULL argument");
    *rows = h->qe_rows;
    *rows_sqrt = h->qe_rows_sqrt;
    return 0;
}

// Diagnostic builds only (-DSOM_STAMPS): hand the BMU kernels a buffer for their in-kernel clock stamps (n_pairs
// workgroups' worth; NULL detaches it), or read it back.  In the product build both calls fail with a message.
int som_debug_stamps(som_handle* h, int64_t n_pairs, uint64_t* out_host) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
#ifdef SOM_STAMPS
    static unsigned long long* buf = nullptr;
    static int64_t cap = 0;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (out_host) {
        if (n_pairs > cap) return fail(h, "som_debug_stamps: more pairs than the buffer holds");
        HIPCHK(h, hipMemcpy(out_host, buf, (size_t)n_pairs * 16, hipMemcpyDeviceToHost));
        return 0;
    }
    if (buf) { (void)hipFree(buf); buf = nullptr; cap = 0; }
    if (n_pairs > 0) {
        HIPCHK(h, hipMalloc((void**)&buf, (size_t)n_pairs * 16));
        HIPCHK(h, hipMemset(buf, 0, (size_t)n_pairs * 16));
        cap = n_pairs;
    }
    HIPCHK(h, hipMemcpyToSymbol(HIP_SYMBOL(g_som_stamps), &buf, sizeof(buf)));
    return 0;
#else
    (void)n_pairs; (void)out_host;
    return fail(h, "som_debug_stamps: this library was built without -DSOM_STAMPS (tools/stamps.py builds the diagnostic one)");
#endif
}

int som_patch_order(int32_t x, int32_t y, int32_t* perm_out) {
    if (x <= 0 || y <= 0 || !perm_out || (int64_t)x * y > 0x7fffffffLL) return 1;
    std::vector<int> perm;
    patch_order(x, y, perm);
    std::copy(perm.begin(), perm.end(), perm_out);
    return 0;
}

int som_exact_stats(som_handle* h, int64_t* rows, int64_t* rows_fallback, int64_t* passes) {
    if (!h) return 1;
    if (rows) *rows = h->ex.stats.rows_total;
    if (rows_fallback) *rows_fallback = h->ex.stats.rows_fallback;
    if (passes) *passes = h->ex.stats.chunks;
    return 0;
}

int som_exact_top2_stats(som_handle* h, int64_t* rows, int64_t* rows_f32) {
    if (!h || !rows || !rows_f32) return fail(h, "som_exact_top2_stats: NULL argument");
    *rows = h->t2.rows; *rows_f32 = h->t2.rows_f32;
    return 0;
}

int som_exact_skip_stats(som_handle* h, int64_t* blocks_run, int64_t* blocks_total) {
    if (!h || !blocks_run || !blocks_total) return 1;
    *blocks_run = h->ex.stats.blocks_run; *blocks_total = h->ex.stats.blocks_total;
    return 0;
}

int som_exact_resident_stats(som_handle* h, int64_t* planned_epochs, int64_t* sorts) {
    if (!h || !planned_epochs || !sorts) return 1;
    *planned_epochs = h->ex.plan.stats().planned; *sorts = h->ex.plan.stats().resorts;
    return 0;
}

int som_exact_scout_stats(som_handle* h, int64_t* scouted_launches, int64_t* transient_planned) {
    if (!h || !scouted_launches || !transient_planned) return 1;
    *scouted_launches = h->ex.plan.stats().scouted; *transient_planned = h->ex.plan.stats().tr_planned;
    return 0;
}

int som_exact_refine_stats(som_handle* h, int64_t* pairs_in, int64_t* pairs_out) {
    if (!h || !pairs_in || !pairs_out) return 1;
    *pairs_in = h->ex.plan.stats().pairs_refined_in; *pairs_out = h->ex.plan.stats().pairs_refined_out;
    return 0;
}

int som_exact_last_counts(som_handle* h, int32_t* counts_out, int64_t n) {
    DeviceGuard dev_guard(h);
    if (!h || !counts_out || n < 0) return fail(h, "som_exact_last_counts: bad argument");
    if (!h->exact || n > h->ex.pass.stride) return fail(h, "som_exact_last_counts: no screen pass of that many rows");
    if (int rc = d2h_blocking(h, counts_out, h->ex.pass.rowcnt, (size_t)n * sizeof(int32_t))) return rc;
    return 0;
}

int som_sync(som_handle* h) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int som_profile_enable(som_handle* h, int32_t on) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    if (!on) if (int rc = resolve_profile(h)) return rc;
    h->prof = on == 2 ? 2 : on != 0;
    return 0;
}

int som_profile_get(som_handle* h, int32_t kernel, double* total_ms, int64_t* launches) {
    DeviceGuard dev_guard(h);
    if (!h || kernel < 0 || kernel >= SOM_K_COUNT) return fail(h, "som_profile_get: bad argument");
    if (int rc = resolve_profile(h)) return rc;
    if (total_ms) *total_ms = h->ms[kernel];
    if (launches) *launches = h->launches[kernel];
    return 0;
}

int som_profile_reset(som_handle* h) {
    DeviceGuard dev_guard(h);
    if (!h) return 1;
    if (int rc = resolve_profile(h)) return rc;
    for (int i = 0; i < SOM_K_COUNT; ++i) { h->ms[i] = 0; h->launches[i] = 0; }
    return 0;
}

}  // extern "C"
