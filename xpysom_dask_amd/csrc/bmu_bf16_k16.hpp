// Fused distance + BMU argmin, bf16, on v_mfma_f32_16x16x32_bf16.
//
// The arithmetic of bmu_bf16.hpp (d' = B + |w~|^2/2 - x~.w~, the norm term as the MFMA's initial accumulator) on a
// stage image in MFMA fragment order.  On random data MI355X holds a higher clock on the 16x16x32 shape than on
// 32x32x16 at equal cycles per flop (MI355X_MICROARCH.md, DVFS give-back item 7), and this kernel is
// power/clock-limited, so the shape is a throughput lever by itself (round 1's 32x32x16 form took 13.99 ms where this one took 11.88).
//
// Geometry: A = 16 units x 32 features (lane l: unit l&15, features 8*(l>>4)+j), B = 32 features x
// 16 samples (lane l: sample l&15), C/D: lane holds sample l&15, units 4*(l>>4)+reg, reg 0..3.
// A wave keeps 4 x 16 samples' B fragments in registers; one A fragment read from LDS feeds 4 MFMAs.
// Stage image (K16_STAGE_UNITS = 64 units): [t16 0..3][kstep32][lane 0..63][8 bf16 of -w~] + [64 x f32 B+|w~|^2/2]
// (+ pad to 1 KiB).
// Key = (bits & ~mask) | (t16<<2 | reg).
//
// Grid = (sample blocks) x (codebook parts): a workgroup scans only its part of the stages and
// merges its winner into out64[n] = (value bits << 32 | unit) with a 64-bit atomicMin.  The host
// picks the number of parts so that the grid fills whole rounds of the resident workgroup slots
// (4096 blocks on 768 slots would idle 11 % in the last round; 4096 x 3 parts is exactly 16).
#pragma once
#include "bmu_bf16.hpp"
#include "exact_scratch.hpp"   // K16_T, K16_STAGE_UNITS (16-unit tiles per stage, units per stage): beside the rule that sizes the exact mode's buffers by them

namespace somhip {

constexpr int K16_SB = 4;             // 16-sample blocks per wave
constexpr int K16_NW = 4;             // waves per workgroup (they share one LDS ring)
constexpr int K16_WG_SAMPLES = K16_NW * 16 * K16_SB;

__host__ __device__ constexpr int k16_stage_bytes(int ks32) { return (K16_T * ks32 + 1) * 1024; }

template <int KS32, class EL = Bf16>
__global__ __launch_bounds__(256) void prep_w_bf16_k16_kernel(const float* __restrict__ W, int K, int D,
                                                              char* __restrict__ Wst, int n_stages,
                                                              const float* __restrict__ unit_wsq,
                                                              const float* __restrict__ scale_max2 = nullptr) {
    using E = typename EL::T;
    using bf16x8 = typename V8<E>::t;
    long id = (long)blockIdx.x * 256 + threadIdx.x;
    long total = (long)n_stages * K16_T * KS32 * 64;
    if (id >= total) return;
    int lane = id & 63;
    long t = id >> 6;
    int ks = t % KS32; t /= KS32;
    int t16 = t % K16_T;
    long stage = t / K16_T;
    long u = stage * K16_STAGE_UNITS + t16 * 16 + (lane & 15);
    int k0 = ks * 32 + (lane >> 4) * 8;
    // cosine distance (distances.py:45-59): rows are scaled to unit length, so that
    // argmin_k (B - x~ . w^~_k) == argmin_k (1 - x.w_k/(|x||w_k|)); a zero row stays zero
    // (its similarity is nan_to_num(0/0) = 0 in the reference, and x~ . 0 = 0 here).
    float scale = 1.0f;
    if (unit_wsq != nullptr && u < K) { float q = unit_wsq[u]; scale = q > 0.0f ? 1.0f / __builtin_sqrtf(q) : 0.0f; }
    if (scale_max2 != nullptr) scale = ex_scale(*scale_max2);   // exact mode on half operands: a power of two
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float f = (u < K && k0 + j < D) ? W[u * D + k0 + j] * scale : 0.0f;
        v[j] = cvt<E>(-f);
    }
    *(bf16x8*)(Wst + stage * k16_stage_bytes(KS32) + ((long)(t16 * KS32 + ks) * 64 + lane) * 16) = v;
}

// The exact mode's codebook preparation up to 128 features (bmu_exact.hpp): the stage image of the units scaled by the power
// of two ex_scale(*scale_max2) AND max_k |w^_k - w~_k|^2, what the MFMA will read instead of the scaled float32 units
// (half_operand_error), in one pass -- prep_w_bf16_k16_kernel + exact_werr_kernel.  One wave per 16-unit tile walks the
// tile's KS32 feature chunks (lane = (unit, 8 features) of each: one 16-byte fragment chunk of the image per chunk), so a
// unit's error is four lanes of one wave.
// Wst_lo (or null): the same fragments of the units' SECOND half -- lo = half(2^11 ((-w^) - hi)), so that -w^ = hi + 2^-11 lo up
// to 2^-11 of lo's own magnitude: what the exact mode's refinement pass (bmu_exact.hpp) multiplies beside hi.
// cm1 / cm2 (or null): the {max |c|^2, max rounding error^2} pairs of the plan's two centroid levels, reset here as
// exact_centroids_kernel resets them when the fused merge (exact_skip.hpp) has written the centroids before the maximum was known.
// (the body, for block `bid` of 256 threads -- shared with exact_prep_images_kernel, exact_skip.hpp, whose centroid blocks are
//  already adding to the levels' error maxima while this one runs: cm_err false leaves those words to them)
template <int KS32, class EL>
__device__ __forceinline__ void prep_w_exact_k16_body(const unsigned bid, const float* __restrict__ W, int K, int D,
                                                      char* __restrict__ Wst, int n_stages,
                                                      const float* __restrict__ scale_max2,
                                                      float* __restrict__ werr2, char* __restrict__ Wst_lo,
                                                      float* __restrict__ cm1, float* __restrict__ cm2, const bool cm_err) {
    using E = typename EL::T;
    using bf16x8 = typename V8<E>::t;
    const int lane = threadIdx.x & 63;
    if (cm1 != nullptr && bid == 0 && threadIdx.x == 0) {
        cm1[0] = *scale_max2; cm2[0] = *scale_max2;
        if (cm_err) { cm1[1] = 0.0f; cm2[1] = 0.0f; }
    }
    const long tile = (long)bid * 4 + (threadIdx.x >> 6);                 // (stage, t16)
    if (tile >= (long)n_stages * K16_T) return;
    const long stage = tile / K16_T;
    const int t16 = (int)(tile - stage * K16_T);
    const long u = stage * K16_STAGE_UNITS + t16 * 16 + (lane & 15);
    const float scale = ex_scale(*scale_max2);
    float er = 0.0f;
#pragma unroll
    for (int ks = 0; ks < KS32; ++ks) {
        const int k0 = ks * 32 + (lane >> 4) * 8;
        bf16x8 v, vl;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float f = (u < K && k0 + j < D) ? W[u * D + k0 + j] * scale : 0.0f;
            const E hb = cvt<E>(-f);
            v[j] = hb;
            const float e = half_operand_error(-f, (float)hb);
            er = __builtin_fmaf(e, e, er);
            const float r = ((-f) - (float)hb) * 2048.0f;     // (exact: a float32 difference of neighbours, a power of two)
            vl[j] = cvt<E>(r == r && __builtin_fabsf(r) < 3.0e38f ? r : 0.0f);
        }
        *(bf16x8*)(Wst + stage * k16_stage_bytes(KS32) + ((long)(t16 * KS32 + ks) * 64 + lane) * 16) = v;
        if (Wst_lo != nullptr) *(bf16x8*)(Wst_lo + stage * k16_stage_bytes(KS32) + ((long)(t16 * KS32 + ks) * 64 + lane) * 16) = vl;
    }
    er += __shfl_xor(er, 16, 64);                            // the unit's four feature quarters
    er += __shfl_xor(er, 32, 64);
    float m = (er == er) ? er : 0.0f;                        // (a NaN unit is left out, as in exact_werr_kernel)
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) atomic_max_pos_f32(werr2, m);
}
template <int KS32, class EL = Bf16>
__global__ __launch_bounds__(256) void prep_w_exact_k16_kernel(const float* __restrict__ W, int K, int D,
                                                               char* __restrict__ Wst, int n_stages,
                                                               const float* __restrict__ scale_max2,
                                                               float* __restrict__ werr2, char* __restrict__ Wst_lo = nullptr,
                                                               float* __restrict__ cm1 = nullptr, float* __restrict__ cm2 = nullptr) {
    prep_w_exact_k16_body<KS32, EL>(blockIdx.x, W, K, D, Wst, n_stages, scale_max2, werr2, Wst_lo, cm1, cm2, true);
}

// _merge_updates (xpysom.py:446-455) fused with the NEXT epoch's operand preparation: one pass over the fused
// accumulator writes the merged float32 codebook, the bf16 stage image of -w~ and |w~_k|^2 (+ its maximum),
// i.e. merge_kernel + prep_w_bf16_k16_kernel + prep_wnorm_kernel (euclidean) in one launch and one read of
// the codebook.  Workgroup = MP_TILES 16-unit tiles, KS32 waves; thread = (unit, 8 features) of each tile, exactly one
// 16-byte fragment chunk of the image.  W = where(den != 0, num / den, W) as merge_kernel computes it.
constexpr int MP_TILES = 4;           // 16-unit tiles per workgroup: their loads are all issued before the first is used
template <int KS32, class EL = Bf16>
__global__ __launch_bounds__(64 * KS32) void merge_prep_k16_kernel(float* __restrict__ W, const float* __restrict__ ACC,
                                                                 int K, int D, int D1p, char* __restrict__ Wst,
                                                                 float* __restrict__ wn, float* __restrict__ wmax2,
                                                                 long n_tiles) {
    using E = typename EL::T;
    using bf16x8 = typename V8<E>::t;
    __shared__ float red[MP_TILES][KS32][16];
    const int lane = threadIdx.x & 63, ks = threadIdx.x >> 6;
    const int k0 = ks * 32 + (lane >> 4) * 8;
    const bool full = k0 + 8 <= D && (D & 3) == 0;         // 16-byte aligned rows on both sides (D1p is a multiple of 4)
    float w[MP_TILES][8], den[MP_TILES];
    long unit[MP_TILES];
#pragma unroll
    for (int i = 0; i < MP_TILES; ++i) {                   // phase 1: every load of the workgroup's tiles
        const long tile = (long)blockIdx.x * MP_TILES + i;
        const long stage = tile / K16_T;
        const long u = stage * K16_STAGE_UNITS + (tile - stage * K16_T) * 16 + (lane & 15);
        unit[i] = (tile < n_tiles && u < K) ? u : -1;
        den[i] = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) w[i][j] = 0.0f;
        if (unit[i] >= 0) {
            den[i] = ACC[u * D1p + D];
            if (full) {
                const f32x4 a = *(const f32x4*)(ACC + u * D1p + k0), c = *(const f32x4*)(ACC + u * D1p + k0 + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { w[i][j] = a[j]; w[i][4 + j] = c[j]; }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (k0 + j < D) w[i][j] = ACC[u * D1p + k0 + j];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MP_TILES; ++i) {                   // phase 2: merge, codebook row, stage image, norm partials
        const long tile = (long)blockIdx.x * MP_TILES + i;
        const long stage = tile / K16_T;
        const int t16 = (int)(tile - stage * K16_T);
        const long u = unit[i];
        if (u >= 0) {
            if (den[i] != 0.0f) {
#pragma unroll
                for (int j = 0; j < 8; ++j) w[i][j] = w[i][j] / den[i];
                if (full) {
                    f32x4 q0, q1;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { q0[j] = w[i][j]; q1[j] = w[i][4 + j]; }
                    *(f32x4*)(W + u * D + k0) = q0;
                    *(f32x4*)(W + u * D + k0 + 4) = q1;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (k0 + j < D) W[u * D + k0 + j] = w[i][j];
                }
            } else {                                       // no row in reach of this unit: the old weights stay
#pragma unroll
                for (int j = 0; j < 8; ++j) w[i][j] = (k0 + j < D) ? W[u * D + k0 + j] : 0.0f;
            }
        }
        if (tile < n_tiles) {
            bf16x8 v;
            float s = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const E b = cvt<E>(w[i][j]);
                v[j] = cvt<E>(-w[i][j]);                 // (rounding is sign-symmetric: -bf16(w) == bf16(-w))
                const float f = (float)b;
                s = __builtin_fmaf(f, f, s);
            }
            *(bf16x8*)(Wst + stage * k16_stage_bytes(KS32) + ((long)(t16 * KS32 + ks) * 64 + lane) * 16) = v;
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            if (lane < 16) red[i][ks][lane] = s;
        }
    }
    __syncthreads();
    if (ks == 0 && lane < 16) {
        float m = 0.0f;
#pragma unroll
        for (int i = 0; i < MP_TILES; ++i) {
            float t = 0.0f;
#pragma unroll
            for (int q = 0; q < KS32; ++q) t += red[i][q][lane];
            if (unit[i] >= 0) { wn[unit[i]] = t; m = fmaxf(m, t); }
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if (lane == 0) atomic_max_pos_f32(wmax2, m);
    }
}

// The chunk walk of the exact mode's candidate selection (bmu_exact.hpp, step 2), for ONE wave and the 64 rows of row block rb
// (lane <-> row): the groups [g_begin, g_end) of all groups -- or, my_list != nullptr, of a tile's list (entries group << 4 | mask).
// The wave reads the masks of 64 groups with one coalesced load (lane = group), walks the groups whose mask is not empty --
// eight at a time, so that their value loads are in flight together --, loads only the stored rows' values (src = gmin + row)
// and keeps the ones at or below thr (bit patterns: every d' is a positive float, a NaN pattern is above every threshold;
// ok false: the row selects nothing).  The 64 lanes test the SAME group at the same time: a group's hits take consecutive
// positions of its list from ONE returning atomic per wave and 64 groups (lane j adds group j's population and hands out the
// base).  Returns the row's number of hits.  ROUND2: the group `arg` is left out (exact_select_kernel).
// Two callers: exact_select_kernel, a launch of its own, and the listed screen's select tail below.
template <bool ROUND2>
__device__ __forceinline__ int ex_select_walk(const uint32_t* __restrict__ src, const unsigned long long* __restrict__ gflags,
                                              long gm_stride, int n_groups, long rb, long row, int lane, bool ok, uint32_t thr,
                                              int arg, const int* __restrict__ my_list, int g_begin, int g_end,
                                              int* __restrict__ plist, int* __restrict__ gcount) {
    const unsigned long long below = (1ull << lane) - 1;
    int mine = 0;
    for (int gb = g_begin; gb < g_end; gb += 64) {
        // lane j <-> the j-th group of this chunk
        const int gid = gb + lane < g_end ? (my_list != nullptr ? (my_list[gb + lane] >> 4) : gb + lane) : -1;
        const unsigned long long fw = gid >= 0 ? gflags[ex_flag_index(rb, gid, n_groups, gm_stride)] : 0ull;
        const unsigned long long any = __ballot(fw != 0ull);
        if (any == 0) continue;
        const uint32_t fw_lo = (uint32_t)fw, fw_hi = (uint32_t)(fw >> 32);
        unsigned long long hits = 0;                       // bit j: the chunk's j-th group is a candidate of this lane's row
        unsigned long long todo = any;
        while (todo != 0) {
            int j[8];
            uint32_t v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                j[q] = todo != 0 ? (int)__builtin_ctzll(todo) : -1;
                if (todo != 0) todo &= todo - 1;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                v[q] = 0xFFFFFFFFu;
                if (j[q] >= 0) {                           // (wave-uniform)
                    const unsigned long long stored = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)fw_hi, j[q]) << 32) |
                                                      (uint32_t)__builtin_amdgcn_readlane((int)fw_lo, j[q]);
                    const int g = __builtin_amdgcn_readlane(gid, j[q]);
                    if ((stored >> lane) & 1ull) v[q] = src[(long)g * gm_stride];   // (only the rows the screen stored)
                }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (j[q] >= 0) {
                    // (ROUND2: the group round 1 scored for this row is not selected again -- by its id: under a tile list
                    //  the chunk's j-th group is not group gb + j)
                    const int g = __builtin_amdgcn_readlane(gid, j[q]);
                    hits |= (unsigned long long)(v[q] <= thr && !(ROUND2 && g == arg)) << j[q];
                }
        }
        if (!ok) hits = 0;
        if (__ballot(hits != 0ull) == 0) continue;
        int c = 0;                                         // lane j: the wave's hits in the chunk's j-th group
        for (todo = any; todo != 0; todo &= todo - 1) {
            const int jj = (int)__builtin_ctzll(todo);
            const unsigned long long mk = __ballot((hits >> jj) & 1ull);
            if (lane == jj) c = (int)__builtin_popcountll(mk);
        }
        int base = 0;
        if (c > 0) base = atomicAdd(gcount + gid, c);
        for (todo = any; todo != 0; todo &= todo - 1) {
            const int jj = (int)__builtin_ctzll(todo);
            const unsigned long long mk = __ballot((hits >> jj) & 1ull);
            if (mk == 0) continue;
            const int o = __builtin_amdgcn_readlane(base, jj);
            const int g = __builtin_amdgcn_readlane(gid, jj);
            if ((hits >> jj) & 1ull) plist[(long)g * gm_stride + o + (int)__builtin_popcountll(mk & below)] = (int)row;
        }
        mine += (int)__builtin_popcountll(hits);
    }
    return mine;
}

// What the listed screen's SELECT TAIL (below) walks and writes: the select kernel's inputs and outputs under a plan.
// plist == nullptr: no tail -- the screen ends as it always did and exact_select_kernel is a launch of its own.
struct ScreenSelect {
    const int* glist = nullptr;       // per tile: (group << 4 | sub-block mask), the groups the plan kept ...
    const int* gcnt = nullptr;        // ... and how many
    int* plist = nullptr;             // [n_groups][gm_stride] the groups' row lists
    int* gcount = nullptr;            // [n_groups] their fill cursors
    int* rowcnt = nullptr;            // [rows] candidate groups per row
    uint32_t* rowmin2_init = nullptr; // a launch that refines: the rows' refined minima start from all ones (or null)
    int* tile_ticket = nullptr;       // [tiles] arrivals of a cut tile's parts; zero at the pass's start (exact_lists_tile)
    int* ticket_tiles = nullptr;      // PassCounters::ticket_tiles
};

// GM (precision 'exact', bmu_exact.hpp): the kernel keeps VALUES only -- the row minimum (out64's upper half; no unit
// indices exist in this instance, the float32 re-score names the unit) and, per stage (= one GROUP of 64 units) and row,
// the group's minimum.  A lane holds its quad's minimum for each of the wave's 4 sample blocks; three v_permlane*_swap +
// v_min steps transpose and reduce so that quad q ends with the full minimum of sample block q -- lane l then owns row
// wave_s0 + l.  A group minimum can only matter to the scan if it is within the row's bound E of the FINAL row minimum,
// hence of the minimum so far: only those are stored (gmin[stage * gm_stride + row], exec-masked), and every wave and
// stage leaves the 64-bit mask of the lanes it stored in gflags[(row / 64) * n_stages + stage] -- on a random
// codebook ~2 % of the matrix is written and read, on the smoothest maps 10-25 %.
// TL (block skipping, exact_skip.hpp): the workgroup walks its tile's dense LIST of 16-unit tiles (group << 2 | sub-block)
// instead of all stages; only the listed tiles' fragments are staged and multiplied.  With GM: the exact mode's screen
// under a plan.  Without: the scout's pick of a pseudo last BMU among a tile's few listed groups (unit indices kept).
// T2 (with GM, never TL: the exact mode's TOP-2 screen, bmu_exact.hpp "top-2"): the window hangs on the SECOND-smallest group
// minimum so far -- a lane keeps the two smallest group minima of its row (two registers more), a group minimum is stored where
// it is within E of the second one, and every part of the codebook hands back its own pair (t2min[(2 part + {0, 1}) t2pitch + row]:
// the second-smallest of a part is never below the second-smallest of all parts; exact_select_kernel<false, true> merges them).
// SEL (with GM and TL, on the work queue below; sel->plist != nullptr): the SELECT TAIL.  At the end of a tile's walk lane l holds
// what exact_select_kernel rebuilds its threshold from -- the row's minimum, its bound E, the seed's cap -- and the masks and
// values that kernel would walk were written a moment ago by this very wave: the wave selects for its own 64 rows here
// (ex_select_walk over the tile's glist), in the shadow of the CU's other workgroups' MFMAs, and the launch of
// exact_select_kernel<false> behind the screen is gone.  What is selected is bit for bit what that kernel selects: the
// threshold is the same float expression min(m + E, seed + float32 share) with the same "finite and positive" guard.
//   A tile with ONE item: the row minimum never leaves the registers -- no atomicMin into out64, which keeps the all-ones the
//   re-score's merge expects.  Masks (this wave's lane 0) and values (the reading lane itself) come back from this CU: a
//   workgroup-scope release / acquire between the walk's stores and the tail's loads.
//   A tile CUT into parts: every part ends as before (stores, atomicMin into out64), publishes -- every storing wave drains,
//   workgroup barrier, one lane: agent-scope release fence, an explicit wait, a relaxed agent-scope add on the tile's ticket --
//   and the part whose add returns parts - 1 is last: it acquires (agent scope: the parts may have run on other XCDs and share
//   128-byte lines of gflags, cut as they are at group boundaries), reads its rows' minima from out64, puts all ones back and
//   runs the tail.  Plain stores + one release fence rather than write-through stores: the walk's stores sit in fold_stage, in
//   the MFMA loop, which this must not touch, and a part releases once.  Nobody waits for anybody: no poll, no spin.
//   EVERY ROW EXACTLY ONCE: exact_list_totals_body gives every tile at least one item (parts_of(0) == 1: a tile whose list is
//   empty too) and the parts of a tile draw the tickets 0 .. parts - 1 exactly once, so exactly one workgroup per tile runs
//   the tail -- rowcnt, rowmin2_init and the merge keys of every row of the pass are written once, as the select kernel did.
// (the kernel's body for one workgroup's worth of rows: tile bx of K16_WG_SAMPLES rows, part by of ny of the codebook stages -- or,
//  TL, of the tile's list.  The kernel below calls it once, or -- the exact mode's screen under a plan -- once per work item.)
template <int KS32, class EL, bool GM, bool TL, bool T2 = false, bool SEL = false>
__device__ __forceinline__ void bmu_bf16_k16_body(const __bf16* __restrict__ Xb, long N,
                                                  const char* __restrict__ Wst, int n_stages, int K,
                                                  unsigned long long* __restrict__ out64,
                                                  uint32_t* __restrict__ gmin, long gm_stride,
                                                  unsigned long long* __restrict__ gflags,
                                                  const float* __restrict__ xsq, const float* __restrict__ xerr,
                                                  const float* __restrict__ xmax2, const float* __restrict__ wmax2,
                                                  const float* __restrict__ werr2, const ExactBound& eb,
                                                  const float* __restrict__ seed, const int* __restrict__ glist,
                                                  const int* __restrict__ gcnt, const long bx, const int by, const int ny,
                                                  float* __restrict__ t2min = nullptr, long t2pitch = 0,
                                                  const ScreenSelect* sel = nullptr, int* s_word = nullptr) {
    static_assert(!T2 || (GM && !TL), "the top-2 screen is the group-minimum instance over every stage");
    static_assert(!SEL || (GM && TL), "the select tail belongs to the listed group-minimum screen");
    using E = typename EL::T;
    using bf16x8 = typename V8<E>::t;
    constexpr int DP = 32 * KS32;
    constexpr int STAGE = k16_stage_bytes(KS32);
    constexpr int PIECES = K16_T * KS32 + 1;
    constexpr uint32_t IDX_MASK = 4 * K16_T - 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int quad = lane >> 4, col = lane & 15;
    const long wave_s0 = bx * K16_WG_SAMPLES + wave * (16 * K16_SB);

    bf16x8 xf[K16_SB][KS32];
#pragma unroll
    for (int sb = 0; sb < K16_SB; ++sb) {
        const long row = wave_s0 + sb * 16 + col;
#pragma unroll
        for (int ks = 0; ks < KS32; ++ks) xf[sb][ks] = *(const bf16x8*)(Xb + row * DP + ks * 32 + quad * 8);
    }

    uint32_t gbest[K16_SB], cbest[K16_SB];   // unsigned: a NaN (either sign) is above every finite positive d'
    int gstage[K16_SB];
    f32x4 accP[K16_SB];
#pragma unroll
    for (int sb = 0; sb < K16_SB; ++sb) {
        gbest[sb] = 0xFFFFFFFFu; cbest[sb] = 0xFFFFFFFFu; gstage[sb] = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) accP[sb][r] = __builtin_inff();
    }

    float run_min = __builtin_inff(), row_e = 0.0f;       // GM: lane l <-> row wave_s0 + l: its minimum so far, its bound E
    int run_arg = 0;                                      //     ... and the group (stage) that holds it
    float run_cap = __builtin_inff();                     //     ... and the seed's cap on what can be selected at all
    float run_min2 = __builtin_inff();                    // T2: ... and its second-smallest group minimum so far
    if (GM) {
        const long r = wave_s0 + lane;
        row_e = r < N ? ex_row_bound(eb, ex_scales(xmax2, wmax2, werr2), xsq[r], xerr[r]) : __builtin_nanf("");
        if (!(row_e == row_e)) row_e = __builtin_inff();   // a row the bound does not cover: keep everything (the scan drops it)
        // seed (exact_seed_kernel): d'(t) + E/2 for the float32 score t of ONE unit of the row's choice (last epoch's BMU),
        // known before the scan.  A unit that beats that one in the float32 kernel has a screen value of at most seed +
        // the float32 share of E (exact_select_kernel applies the same cap): no group minimum above it is ever selected
        if (seed != nullptr && r < N) {
            const float sd = seed[r] + ex_f32_share(eb, ex_scales(xmax2, wmax2, werr2), xsq[r]);
            if (sd == sd) run_cap = sd;
        }
    }
    // this workgroup's share of the codebook stages: the loop index s walks [s_begin, s_end)  (TL: see the tile-list loop below)
    // (TL without GM: the scout of exact_skip.hpp -- the plain kernel, unit indices kept, over a tile's few listed groups)
    const int n_walk = n_stages;
    const int s_begin = TL ? 0 : (int)((long)n_walk * by / ny);
    const int s_end = TL ? 0 : (int)((long)n_walk * (by + 1) / ny);
    auto item_of = [&](int s) -> int { return s < s_end ? ((s << 4) | 15) : 15; };
    auto dma_item = [&](int it, char* dst) {
        const char* src = Wst + (long)(it >> 4) * STAGE;
        for (int p = wave; p < PIECES; p += K16_NW) lds_dma_16(src + (long)p * 1024 + lane * 16, dst + p * 1024);
    };
    int it_prev = 15, it_cur = item_of(s_begin), it_next = item_of(s_begin + 1);
    if (s_begin < s_end) dma_item(it_cur, smem);

    auto reduce_tile = [&](const f32x4 (&acc)[K16_SB], int t16) {
        if (GM) {
            // the exact mode's screen needs VALUES only (the row minimum and the groups' minima): which unit holds
            // them is decided by the float32 re-score.  Two v_min3 per tile and sample block, no key packing.
#pragma unroll
            for (int sb = 0; sb < K16_SB; ++sb) {
                cbest[sb] = min(min(cbest[sb], __float_as_uint(acc[sb][0])), __float_as_uint(acc[sb][1]));
                cbest[sb] = min(min(cbest[sb], __float_as_uint(acc[sb][2])), __float_as_uint(acc[sb][3]));
            }
            return;
        }
#pragma unroll
        for (int sb = 0; sb < K16_SB; ++sb) {
            uint32_t key[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float f = acc[sb][r];
                key[r] = (__float_as_uint(f) & ~IDX_MASK) | (uint32_t)(t16 * 4 + r);
            }
            cbest[sb] = min(min(cbest[sb], key[0]), key[1]);
            cbest[sb] = min(min(cbest[sb], key[2]), key[3]);
        }
    };
    auto fold_stage = [&](int stage, bool live) {
        if (GM && live) {
            static_assert(!GM || K16_SB == 4, "the group-minimum transpose pairs four 16-sample blocks with four lane quads");
            // rows of 16 lanes (quads) q0..q3 each hold (v0, v1, v2, v3): after the three steps quad q holds min over quads of v_q
            auto a = __builtin_amdgcn_permlane16_swap(cbest[0], cbest[K16_SB > 1 ? 1 : 0], false, false);
            const uint32_t t01 = min(a[0], a[1]);         // quads: (v0 q01, v1 q01, v0 q23, v1 q23)
            auto b = __builtin_amdgcn_permlane16_swap(cbest[K16_SB > 2 ? 2 : 0], cbest[K16_SB > 3 ? 3 : 0], false, false);
            const uint32_t t23 = min(b[0], b[1]);         // quads: (v2 q01, v3 q01, v2 q23, v3 q23)
            auto c = __builtin_amdgcn_permlane32_swap(t01, t23, false, false);
            const uint32_t full = min(c[0], c[1]);         // quads: (v0, v1, v2, v3), each over all four quads
            const float f = __uint_as_float(full);         // (positive, or a NaN pattern: compares false, never kept)
            const bool keep = f <= __builtin_fminf((T2 ? run_min2 : run_min) + row_e, run_cap);
            if (f < run_min) run_arg = stage;              // (the group that holds the row minimum: the first re-score round)
            // (T2: the two smallest so far, a NaN pattern taking neither place: compares, not min / max)
            if (T2) run_min2 = f < run_min ? run_min : f < run_min2 ? f : run_min2;
            run_min = __builtin_fminf(run_min, f);
            if (keep) gmin[(long)stage * gm_stride + wave_s0 + lane] = full;
            const unsigned long long mask = __ballot(keep);
            if (lane == 0) gflags[ex_flag_index(wave_s0 >> 6, stage, n_stages, gm_stride)] = mask;
        }
        // a later stage wins on smaller VALUE bits only: on equal values the key's index bits (tile << 2 | register) say
        // nothing across stages, and the earlier stage holds the lower unit (c < (g & ~M)  <=>  (c & ~M) < (g & ~M))
#pragma unroll
        for (int sb = 0; sb < K16_SB; ++sb) {
            if (!GM && cbest[sb] < (gbest[sb] & ~IDX_MASK)) { gbest[sb] = cbest[sb]; gstage[sb] = stage; }   // (GM: run_min is the row minimum)
            cbest[sb] = 0xFFFFFFFFu;
        }
    };

    SOM_STAMP_BEGIN();
    if (TL) {
        // TILE LISTS (block skipping, exact_skip.hpp): the workgroup walks its tile's dense list of 16-unit tiles
        // (group << 2 | sub-block, ascending), FOUR to a barrier whatever groups they belong to -- late in a schedule a
        // group keeps one or two of its four tiles, and a barrier per group left the pipe waiting.  A slot of the ring holds
        // the four tiles' fragments (by LDS-DMA) and their 16 initial accumulators each (a wave per tile: a plain load one
        // chunk ahead, written into the slot's tail before the next barrier).  A group's minimum is folded when its last
        // tile is in (its tiles are consecutive in the list, across chunks too).  The parts of a tile's list are cut at
        // group boundaries: one part stores a group's minima.
        const int* tl = glist + bx * (4 * n_stages);
        const int n_t = gcnt[bx];
        auto bound = [&](int y) -> int {
            int b = (int)((long)n_t * y / ny);
            while (b > 0 && b < n_t && (tl[b] >> 2) == (tl[b - 1] >> 2)) ++b;
            return __builtin_amdgcn_readfirstlane(b);
        };
        const int b0 = bound(by), e0 = bound(by + 1);
        auto ent = [&](int i) -> int { return i < e0 ? __builtin_amdgcn_readfirstlane(tl[i]) : -1; };
        constexpr int TQ = K16_T * KS32 * 1024;              // the slot's tail: [tile j][16] initial accumulators
        auto dma_chunk = [&](const int (&en)[4], char* dst) {
            for (int p = wave; p < K16_T * KS32; p += K16_NW) {
                const int j = p / KS32, ks = p - j * KS32;
                if (en[j] >= 0)
                    lds_dma_16(Wst + (long)(en[j] >> 2) * STAGE + (long)(((en[j] & 3) * KS32 + ks) * 1024) + lane * 16, dst + p * 1024);
            }
        };
        // wave w <-> the chunk's tile w: its 16 initial accumulators (lanes 0..15)
        auto load_wq = [&](const int (&en)[4]) -> float {
            const int e = en[wave];
            return (e >= 0 && lane < 16) ? *(const float*)(Wst + (long)(e >> 2) * STAGE + TQ + ((e & 3) * 16 + lane) * 4) : 0.0f;
        };
        int cur[4], nxt[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { cur[j] = ent(b0 + j); nxt[j] = ent(b0 + 4 + j); }
        if (b0 < e0) {
            dma_chunk(cur, smem);
            const float w0 = load_wq(cur);
            if (lane < 16) *(float*)(smem + TQ + (wave * 16 + lane) * 4) = w0;
        }
        int k = 0;
        for (int c = b0; c < e0; c += 4, ++k) {
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            int nn[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) nn[j] = ent(c + 8 + j);
            char* sn = smem + ((k + 1) & 1) * STAGE;
            float wqn = 0.0f;
            if (c + 4 < e0) { dma_chunk(nxt, sn); wqn = load_wq(nxt); }
            const char* st = smem + (k & 1) * STAGE;
            const float* wq = (const float*)(st + TQ);
            auto load_tile = [&](int j, bf16x8 (&a)[KS32], f32x4& wv) {
#pragma unroll
                for (int ks = 0; ks < KS32; ++ks) a[ks] = *(const bf16x8*)(st + (j * KS32 + ks) * 1024 + lane * 16);
                wv = *(const f32x4*)(wq + j * 16 + 4 * quad);
            };
            // MFMAs of one tile, its reduction, and the group's fold when the next tile belongs to another group
            auto run_tile = [&](const bf16x8 (&a)[KS32], const f32x4& wv, int e, int e_next) {
                f32x4 acc[K16_SB];
#pragma unroll
                for (int sb = 0; sb < K16_SB; ++sb) acc[sb] = wv;
#pragma unroll
                for (int ks = 0; ks < KS32; ++ks)
#pragma unroll
                    for (int sb = 0; sb < K16_SB; ++sb) acc[sb] = mfma16(a[ks], xf[sb][ks], acc[sb]);
                reduce_tile(acc, e & 3);                       // (GM: values only, the tile's place in its group is not kept)
                if (e_next < 0 || (e_next >> 2) != (e >> 2)) fold_stage(e >> 2, true);
            };
            // (the tiles' operands alternate between two register sets: the next tile's are read under this tile's MFMAs)
            bf16x8 aA[KS32], aB[KS32];
            f32x4 wvA, wvB;
            load_tile(0, aA, wvA);
            if (cur[1] >= 0) load_tile(1, aB, wvB);
            run_tile(aA, wvA, cur[0], cur[1] >= 0 ? cur[1] : -1);
            if (cur[1] >= 0) {
                if (cur[2] >= 0) load_tile(2, aA, wvA);
                run_tile(aB, wvB, cur[1], cur[2] >= 0 ? cur[2] : -1);
                if (cur[2] >= 0) {
                    if (cur[3] >= 0) load_tile(3, aB, wvB);
                    run_tile(aA, wvA, cur[2], cur[3] >= 0 ? cur[3] : -1);
                    if (cur[3] >= 0) run_tile(aB, wvB, cur[3], nxt[0]);
                }
            }
            if (c + 4 < e0 && lane < 16) *(float*)(sn + TQ + (wave * 16 + lane) * 4) = wqn;
#pragma unroll
            for (int j = 0; j < 4; ++j) { cur[j] = nxt[j]; nxt[j] = nn[j]; }
        }
    }
    for (int s = s_begin; s < s_end; ++s) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const int it_next2 = item_of(s + 2);
        if (s + 1 < s_end) dma_item(it_next, smem + ((s + 1 - s_begin) & 1) * STAGE);
        const char* st = smem + ((s - s_begin) & 1) * STAGE;
        const float* wq = (const float*)(st + K16_T * KS32 * 1024);

        f32x4 wv = *(const f32x4*)(wq + 4 * quad);
        bf16x8 a[KS32];
#pragma unroll
        for (int ks = 0; ks < KS32; ++ks) a[ks] = *(const bf16x8*)(st + ks * 1024 + lane * 16);

#pragma unroll
        for (int t16 = 0; t16 < K16_T; ++t16) {
            f32x4 wvN;
            bf16x8 aN[KS32];
            if (t16 + 1 < K16_T) {
                wvN = *(const f32x4*)(wq + (t16 + 1) * 16 + 4 * quad);
#pragma unroll
                for (int ks = 0; ks < KS32; ++ks)
                    aN[ks] = *(const bf16x8*)(st + ((t16 + 1) * KS32 + ks) * 1024 + lane * 16);
            }
            f32x4 accT[K16_SB];
#pragma unroll
            for (int sb = 0; sb < K16_SB; ++sb) accT[sb] = wv;
#pragma unroll
            for (int ks = 0; ks < KS32; ++ks)
#pragma unroll
                for (int sb = 0; sb < K16_SB; ++sb)
                    accT[sb] = mfma16(a[ks], xf[sb][ks], accT[sb]);
            reduce_tile(accP, (t16 + K16_T - 1) % K16_T);
            if (t16 == 0) fold_stage(it_prev >> 4, s > s_begin);
#pragma unroll
            for (int sb = 0; sb < K16_SB; ++sb) accP[sb] = accT[sb];
            if (t16 + 1 < K16_T) {
                wv = wvN;
#pragma unroll
                for (int ks = 0; ks < KS32; ++ks) a[ks] = aN[ks];
            }
        }
        // (explicit sched_group_barrier / iglp_opt interleave requests were measured: equal or worse than
        //  hipcc's own schedule of this block -- DESIGN.md 3.4)
        it_prev = it_cur; it_cur = it_next; it_next = it_next2;
    }
    if (!TL) {
        reduce_tile(accP, K16_T - 1);
        fold_stage(it_prev >> 4, s_begin < s_end);
    }
    SOM_STAMP_END();

    if (GM) {
        // the row minimum IS the minimum so far after the last group (lane l <-> row wave_s0 + l): the plain value, every
        // bit of it, and the group that holds it (no unit indices exist here); parts merge by value, then lower group
        const long row = wave_s0 + lane;
        if (SEL && sel->plist != nullptr) {
            // the SELECT TAIL (see above): this workgroup's waves select for their own 64 rows -- if the tile's minima are final here
            // (ln: the lane again, opaque to the compiler -- what depends on the lane alone (1 << lane, its masks) is otherwise
            //  computed once in front of the queue's loop and held in registers through every walk: this instance has none to spare)
            int ln = lane;
            asm volatile("" : "+v"(ln));
            const long row = wave_s0 + ln;
            const bool live = row < N;
            float m = run_min;
            if (ny > 1) {
                if (live) atomicMin(out64 + row, ((unsigned long long)__float_as_uint(run_min) << 32) | (uint32_t)run_arg);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // every storing wave drains
                __syncthreads();
                if (wave == 0 && ln == 0) {                            // (not tid: a register held across the walk for this alone)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (the fence's own wait may be dropped: keep this one, in this order)
                    const int ticket = __hip_atomic_fetch_add(sel->tile_ticket + bx, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const int last = ticket == ny - 1 ? 1 : 0;
                    if (last) {
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        atomicAdd(sel->ticket_tiles, 1);
                    }
                    *s_word = last;                                      // (the queue's item word: everyone has read the item)
                }
                __syncthreads();
                const int last = *s_word;
                __syncthreads();                                         // (... before the queue's next item lands in that word)
                if (!last) return;
                // (agent-scope accesses: the other parts' atomics have gone to memory past every cache, and so do these)
                const unsigned long long k64 = live ? __hip_atomic_load(out64 + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ~0ull;
                if (live) __hip_atomic_store(out64 + row, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                m = __uint_as_float((uint32_t)(k64 >> 32));
            } else {
                // (ASSUMES the default, non-threadgroup-split mode: the waves of a workgroup share one CU and its L1, so that behind a
                //  workgroup-scope release, a drained vmcnt and an acquire a wave's loads see what its own lanes stored.  Under
                //  tgsplit the workgroup's waves may sit on different CUs and this pair would have to be the agent-scope one.)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            }
            // exact_select_kernel's threshold, from the registers (run_cap is seed + ex_f32_share; a row the bound does not cover
            // has row_e = inf here and a NaN there: neither passes the guard unless the seed's cap alone is a finite number, and
            // then both give the cap)
            const float thr_f = __builtin_fminf(m + row_e, run_cap);
            const bool ok = live && thr_f > 0.0f && thr_f < 3.0e38f;
            const uint32_t thr = ok ? __float_as_uint(thr_f) : 0u;
            const int mine = ex_select_walk<false>(gmin + (live ? row : 0), gflags, gm_stride, n_stages, wave_s0 >> 6, row, ln, ok, thr, -1,
                                                   sel->glist + bx * (long)n_stages, 0, sel->gcnt[bx], sel->plist, sel->gcount);
            if (live) {
                sel->rowcnt[row] = mine;
                if (sel->rowmin2_init != nullptr) sel->rowmin2_init[row] = 0xFFFFFFFFu;
            }
            return;
        }
        if (row < N) atomicMin(out64 + row, ((unsigned long long)__float_as_uint(run_min) << 32) | (uint32_t)run_arg);
        if (T2 && row < N) {
            t2min[(long)(2 * by) * t2pitch + row] = run_min;
            t2min[(long)(2 * by + 1) * t2pitch + row] = run_min2;
        }
        return;
    }

#pragma unroll
    for (int sb = 0; sb < K16_SB; ++sb) {
        uint32_t code = gbest[sb] & IDX_MASK;
        uint32_t unit = (uint32_t)gstage[sb] * K16_STAGE_UNITS + (code >> 2) * 16 + quad * 4 + (code & 3);
        // all distances are positive floats: (value bits, unit) orders as one unsigned 64-bit key
        unsigned long long comp = ((unsigned long long)(gbest[sb] & ~IDX_MASK) << 32) | unit;
        unsigned long long o = __shfl_xor(comp, 16, 64);
        if (o < comp) comp = o;
        o = __shfl_xor(comp, 32, 64);
        if (o < comp) comp = o;
        const long row = wave_s0 + sb * 16 + col;
        if (quad == 0 && row < N) atomicMin(out64 + row, comp);
    }
}

// items (TL; nullptr: the grid is (tiles, parts)): the screen under a plan as a WORK QUEUE.  The tiles' lists are uneven -- mid-schedule
// the median tile lists ~100 blocks, a few list 700 -- and a grid of one workgroup per tile ended in a tail of a few long walks
// that held a fifth to two fifths of the launch (tools/wg_timeline.py).  exact_items_kernel cuts every list into parts of about
// equal length (item = (tile, part | parts << 16)); a workgroup per slot of the chip takes items off one counter until none is left
// (every workgroup reaches `it >= *n_items`: the grid drains).  A part re-reads its tile's rows: only the long lists are cut.
template <int KS32, class EL = Bf16, bool GM = false, bool TL = false, bool T2 = false>
__global__ __launch_bounds__(64 * K16_NW, (TL && GM) ? 3 : 2) void bmu_bf16_k16_kernel(const __bf16* __restrict__ Xb, long N,
                                                              const char* __restrict__ Wst, int n_stages, int K,
                                                              unsigned long long* __restrict__ out64,
                                                              uint32_t* __restrict__ gmin = nullptr, long gm_stride = 0,
                                                              unsigned long long* __restrict__ gflags = nullptr,
                                                              const float* __restrict__ xsq = nullptr,
                                                              const float* __restrict__ xerr = nullptr,
                                                              const float* __restrict__ xmax2 = nullptr,
                                                              const float* __restrict__ wmax2 = nullptr,
                                                              const float* __restrict__ werr2 = nullptr,
                                                              ExactBound eb = ExactBound(),
                                                              const float* __restrict__ seed = nullptr,
                                                              const int* __restrict__ glist = nullptr,
                                                              const int* __restrict__ gcnt = nullptr,
                                                              const int2* __restrict__ items = nullptr,
                                                              const int* __restrict__ n_items = nullptr,
                                                              int* __restrict__ item_ctr = nullptr,
                                                              float* __restrict__ t2min = nullptr, long t2pitch = 0,
                                                              ScreenSelect sel = ScreenSelect()) {
    if (TL && items != nullptr) {
        __shared__ int s_item;
        const int n = *n_items;
        for (;;) {
            if (threadIdx.x == 0) s_item = atomicAdd(item_ctr, 1);
            __syncthreads();                                 // (everyone is done with the previous item's LDS ring too)
            const int it = s_item;
            __syncthreads();
            if (it >= n) return;
            const int2 iv = items[it];
            bmu_bf16_k16_body<KS32, EL, GM, TL, false, GM && TL>(Xb, N, Wst, n_stages, K, out64, gmin, gm_stride, gflags, xsq, xerr, xmax2, wmax2,
                                                                 werr2, eb, seed, glist, gcnt, (long)iv.x, iv.y & 0xFFFF, iv.y >> 16, nullptr, 0,
                                                                 &sel, &s_item);
        }
    }
    bmu_bf16_k16_body<KS32, EL, GM, TL, T2>(Xb, N, Wst, n_stages, K, out64, gmin, gm_stride, gflags, xsq, xerr, xmax2, wmax2, werr2, eb, seed,
                                            glist, gcnt, (long)blockIdx.x, (int)blockIdx.y, (int)gridDim.y, t2min, t2pitch);
}

// out64 -> raveled ids (a padding unit can only win on a NaN row: numpy's argmin gives 0 there)
__global__ __launch_bounds__(256) void bmu_finalize_kernel(const unsigned long long* __restrict__ out64, long N, int K,
                                                           int* __restrict__ out) {
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    uint32_t u = (uint32_t)out64[i];
    out[i] = u < (uint32_t)K ? (int)u : 0;
}

}  // namespace somhip
