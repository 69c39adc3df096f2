// The update half of XPySom._update / _merge_updates (xpysom.py:420-455), restructured.
//
// The reference materialises g[n,i,j] = h(bmu_n -> (i,j)) * eta for every sample and
// multiplies g^T (K x n) by x (n x D).  h depends on n only through bmu_n, and on the
// rectangular topology every neighbourhood of neighborhoods.py is a short sum of
// products of a function of the row offset and a function of the column offset:
//     g[n,i,j] = sum_t  Px_t[i, ci_n] * Py_t[j, cj_n]
//   gaussian     (:14-33)   t=1 : ex * ey                      ex = exp(-(i-a)^2/d) [* box mask]
//   mexican_hat  (:57-74)   t=2 : ex(1-2px/d) * ey  -  ex * (2py/d)ey
//   bubble       (:99-112)  t=1 : box * box
//   triangle     (:114-130) t=1 : tri * tri
// The hexagonal topology (gaussian_generic / mexican_hat_generic, :35-97; coordinates xpysom.py:201-206)
// shifts every second map column-index row j by -0.5 in x: xx[j,i] = i - s(j)/2, s(j) = 1 iff (Y-1-j) even.
// The x offset between unit (i,j) and BMU (ci,cj) is then (i - ci) + (s(cj) - s(j))/2: one of three values
// per (s(j), s(cj)) class, so the hexagonal neighbourhood is the rectangular one summed over 3 classes
//   {s(j)=s(cj): +0}, {s(j)=0,s(cj)=1: +1/2}, {s(j)=1,s(cj)=0: -1/2}
// with the class indicator folded into the column factor: nt = 3 (gaussian), 6 (mexican hat).
// Hence, exactly (only the float summation order differs):
//     S[b,:] = sum_{n: bmu_n = b} x_n,  c[b] = #{n: bmu_n = b}          (segment sum, HBM/atomic bound)
//     [num|den](i,j,:) = sum_t sum_a Px_t[i,a] sum_b Py_t[j,b] [S|c](a,b,:)   (two small exact-f32 MFMA GEMMs)
// which replaces the 2*N*K*D-flop GEMM of xpysom.py:437-438 by 2*K*(X+Y)*(D+1) flops.
#pragma once
#include <type_traits>
#include "som_common.hpp"
#include "unit_sort.hpp"   // RS_BLOCK, CS_MAX_K, CS_BLOCK: the sorts' block sizes, beside the rule that sizes their buffers

namespace somhip {

// ---- segment sum: SC[b][0..D-1] = sum_{bmu_n = b} x_n ; SC[b][D] = #{bmu_n = b} ------------------
// The rows are first ordered by BMU (stable sort of (bmu_n, n) pairs, below: the sorted order is a
// function of the BMUs alone).  A unit's rows are then ONE run of the sorted order, and the sum of a run is
// formed by a tree whose shape depends on N only -- no atomics, one fixed order:
//   wave   walks a chunk of consecutive entries (level 0: SEG_CHUNK sorted rows, gathered as whole 4*D-byte rows,
//          eight in flight; upper levels: SEG_CHUNK_UP entries of a partial list) with the running sum of the
//          current unit in registers (lane = feature pair).  A run that begins and ends inside the chunk is
//          complete: the wave adds it to SC[unit] with a plain read-modify-write (it is that unit's only writer in
//          the launch).  A run cut by the chunk's edge leaves a PARTIAL (key, vector, count) in one of the wave's
//          two slots: slot 0 = its first run if that continues the previous chunk, slot 1 = its last run if the
//          next chunk continues it.  Unused slots carry key -1; a chunk that is one run open on both sides fills
//          slot 0 and gives slot 1 the same key with a zero vector, so one unit's partials stay adjacent.
//   block  the slots of a workgroup's waves live in LDS; after a barrier wave 0 walks them the same way.  Only
//          runs cut by the BLOCK's edges survive, as the two entries 2b, 2b+1 of the next level's list in HBM.
//   level  the next level is the same kernel over that list, until one block holds the whole list
//          (1 Mi rows, 16 waves per block: 1 048 576 rows -> 4 096 entries -> 32 entries -> done).
// So two epochs from the same state are bitwise equal, and a unit that wins every row costs a few tiny
// passes instead of N/32 serialised atomics on one address.
constexpr int SEG_CHUNK = 32;      // rows per wave, level 0
constexpr int SEG_CHUNK_UP = 16;   // partial entries per wave, upper levels: at least this (two groups of eight loads: a short
                                   // latency chain), up to 64 when that lets ONE workgroup finish the list (seg_chunk_up)
constexpr int SEG_MAX_WAVES = 16;  // waves per workgroup (fewer when 2 * waves * D1p floats would not fit in LDS)

// ---- stable LSD radix sort of (key, value) pairs, 8 bits a pass: the rows by BMU for the segment sum (maps too large for the
// counting sort below), the rows by their last BMU's patch for the exact mode's resident order (exact_skip.hpp).  Hand-written
// for these two jobs (keys of 10 .. 20 bits, values = row indices, 10^5 .. 10^7 items): per pass
//   rs_hist_kernel     block = RS_BLOCK consecutive items: LDS histogram of the pass's digit -> table[digit * B + block]
//   rs_scan_kernel     a wave per digit: exclusive scan of its block counts in place, its total -> tot[digit]
//   rs_scatter_kernel  block = the same RS_BLOCK items, all loaded up front: item (q, wave, lane) = 256 q + 64 wave + lane.  The first
//                      destination of a (digit, block) run = the totals of the lower digits + the block's place in its digit; every
//                      (q, wave) leaves its count of each digit in an LDS cell, the digit's thread turns the cells into first
//                      destinations in item order, and an item's destination = its cell + its rank among the wave's items of the
//                      same digit: the order of equal digits is the order of the items -- STABLE, and the same order on every run
//                      (no atomics decide a place; two barriers a block)
// vin == nullptr: the values are the items' own indices (first pass of a sort of row ids).
__global__ __launch_bounds__(256) void rs_hist_kernel(const int* __restrict__ keys, long n, int shift, int B, int* __restrict__ table) {
    __shared__ int hist[256];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const long i0 = (long)blockIdx.x * RS_BLOCK;
#pragma unroll
    for (int q = 0; q < RS_BLOCK / 256; ++q) {
        const long i = i0 + q * 256 + threadIdx.x;
        if (i < n) atomicAdd(&hist[(keys[i] >> shift) & 255], 1);
    }
    __syncthreads();
    table[(long)threadIdx.x * B + blockIdx.x] = hist[threadIdx.x];
}

// one wave per digit: exclusive scan of the digit's B block counts in place, the digit's total -> tot[digit]
__global__ __launch_bounds__(256) void rs_scan_kernel(int* __restrict__ table, int B, int* __restrict__ tot) {
    const int d = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    int* t = table + (long)d * B;
    int carry = 0;
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int b = b0 + lane;
        const int v = b < B ? t[b] : 0;
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
        if (b < B) t[b] = carry + incl - v;
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) tot[d] = carry;
}

__global__ __launch_bounds__(256) void rs_scatter_kernel(const int* __restrict__ kin, const int* __restrict__ vin, long n, int shift,
                                                         int B, const int* __restrict__ table, const int* __restrict__ tot,
                                                         int* __restrict__ kout, int* __restrict__ vout) {
    constexpr int Q = RS_BLOCK / 256;                        // 256-item steps of the block
    __shared__ __attribute__((aligned(16))) int cell[4 * Q][256];   // [4 q + wave][digit]: the (step, wave)'s items of the digit, then their first destination
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long i0 = (long)blockIdx.x * RS_BLOCK;
    // every load of the block first: the items stay in registers, and no load waits behind a barrier
    int key[Q], val[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const long i = i0 + q * 256 + tid;
        key[q] = i < n ? kin[i] : 0;
        val[q] = i < n ? (vin != nullptr ? vin[i] : (int)i) : 0;
    }
    const int mine = tot[tid];
    const int place = table[(long)tid * B + blockIdx.x];
    {
        int4* z = reinterpret_cast<int4*>(&cell[0][0]);
#pragma unroll
        for (int k = 0; k < 4 * Q * 256 / 4 / 256; ++k) z[k * 256 + tid] = make_int4(0, 0, 0, 0);
    }
    // first destination of digit `tid`: the totals of the digits below it + this block's place inside the digit
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();                                         // (the cells are zero)
    int cur = incl - mine + place;
    for (int w = 0; w < wave; ++w) cur += wsum[w];
    // an item's rank among its wave's items of the same digit (lower lane first); the digit's leader leaves their number in
    // the (step, wave)'s cell -- one leader per cell, so no two lanes write one
    int dgrank[Q];                                           // digit | rank << 8
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const bool live = i0 + q * 256 + tid < n;
        const int dg = (key[q] >> shift) & 255;
        unsigned long long peers = __ballot(live);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long m = __ballot((dg >> b) & 1);
            peers &= ((dg >> b) & 1) ? m : ~m;
        }
        const int rank = (int)__builtin_popcountll(peers & ((1ull << lane) - 1ull));
        if (live && rank == 0) cell[4 * q + wave][dg] = (int)__builtin_popcountll(peers);
        dgrank[q] = dg | (rank << 8);
    }
    __syncthreads();
    // thread d walks its digit's cells in item order (step, then wave): counts -> first destinations.  These are the places
    // the waves would take one after the other: the order of equal digits is the order of the items -- STABLE
    {
        int c[4 * Q];
#pragma unroll
        for (int k = 0; k < 4 * Q; ++k) c[k] = cell[k][tid];
#pragma unroll
        for (int k = 0; k < 4 * Q; ++k) { cell[k][tid] = cur; cur += c[k]; }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        if (i0 + q * 256 + tid < n) {
            const int dest = cell[4 * q + wave][dgrank[q] & 255] + (dgrank[q] >> 8);
            kout[dest] = key[q]; vout[dest] = val[q];
        }
    }
}

// ---- stable counting sort of the rows by BMU for maps of at most CS_MAX_K units ------------------------------------
// (sorted by unit, rows ascending inside a unit: exactly what the stable radix sort returns, so the run sum adds in the same
// fixed order.)  The library merge sort used before took six to seven launches at 100 000 rows (55 us of a 0.4 ms epoch at 64 x 64 x 32);
// with few units a histogram per 1 024-row block is small: table[unit][block], three launches.
//   cs_hist_kernel     block = 1 024 rows: LDS histogram of its units -> table[k * B + block]
//   cs_scan_kernel     wave per unit: exclusive scan of its B block counts in place, the unit's total -> tot[k]
//   cs_scatter_kernel  block = 1 024 rows: first destination of every (unit, block) = scan of tot over the units + the block's
//                      prefix; the block's 16 waves take their turns in order, a wave ranks its rows among equal units by
//                      ballots over the unit's bits (lower lane = lower row first)
__global__ __launch_bounds__(256) void cs_hist_kernel(const int* __restrict__ bmu, long N, int K, int B, int* __restrict__ table) {
    extern __shared__ int cs_lds[];
    for (int k = threadIdx.x; k < K; k += 256) cs_lds[k] = 0;
    __syncthreads();
    const long r0 = (long)blockIdx.x * CS_BLOCK;
#pragma unroll
    for (int q = 0; q < CS_BLOCK / 256; ++q) {
        const long r = r0 + q * 256 + threadIdx.x;
        if (r < N) atomicAdd(&cs_lds[bmu[r]], 1);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256) table[(long)k * B + blockIdx.x] = cs_lds[k];
}

__global__ __launch_bounds__(256) void cs_scan_kernel(int* __restrict__ table, int K, int B, int* __restrict__ tot) {
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (k >= K) return;
    int* t = table + (long)k * B;
    int carry = 0;
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int b = b0 + lane;
        const int v = b < B ? t[b] : 0;
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
        if (b < B) t[b] = carry + incl - v;
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) tot[k] = carry;
}

__global__ __launch_bounds__(CS_BLOCK) void cs_scatter_kernel(const int* __restrict__ bmu, long N, int K, int B, int bits,
                                                             const int* __restrict__ table, const int* __restrict__ tot,
                                                             int* __restrict__ skey, int* __restrict__ srow) {
    extern __shared__ int cs_lds[];                        // base[K]: next destination of every unit for this block
    __shared__ int wsum[CS_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // exclusive scan of tot over the units (every block does it: K <= 8 192), + this block's prefix inside the unit
    const int per = (K + CS_BLOCK - 1) / CS_BLOCK;         // units per thread, consecutive
    const int k0 = tid * per;
    int mine = 0;
    for (int i = 0; i < per; ++i) if (k0 + i < K) mine += tot[k0 + i];
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    int run = before + incl - mine;
    for (int i = 0; i < per; ++i)
        if (k0 + i < K) { cs_lds[k0 + i] = run + table[(long)(k0 + i) * B + blockIdx.x]; run += tot[k0 + i]; }
    __syncthreads();
    const long r = (long)blockIdx.x * CS_BLOCK + tid;
    const bool live = r < N;
    const int key = live ? bmu[r] : 0;
    // the lanes of this wave with the same unit
    unsigned long long peers = __ballot(live);
    for (int b = 0; b < bits; ++b) {
        const unsigned long long m = __ballot((key >> b) & 1);
        peers &= ((key >> b) & 1) ? m : ~m;
    }
    const int leader = live ? (int)__builtin_ctzll(peers) : lane;
    const int rank = (int)__builtin_popcountll(peers & ((1ull << lane) - 1));
    const int count = (int)__builtin_popcountll(peers);
    int dest = 0;
    for (int w = 0; w < CS_BLOCK / 64; ++w) {              // waves in row order: the sort is stable
        if (wave == w) {
            int old = 0;
            if (live && lane == leader) { old = cs_lds[key]; cs_lds[key] = old + count; }
            old = __shfl(old, leader, 64);
            dest = old + rank;
        }
        __syncthreads();
    }
    if (live) { skey[dest] = key; srow[dest] = (int)r; }
}

__host__ __device__ inline int seg_waves_per_block(int D1p) {
    int nw = SEG_MAX_WAVES;
    while (nw > 1 && (long)2 * nw * (D1p + 1) * 4 > 64 * 1024) nw >>= 1;
    return nw;
}
// upper levels: entries per wave for a list of n entries -- the smallest multiple of 8 in [SEG_CHUNK_UP, 64] with
// which nw waves cover the list, else SEG_CHUNK_UP
__host__ __device__ inline int seg_chunk_up(long n, int nw) {
    long c = ((n + nw - 1) / nw + 7) / 8 * 8;
    return (c <= 64) ? (int)(c < SEG_CHUNK_UP ? SEG_CHUNK_UP : c) : SEG_CHUNK_UP;
}
// entries the list left behind by a level with n entries, chunk c and nw waves per block
__host__ __device__ inline long seg_next_entries(long n, int c, int nw) { return 2 * ((n + (long)c * nw - 1) / ((long)c * nw)); }

// One chunk walk.  Entry i (< cnt <= 64) has key readlane(my_key, i), count readlane(my_cnt, i) and its vector at
// ROWS ? X + readlane(my_row, i) * D : list + i * D1p.  Complete runs go to SC, the two possible partials to
// slot0 / slot1 (rows of D1p floats); key0 / key1 return the slots' keys (-1 = unused).
// WEIGHTED (with ROWS only): my_cnt holds the rows' sample weights w >= 0 instead of 1.0f.  A row enters the sum as
// fmaf(w, x, acc) at the place and in the order the unweighted walk forms acc + x (fmaf(1, x, acc) rounds like acc + x:
// weights of 1.0 give the unweighted sums bit for bit), and the count column carries the sum of the weights.  A row of
// weight 0 is not loaded at all -- it is absent, not multiplied by 0, so its NaN / infinite features stay out of its unit.
// MASKED (with ROWS only; missing values, SOM_MISSING_NAN): a NaN feature is "not observed".  A row enters as x~ (x where
// observed, 0 otherwise) at the place and in the order the unmasked walk adds x -- complete rows give the unmasked sums bit
// for bit -- and next to every feature sum the walk keeps the feature's COUNT, the sum of m (1 where observed, 0 otherwise;
// WEIGHTED: of w m).  D is then the width of the rows; the row written is [S (D) | C (D) | total count] of width 2 D + 1
// <= D1p, and everything above level 0 walks it as a list of 2 D features with the count in column 2 D.
template <bool ROWS, bool VEC2, bool WEIGHTED = false, bool MASKED = false>
__device__ __forceinline__ void seg_walk(const float* __restrict__ X, const float* list, int my_key, int my_row,
                                         float my_cnt, int cnt, bool open_left, bool open_right, int D, int D1p,
                                         int accumulate, float* __restrict__ SC, float* __restrict__ cnt_dense,
                                         float* slot0, float* slot1, int& key0, int& key1) {
    static_assert(ROWS || !MASKED, "run sum: only the walk over rows sees missing values");
    const int lane = threadIdx.x & 63;
    const int CD = MASKED ? 2 * D : D;                    // the count's column
    key0 = -1; key1 = -1;
    bool slot1_zero = false;
    for (int f0 = 0; f0 < D; f0 += 256) {                 // 4 features per lane per sweep
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        float cm[4] = {0.f, 0.f, 0.f, 0.f};              // MASKED: the features' counts (unused otherwise)
        int cur = __builtin_amdgcn_readfirstlane(my_key);
        int run_begin = 0;
        float run = 0.f;
        // feature of acc[j]: VEC2: f0 + 128*(j>>1) + 2*lane + (j&1);  scalar: f0 + lane + 64*j
        auto put = [&](float* dst, bool add, long unit = -1) {   // this lane's 4 sums (and the count) into one row
            if (VEC2) {
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const int d = f0 + 128 * jj + 2 * lane;
                    if (d < D) {
                        float2 t = make_float2(acc[2 * jj], acc[2 * jj + 1]);
                        if (add) { const float2 o = *(const float2*)(dst + d); t.x += o.x; t.y += o.y; }
                        *(float2*)(dst + d) = t;
                        if (MASKED) {                        // (D even: D + d is 8-byte aligned as d is)
                            float2 c = make_float2(cm[2 * jj], cm[2 * jj + 1]);
                            if (add) { const float2 o = *(const float2*)(dst + D + d); c.x += o.x; c.y += o.y; }
                            *(float2*)(dst + D + d) = c;
                        }
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int d = f0 + lane + 64 * j;
                    if (d < D) {
                        dst[d] = add ? dst[d] + acc[j] : acc[j];
                        if (MASKED) dst[D + d] = add ? dst[D + d] + cm[j] : cm[j];
                    }
                }
            }
            if (f0 == 0 && lane == 0) {
                const float c = add ? dst[CD] + run : run;
                dst[CD] = c;
                if (unit >= 0) cnt_dense[unit] = c;          // the counts once more, densely (the transform's count path)
            }
        };
        auto flush = [&](int end) {                       // the run [run_begin, end) of unit `cur` ends here
            if (cur >= 0) {
                const bool first = run_begin == 0, last = end == cnt;
                if (first && open_left) {
                    put(slot0, false);
                    key0 = cur;
                    if (last && open_right) { key1 = cur; slot1_zero = true; }
                } else if (last && open_right) {
                    put(slot1, false);
                    key1 = cur;
                } else {
                    put(SC + (long)cur * D1p, accumulate != 0, cur);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) { acc[j] = 0.f; if (MASKED) cm[j] = 0.f; }
            run = 0.f;
        };
        for (int i0 = 0; i0 < cnt; i0 += 8) {
            float v[8][4];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u;
                const int ii = i < cnt ? i : 0;
                bool live = i < cnt && __builtin_amdgcn_readlane(my_key, ii) >= 0;
                if (ROWS && WEIGHTED) live = live && __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_cnt), ii)) != 0.0f;
                const float* x = ROWS ? X + (long)__builtin_amdgcn_readlane(my_row, ii) * D : list + (long)ii * D1p;
                if (VEC2) {
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        const int d = f0 + 128 * jj + 2 * lane;
                        float2 t = make_float2(0.f, 0.f);
                        if (live && d < D) t = *(const float2*)(x + d);   // D even: d + 1 < D, 8-byte aligned
                        v[u][2 * jj] = t.x; v[u][2 * jj + 1] = t.y;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int d = f0 + lane + 64 * j;
                        v[u][j] = (live && d < D) ? x[d] : 0.f;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u;
                if (i < cnt) {
                    const int b = __builtin_amdgcn_readlane(my_key, i);
                    if (b != cur) { flush(i); cur = b; run_begin = i; }
                    const float w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_cnt), i));
                    if (MASKED) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const bool seen = v[u][j] == v[u][j];
                            const float xt = seen ? v[u][j] : 0.f, m = seen ? 1.f : 0.f;
                            acc[j] = WEIGHTED ? __builtin_fmaf(w, xt, acc[j]) : acc[j] + xt;
                            cm[j] = WEIGHTED ? __builtin_fmaf(w, m, cm[j]) : cm[j] + m;
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[j] = (ROWS && WEIGHTED) ? __builtin_fmaf(w, v[u][j], acc[j]) : acc[j] + v[u][j];
                    }
                    run += w;
                }
            }
        }
        flush(cnt);
        if (slot1_zero) {                                 // one run, open on both sides: slot 1 = (key, 0)
#pragma unroll
            for (int j = 0; j < 4; ++j) { acc[j] = 0.f; if (MASKED) cm[j] = 0.f; }
            run = 0.f;
            put(slot1, false);
        }
    }
}

// LEVEL0: keys = sorted BMUs, srow = sorted row ids, rows gathered from X (count 1 each).
// !LEVEL0: keys / vin = the previous level's partial list ([n] keys, [n][D1p] vectors, count in column D).
// WEIGHTED (LEVEL0 only): wgt[row id] is the row's sample weight (float32, finite, >= 0) -- the count 1 of the row becomes
// its weight, its features enter the sum times the weight (seg_walk); the upper levels do not know the difference.
// MASKED (LEVEL0 only): NaN features are missing values -- D is the rows' width, the list written has 2 * D features (sums,
// then per-feature counts) and the count in column 2 * D (seg_walk); D1p >= 2 * D + 1.
// VEC2 (D even): a lane owns feature pairs (8-byte accesses, one instruction per 128 features of a row).
// accumulate == 0: SC was zeroed and every unit is written at most once in the whole pass: plain stores.
// Dynamic LDS: blockDim.x / 64 > 1 ? 2 * waves * (D1p + 1) floats : none (a one-wave block writes its slots
// straight to the next list).
template <bool LEVEL0, bool VEC2, bool WEIGHTED = false, bool MASKED = false>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void runsum_kernel(const float* __restrict__ X,
                                                                   const int* __restrict__ keys,
                                                                   const int* __restrict__ srow,
                                                                   const float* __restrict__ vin, long n, int chunk,
                                                                   int D, int D1p, int accumulate, float* __restrict__ SC,
                                                                   float* __restrict__ cnt_dense, int* __restrict__ kout,
                                                                   float* __restrict__ vout,
                                                                   const float* __restrict__ wgt = nullptr) {
    static_assert(LEVEL0 || !WEIGHTED, "run sum: only level 0 reads rows, so only level 0 is weighted");
    static_assert(LEVEL0 || !MASKED, "run sum: only level 0 reads rows, so only level 0 sees missing values");
    const int LD = MASKED ? 2 * D : D;                    // features of a list entry, = the column of its count
    extern __shared__ __attribute__((aligned(16))) float seg_lds[];
    const int C = LEVEL0 ? SEG_CHUNK : chunk;             // <= 64: lane i holds entry i
    const int lane = threadIdx.x & 63;
    const int nw = blockDim.x >> 6, wave = threadIdx.x >> 6;
    const long blk = blockIdx.x;
    const long p0 = (blk * nw + wave) * C;
    float* slots = seg_lds;                               // [2 * nw][D1p]
    int* slot_keys = (int*)(seg_lds + (long)2 * nw * D1p);   // [2 * nw]
    const bool direct = nw == 1;
    int k0 = -1, k1 = -1;
    if (p0 < n) {
        const int cnt = (int)((n - p0 < C) ? (n - p0) : C);
        // lane i < cnt holds the i-th (key, row, count) of the chunk
        const int my_key = lane < cnt ? keys[p0 + lane] : -1;
        const int my_row = (LEVEL0 && lane < cnt) ? srow[p0 + lane] : 0;
        const float my_cnt = LEVEL0 ? (WEIGHTED ? (lane < cnt ? wgt[my_row] : 0.0f) : 1.0f)
                                    : ((lane < cnt && my_key >= 0) ? vin[(p0 + lane) * D1p + D] : 0.0f);
        const int first_key = __builtin_amdgcn_readfirstlane(my_key);
        const int last_key = __builtin_amdgcn_readlane(my_key, cnt - 1);
        const int prev_key = p0 > 0 ? keys[p0 - 1] : -2;
        const int next_key = p0 + cnt < n ? keys[p0 + cnt] : -2;
        const bool open_left = first_key >= 0 && __builtin_amdgcn_readfirstlane(prev_key) == first_key;
        const bool open_right = last_key >= 0 && __builtin_amdgcn_readfirstlane(next_key) == last_key;
        float* s0 = direct ? vout + (2 * blk) * (long)D1p : slots + (long)(2 * wave) * D1p;
        float* s1 = direct ? vout + (2 * blk + 1) * (long)D1p : slots + (long)(2 * wave + 1) * D1p;
        seg_walk<LEVEL0, VEC2, WEIGHTED, MASKED>(X, LEVEL0 ? nullptr : vin + p0 * (long)D1p, my_key, my_row, my_cnt, cnt, open_left,
                               open_right, D, D1p, accumulate, SC, cnt_dense, s0, s1, k0, k1);
    }
    if (direct) {
        if (lane == 0 && p0 < n) { kout[2 * blk] = k0; kout[2 * blk + 1] = k1; }
        return;
    }
    if (lane == 0) { slot_keys[2 * wave] = k0; slot_keys[2 * wave + 1] = k1; }
    __syncthreads();
    if (wave != 0) return;
    // wave 0: the block's 2 * nw slots as one chunk.  A filled slot 0 of the first wave continues the previous
    // block by construction, a filled slot 1 of the last wave is continued by the next one.
    const int cnt2 = 2 * nw;
    const int my_key2 = lane < cnt2 ? slot_keys[lane] : -1;
    const float my_cnt2 = (lane < cnt2 && my_key2 >= 0) ? slots[(long)lane * D1p + LD] : 0.0f;
    const bool open_left2 = __builtin_amdgcn_readfirstlane(my_key2) >= 0;
    const bool open_right2 = __builtin_amdgcn_readlane(my_key2, cnt2 - 1) >= 0;
    int g0 = -1, g1 = -1;
    seg_walk<false, VEC2>(nullptr, slots, my_key2, 0, my_cnt2, cnt2, open_left2, open_right2, LD, D1p, accumulate, SC,
                          cnt_dense, vout + (2 * blk) * (long)D1p, vout + (2 * blk + 1) * (long)D1p, g0, g1);
    if (lane == 0) { kout[2 * blk] = g0; kout[2 * blk + 1] = g1; }
}

// ---- neighbourhood factor tables ---------------------------------------------------------------
// P1: stage-1 matrices  [nt][Y][Y]   (Py_t[j][b])
// P2: stage-2 matrix    [X][nt*X]    (Px_t[i][a] at column t*X + a), carries eta.
// wide != 0: float64 evaluation rounded once to float32 (NumPy >= 2 with a numpy.float64 sigma);
// wide == 0: mimic the float32 evaluation: the exponent argument is rounded to float32
// (the dominant error term) before a correctly rounded exp.
struct NeighParams {
    double sigma, eta, d;   // d = 2*std_coeff^2*sigma^2 (host, double)
    int kind, compact, wide, X, Y, nt;
    int hex, base_nt, ncls; // hexagonal topology: nt = ncls * base_nt, one copy of the terms per parity class
    int swapped;            // mexican_hat + compact_support on the rectangular topology: row stage first (see below)
    int rsel;               // which of the two band-range buffers this build of the tables fills (BandRanges, below)
    int torus;              // toroidal topology: the rectangular grid, periodic on both axes (neigh_offset)
};

__device__ __forceinline__ double neigh_exp(double delta2, const NeighParams& p) {
    if (p.wide) return exp(-delta2 / p.d);
    float a = -(float)delta2 / (float)p.d;
    return (double)(float)exp((double)a);
}
// the reference's support mask, literally: n > c - sigma  and  n < c + sigma  in float64 (neighborhoods.py:29-31,
// 50-54, 105-110) on the units' coordinates.  c -/+ sigma is rounded before the compare, so a sigma within an ulp of
// a lattice distance (asymptotic decay produces them: 5 / (1 + 2/3) = 3.0000000000000004) decides the boundary unit
// differently than |n - c| < sigma would, and differently for different c.  n, c: absolute coordinates (hexagonal x:
// half-unit row offsets included -- which is why compact_support needs the fourth parity class).
__device__ __forceinline__ double neigh_box(double n, double c, const NeighParams& p) {
    return (n > c - p.sigma && n < c + p.sigma) ? 1.0 : 0.0;
}
// the offset of unit coordinate n from BMU coordinate c along axis `which` (0 = x, side X; 1 = y, side Y).  Toroidal: the
// NEAREST image, dl - L round(dl / L), |offset| <= L / 2 -- one image, never a sum over images; at the tie |offset| = L / 2
// (even L) the sign is rint's, and every neighbourhood is even in the offset.
__device__ __forceinline__ double neigh_offset(int which, double n, double c, const NeighParams& p) {
    double dl = n - c;
    if (p.torus) { const double L = (double)(which == 0 ? p.X : p.Y); dl -= L * rint(dl / L); }
    return dl;
}
// the support mask of the unit at offset dl = neigh_offset(..., n, c): the reference's compare on the coordinates (above), or
// on the torus, which has no reference, the open interval on the wrapped offset itself
__device__ __forceinline__ double neigh_mask(double n, double c, double dl, const NeighParams& p) {
    if (p.torus) return (dl > -p.sigma && dl < p.sigma) ? 1.0 : 0.0;
    return neigh_box(n, c, p);
}
__device__ __forceinline__ double neigh_round(double v, const NeighParams& p) { return p.wide ? v : (double)(float)v; }

// value of factor `which` (0 = row factor Px, 1 = column factor Py) of base term t for unit coordinate n and
// BMU coordinate c (absolute: on the hexagonal topology the x coordinates carry their rows' half-unit offsets; on the
// toroidal one the offset n - c is wrapped to its nearest image first, and everything below sees only that)
__device__ double neigh_factor(int which, int t, double n, double c, const NeighParams& p) {
    const double dl = neigh_offset(which, n, c, p);
    const double d2 = dl * dl;
    switch (p.kind) {
    case 0: {   // gaussian
        double e = neigh_exp(d2, p);
        if (p.compact) e *= neigh_mask(n, c, dl, p);
        return e;
    }
    case 1: {   // mexican hat: (ex(1-2px/d)) * ey  -  ex * ((2py/d) ey)
        double e = neigh_exp(d2, p);
        double q = p.wide ? (2.0 / p.d) * d2 : (double)((float)(2.0 / p.d) * (float)d2);
        if (!p.compact) {
            if (t == 0) return which == 0 ? neigh_round(e * (1.0 - q), p) : e;
            return which == 0 ? -e : neigh_round(q * e, p);
        }
        // compact_support as the reference computes it (neighborhoods.py:69-71, :91-93): px is multiplied by a mask M,
        // py is not, so with A = ex (1 - 2 px / d), Q = (2 py / d) ey:
        //     h = M (A ey - ex Q) + (1 - M)(ey - Q)
        // Hexagonal (generic): M = mx(i; ci) my(j; cj), and 1 - M = (1 - mx) + mx (1 - my): four separable terms
        //     [mx A][my ey]  +  [-mx ex][my Q]  +  [1 - mx][ey - Q]  +  [mx][(1 - my)(ey - Q)].
        // The last two never overlap (at most one is nonzero for a pair of units), so nothing cancels: written as
        // [-mx][my (ey - Q)] + [1][ey - Q] they would, inside the box, add and subtract ey - Q -- up to exp(px / d)
        // times the h they sum to -- and leave its float32 rounding behind.
        // Rectangular: M = m1(i; ci) m2(i; cj) -- the second mask compares the ROW index with the BMU's COLUMN --:
        // the same four terms with my = m2, which is applied between the row stage and the column stage (`swapped`,
        // mask_rows_kernel: terms 0 and 1 times m2, term 3 times 1 - m2).  (Toroidal: refused by som_create.)
        const double m = neigh_box(n, c, p);
        if (which == 0) {
            if (t == 0) return neigh_round(m * e * (1.0 - q), p);
            return t == 1 ? -m * e : t == 2 ? 1.0 - m : m;
        }
        const double my = p.hex ? m : 1.0;
        const double qe = neigh_round(q * e, p);
        if (t == 0) return my * e;
        if (t == 1) return my * qe;
        return (t == 3 && p.hex ? 1.0 - m : 1.0) * neigh_round(e - qe, p);
    }
    case 2:     // bubble
        return neigh_mask(n, c, dl, p);
    default: {  // triangle
        double v = p.sigma - fabs(dl);
        if (v < 0.0) v = 0.0;
        if (p.compact) v *= neigh_mask(n, c, dl, p);
        return neigh_round(v, p);
    }
    }
}

// p_dev != nullptr: the parameters are read from device memory instead (a captured hipGraph replays
// this launch with new sigma / eta every epoch; store_params_kernel refreshes them before the replay).
__global__ void store_params_kernel(NeighParams p, NeighParams* __restrict__ dst) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *dst = p;
}

// ---- nonzero column ranges of the tables ("bands"; the GEMMs that walk them: leftmul_f32_kernel below) -------------
// Per 32-row tile of a table (the rows of one v_mfma_f32_32x32x2_f32 A operand) and per column segment (one per
// neighbourhood term) an entry {segw - first nonzero column, last nonzero column + 1} in segment coordinates; both
// fields only grow (atomicMax from {0, 0} = the tile holds no nonzero).  Layout of one buffer:
//   stage 1 (P1, [nt][Y][Y], one segment of Y columns per table):  entry t * ty + j / 32,         ty = ceil(Y / 32)
//   stage 2 (P2, [X][nt * X], nt segments of X columns):           nt * ty + (i / 32) * nt + t
// neigh_tables_kernel fills them from the float32 values it STORES (never from a formula for where the zeros ought to
// be), so a range contains every nonzero of its tile: that is the whole correctness argument of the skipping.  There
// are two buffers: a build of the tables fills buffer rsel and zeroes the other one, whose last readers (the GEMMs of
// the build before) are done; the host alternates rsel from build to build, so no launch is spent on clearing.
constexpr int LM_TILE = 32;     // rows of H per range entry
constexpr int LM_KG = 8;        // columns per skipping decision: four MFMA k steps (a tile's range is rounded outwards to it)
constexpr int LM_BK = 32;       // columns a workgroup of the GEMMs stages at a time (the k chunk)

__host__ __device__ inline int band_tiles(int rows) { return (rows + LM_TILE - 1) / LM_TILE; }
__host__ __device__ inline long band_entries(int X, int Y, int nt) { return (long)nt * (band_tiles(Y) + band_tiles(X)); }
__host__ __device__ inline long band_entry_stage1(int t, int j, int Y) { return (long)t * band_tiles(Y) + j / LM_TILE; }
__host__ __device__ inline long band_entry_stage2(int i, int t, int Y, int nt) {
    return (long)nt * band_tiles(Y) + (long)(i / LM_TILE) * nt + t;
}
// what the GEMMs make of the entries (host-callable: tests/test_transform_bands_cpu.py runs them against a NumPy model)
// a tile's range of one segment, rounded outwards to LM_KG columns: [tlo, thi), empty = {0, 0}
__host__ __device__ inline void band_tile_range(int2 v, int segw, int& tlo, int& thi) {
    tlo = 0; thi = 0;
    if (v.y > 0) {
        const int hi = v.y < segw ? v.y : segw;
        tlo = ((segw - v.x) / LM_KG) * LM_KG;
        thi = ((hi + LM_KG - 1) / LM_KG) * LM_KG;
    }
}
// are the LM_KG columns from k0 on (a multiple of LM_KG) inside [tlo, thi)?
__host__ __device__ inline bool band_group_on(int k0, int tlo, int thi) { return k0 < thi && k0 + LM_KG > tlo; }
// the columns a workgroup stages: the union over its ntiles tiles (entries tiles[t * nseg + sg]) and all segments, the
// lower end rounded down to a chunk; every segment is walked over the same [lo, hi).  Nothing nonzero: lo = hi = 0.
// (step: the entries' distance -- 2 for one piece of a toroidal table, below)
__host__ __device__ inline void band_union(const int2* tiles, int ntiles, int nseg, int segw, int chunk, int& lo, int& hi,
                                           int step = 1) {
    lo = segw; hi = 0;
    for (int i = 0; i < ntiles * nseg; ++i) {
        const int2 v = tiles[(long)i * step];
        if (v.y > 0) {
            const int l = ((segw - v.x) / chunk) * chunk, u = v.y < segw ? v.y : segw;
            lo = l < lo ? l : lo;
            hi = u > hi ? u : hi;
        }
    }
    if (hi <= lo) lo = hi = 0;
}

// an entry after one more nonzero at column `col` (what neigh_tables_kernel's atomicMax pairs leave; the CPU test's hook builds entries with it)
__host__ __device__ inline int2 band_entry_with(int2 v, int col, int segw) {
    v.x = v.x > segw - col ? v.x : segw - col;
    v.y = v.y > col + 1 ? v.y : col + 1;
    return v;
}

// Toroidal tables.  The nonzeros of a tile that touches the seam lie in TWO runs of a row, [0, w) and [L - w, L), and one
// range around both is the whole row.  So every segment is cut at band_wrap_mid(segw), the multiple of LM_KG nearest its
// middle, into a LOW piece [0, mid) and a HIGH piece [mid, segw), and a tile has one entry per segment AND PIECE: entry
// 2 e + piece where a rectangular table has entry e, the same {segw - first, last + 1} pair in SEGMENT coordinates, fed
// only by the nonzeros of its own piece (so a low range ends at or before mid and a high one begins at or after it: mid
// is a multiple of LM_KG, and rounding a range outwards to whole groups never crosses it).  A tile away from the seam
// has two adjacent ranges or one empty piece; a seam tile has [0, w) low and [L - w, L) high.  A workgroup stages the
// union per piece and walks low then high: ascending columns, no column twice (the pieces are disjoint -- the high union's
// lower end is rounded down to LM_KG, not to a chunk, so that it cannot reach below mid).
// The cut is the middle and not the nearest chunk boundary because a side of three tiles (96) has a seam tile on either
// side of every chunk boundary: rows 0..31 reach columns [0, 32 + w) and rows 64..95 columns [64 - w, 96).
// mid is 0 for a side below 8 (beside a long one): the low piece is empty and the high one is the old range.
__host__ __device__ inline int band_wrap_mid(int segw) { return ((segw / 2 + LM_KG / 2) / LM_KG) * LM_KG; }
__host__ __device__ inline int band_wrap_piece(int col, int segw) { return col >= band_wrap_mid(segw) ? 1 : 0; }

// the ranges as a launch gets them: base == nullptr: none (walk everything); else buffer (p_dev ? p_dev->rsel : sel),
// `stride` entries apart, `base` already advanced to the launch's first tile (a captured launch reads rsel where
// store_params_kernel puts it before every replay)
struct BandRanges {
    const int2* base;
    const NeighParams* p_dev;
    long stride;
    int sel;
};
__device__ __forceinline__ const int2* band_ranges_of(const BandRanges& b) {
    if (b.base == nullptr) return nullptr;
    return b.base + (long)(b.p_dev ? b.p_dev->rsel : b.sel) * b.stride;
}

// Workgroup = 16 waves = one 32-row tile of a table x 64 of its columns (wave w: rows 2 w, 2 w + 1 of the tile; lane: a
// column): blocks [0, nt ty cy) are stage 1's (term, tile, column chunk), the rest stage 2's (tile, term, column chunk),
// cy = ceil(Y / 64).  A workgroup's nonzeros belong to ONE range entry, so the waves' ballots are combined in LDS and the
// entry gets one pair of atomicMax per workgroup: side / 64 pairs per entry (all entries of a map share a cache line or
// two, where atomics are served one after the other).  neigh_tables_grid() is the grid.
// bands != nullptr: two buffers of band_entries() each (see above); this launch fills buffer p.rsel, zeroes the other.
constexpr int NT_THREADS = 1024, NT_COLS = 64;
__host__ __device__ inline long neigh_tables_grid(int X, int Y, int nt, int swapped) {
    if (swapped) return ((long)nt * Y * Y + (long)X * nt * X + NT_THREADS - 1) / NT_THREADS;   // one thread per entry
    return (long)nt * (band_tiles(Y) * ((Y + NT_COLS - 1) / NT_COLS) + band_tiles(X) * ((X + NT_COLS - 1) / NT_COLS));
}

__global__ __launch_bounds__(NT_THREADS) void neigh_tables_kernel(NeighParams p_val, const NeighParams* __restrict__ p_dev,
                                                                  float* __restrict__ P1, float* __restrict__ P2,
                                                                  int2* __restrict__ bands) {
    const NeighParams p = p_dev ? *p_dev : p_val;
    const long id = (long)blockIdx.x * NT_THREADS + threadIdx.x;
    if (p.swapped) {
        // row stage first (X == Y): P1 = the row factors [nt][X][X] (Fx_t[i][a], with eta), P2 = the column factors
        // [Y][nt*Y] (Gy_t[j][b] at column t*Y + b)   (this pipeline walks whole tables: no ranges, one thread per entry)
        const long n1 = (long)p.nt * p.Y * p.Y;
        const long n2 = (long)p.X * p.nt * p.X;
        if (id < n1) {
            int a = id % p.X;
            long r = id / p.X;
            int i = r % p.X;
            int t = r / p.X;
            double v = neigh_factor(0, t, (double)i, (double)a, p);
            P1[id] = p.wide ? (float)(v * p.eta) : (float)v * (float)p.eta;
        } else if (id < n1 + n2) {
            long q = id - n1;
            int col = q % ((long)p.nt * p.Y);
            int j = q / ((long)p.nt * p.Y);
            int t = col / p.Y, b = col % p.Y;
            P2[q] = (float)neigh_factor(1, t, (double)j, (double)b, p);
        }
        return;
    }
    __shared__ int s_first[NT_THREADS / 64], s_end[NT_THREADS / 64];
    const long nb = band_entries(p.X, p.Y, p.nt) * (p.torus ? 2 : 1);   // (toroidal: an entry per piece, band_wrap_mid)
    if (bands != nullptr && id < nb) bands[(p.rsel ? 0 : nb) + id] = make_int2(0, 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ty = band_tiles(p.Y), cy = (p.Y + NT_COLS - 1) / NT_COLS, cx = (p.X + NT_COLS - 1) / NT_COLS;
    int blk = blockIdx.x;
    const bool stage1 = blk < p.nt * ty * cy;
    int t, tile, chunk;
    if (stage1) { chunk = blk % cy; tile = (blk / cy) % ty; t = blk / (cy * ty); }
    else { blk -= p.nt * ty * cy; chunk = blk % cx; t = (blk / cx) % p.nt; tile = blk / (cx * p.nt); }
    const int side = stage1 ? p.Y : p.X;
    const int c = chunk * NT_COLS + lane;               // the BMU coordinate: b (stage 1) or a (stage 2)
    const int cls = t / p.base_nt;
    unsigned long long nz = 0;                          // the columns of this chunk in which the wave STORED a nonzero
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int r = tile * LM_TILE + wave * 2 + q;    // the unit coordinate: j (stage 1) or i (stage 2)
        const bool in = r < side && c < side;
        float stored = 0.0f;
        if (in && stage1) {
            double v = neigh_factor(1, t % p.base_nt, (double)r, (double)c, p);
            if (p.hex) {                               // class indicator on (s(j), s(cj)): s = the row is shifted by -0.5
                const int sj = ((p.Y - 1 - r) & 1) == 0, sb = ((p.Y - 1 - c) & 1) == 0;
                bool on;
                if (p.ncls == 3) on = cls == 0 ? sj == sb : cls == 1 ? (sj == 0 && sb == 1) : (sj == 1 && sb == 0);
                else on = cls == 0 ? (sj == 0 && sb == 0) : cls == 1 ? (sj == 0 && sb == 1) : cls == 2 ? (sj == 1 && sb == 0)
                                                                                                      : (sj == 1 && sb == 1);
                if (!on) v = 0.0;
            }
            stored = (float)v;
            P1[((long)t * p.Y + r) * p.Y + c] = stored;
        } else if (in) {
            // x coordinates of the class: unit rows of classes 2, 3 and BMU rows of classes 1, 3 are shifted by -0.5
            // (three classes: only the difference matters, the both-shifted rows share class 0 with the unshifted ones)
            const double off_n = p.hex && (cls == 2 || cls == 3) ? -0.5 : 0.0;
            const double off_c = p.hex && (cls == 1 || cls == 3) ? -0.5 : 0.0;
            double v = neigh_factor(0, t % p.base_nt, (double)r + off_n, (double)c + off_c, p);
            stored = p.wide ? (float)(v * p.eta) : (float)v * (float)p.eta;
            P2[((long)r * p.nt + t) * p.X + c] = stored;
        }
        nz |= __ballot(in && stored != 0.0f);
    }
    if (bands == nullptr) return;
    if (p.torus) {
        // the same record once per piece, from the columns of this chunk that lie in it (mid need not be a multiple of 64)
        const int nlow = min(max(band_wrap_mid(side) - chunk * NT_COLS, 0), NT_COLS);
        const unsigned long long low = nlow >= 64 ? ~0ull : (1ull << nlow) - 1ull;
        for (int piece = 0; piece < 2; ++piece) {
            const unsigned long long m = piece ? nz & ~low : nz & low;
            if (lane == 0) {
                s_first[wave] = m != 0 ? chunk * NT_COLS + (int)__builtin_ctzll(m) : side;
                s_end[wave] = m != 0 ? chunk * NT_COLS + 64 - (int)__builtin_clzll(m) : 0;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                int first = side, end = 0;
                for (int w = 0; w < NT_THREADS / 64; ++w) { first = min(first, s_first[w]); end = max(end, s_end[w]); }
                if (end > 0) {
                    const long e = stage1 ? band_entry_stage1(t, tile * LM_TILE, p.Y) : band_entry_stage2(tile * LM_TILE, t, p.Y, p.nt);
                    int* r = (int*)(bands + (p.rsel ? nb : 0) + 2 * e + piece);
                    atomicMax(r, side - first);
                    atomicMax(r + 1, end);
                }
            }
            __syncthreads();
        }
        return;
    }
    if (lane == 0) {
        s_first[wave] = nz != 0 ? chunk * NT_COLS + (int)__builtin_ctzll(nz) : side;
        s_end[wave] = nz != 0 ? chunk * NT_COLS + 64 - (int)__builtin_clzll(nz) : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int first = side, end = 0;
        for (int w = 0; w < NT_THREADS / 64; ++w) { first = min(first, s_first[w]); end = max(end, s_end[w]); }
        if (end > 0) {
            const long e = stage1 ? band_entry_stage1(t, tile * LM_TILE, p.Y) : band_entry_stage2(tile * LM_TILE, t, p.Y, p.nt);
            int* r = (int*)(bands + (p.rsel ? nb : 0) + e);
            atomicMax(r, side - first);
            atomicMax(r + 1, end);
        }
    }
}

// `swapped` pipeline, between its two stages: V[i][t][b][:] *= m2(i, b) for terms 0 and 1 and *= 1 - m2(i, b) for term
// 3 (neigh_factor), where m2 is the reference's second mask on px -- row index i against BMU column b
// (neighborhoods.py:70).
__global__ __launch_bounds__(256) void mask_rows_kernel(NeighParams p_val, const NeighParams* __restrict__ p_dev,
                                                        float* __restrict__ V, int D1p) {
    const NeighParams p = p_dev ? *p_dev : p_val;
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    const long per_i = (long)p.nt * p.Y * D1p;
    const long total = (long)p.X * per_i;
    if (id >= total) return;
    const int i = (int)(id / per_i);
    const long r = id - (long)i * per_i;
    const int t = (int)(r / ((long)p.Y * D1p));
    const int b = (int)((r / D1p) % p.Y);
    if (t == 2) return;
    if ((neigh_box((double)i, (double)b, p) != 0.0) == (t == 3)) V[id] = 0.0f;
}

// ---- OUT[b] = H (Ro x Ri) * M[b] (Ri x C), exact float32 on v_mfma_f32_32x32x2_f32 ---------------
// Workgroup = 4 waves as 2 (rows) x 2 (cols); wave tile 64 x 64 (2 x 2 MFMA tiles); block tile
// 128 x 128; k chunk 32.  The next chunk's global loads are issued into registers before the MFMAs of
// the current chunk and written to LDS after them (one LDS buffer, two barriers per chunk), so HBM/L2
// latency hides under the 64 MFMAs per wave.
//
// Bands.  Late in training sigma is small and the neighbourhood tables underflow to EXACT float32 zeros
// away from the diagonal (exp(-dx^2/d) < 2^-150 for |dx| > ~7 sigma at std_coeff 0.5; bubble / triangle
// are compact by definition).  neigh_tables_kernel records, per 32-row tile of H and per column segment
// (one per neighbourhood term), the column range that holds every nonzero (above).  A workgroup stages
// 32-column chunks over the union of its tiles' ranges only, and a wave issues the MFMAs of an a-tile only
// for the LM_KG-column groups inside that tile's own range (a wave-uniform test; the k order of the steps that
// remain is the ascending one of the full walk).  A skipped step would have added 0 * m = +0 to a float32
// accumulator, so the result is bit-identical for finite data.
constexpr int LM_BM = 128, LM_BN = 128;               // (LM_BK = 32, the k chunk: with the ranges, above)
constexpr int LM_NARROW = 8;    // a last column tile this narrow goes to leftmul_narrow_f32_kernel (VALU) instead of a
                                // mostly empty 128-wide MFMA tile (64x64x32: 32 columns as a partial MFMA tile 11 us, as VALU 14)

// No ranges (br.base == nullptr): the whole of H (one segment [0, Ri)); else br.base is the entry of the launch's first
// 32-row tile, segment 0.  C columns are computed; rows of M are ld, rows of OUT ldo floats apart.
// BM = rows of H per workgroup: 128 (waves 2 x 2, each 64 rows x 64 columns) or 64 (waves 1 x 4, each 64 rows x 32
// columns; launch_leftmul in somhip.hip chooses).
// WRAP: the ranges are a toroidal table's, two per tile and segment (band_wrap_mid); every segment is walked over the
// union of the low pieces, then over the union of the high pieces.  The body of two kernels, below: WRAP is a compile-time
// constant in each, so the rectangular / hexagonal kernel is the code it was.
template <int A> using a_is = std::integral_constant<int, A>;
template <int BM, bool WRAP>
__device__ __forceinline__ void leftmul_f32_body(const float* __restrict__ H, int Ro, int Ri,
                                                 const float* __restrict__ M, long m_batch_stride,
                                                 float* __restrict__ OUT, long o_batch_stride, long C,
                                                 long ld, long ldo, BandRanges br, int nseg, int segw) {
    static_assert(BM == 128 || BM == 64, "leftmul: 128- or 64-row tiles");
    static_assert(LM_BK % LM_KG == 0 && LM_KG % 2 == 0, "leftmul: whole MFMA steps per skipping group, whole groups per chunk");
    constexpr int NT = BM / LM_TILE;                     // range entries (32-row tiles) per workgroup
    constexpr int TC = BM / 64;                          // 32-column tiles per wave: 2 (64 columns) or 1 (32 columns)
    constexpr int HQ = BM / 32;                          // 4-float pieces of the H tile per thread
    __shared__ float Hs[BM][LM_BK + 1];
    __shared__ __attribute__((aligned(16))) float Ms[LM_BK][LM_BN + 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, col = lane & 31;
    const int wr = BM == 128 ? wave >> 1 : 0;            // this wave's 64 rows ...
    const int wcol = BM == 128 ? (wave & 1) * 64 : wave * 32;   // ... and its first column inside the 128-column tile
    const long c0 = (long)blockIdx.x * LM_BN;
    const int i0 = blockIdx.y * BM;
    const int2* __restrict__ ranges = band_ranges_of(br);
    const float* Mb = M + (long)blockIdx.z * m_batch_stride;
    float* Ob = OUT + (long)blockIdx.z * o_batch_stride;

    f32x16 acc[2][TC];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int t = 0; t < TC; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][t][r] = 0.0f;

    // this thread's share of the staged chunk: four 4-float pieces of each operand tile -- piece q of the H tile
    // (128 x 32) is row (tid + 256 q) >> 3, columns 4 ((tid + 256 q) & 7) .. + 3; of the M tile (32 x 128) row
    // (tid + 256 q) >> 5, columns 4 ((tid + 256 q) & 31) .. + 3.  A piece that lies inside the operand and is
    // 16-byte aligned is ONE global_load_dwordx4 (the common case: 8 loads per thread and chunk where the scalar
    // form needed 32 loads with their 64-bit address arithmetic); otherwise its four floats are loaded one by one.
    f32x4 hreg[HQ], mreg[4];
    auto fetch = [&](int r0, int kend) __attribute__((always_inline)) {               // chunk [r0, r0 + 32) clipped to columns < kend
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + q * 256;
            if (q < HQ) {
                const int i = idx >> 3, k = (idx & 7) * 4;
                const float* src = H + (long)(i0 + i) * Ri + r0 + k;
                // (the piece's own address decides: a banded chunk starts at sg * segw + lo, any float offset)
                if (((uintptr_t)src & 15) == 0 && i0 + i < Ro && r0 + k + 3 < kend) hreg[q] = *(const f32x4*)src;
                else
#pragma unroll
                    for (int e = 0; e < 4; ++e) hreg[q][e] = (i0 + i < Ro && r0 + k + e < kend) ? src[e] : 0.0f;
            }
            {
                const int kk = idx >> 5, c = (idx & 31) * 4;
                const float* src = Mb + (long)(r0 + kk) * ld + c0 + c;
                if (((uintptr_t)src & 15) == 0 && r0 + kk < kend && c0 + c + 3 < C) mreg[q] = *(const f32x4*)src;
                else
#pragma unroll
                    for (int e = 0; e < 4; ++e) mreg[q][e] = (r0 + kk < kend && c0 + c + e < C) ? src[e] : 0.0f;
            }
        }
    };
    auto stash = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + q * 256;
            if (q < HQ) {
                const int i = idx >> 3, k = (idx & 7) * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e) Hs[i][k + e] = hreg[q][e];      // (33-float rows: conflict-free reads, scalar writes)
            }
            *(f32x4*)&Ms[idx >> 5][(idx & 31) * 4] = mreg[q];               // 132-float rows: 16-byte aligned
        }
    };

    // the chunks to walk (uniform over the workgroup): every segment is walked over the union [lo, hi) of the
    // nonzero ranges of the workgroup's tiles and segments, LM_BK columns at a time, clipped to hi
    // (WRAP: [lo, hi) is the union of the low pieces, [lo2, hi2) that of the high pieces, walked behind it)
    int lo = 0, hi = Ri, ns = 1, sw = Ri;
    int lo2 = 0, hi2 = 0;
    const int my_tiles = min(NT, band_tiles(Ro - i0));   // (the entries of tiles past the last row do not exist)
    bool dense = true;                                   // every tile of the workgroup covers [lo, hi) in every segment
    if (WRAP) {                                          // (a WRAP launch always has ranges)
        ns = nseg; sw = segw;
        const int2* mine = ranges + (long)blockIdx.y * NT * nseg * 2;
        band_union(mine, my_tiles, nseg, segw, LM_BK, lo, hi, 2);
        band_union(mine + 1, my_tiles, nseg, segw, LM_KG, lo2, hi2, 2);   // (LM_KG: never below the cut, band_wrap_mid)
        dense = my_tiles == NT;
        for (int i = 0; i < my_tiles * nseg; ++i) {
            int l, u;
            band_tile_range(mine[2 * i], segw, l, u);
            dense = dense && l <= lo && u >= hi;
            band_tile_range(mine[2 * i + 1], segw, l, u);
            dense = dense && l <= lo2 && u >= hi2;
        }
    } else if (ranges != nullptr) {
        ns = nseg; sw = segw;
        const int2* mine = ranges + (long)blockIdx.y * NT * nseg;
        band_union(mine, my_tiles, nseg, segw, LM_BK, lo, hi);
        dense = my_tiles == NT;
        for (int i = 0; i < my_tiles * nseg; ++i) {
            int l, u;
            band_tile_range(mine[i], segw, l, u);
            dense = dense && l <= lo && u >= hi;
        }
    }
    const int per = (hi - lo + LM_BK - 1) / LM_BK;     // chunks per segment (WRAP: of its low piece)
    const int per2 = WRAP ? (hi2 - lo2 + LM_BK - 1) / LM_BK : 0;   // ... of its high piece
    const int pers = per + per2;
    const int total = pers * ns;
    auto chunk_at = [&](int c, int& sg, int& j, int& r0, int& kend) __attribute__((always_inline)) {
        sg = c / pers; j = c - sg * pers;
        if (WRAP && j >= per) {
            r0 = sg * sw + lo2 + (j - per) * LM_BK;
            kend = sg * sw + hi2;
        } else {
            r0 = sg * sw + lo + j * LM_BK;
            kend = sg * sw + hi;
        }
    };
    // this wave's two a-tiles: their own ranges in the segment being walked (wave-uniform; no ranges: everything)
    const int wtile = __builtin_amdgcn_readfirstlane(wr) * 2;
    int tlo[2] = {0, 0}, thi[2] = {0, 0};
    // the MFMA steps of columns [g LM_KG, g LM_KG + LM_KG) of the staged chunk for a-tiles [a0, a1)
    auto steps = [&](int g, auto first, auto end) __attribute__((always_inline)) {
        constexpr int a0 = decltype(first)::value, a1 = decltype(end)::value;
#pragma unroll
        for (int kk = 0; kk < LM_KG; kk += 2) {
            const int k = g * LM_KG + kk;
            float av[2], bv[TC];
#pragma unroll
            for (int a = 0; a < 2; ++a) if (a >= a0 && a < a1) av[a] = Hs[wr * 64 + a * 32 + col][k + half];
#pragma unroll
            for (int t = 0; t < TC; ++t) bv[t] = Ms[k + half][wcol + t * 32 + col];
#pragma unroll
            for (int a = 0; a < 2; ++a)
                if (a >= a0 && a < a1)
#pragma unroll
                    for (int t = 0; t < TC; ++t)
                        acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[t], acc[a][t], 0, 0, 0);
        }
    };
    auto store = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int t = 0; t < TC; ++t) {
                long c = c0 + wcol + t * 32 + col;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    int i = i0 + wr * 64 + a * 32 + mfma32_row(r, half);
                    if (i < Ro && c < C) Ob[(long)i * ldo + c] = acc[a][t][r];
                }
            }
    };
    // The walk, in two forms that share nothing after the prologue (one loop with both forms inside makes the compiler
    // keep the accumulators twice: 128 AGPRs, a workgroup per CU less).  DENSE: every tile of the workgroup is nonzero
    // over the whole of [lo, hi) in every segment, or there are no ranges -- 16 MFMA steps per chunk and a-tile in one
    // straight run.  Otherwise each a-tile runs the LM_KG-column groups of its own range, ascending.
    auto walk = [&](auto dense_form) __attribute__((always_inline)) {
        constexpr bool DENSE = decltype(dense_form)::value;
        int sg = 0, j = 0;
        if (total > 0) { int r0, kend; chunk_at(0, sg, j, r0, kend); fetch(r0, kend); }
        for (int c = 0; c < total; ++c) {
            __syncthreads();                            // everyone is done reading the previous chunk
            stash();
            __syncthreads();
            const int piece = WRAP && j >= per;         // (per == 0: a segment begins with its high piece)
            const int kc = piece ? lo2 + (j - per) * LM_BK : lo + j * LM_BK;   // the staged chunk's first column, in segment coordinates
            if (!DENSE && (j == 0 || (WRAP && j == per))) {   // a new segment (or piece): this wave's tiles' ranges in it
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    int2 v = make_int2(0, 0);
                    if (wtile + a < my_tiles) {
                        const long e = ((long)blockIdx.y * NT + wtile + a) * nseg + sg;
                        v = ranges[WRAP ? 2 * e + piece : e];
                    }
                    int l, u;
                    band_tile_range(v, segw, l, u);
                    tlo[a] = __builtin_amdgcn_readfirstlane(l);
                    thi[a] = __builtin_amdgcn_readfirstlane(u);
                }
            }
            if (c + 1 < total) { int r0, kend; chunk_at(c + 1, sg, j, r0, kend); fetch(r0, kend); }   // in flight under the MFMAs below
            if (DENSE) {
#pragma unroll
                for (int g = 0; g < LM_BK / LM_KG; ++g) steps(g, a_is<0>(), a_is<2>());
            } else {
                int g0[2], g1[2];                       // (tlo, thi: multiples of LM_KG)
#pragma unroll
                for (int a = 0; a < 2; ++a) { g0[a] = max(tlo[a] - kc, 0) / LM_KG; g1[a] = min((thi[a] - kc) / LM_KG, LM_BK / LM_KG); }
#pragma unroll 1
                for (int g = g0[0]; g < g1[0]; ++g) steps(g, a_is<0>(), a_is<1>());
#pragma unroll 1
                for (int g = g0[1]; g < g1[1]; ++g) steps(g, a_is<1>(), a_is<2>());
            }
        }
        store();
    };
    if (dense) walk(std::integral_constant<bool, true>());
    else walk(std::integral_constant<bool, false>());
}

template <int BM>
__global__ __launch_bounds__(256, BM == 128 ? 3 : 5) void leftmul_f32_kernel(const float* __restrict__ H, int Ro, int Ri,
                                                          const float* __restrict__ M, long m_batch_stride,
                                                          float* __restrict__ OUT, long o_batch_stride, long C,
                                                          long ld, long ldo, BandRanges br, int nseg, int segw) {
    leftmul_f32_body<BM, false>(H, Ro, Ri, M, m_batch_stride, OUT, o_batch_stride, C, ld, ldo, br, nseg, segw);
}
// the same product over a toroidal table's ranges (br.base != nullptr; launch_leftmul in somhip.hip takes it for those only)
template <int BM>
__global__ __launch_bounds__(256, BM == 128 ? 3 : 5) void leftmul_wrap_f32_kernel(const float* __restrict__ H, int Ro, int Ri,
                                                          const float* __restrict__ M, long m_batch_stride,
                                                          float* __restrict__ OUT, long o_batch_stride, long C,
                                                          long ld, long ldo, BandRanges br, int nseg, int segw) {
    leftmul_f32_body<BM, true>(H, Ro, Ri, M, m_batch_stride, OUT, o_batch_stride, C, ld, ldo, br, nseg, segw);
}

// The columns [c_begin, C) of the same product when they are too few for a 128-wide MFMA tile (the count
// column and its padding behind input_len = 128: D1p = 132 = 128 + 4): a VALU kernel, thread = (row, column
// parity), k-ordered fmaf chains over the same chunks in the same order -- bit for bit what the MFMA tile
// computes (v_mfma_f32_32x32x2_f32 is that chain; skipped chunks add exact zeros) at a few percent of its time.
// Grid = (1, row blocks, batch).
template <int NQ>                                       // columns handled per thread: live <= 2 * NQ <= LM_NARROW
__global__ __launch_bounds__(256) void leftmul_narrow_f32_kernel(const float* __restrict__ H, int Ro, int Ri,
                                                                 const float* __restrict__ M, long m_batch_stride,
                                                                 float* __restrict__ OUT, long o_batch_stride, long C,
                                                                 long ld, long ldo, long c_begin, BandRanges br, int nseg,
                                                                 int segw) {
    __shared__ float Hs[LM_BM][LM_BK + 1];
    __shared__ float Ms[LM_BK][2 * NQ];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.y * LM_BM;
    const float* Mb = M + (long)blockIdx.z * m_batch_stride;
    float* Ob = OUT + (long)blockIdx.z * o_batch_stride;
    const int live = (int)(C - c_begin);                // <= LM_NARROW
    const int row = tid & (LM_BM - 1), par = tid >> 7;  // 256 threads = 128 rows x 2 column parities
    float acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0f;

    // the union of the block's four tiles and all segments (the chunks the MFMA kernel's 128-row workgroup stages)
    const int2* __restrict__ ranges = band_ranges_of(br);
    int lo = 0, hi = Ri, ns = 1, sw = Ri;
    if (ranges != nullptr) {
        ns = nseg; sw = segw;
        constexpr int NT = LM_BM / LM_TILE;
        band_union(ranges + (long)blockIdx.y * NT * nseg, min(NT, band_tiles(Ro - i0)), nseg, segw, LM_BK, lo, hi);
    }
    const int per = (hi - lo + LM_BK - 1) / LM_BK;
    const int total = per * ns;
    for (int c = 0; c < total; ++c) {
        const int sg = c / per, j = c - sg * per;
        const int r0 = sg * sw + lo + j * LM_BK, kend = sg * sw + hi;
        __syncthreads();
        for (int idx = tid; idx < LM_BM * LM_BK; idx += 256) {
            const int i = idx >> 5, k = idx & 31;
            Hs[i][k] = (i0 + i < Ro && r0 + k < kend) ? H[(long)(i0 + i) * Ri + r0 + k] : 0.0f;
        }
        for (int idx = tid; idx < LM_BK * 2 * NQ; idx += 256) {
            const int k = idx / (2 * NQ), cc = idx - k * (2 * NQ);
            Ms[k][cc] = (r0 + k < kend && cc < live) ? Mb[(long)(r0 + k) * ld + c_begin + cc] : 0.0f;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < LM_BK; ++k) {
            const float hv = Hs[row][k];
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q] = __builtin_fmaf(hv, Ms[k][2 * q + par], acc[q]);
        }
    }
    const int i = i0 + row;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        if (i < Ro && 2 * q + par < live) Ob[(long)i * ldo + c_begin + 2 * q + par] = acc[q];
}

// ---- the update as the reference states it: num = g^T x, den = sum_n g  (xpysom.py:434-441) -----------------------
// The FAITHFUL form, kept beside the bucketed one for cross-checking and for the record: a K x N x D
// float32 MFMA GEMM whose A operand g[n, k] = sum_t Px_t[i_k, ci_n] Py_t[j_k, cj_n] is generated from the
// neighbourhood tables on the way into LDS and never exists in memory.  Same tiling as leftmul_f32_kernel (128 units
// x 128 features per workgroup, 32-row chunks of the samples as the k axis).  2 N K D flop: 17.6 TFLOP per epoch at
// 256 x 256 x 128 with 1 Mi rows, where the bucketed form needs 8.7 GFLOP.
__global__ __launch_bounds__(256) void faithful_update_f32_kernel(const float* __restrict__ X, const int* __restrict__ bmu,
                                                                  long N, int D, int D1p, int Xm, int Ym, int nt,
                                                                  const float* __restrict__ P1, const float* __restrict__ P2,
                                                                  float* __restrict__ ACC) {
    __shared__ float Gs[LM_BM][LM_BK + 1];               // g[unit][row of the chunk]
    __shared__ __attribute__((aligned(16))) float Xs[LM_BK][LM_BN + 4];
    __shared__ int ci_s[LM_BK], cj_s[LM_BK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, col = lane & 31;
    const int wr = wave >> 1, wc = wave & 1;
    const long c0 = (long)blockIdx.x * LM_BN;            // first feature column of the tile
    const int u0 = blockIdx.y * LM_BM;                   // first unit of the tile
    const int K = Xm * Ym;
    // this thread generates g for the 16 units (tid >> 5) + 8 q and the chunk row tid & 31
    int iu[16], ju[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int u = u0 + (tid >> 5) + 8 * q;
        iu[q] = u < K ? u / Ym : -1;
        ju[q] = u < K ? u % Ym : 0;
    }
    float den[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) den[q] = 0.0f;
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][t][r] = 0.0f;

    for (long r0 = 0; r0 < N; r0 += LM_BK) {
        __syncthreads();                                 // everyone is done with the previous chunk
        if (tid < LM_BK) {
            const long n = r0 + tid;
            const int b = n < N ? bmu[n] : -1;
            ci_s[tid] = b >= 0 ? b / Ym : -1;
            cj_s[tid] = b >= 0 ? b % Ym : 0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {                    // the rows of the chunk: 32 x 128 features (16-byte pieces)
            const int idx = tid + q * 256;
            const int kk = idx >> 5, c = (idx & 31) * 4;
            const long n = r0 + kk;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (n < N && c0 + c + e < D) v[e] = X[n * D + c0 + c + e];
            *(f32x4*)&Xs[kk][c] = v;
        }
        __syncthreads();
        {
            const int k = tid & 31;
            const int ci = ci_s[k], cj = cj_s[k];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                float g = 0.0f;
                if (ci >= 0 && iu[q] >= 0)
                    for (int t = 0; t < nt; ++t)
                        g = __builtin_fmaf(P2[(long)iu[q] * nt * Xm + t * Xm + ci], P1[((long)t * Ym + ju[q]) * Ym + cj], g);
                Gs[(tid >> 5) + 8 * q][k] = g;
                den[q] += g;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < LM_BK; k += 2) {
            float av[2], bv[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) av[a] = Gs[wr * 64 + a * 32 + col][k + half];
#pragma unroll
            for (int t = 0; t < 2; ++t) bv[t] = Xs[k + half][wc * 64 + t * 32 + col];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[t], acc[a][t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const long c = c0 + wc * 64 + t * 32 + col;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int u = u0 + wr * 64 + a * 32 + mfma32_row(r, half);
                if (u < K && c < D) ACC[(long)u * D1p + c] = acc[a][t][r];
            }
        }
    if (blockIdx.x == 0) {                               // den: the 32 threads of a half-wave hold one unit's partial sums
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            float s = den[q];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            const int u = u0 + (tid >> 5) + 8 * q;
            if ((tid & 31) == 0 && u < K) ACC[(long)u * D1p + D] = s;
        }
    }
}

// ---- the count column's own transform ---------------------------------------------------------------
// den = sum_t Px_t C Py_t^T with C[a][b] = the count of unit (a, b): two X x Y x {Y, nt X} products, 33 MFLOP each
// at 256 x 256.  Kept out of the batched MFMA transform, whose column tiles are 128 wide: input_len = 128 would
// give the count a second, empty tile.  OUT[i*oi + j*oj] = sum_k A[i*ai + k*ak] * B[k*bk + j*bj], k ascending,
// one fmaf chain per output: exactly the chain the MFMA tiles computed for this column (skipped zero bands
// add exact zeros), so the denominator is bit for bit what it was.  The operands are columns of wide arrays
// (one float per 528-byte row) or small dense matrices, so the kernel is latency-bound: a workgroup (16 x 16 outputs,
// one per thread: 256 workgroups at 256 x 256) issues the loads of SG_KC = 256 k-steps of both operands at once --
// one round trip per 256 k-steps -- before it multiplies.
constexpr int SG_KC = 256, SG_T = 16;   // k-steps staged at once; output tile side (one output per thread)
__global__ __launch_bounds__(256) void strided_gemm_f32_kernel(const float* __restrict__ A, long ai, long ak,
                                                               const float* __restrict__ B, long bk, long bj,
                                                               float* __restrict__ OUT, long oi, long oj, int M, int N,
                                                               int Kd, long a_batch, long b_batch, long o_batch) {
    __shared__ float As[SG_T][SG_KC + 1];
    __shared__ float Bs[SG_KC][SG_T + 1];
    const int tx = threadIdx.x & (SG_T - 1), ty = threadIdx.x / SG_T;   // 16 x 16
    const int i0 = blockIdx.y * SG_T, j0 = blockIdx.x * SG_T;
    A += (long)blockIdx.z * a_batch; B += (long)blockIdx.z * b_batch; OUT += (long)blockIdx.z * o_batch;
    // the unit-stride axis of each operand goes along consecutive threads (either k or the row / column index)
    const bool a_k_fast = ak <= ai, b_j_fast = bj <= bk;
    float acc = 0.f;
    for (int k0 = 0; k0 < Kd; k0 += SG_KC) {
        __syncthreads();
        constexpr int PER = SG_T * SG_KC / 256;                  // elements of each operand per thread
        float ra[PER], rb[PER];
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int e = q * 256 + threadIdx.x;
            const int ar = a_k_fast ? e / SG_KC : e % SG_T, akk = a_k_fast ? e % SG_KC : e / SG_T;
            ra[q] = (i0 + ar < M && k0 + akk < Kd) ? A[(long)(i0 + ar) * ai + (long)(k0 + akk) * ak] : 0.0f;
            const int bc = b_j_fast ? e % SG_T : e / SG_KC, bkk = b_j_fast ? e / SG_T : e % SG_KC;
            rb[q] = (k0 + bkk < Kd && j0 + bc < N) ? B[(long)(k0 + bkk) * bk + (long)(j0 + bc) * bj] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int e = q * 256 + threadIdx.x;
            const int ar = a_k_fast ? e / SG_KC : e % SG_T, akk = a_k_fast ? e % SG_KC : e / SG_T;
            As[ar][akk] = ra[q];
            const int bc = b_j_fast ? e % SG_T : e / SG_KC, bkk = b_j_fast ? e / SG_T : e % SG_KC;
            Bs[bkk][bc] = rb[q];
        }
        __syncthreads();
        const int kn = Kd - k0 < SG_KC ? Kd - k0 : SG_KC;
#pragma unroll 8
        for (int k = 0; k < kn; ++k) acc = __builtin_fmaf(As[ty][k], Bs[k][tx], acc);
    }
    const int i = i0 + ty, j = j0 + tx;
    if (i < M && j < N) OUT[(long)i * oi + (long)j * oj] = acc;
}

// ---- merge: W = where(den != 0, num/den, W)  (xpysom.py:446-455) ---------------------------------
// (Wp, inv: the exact mode's copy of the codebook in patch order -- inv[unit] = position, som_common.hpp -- kept in step)
__global__ __launch_bounds__(256) void merge_kernel(float* __restrict__ W, const float* __restrict__ ACC,
                                                    long K, int D, int D1p, float* __restrict__ Wp = nullptr,
                                                    const int* __restrict__ inv = nullptr) {
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= K * D) return;
    long k = i / D;
    int d = (int)(i - k * D);
    float den = ACC[k * D1p + D];
    if (den != 0.0f) {
        const float v = ACC[k * D1p + d] / den;
        W[i] = v;
        if (Wp != nullptr) {
            Wp[(long)inv[k] * D + d] = v;
        }
    }
}

// ---- merge of a handle with missing values (SOM_MISSING_NAN): a denominator per unit AND feature ----
// ACC row k = [num (D) | den (D) | total]: W[k][d] = num[k][d] / den[k][d] where den[k][d] != 0, else W[k][d] stays bit for bit
__global__ __launch_bounds__(256) void merge_masked_kernel(float* __restrict__ W, const float* __restrict__ ACC, long K, int D,
                                                           int D1p) {
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= K * D) return;
    long k = i / D;
    int d = (int)(i - k * D);
    const float den = ACC[k * D1p + D + d];
    if (den != 0.0f) W[i] = ACC[k * D1p + d] / den;
}

// ---- quantization error: sum_n |x_n - W[bmu_n]|  (xpysom.py:703-705) -----------------------------
// (persistent: a wave walks rows wave, wave + waves, ... and keeps its sum in a double; ONE atomic per workgroup -- a workgroup
//  per four rows put 262 144 double atomics of a million-row call on one address: 3.2 ms of a 0.3 ms kernel)
__global__ __launch_bounds__(256) void qe_kernel(const float* __restrict__ X, const int* __restrict__ bmu,
                                                 const float* __restrict__ W, long N, int D,
                                                 double* __restrict__ sum_out) {
    __shared__ double part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long waves = (long)gridDim.x * 4;
    double acc = 0.0;
    for (long row = (long)blockIdx.x * 4 + wave; row < N; row += waves) {
        const float* x = X + row * D;
        const float* w = W + (long)bmu[row] * D;
        float s = 0.0f;
        for (int k = lane; k < D; k += 64) { float df = x[k] - w[k]; s = __builtin_fmaf(df, df, s); }
        s = wave_sum(s);
        acc += (double)__builtin_sqrtf(s);
    }
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sum_out, (part[0] + part[1]) + (part[2] + part[3]));
}

}  // namespace somhip
