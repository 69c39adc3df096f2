// The k nearest units of every row (som_bmu_topk*, som_unit_rank_counts*; include/somhip.h): the float32 MFMA scan with a top-k
// epilogue, the (n, K) score matrix never written.
//
// For a row x_n, s_nk is the float32 activation score of the handle's distance -- score_f32<MODE> (bmu_f32.hpp) of the k-ordered
// float32 fma chain v_mfma_f32_32x32x2_f32 forms from 0, |w_k|^2 and |x_n|^2 in NumPy's pairwise order: bit for bit the entry
// dist_matrix_f32_kernel<MODE> writes.  The list of row n: the k units with the smallest s_nk, ascending by (score, unit id) -- equal
// scores (-0 == +0) go to the lower id -- of the scores that are < +inf (NaN and +inf never enter; -inf does).  A slot nothing fills
// holds id -1 and a NaN score.
//
//   bmu_topk_f32_kernel<MODE, KK>   the scan, KK = 4 or 8 list slots (a call of k runs the next instance up; the spare slots are
//                                   kept and never reported: the k best of the KK best are the k best).  grid = row tiles x parts
//   topk_merge_kernel<KK>           a thread per row: the k lowest (score, id) over the parts' lists; spare slots dropped, an
//                                   unfilled slot written as -1 / NaN
//   topk_dist_kernel                a wave per (row, slot): sqrt(sum_d (x_d - W[id][d])^2) in bmu_dist_kernel's arithmetic (diag.hpp)
//   unit_rank_counts_kernel         a thread per (row, slot): counts[slot][id] += 1, integer atomics only
//
// The scan's mapping is bmu_f32_kernel's: A operand = units, B operand = samples.  A workgroup = 4 waves x 32 samples; a lane owns
// ONE sample (lane & 31) and accumulator register r of block rb is unit u0 + 32 rb + mfma32_row(r, lane >> 5), ascending in r.  The
// lane's list -- KK scores and KK unit ids, sorted -- lives in registers.  Both operands go through LDS in chunks of F32_KC features
// (+1 padded rows: conflict-free fragment reads), two buffers, ONE barrier per chunk, density.hpp's scheme: in front of a chunk's
// MFMAs the chunk after it is written from registers to the other buffer and the chunk after that is loaded into the registers.
// The rows' chunk is staged again for every 128-unit stage: it comes from L2, under a chunk's 64 MFMAs per wave.
//
// Epilogue, per 32 x 32 tile: the 16 scores are formed and reduced with fminf; only a lane whose tile minimum is `<` its k-th score
// walks the 16 registers, and each score that is `<` the k-th is inserted by an unrolled compare-and-shift (no dynamic indexing, no
// scratch).  A lane meets its units in ascending id order and inserts BEHIND every score that is <= the new one, so within a lane
// the list is the stable order; `<` against the k-th keeps the earlier, lower id on an equal score.  Padding units (>= K) are set to
// +inf and never compete.  The two lane halves hold disjoint units: at the end each takes the other's list through
// __shfl_xor(.., 32) and inserts it by (score, id).
//
// Codebook parts, so that few rows still fill the chip: part p scans the 128-unit stages [p * per, (p + 1) * per) and writes its
// list to scratch ([part][row][KK] scores and ids); topk_merge_kernel joins them by the total order (score, id).  No atomics: the
// result is identical for every part count.  The count is pure host arithmetic (topk_plan).
//
// Tails: every load is unconditional on an address clamped into its array (density.hpp).  Padding features are staged as zeros on
// both sides, padding units never compete, padding rows (>= N: a copy of the last row) are never written.  Any D >= 1, K >= 1,
// N >= 1; row offsets are 64-bit.
//
// Registers (hipcc -O3, gfx950; -Rpass-analysis=kernel-resource-usage), two waves per SIMD asked for; VGPRs of <MODE, KK>:
//     part, 4: 195    part, 8: 237    sq, 4: 199    sq, 8: 241    cosine, 4: 202    cosine, 8: 247
// no AGPRs, no scratch, no SGPR or VGPR spills in any of the six (64 accumulator registers, 32 of the chunk in flight, the list's
// 2 KK, a tile's 16 scores).  That took three pins (asm volatile("" : "+v"(..)), an empty statement the compiler cannot look
// through): left alone it forms a stage's 64 unit ids and 64 tail masks and the staging's 32 row offsets ahead of the MFMAs and
// holds them across, and spills (77 SGPRs, up to 101 VGPRs).  LDS: 68 608 bytes (two buffers of both tiles' chunk, two of a
// stage's |w|^2): two workgroups per CU, the barriers of one under the MFMAs of the other.  topk_merge_kernel 24 / 33 VGPRs,
// topk_dist_kernel 24, unit_rank_counts_kernel 12, none with scratch.
#pragma once
#include "bmu_f32.hpp"

namespace somhip {

constexpr int TOPK_MAX = 8;
constexpr int TOPK_LD = F32_KC + 1;
// bytes of dynamic LDS bmu_topk_f32_kernel needs: two buffers of the unit stage's and the row tile's chunk, two of a stage's |w|^2
constexpr size_t TOPK_LDS_BYTES = (size_t)(2 * ((F32_UB + F32_SB) * TOPK_LD + F32_UB)) * sizeof(float);
// Rows per pass of a call: the lists (ids, scores, distances: 12 bytes a slot) and the partial lists (8 bytes a slot and part) are
// sized for one pass, so the scratch of a call stays bounded whatever n_rows is -- 24 MiB of lists at k = 8, and 16 MiB of partial
// lists per part (2 048 row tiles fill the chip on their own: one part).
constexpr long TOPK_PASS_ROWS = 262144;

// Launch geometry: pure host arithmetic (som_debug_topk_plan, include/somhip_test.h).  slots: workgroups of the scan the chip holds
// at once; forced > 0: the part count asked for (SOM_TOPK_PARTS), clamped the same way.  The codebook's 128-unit stages are cut
// into as many parts as it takes to reach `slots` workgroups, never more than there are stages; a count that would leave parts
// without a stage is lowered to the parts that have one.
struct TopkPlan { long row_tiles, stages, parts, per; };
inline TopkPlan topk_plan(long n_rows, int K, long slots, int forced) {
    TopkPlan p;
    p.row_tiles = (n_rows + F32_SB - 1) / F32_SB;
    p.stages = ((long)K + F32_UB - 1) / F32_UB;
    long s = forced > 0 ? (long)forced : (slots + p.row_tiles - 1) / p.row_tiles;
    s = s < 1 ? 1 : (s > p.stages ? p.stages : s);
    p.per = (p.stages + s - 1) / s;
    p.parts = (p.stages + p.per - 1) / p.per;
    return p;
}

// (score, id) strictly before (score, id): the total order of the lists
__device__ __forceinline__ bool topk_before(float sa, int ia, float sb, int ib) { return sa < sb || (sa == sb && ia < ib); }

// v (unit u) into the sorted list, behind every entry whose score is <= v: the caller's units arrive in ascending id order
template <int KK>
__device__ __forceinline__ void topk_insert_stable(float (&sc)[KK], int (&id)[KK], float v, int u) {
#pragma unroll
    for (int j = KK - 1; j >= 1; --j) {
        const bool shift = v < sc[j - 1], here = v < sc[j];
        sc[j] = shift ? sc[j - 1] : (here ? v : sc[j]);
        id[j] = shift ? id[j - 1] : (here ? u : id[j]);
    }
    const bool first = v < sc[0];
    sc[0] = first ? v : sc[0];
    id[0] = first ? u : id[0];
}

// ... by (score, id): for entries that arrive in any order (the other lane half's list, the parts' lists)
template <int KK>
__device__ __forceinline__ void topk_insert_ordered(float (&sc)[KK], int (&id)[KK], float v, int u) {
#pragma unroll
    for (int j = KK - 1; j >= 1; --j) {
        const bool shift = topk_before(v, u, sc[j - 1], id[j - 1]), here = topk_before(v, u, sc[j], id[j]);
        sc[j] = shift ? sc[j - 1] : (here ? v : sc[j]);
        id[j] = shift ? id[j - 1] : (here ? u : id[j]);
    }
    const bool first = topk_before(v, u, sc[0], id[0]);
    sc[0] = first ? v : sc[0];
    id[0] = first ? u : id[0];
}

// one 32 x 32 tile's 16 scores of the lane's sample into its list.  TAIL: the tile may hold padding units (>= K: the codebook's
// last tile), which score +inf -- under a branch of the whole workgroup, so that the 16 masks exist in that tile alone
template <int MODE, int KK, bool TAIL>
__device__ __forceinline__ void topk_tile(const f32x16& acc, const float* __restrict__ wq32, float xsq, int unit0, int half, int K,
                                          float (&sc)[KK], int (&id)[KK]) {
    float v[16];
    // register r is unit ub + (r & 3) + 8 (r >> 2), a unit of the codebook where that offset is < lim.  Both are pinned HERE: left
    // to the compiler, the 64 ids and the 64 tail masks of a stage are formed at the top of the stage loop and spill.
    int h4 = 4 * half;
    asm volatile("" : "+v"(h4));
    const int ub = unit0 + h4, lim = K - ub;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 wv = *(const f32x4*)(wq32 + 8 * q + 4 * half);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * q + i;
            v[r] = score_f32<MODE>(acc[r], wv[i], xsq);
            if (TAIL && (r & 3) + 8 * (r >> 2) >= lim) v[r] = __builtin_inff();
        }
    }
    float m = __builtin_fminf(v[0], v[1]);
#pragma unroll
    for (int r = 2; r < 16; ++r) m = __builtin_fminf(m, v[r]);
    if (m < sc[KK - 1]) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (v[r] < sc[KK - 1]) topk_insert_stable<KK>(sc, id, v[r], ub + (r & 3) + 8 * (r >> 2));
    }
}

// grid: (row tiles, parts).  X: the pass's rows [N][D]; out_sc / out_id: [parts][N][KK]
template <int MODE, int KK>
__global__ __launch_bounds__(256, 2) void bmu_topk_f32_kernel(const float* __restrict__ X, long N, int D, int Dp,
                                                              const float* __restrict__ W, const float* __restrict__ wsq, int K,
                                                              const float* __restrict__ xsq, int stages, int per,
                                                              float* __restrict__ out_sc, int* __restrict__ out_id) {
    extern __shared__ __attribute__((aligned(16))) float topk_lds[];
    constexpr int LD = TOPK_LD;
    constexpr int BUF = (F32_UB + F32_SB) * LD;          // one chunk of both tiles: the units' rows, then the samples'
    float* wq = topk_lds + 2 * BUF;                      // [2][128] (16-byte aligned: 2 * 256 * 33 floats in front of it)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, col = lane & 31;
    const long s0 = (long)blockIdx.x * F32_SB;
    const long my_sample = s0 + wave * 32 + col;
    const int g0 = (int)blockIdx.y * per;                // the part's stages [g0, g1)
    const int g1 = g0 + per < stages ? g0 + per : stages;
    if (g0 >= g1) return;                                // (the whole workgroup, before any barrier; topk_plan leaves none such)
    float xs = 0.0f;
    if (MODE != SCORE_EUCLID_PART) xs = xsq[my_sample < N ? my_sample : N - 1];
    float sc[KK];
    int id[KK];
#pragma unroll
    for (int j = 0; j < KK; ++j) { sc[j] = __builtin_inff(); id[j] = -1; }
    // staging: thread t holds feature t & 31 of rows (t >> 5) + 8 i, i = 0 .. 15, of both tiles.  The part's chunks form ONE
    // sequence (stage by stage, 32 features at a time) and three cursors walk it: the chunk whose MFMAs run (LDS buffer b), the
    // chunk held in registers (written to buffer b ^ 1 in front of those MFMAs) and the chunk being loaded (density.hpp).
    constexpr int ST = F32_UB * F32_KC / 256;             // 16
    const int sk = tid & 31, sr = tid >> 5;
    float wreg[ST], xreg[ST], wqreg;
    auto next = [&](int& g, int& kc) { kc += F32_KC; if (kc >= Dp) { kc = 0; ++g; } };
    const int xlim = N - 1 - s0 < F32_SB - 1 ? (int)(N - 1 - s0) : F32_SB - 1;
    const float* xb = X + s0 * (long)D;
    auto fetch = [&](int g, int kc) {
        const int u0 = (g < g1 ? g : g1 - 1) * F32_UB;    // (past the part: the last stage again, loaded and never used)
        const unsigned fo = (unsigned)(kc + sk < D ? kc + sk : D - 1);
        const int wlim = K - 1 - u0 < F32_UB - 1 ? K - 1 - u0 : F32_UB - 1;
        const float* wb = W + (long)u0 * D;
        // the 32 row offsets are formed HERE, a min and a 24-bit multiply-add each (a row of the tile < 128; D < 2^24: the host's
        // topk_check refuses wider rows): left to the compiler they are loop invariants held in 32 registers across the MFMAs,
        // and the list spills
        unsigned wl = (unsigned)wlim, xl = (unsigned)xlim;
        asm volatile("" : "+v"(wl), "+v"(xl));
#pragma unroll
        for (int i = 0; i < ST; ++i) {
            const unsigned r = (unsigned)(sr + 8 * i);
            wreg[i] = wb[__umul24(r < wl ? r : wl, (unsigned)D) + fo];
            xreg[i] = xb[__umul24(r < xl ? r : xl, (unsigned)D) + fo];
        }
        const int qr = tid & (F32_UB - 1);
        wqreg = wsq[u0 + (qr < wlim ? qr : wlim)];
    };
    // registers -> LDS buffer `buf`; a padding feature is 0 on both sides; the stage's |w|^2 goes with its first chunk
    auto stage = [&](int buf, int g, int kc) {
        float* Wd = topk_lds + buf * BUF;
        float* Xd = Wd + F32_UB * LD;
        const bool kin = kc + sk < D;
#pragma unroll
        for (int i = 0; i < ST; ++i) {
            Wd[(sr + 8 * i) * LD + sk] = kin ? wreg[i] : 0.0f;
            Xd[(sr + 8 * i) * LD + sk] = kin ? xreg[i] : 0.0f;
        }
        if (kc == 0 && tid < F32_UB) wq[((g - g0) & 1) * F32_UB + tid] = wqreg;
    };
    int wg = g0, fg = g0, wkc = 0, fkc = 0, b = 0;        // the cursors of the chunk in registers and of the chunk to load
    fetch(fg, fkc); next(fg, fkc);
    stage(0, wg, wkc); next(wg, wkc);
    fetch(fg, fkc); next(fg, fkc);
    __syncthreads();
    for (int g = g0; g < g1; ++g) {
        f32x16 acc[4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[rb][r] = 0.0f;
        for (int kc = 0; kc < Dp; kc += F32_KC) {
            // the chunk after this one into the other buffer (last read before the barrier that ended the chunk before this one;
            // behind the part's last chunk: a chunk nobody reads), the one after that into the registers
            stage(b ^ 1, wg, wkc); next(wg, wkc);
            fetch(fg, fkc); next(fg, fkc);
            const float* wrow = topk_lds + b * BUF + col * LD + half;
            const float* xrow = topk_lds + b * BUF + (F32_UB + wave * 32 + col) * LD + half;
            // (two turns of eight steps: unrolled whole, the scheduler hoists a chunk's 80 fragment reads and the KK = 8 list spills)
#pragma unroll 8
            for (int k = 0; k < F32_KC; k += 2) {
                const float bx = xrow[k];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb)
                    acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wrow[rb * 32 * LD + k], bx, acc[rb], 0, 0, 0);
            }
            if (kc + F32_KC >= Dp) {
                const float* wqs = wq + ((g - g0) & 1) * F32_UB;
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) {
                    const int unit0 = g * F32_UB + rb * 32;
                    if (unit0 + 32 > K) topk_tile<MODE, KK, true>(acc[rb], wqs + rb * 32, xs, unit0, half, K, sc, id);
                    else topk_tile<MODE, KK, false>(acc[rb], wqs + rb * 32, xs, unit0, half, K, sc, id);
                }
            }
            __syncthreads();                             // the chunk just written is visible; the chunk just read may be overwritten
            b ^= 1;
        }
    }
    // the other lane half's list, entry by entry, by (score, id); both halves end with the same list, half 0 writes it
    float osc[KK];
    int oid[KK];
#pragma unroll
    for (int j = 0; j < KK; ++j) { osc[j] = __shfl_xor(sc[j], 32, 64); oid[j] = __shfl_xor(id[j], 32, 64); }
#pragma unroll
    for (int j = 0; j < KK; ++j) topk_insert_ordered<KK>(sc, id, osc[j], oid[j]);
    // (the lane's sample once more, from a thread id the compiler cannot tie to the first: nothing of it is held across the scan)
    int t2 = threadIdx.x;
    asm volatile("" : "+v"(t2));
    const long row = s0 + (t2 >> 6) * 32 + (t2 & 31);
    if ((t2 & 32) == 0 && row < N) {
        const size_t o = ((size_t)blockIdx.y * (size_t)N + (size_t)row) * KK;
#pragma unroll
        for (int j = 0; j < KK; ++j) { out_sc[o + j] = sc[j]; out_id[o + j] = id[j]; }
    }
}

// a thread per row: the parts' lists ([parts][N][KK]) joined by (score, id); the first k slots go out, row-major (N, k); an
// unfilled slot (id -1) takes a NaN score.  score may be nullptr.
template <int KK>
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ part_sc, const int* __restrict__ part_id, long N,
                                                         int parts, int k, int* __restrict__ ids, float* __restrict__ score) {
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    if (row >= N) return;
    float sc[KK];
    int id[KK];
#pragma unroll
    for (int j = 0; j < KK; ++j) { sc[j] = part_sc[(size_t)row * KK + j]; id[j] = part_id[(size_t)row * KK + j]; }
    for (int p = 1; p < parts; ++p) {
        const size_t o = ((size_t)p * (size_t)N + (size_t)row) * KK;
#pragma unroll
        for (int j = 0; j < KK; ++j) topk_insert_ordered<KK>(sc, id, part_sc[o + j], part_id[o + j]);
    }
#pragma unroll
    for (int j = 0; j < KK; ++j)
        if (j < k) {
            ids[(size_t)row * k + j] = id[j];
            if (score != nullptr) score[(size_t)row * k + j] = id[j] < 0 ? __builtin_nanf("") : sc[j];
        }
}

// dist[i] = sqrt(sum_d (x_nd - W[ids[i]][d])^2) for slot i = n * k + j: bmu_dist_kernel's lanes, fma chain, wave_sum and sqrtf; an
// unfilled slot gets NaN.  Persistent waves: grid = min(cdiv(slots, 4), 4096) workgroups of four.
__global__ __launch_bounds__(256) void topk_dist_kernel(const float* __restrict__ X, const int* __restrict__ ids,
                                                        const float* __restrict__ W, long slots, int k, int D,
                                                        float* __restrict__ dist) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long waves = (long)gridDim.x * 4;
    for (long i = (long)blockIdx.x * 4 + wave; i < slots; i += waves) {
        const int u = ids[i];
        if (u < 0) {                                     // (the whole wave: one slot per wave)
            if (lane == 0) dist[i] = __builtin_nanf("");
            continue;
        }
        const float* x = X + (i / k) * D;
        const float* w = W + (long)u * D;
        float s = 0.0f;
        for (int d = lane; d < D; d += 64) {
            float df = x[d] - w[d]; s = __builtin_fmaf(df, df, s);
        }
        s = wave_sum(s);
        if (lane == 0) dist[i] = __builtin_sqrtf(s);
    }
}

// counts[j][u] += 1 for every slot i = n * k + j that holds unit u >= 0: integer atomics only, so the same lists give the same
// counts under any launch geometry, and the counts of passes and calls add
__global__ __launch_bounds__(256) void unit_rank_counts_kernel(const int* __restrict__ ids, long slots, int k, int K,
                                                               unsigned long long* __restrict__ counts) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= slots) return;
    const int u = ids[i];
    if (u < 0 || u >= K) return;
    atomicAdd(counts + (size_t)(i % k) * K + u, 1ULL);
}

}  // namespace somhip
