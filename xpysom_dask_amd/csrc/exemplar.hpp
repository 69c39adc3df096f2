// The k nearest rows of every unit (som_unit_nearest_rows*; include/somhip.h holds the definition): the float32 MFMA scan of topk.hpp
// reduced the other way round -- a list per UNIT over the rows -- the (n, K) score matrix never written.
//
//   unit_nearest_rows_f32_kernel<MODE, KK>   the scan, KK = 4 or 8 list slots (a call of k runs the next instance up; the spare slots
//                                            are kept: the k best of the KK best are the k best).  grid = unit tiles x row parts
//   exemplar_merge_kernel<KK>                a thread per unit: the KK lowest (score, id) over the parts' lists and the running list
//                                            of the passes before; the distances of the entries that stay are carried along
//   exemplar_dist_kernel                     a wave per (unit, slot): sqrt(sum_d (x_d - W[u][d])^2) in bmu_dist_kernel's arithmetic
//                                            (diag.hpp) for the slots that hold a row of this pass
//
// The scan's mapping is bmu_f32_kernel's with the roles swapped: A operand = samples, B operand = units.  A workgroup = 4 waves x 32
// units; a lane owns ONE unit (lane & 31 of its wave's block) and accumulator register r of row block rb is row
// stage * 128 + 32 rb + mfma32_row(r, lane >> 5), ascending in r.  The MFMA's products commute, so a score is bit for bit the entry
// dist_matrix_f32_kernel<MODE> writes.  The lane's list -- KK scores and KK row ids, sorted -- lives in registers.  A workgroup sweeps
// its row part in stages of 128 rows (4 row blocks x 16 registers = 64 accumulators).  Both operands go through LDS in chunks of
// F32_KC features (+1 padded rows: conflict-free fragment reads), two buffers, ONE barrier per chunk, density.hpp's scheme: in front
// of a chunk's MFMAs the chunk after it is written from registers to the other buffer and the chunk after that is loaded into the
// registers.  The unit tile's chunk is staged again for every row stage: it comes from L2, under a chunk's 64 MFMAs per wave.
//
// Epilogue, per 32 x 32 tile: the 16 scores are formed (|x|^2 of the stage's rows from LDS, |w|^2 of the lane's unit in a register)
// and reduced with fminf; only a lane whose tile minimum is `<` its k-th score walks the 16 registers, and each score that is `<`
// the k-th is inserted by an unrolled compare-and-shift (topk_insert_stable: no dynamic indexing, no scratch).  A lane meets its
// rows in ascending id order and inserts BEHIND every score that is <= the new one, so within a lane the list is the stable order.
// Padding rows (>= N) are set to +inf and never compete; NaN and +inf never pass `<`.  The two lane halves hold disjoint rows of the
// same unit: at the end each takes the other's list through __shfl_xor(.., 32) and inserts it by (score, id).  Padding units
// (>= K: a copy of the last unit) are never written.
//
// Row parts, so that a small map still fills the chip: part p sweeps the stages [p * per, (p + 1) * per) and writes its list to
// scratch ([part][K][KK] scores and ids); exemplar_merge_kernel joins them by the total order (score, id).  No atomics: the result
// is identical for every part count.  The count is pure host arithmetic (exemplar_plan).  The grid is (unit tiles, parts) with the
// unit tiles fastest: the workgroups resident together walk the same row part, whose rows then come from L2 as the codebook does in
// the BMU search.
//
// Tails: every load is unconditional on an address clamped into its array (density.hpp).  Padding features are staged as zeros on
// both sides.  Any D >= 1 (< 2^24: a 24-bit multiply forms the staging offsets), K >= 1, 1 <= N <= 2^31-1; a stage's first row
// offset is 64-bit.
//
// Registers (hipcc -O3, gfx950; -Rpass-analysis=kernel-resource-usage), two waves per SIMD asked for; VGPRs of <MODE, KK>:
//     sq, 4: 214    sq, 8: 256    cosine, 4: 201    cosine, 8: 246
// no AGPRs, no scratch, no SGPR or VGPR spills in any of the four (64 accumulator registers, 32 of the chunk in flight, the list's
// 2 KK, a tile's 16 scores); <sq, 8> takes every register two waves per SIMD leave.  That took topk.hpp's pins (asm volatile("" :
// "+v"(..))) on the tile's first row and the staging's row limits, one more behind a tile's inserts (the four tiles of a stage run
// one after the other), and the final write's unit rebuilt from the lane's number (mbcnt) and the wave's (a scalar): the thread id
// arrives in v0 and nowhere else, and held across the scan it was the one register <sq, 8> spilled.  LDS: 68 608 bytes (two
// buffers of both tiles' chunk, two of a stage's |x|^2): two workgroups per CU.  exemplar_merge_kernel 36 / 55 VGPRs,
// exemplar_dist_kernel 23, none with scratch.
#pragma once
#include "bmu_f32.hpp"
#include "topk.hpp"

namespace somhip {

constexpr int EX_LD = F32_KC + 1;
// bytes of dynamic LDS unit_nearest_rows_f32_kernel needs: two buffers of the row stage's and the unit tile's chunk, two of a stage's |x|^2
constexpr size_t EX_LDS_BYTES = (size_t)(2 * ((F32_SB + F32_UB) * EX_LD + F32_SB)) * sizeof(float);
// Host rows per pass of a call: the staged rows are bounded whatever n_rows is; device rows are swept where they are, in one pass.
constexpr long EX_PASS_ROWS = 1048576;
constexpr long EX_MAX_PARTS = 65535;                     // (the grid's second dimension)

// Launch geometry: pure host arithmetic (som_debug_exemplar_plan, include/somhip_test.h).  slots: workgroups of the scan the chip
// holds at once; forced > 0: the part count asked for (SOM_EXEMPLAR_PARTS), clamped the same way.  The rows' 128-row stages are cut
// into as many parts as it takes to reach `slots` workgroups, never more than there are stages (or than a grid dimension holds); a
// count that would leave parts without a stage is lowered to the parts that have one.
struct ExemplarPlan { long unit_tiles, stages, parts, per; };
inline ExemplarPlan exemplar_plan(long n_rows, int K, long slots, int forced) {
    ExemplarPlan p;
    p.unit_tiles = ((long)K + F32_UB - 1) / F32_UB;
    p.stages = (n_rows + F32_SB - 1) / F32_SB;
    long s = forced > 0 ? (long)forced : (slots + p.unit_tiles - 1) / p.unit_tiles;
    s = s > EX_MAX_PARTS ? EX_MAX_PARTS : s;
    s = s < 1 ? 1 : (s > p.stages ? p.stages : s);
    p.per = (p.stages + s - 1) / s;
    p.parts = (p.stages + p.per - 1) / p.per;
    return p;
}

// one 32 x 32 tile's 16 scores of the lane's unit into its list.  xq32: |x|^2 of the tile's 32 rows (LDS); row0: the id of the tile's
// first row; TAIL: the tile may hold padding rows (local row >= lim), which score +inf -- under a branch of the whole workgroup
template <int MODE, int KK, bool TAIL>
__device__ __forceinline__ void exemplar_tile(const f32x16& acc, const float* __restrict__ xq32, float wsq, int row0, int lim,
                                              int half, float (&sc)[KK], int (&id)[KK]) {
    float v[16];
    // register r is row rb + (r & 3) + 8 (r >> 2).  The half's offset is pinned HERE (topk.hpp): left to the compiler, the 64 ids
    // and the 64 tail masks of a stage are formed at the top of the stage loop and spill.
    int h4 = 4 * half;
    asm volatile("" : "+v"(h4));
    const int rb = row0 + h4, lm = lim - h4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 xv = *(const f32x4*)(xq32 + 8 * q + h4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * q + i;
            v[r] = score_f32<MODE>(acc[r], wsq, xv[i]);
            if (TAIL && (r & 3) + 8 * (r >> 2) >= lm) v[r] = __builtin_inff();
        }
    }
    float m = __builtin_fminf(v[0], v[1]);
#pragma unroll
    for (int r = 2; r < 16; ++r) m = __builtin_fminf(m, v[r]);
    if (m < sc[KK - 1]) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (v[r] < sc[KK - 1]) topk_insert_stable<KK>(sc, id, v[r], rb + (r & 3) + 8 * (r >> 2));
    }
    asm volatile("" : "+v"(sc[KK - 1]));
}

// grid: (unit tiles, parts).  X: the pass's rows [N][D], row n listed as id0 + n; out_sc / out_id: [parts][K][KK]
template <int MODE, int KK>
__global__ __launch_bounds__(256, 2) void unit_nearest_rows_f32_kernel(const float* __restrict__ X, long N, int D, int Dp,
                                                                       const float* __restrict__ W, const float* __restrict__ wsq,
                                                                       int K, const float* __restrict__ xsq, int id0, int stages,
                                                                       int per, float* __restrict__ out_sc, int* __restrict__ out_id) {
    static_assert(MODE == SCORE_EUCLID_SQ || MODE == SCORE_COSINE, "ranking rows for one unit needs |x|^2: never the PART form");
    extern __shared__ __attribute__((aligned(16))) float ex_lds[];
    constexpr int LD = EX_LD;
    constexpr int BUF = (F32_SB + F32_UB) * LD;          // one chunk of both tiles: the rows', then the units'
    float* xq = ex_lds + 2 * BUF;                        // [2][128] (16-byte aligned: 2 * 256 * 33 floats in front of it)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, col = lane & 31;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    const int u0 = (int)blockIdx.x * F32_UB;
    const int g0 = (int)blockIdx.y * per;                // the part's stages [g0, g1)
    const int g1 = g0 + per < stages ? g0 + per : stages;
    if (g0 >= g1) return;                                // (the whole workgroup, before any barrier; exemplar_plan leaves none such)
    const int my_unit = u0 + wave * 32 + col;
    const float ws = wsq[my_unit < K ? my_unit : K - 1];
    float sc[KK];
    int id[KK];
#pragma unroll
    for (int j = 0; j < KK; ++j) { sc[j] = __builtin_inff(); id[j] = -1; }
    // staging: thread t holds feature t & 31 of rows (t >> 5) + 8 i, i = 0 .. 15, of both tiles.  The part's chunks form ONE sequence
    // (stage by stage, 32 features at a time) and three cursors walk it: the chunk whose MFMAs run (LDS buffer b), the chunk held in
    // registers (written to buffer b ^ 1 in front of those MFMAs) and the chunk being loaded (topk.hpp).
    constexpr int ST = F32_SB * F32_KC / 256;             // 16
    const int sk = tid & 31, sr = tid >> 5;
    float xreg[ST], wreg[ST], xqreg;
    auto next = [&](int& g, int& kc) { kc += F32_KC; if (kc >= Dp) { kc = 0; ++g; } };
    const int wlim = K - 1 - u0 < F32_UB - 1 ? K - 1 - u0 : F32_UB - 1;
    const float* wb = W + (long)u0 * D;
    auto fetch = [&](int g, int kc) {
        const long r0 = (long)(g < g1 ? g : g1 - 1) * F32_SB;   // (past the part: the last stage again, loaded and never used)
        const unsigned fo = (unsigned)(kc + sk < D ? kc + sk : D - 1);
        const int xlim = N - 1 - r0 < F32_SB - 1 ? (int)(N - 1 - r0) : F32_SB - 1;
        const float* xb = X + r0 * (long)D;
        // the 32 row offsets are formed HERE, a min and a 24-bit multiply-add each (a row of the tile < 128; D < 2^24, the host
        // refuses wider rows): left to the compiler they are held in 32 registers across the MFMAs, and the list spills (topk.hpp)
        unsigned xl = (unsigned)xlim, wl = (unsigned)wlim;
        asm volatile("" : "+v"(xl), "+v"(wl));
#pragma unroll
        for (int i = 0; i < ST; ++i) {
            const unsigned r = (unsigned)(sr + 8 * i);
            xreg[i] = xb[__umul24(r < xl ? r : xl, (unsigned)D) + fo];
            wreg[i] = wb[__umul24(r < wl ? r : wl, (unsigned)D) + fo];
        }
        const int qr = tid & (F32_SB - 1);
        xqreg = xsq[r0 + (qr < xlim ? qr : xlim)];
    };
    // registers -> LDS buffer `buf`; a padding feature is 0 on both sides; the stage's |x|^2 goes with its first chunk
    auto stage = [&](int buf, int g, int kc) {
        float* Xd = ex_lds + buf * BUF;
        float* Wd = Xd + F32_SB * LD;
        const bool kin = kc + sk < D;
#pragma unroll
        for (int i = 0; i < ST; ++i) {
            Xd[(sr + 8 * i) * LD + sk] = kin ? xreg[i] : 0.0f;
            Wd[(sr + 8 * i) * LD + sk] = kin ? wreg[i] : 0.0f;
        }
        if (kc == 0 && tid < F32_SB) xq[((g - g0) & 1) * F32_SB + tid] = xqreg;
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
            const float* xrow = ex_lds + b * BUF + col * LD + half;
            const float* wrow = ex_lds + b * BUF + (F32_SB + wave * 32 + col) * LD + half;
            // (two turns of eight steps: unrolled whole, the scheduler hoists a chunk's 80 fragment reads and the KK = 8 list spills)
#pragma unroll 8
            for (int k = 0; k < F32_KC; k += 2) {
                const float bw = wrow[k];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb)
                    acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(xrow[rb * 32 * LD + k], bw, acc[rb], 0, 0, 0);
            }
            if (kc + F32_KC >= Dp) {
                const float* xqs = xq + ((g - g0) & 1) * F32_SB;
                const long behind = N - (long)g * F32_SB;                   // rows of the stage and behind it: >= 1
                const int left = behind < F32_SB ? (int)behind : F32_SB;
                const int row0 = (int)((unsigned)id0 + (unsigned)g * (unsigned)F32_SB);
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) {
                    if (left < 32 * rb + 32)
                        exemplar_tile<MODE, KK, true>(acc[rb], xqs + rb * 32, ws, row0 + 32 * rb, left - 32 * rb, half, sc, id);
                    else exemplar_tile<MODE, KK, false>(acc[rb], xqs + rb * 32, ws, row0 + 32 * rb, 32, half, sc, id);
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
    // (the lane's unit once more, from the lane's number and the wave's, a scalar: the thread id itself is not held across the scan)
    const int l2 = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int unit = (int)blockIdx.x * F32_UB + wave_s * 32 + (l2 & 31);
    if ((l2 & 32) == 0 && unit < K) {
        const size_t o = ((size_t)blockIdx.y * (size_t)K + (size_t)unit) * KK;
#pragma unroll
        for (int j = 0; j < KK; ++j) { out_sc[o + j] = sc[j]; out_id[o + j] = id[j]; }
    }
}

// a thread per unit: the running list of the passes before (run_*: [K][KK], read where have_run) and this pass's parts' lists
// ([parts][K][KK]) joined by (score, id) into the running list.  run_dist travels with its entry: a slot keeps the distance the
// same row id had before, a slot with a row of this pass gets NaN until exemplar_dist_kernel fills it.
template <int KK>
__global__ __launch_bounds__(256) void exemplar_merge_kernel(const float* __restrict__ part_sc, const int* __restrict__ part_id, int K,
                                                             int parts, int have_run, float* __restrict__ run_sc,
                                                             int* __restrict__ run_id, float* __restrict__ run_dist) {
    const int u = (int)blockIdx.x * 256 + threadIdx.x;
    if (u >= K) return;
    const size_t ro = (size_t)u * KK;
    float sc[KK], od[KK];
    int id[KK], old[KK];
#pragma unroll
    for (int j = 0; j < KK; ++j) {
        sc[j] = have_run ? run_sc[ro + j] : __builtin_inff();
        id[j] = old[j] = have_run ? run_id[ro + j] : -1;
        od[j] = have_run ? run_dist[ro + j] : __builtin_nanf("");
    }
    for (int p = 0; p < parts; ++p) {
        const size_t o = ((size_t)p * (size_t)K + (size_t)u) * KK;
#pragma unroll
        for (int j = 0; j < KK; ++j) topk_insert_ordered<KK>(sc, id, part_sc[o + j], part_id[o + j]);
    }
#pragma unroll
    for (int j = 0; j < KK; ++j) {
        float d = __builtin_nanf("");
#pragma unroll
        for (int i = 0; i < KK; ++i) d = (id[j] >= 0 && old[i] == id[j]) ? od[i] : d;
        run_sc[ro + j] = sc[j];                          // (an empty slot: +inf, id -1 -- what the next pass's merge starts from)
        run_id[ro + j] = id[j];
        run_dist[ro + j] = d;
    }
}

// run_dist[u][j] = sqrt(sum_d (x_d - W[u][d])^2) for j < k where the slot holds a row of this pass, id0 <= id < id0 + N:
// bmu_dist_kernel's lanes, fma chain, wave_sum and sqrtf.  Always Euclidean, and not what orders the list.  Persistent waves:
// grid = min(cdiv(K * k, 4), 4096) workgroups of four.
template <int KK>
__global__ __launch_bounds__(256) void exemplar_dist_kernel(const float* __restrict__ X, long N, int id0, const int* __restrict__ run_id,
                                                            const float* __restrict__ W, int K, int k, int D,
                                                            float* __restrict__ run_dist) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long waves = (long)gridDim.x * 4, slots = (long)K * k;
    for (long i = (long)blockIdx.x * 4 + wave; i < slots; i += waves) {
        const int u = (int)(i / k), j = (int)(i % k);
        const long n = (long)run_id[(size_t)u * KK + j] - id0;
        if (n < 0 || n >= N) continue;                   // (the whole wave: one slot per wave.  Empty, or a row of an earlier pass)
        const float* x = X + n * D;
        const float* w = W + (long)u * D;
        float s = 0.0f;
        for (int d = lane; d < D; d += 64) {
            float df = x[d] - w[d]; s = __builtin_fmaf(df, df, s);
        }
        s = wave_sum(s);
        if (lane == 0) run_dist[(size_t)u * KK + j] = __builtin_sqrtf(s);
    }
}

}  // namespace somhip
