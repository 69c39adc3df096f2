// Data density per unit (som_unit_density*, include/somhip.h): Ultsch's P-matrix, counted during the N x K x D scan.
//
// For float32 rows x_n, the codebook w_k, a pivot c and radii r_1 .. r_R (1 <= R <= 8):
//     P[j][k] = #{ n : sq(n, k) <= r2_j }        r2_j = float32(r_j * r_j), the product formed in double (the host's)
//     x' = fl32(x - c)    w' = fl32(w - c)
//     sq(n, k) = fl32( fmaf(-2, <x'_n, w'_k>, |w'_k|^2) + |x'_n|^2 )                  -- score_f32<SCORE_EUCLID_SQ>, bmu_f32.hpp
// The cross term is a k-ordered float32 fma chain on v_mfma_f32_32x32x2_f32; |w'|^2 and |x'|^2 are float32 sums of the D rounded
// squares in ONE fixed order (density_row below: lane l of a wave adds features l, l + 64, ... in ascending order, the 64 lane
// sums join in wave_sum's xor tree).  Always Euclidean, always float32, whatever the handle's distance and precision are.
// A row that holds a NaN or +-inf has sq = NaN or +inf against every unit and is counted nowhere (the comparison is false).
//
// Why a pivot: the GEMM form cancels on un-centred data (rows of spread 1e-3 around 30: the float32 error bound of sq exceeds every
// distance).  Distances are translation invariant and the subtraction costs one rounding per element; with c the midrange of the
// codebook the same rows are counted to within 0.23 % of sq.  The caller passes c; a zero pivot subtracts nothing.
//
//   density_center_units_kernel   W' = fl(W - c) and |w'|^2, one wave per unit            (K x D)
//   density_row_sq_kernel         |x'|^2 with x' formed on the fly, one wave per row      (N x D; no centred copy of the rows)
//   unit_density_f32_kernel<R>    the scan.  A workgroup owns ONE tile of 128 units and a slab of consecutive 128-row tiles
//                                 (density_plan): rows inside, units outside, so the counters live in registers over the whole slab.
//
// The scan's tiling is bmu_masked_f32_kernel's with the operands swapped: A operand = samples, B operand = units.  Wave v of the
// four owns units u0 + 32 v .. + 31 (a lane owns ONE unit, lane & 31) against all 128 rows of the tile: accumulator register r of
// block rb is row 32 rb + mfma32_row(r, lane >> 5).  Both operands go through LDS in chunks of 32 features (+1 padded rows:
// conflict-free fragment reads), two buffers, ONE barrier per chunk: in front of a chunk's MFMAs the chunk after it is written from
// registers to the other buffer and the chunk after that is loaded into the registers (loading inside the staging loop halved the
// masked kernel's rate).  x - c is formed at the write to LDS: there is no centred copy of the rows, and no wait on a fresh load.
// The unit tile's chunk is staged again for every row tile: it comes from L2, under a chunk's 64 MFMAs per wave.
//
// Counting: R per-lane int32 counters, pure VALU compares in the epilogue of every (row tile, unit tile); the lane halves join
// in one __shfl_xor at the end of the slab and ONE atomicAdd on unsigned long long counts[R][K] goes out per (unit, radius) with a
// non-zero count.  Integer atomics only: the same rows give the same counts whatever the grid.  (A lane counts at most half the
// rows of its slab, and a call holds at most 2^31 - 1 rows: no overflow.)
//
// Tails: every load is unconditional on an address clamped into its array.  Padding units (>= K) hold a copy of the last unit and
// are never written.  Padding rows (>= N) hold a copy of the last row -- it would be counted -- and are masked out through their
// |x'|^2, which is staged as NaN: the comparison is false, exactly as for a non-finite row.  Padding features are staged as zeros
// on both sides.  Any N >= 1, K >= 1, D >= 1; row offsets are 64-bit.
//
// Instances R = 1, 2, 4, 8 (a call of R radii runs the next one up, its spare radii NaN: never counted); float32 only -- no 16-bit
// instance.  Registers (hipcc -O3, gfx950; -Rpass-analysis=kernel-resource-usage), two waves per SIMD asked for: R = 1, 2, 4, 8:
// 173, 175, 181, 202 VGPRs (64 accumulator registers, 34 of the chunk in flight, a chunk's unrolled fragment reads), no AGPRs, no
// scratch, no spills; 68 608 bytes of LDS: two workgroups per CU, the barriers of one under the MFMAs of the other.
// Measured (profiles/density.md): x 1.43 the float32 search's time at one radius, x 1.62 at eight.
#pragma once
#include "bmu_f32.hpp"

namespace somhip {

constexpr int DEN_MAX_RADII = 8;
constexpr int DEN_LD = F32_KC + 1;
// bytes of dynamic LDS unit_density_f32_kernel needs: two buffers of the unit tile's and the row tile's chunk, two of a row tile's |x'|^2
constexpr size_t DEN_LDS_BYTES = (size_t)(2 * ((F32_UB + F32_SB) * DEN_LD + F32_SB)) * sizeof(float);

struct DensityRadii { float r2[DEN_MAX_RADII]; };

// Launch geometry: pure host arithmetic (som_debug_density_plan, include/somhip_test.h).  slots: workgroups of the scan the chip
// holds at once; forced > 0: the slab count asked for (SOM_DENSITY_SLABS), clamped the same way.  Small maps still fill the chip:
// the rows are cut into as many slabs as it takes to reach `slots` workgroups, never more than there are row tiles; a slab count
// that leaves whole slabs without a row tile is lowered to the slabs that have one.
struct DensityPlan { long unit_tiles, row_tiles, slabs, per; };
inline DensityPlan density_plan(long n_rows, int K, long slots, int forced) {
    DensityPlan p;
    p.unit_tiles = ((long)K + F32_UB - 1) / F32_UB;
    p.row_tiles = (n_rows + F32_SB - 1) / F32_SB;
    long s = forced > 0 ? (long)forced : (slots + p.unit_tiles - 1) / p.unit_tiles;
    s = s < 1 ? 1 : (s > p.row_tiles ? p.row_tiles : s);
    p.per = (p.row_tiles + s - 1) / s;
    p.slabs = (p.row_tiles + p.per - 1) / p.per;
    return p;
}

// lane's share of one row's centred squares, joined over the wave: sum_d fl(fl(a_d - c_d)^2); out (or nullptr) takes fl(a - c)
__device__ __forceinline__ float density_row(const float* __restrict__ a, const float* __restrict__ pivot, int D, int lane,
                                             float* __restrict__ out) {
    float s = 0.0f;
    for (int k = lane; k < D; k += 64) {
        const float d = __fsub_rn(a[k], pivot[k]);
        if (out != nullptr) out[k] = d;
        s = __fadd_rn(s, __fmul_rn(d, d));
    }
    return wave_sum(s);
}

__global__ __launch_bounds__(256) void density_center_units_kernel(const float* __restrict__ W, const float* __restrict__ pivot, int K,
                                                                   int D, float* __restrict__ Wc, float* __restrict__ wsq) {
    const int lane = threadIdx.x & 63;
    const long unit = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (unit >= K) return;                               // (a whole wave; the kernel has no barrier)
    const float q = density_row(W + unit * D, pivot, D, lane, Wc + unit * D);
    if (lane == 0) wsq[unit] = q;
}

__global__ __launch_bounds__(256) void density_row_sq_kernel(const float* __restrict__ X, const float* __restrict__ pivot, long N, int D,
                                                             float* __restrict__ xsq) {
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * 4;
    for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < N; row += waves) {
        const float q = density_row(X + row * D, pivot, D, lane, nullptr);
        if (lane == 0) xsq[row] = q;
    }
}

// grid: unit_tiles * slabs workgroups, the unit tile fastest (the workgroups of a slab read the same rows at about the same time)
template <int R>
__global__ __launch_bounds__(256, 2) void unit_density_f32_kernel(const float* __restrict__ X, long N, int D, int Dp,
                                                                  const float* __restrict__ pivot, const float* __restrict__ xsq,
                                                                  const float* __restrict__ Wc, const float* __restrict__ wsq, int K,
                                                                  int unit_tiles, long row_tiles, long per, DensityRadii rad,
                                                                  int n_radii, unsigned long long* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) float den_lds[];
    constexpr int LD = DEN_LD;
    constexpr int BUF = (F32_UB + F32_SB) * LD;          // one chunk of both tiles: the units' rows, then the samples'
    float* xq = den_lds + 2 * BUF;                       // [2][128] (16-byte aligned: 2 * 256 * 33 floats in front of it)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, col = lane & 31;
    const int u0 = (int)(blockIdx.x % (unsigned)unit_tiles) * F32_UB;
    const long t0 = (long)(blockIdx.x / (unsigned)unit_tiles) * per;
    const long t1 = t0 + per < row_tiles ? t0 + per : row_tiles;
    if (t0 >= t1) return;                                // (the whole workgroup, before any barrier; density_plan leaves none such)
    const int my_unit = u0 + wave * 32 + col;
    const float wq = my_unit < K ? wsq[my_unit] : 0.0f;
    int cnt[R];
#pragma unroll
    for (int j = 0; j < R; ++j) cnt[j] = 0;
    // staging: thread t holds feature t & 31 of rows (t >> 5) + 8 i, i = 0 .. 15, of both tiles (bmu_masked_f32_kernel's scheme).
    // The chunks of the slab form ONE sequence (tile by tile, 32 features at a time) and three cursors walk it: the chunk whose
    // MFMAs run (in LDS buffer b), the chunk held in registers (written to buffer b ^ 1 in front of those MFMAs) and the chunk
    // being loaded (issued behind that write: its latency lies under this chunk's MFMAs).  One barrier per chunk.
    constexpr int ST = F32_UB * F32_KC / 256;             // 16
    const int sk = tid & 31, sr = tid >> 5;
    float wreg[ST], xreg[ST], pvreg, xqreg;
    auto next = [&](long& t, int& kc) { kc += F32_KC; if (kc >= Dp) { kc = 0; ++t; } };
    // Every load is UNCONDITIONAL, on an address clamped into the arrays: a load under a per-lane condition becomes a branch
    // around it, 32 of them per chunk, and nothing else of the wave is scheduled across them.  What a clamped load brings in is
    // dropped at the write to LDS (padding features), or needs no dropping: a padding row's scores are NaN through its |x'|^2,
    // a padding unit's counters are never written, and a row or unit reaches no other row's or unit's scores.
    const float* wb = Wc + (long)u0 * D;
    const int wlim = K - 1 - u0 < F32_UB - 1 ? K - 1 - u0 : F32_UB - 1;
    auto fetch = [&](long t, int kc) {
        const long s0 = (t < t1 ? t : t1 - 1) * F32_SB;   // (past the slab: the last tile again, loaded and never used)
        const unsigned fo = (unsigned)(kc + sk < D ? kc + sk : D - 1);
        const int xlim = N - 1 - s0 < F32_SB - 1 ? (int)(N - 1 - s0) : F32_SB - 1;
        const float* xb = X + s0 * (long)D;
        pvreg = pivot[fo];
#pragma unroll
        for (int i = 0; i < ST; ++i) {
            const int r = sr + 8 * i;
            wreg[i] = wb[(unsigned)(r < wlim ? r : wlim) * (unsigned)D + fo];
            xreg[i] = xb[(unsigned)(r < xlim ? r : xlim) * (unsigned)D + fo];
        }
        const int qr = tid & (F32_SB - 1);
        xqreg = xsq[s0 + (qr < xlim ? qr : xlim)];
    };
    // registers -> LDS buffer `buf`; x - c is formed HERE, not at the load, so that nothing waits for a load it has just issued.
    // A padding feature is 0 on both sides; the tile's |x'|^2 goes with its first chunk, a padding row's as NaN: counted nowhere.
    auto stage = [&](int buf, long t, int kc) {
        float* Wd = den_lds + buf * BUF;
        float* Xd = Wd + F32_UB * LD;
        const bool kin = kc + sk < D;
#pragma unroll
        for (int i = 0; i < ST; ++i) {
            Wd[(sr + 8 * i) * LD + sk] = kin ? wreg[i] : 0.0f;
            Xd[(sr + 8 * i) * LD + sk] = kin ? __fsub_rn(xreg[i], pvreg) : 0.0f;
        }
        if (kc == 0 && tid < F32_SB) xq[(int)((t - t0) & 1) * F32_SB + tid] = t * F32_SB + tid < N ? xqreg : __builtin_nanf("");
    };
    long wt = t0, ft = t0;                               // the cursors of the chunk in registers and of the chunk to load
    int wkc = 0, fkc = 0, b = 0;
    fetch(ft, fkc); next(ft, fkc);
    stage(0, wt, wkc); next(wt, wkc);
    fetch(ft, fkc); next(ft, fkc);
    __syncthreads();
    for (long t = t0; t < t1; ++t) {
        f32x16 acc[4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[rb][r] = 0.0f;
        for (int kc = 0; kc < Dp; kc += F32_KC) {
            // the chunk after this one into the other buffer (last read before the barrier that ended the chunk before this one;
            // behind the slab's last chunk: a chunk nobody reads), the one after that into the registers
            stage(b ^ 1, wt, wkc); next(wt, wkc);
            fetch(ft, fkc); next(ft, fkc);
            const float* xrow = den_lds + b * BUF + (F32_UB + col) * LD + half;
            const float* wrow = den_lds + b * BUF + (wave * 32 + col) * LD + half;
#pragma unroll
            for (int k = 0; k < F32_KC; k += 2) {
                const float bu = wrow[k];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb)
                    acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(xrow[rb * 32 * LD + k], bu, acc[rb], 0, 0, 0);
            }
            if (kc + F32_KC >= Dp) {
                // the epilogue: register r of block rb is row 32 rb + mfma32_row(r, half) = 32 rb + 8 (r >> 2) + 4 half + (r & 3)
                const float* xqt = xq + (int)((t - t0) & 1) * F32_SB;
#pragma unroll
                for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x4 xs = *(const f32x4*)(xqt + rb * 32 + 8 * q + 4 * half);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float sq = score_f32<SCORE_EUCLID_SQ>(acc[rb][4 * q + i], wq, xs[i]);
#pragma unroll
                            for (int j = 0; j < R; ++j) cnt[j] += sq <= rad.r2[j] ? 1 : 0;
                        }
                    }
            }
            __syncthreads();                             // the chunk just written is visible; the chunk just read may be overwritten
            b ^= 1;
        }
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int total = cnt[j] + __shfl_xor(cnt[j], 32, 64);
        if (j < n_radii && half == 0 && my_unit < K && total > 0) atomicAdd(counts + (size_t)j * K + my_unit, (unsigned long long)total);
    }
}

}  // namespace somhip
