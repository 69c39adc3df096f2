// Row moments for the codebook initialisers (som_row_moments*, include/somhip.h): with d_n = x_n - p formed in float32,
//   wsum = sum_n w_n      s1[a] = sum_n w_n d_na      gram[a][b] = sum_n w_n d_na d_nb
//   moments_sums_kernel         wsum and s1: every product w_n * d_na is exact in double and is added in double.  One partial
//                               [D + 1] per workgroup; a workgroup owns a contiguous run of rows, its wave v the rows v, v + 4, ...
//                               of the run, lane l the features l, l + 64, ...
//   moments_sums_reduce_kernel  adds the workgroups' partials: sixteen strided runs in ascending order, joined in a fixed tree
//   moments_gram_kernel         the Gram matrix as a GEMM whose reduction runs over the rows, on v_mfma_f32_32x32x2_f32 with the
//                               operand mapping of bmu_f32.hpp: two rows per MFMA step, a 32-feature block per operand.  The A
//                               operand carries fl(w_n * d_na), the B operand d_nb, so one step adds w d_a d_b of two rows to a
//                               32 x 32 tile of (a, b).  The float32 chain of an accumulator covers ONE chunk of MOM_R rows (MOM_R / 2
//                               steps from zero); the chunk's result is widened and added to a double accumulator.  Only tiles with
//                               a-block <= b-block are computed.  A wave owns one tile over the chunks s, s + S, ... of its row split
//                               s; the four waves of a workgroup work on four tiles over the SAME rows, which they share through L1.
//   moments_gram_reduce_kernel  adds the splits' partials the same way and writes gram[a][b] and gram[b][a] from the one sum (of a
//                               diagonal tile only a <= b is taken: the mirror is the same bits by construction)
// A row of weight 0 is SELECTED out: both operands are 0 for it, whatever its features hold.  The kernels know no NaN handling.
// No floating-point atomics; every grid and every order of addition is a function of (n_rows, D) alone (moments_plan below), so
// the same rows give the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include "som_common.hpp"

namespace somhip {

constexpr int MOM_R = 256;                 // rows per float32 chain of the Gram kernel (SOM_MOMENTS_CHUNK_ROWS, include/somhip_test.h)
constexpr int MOM_MAX_D = 2048;            // SOM_MOMENTS_MAX_FEATURES (include/somhip.h)
constexpr int MOM_TILE = 32 * 32;          // accumulators of a tile
constexpr long MOM_SPLIT_WORKGROUPS = 1024;   // the Gram grid aims at this many workgroups: four per CU
constexpr long MOM_SUM_MAX_GRID = 2048;
constexpr int MOM_RED_WAVES = 16;           // waves of a reduction workgroup
constexpr long MOM_SUM_ROWS = 256;         // rows per workgroup of the sums kernel at least

// launch geometry: host and device agree on it, and it is a function of (n_rows, D) alone
__host__ __device__ inline long mom_blocks(int D) { return (D + 31) / 32; }
__host__ __device__ inline long mom_tiles(int D) { const long nb = mom_blocks(D); return nb * (nb + 1) / 2; }
__host__ __device__ inline long mom_tile_groups(int D) { return (mom_tiles(D) + 3) / 4; }
__host__ __device__ inline long mom_chunks(long N) { return (N + MOM_R - 1) / MOM_R; }
// row splits: one round of the split is mom_split_cap(D) chunks; never more splits than chunks
__host__ __device__ inline long mom_split_cap(int D) { const long tg = mom_tile_groups(D); return (MOM_SPLIT_WORKGROUPS + tg - 1) / tg; }
__host__ __device__ inline long mom_splits(long N, int D) {
    const long c = mom_chunks(N), cap = mom_split_cap(D);
    return c < 1 ? 1 : (c < cap ? c : cap);
}
__host__ __device__ inline long mom_sum_grid(long N) {
    const long g = (N + MOM_SUM_ROWS - 1) / MOM_SUM_ROWS;
    return g < 1 ? 1 : (g > MOM_SUM_MAX_GRID ? MOM_SUM_MAX_GRID : g);
}
// tile t of the upper triangle, row by row: (a-block, b-block), a-block <= b-block
__host__ __device__ inline void mom_tile_blocks(long t, int D, int* ab, int* bb) {
    const long nb = mom_blocks(D);
    long a = 0;
    while (t >= nb - a) { t -= nb - a; ++a; }
    *ab = (int)a; *bb = (int)(a + t);
}

template <bool WEIGHTED>
__global__ __launch_bounds__(256) void moments_sums_kernel(const float* __restrict__ X, const float* __restrict__ wgt,
                                                           const float* __restrict__ pivot, long N, int D,
                                                           double* __restrict__ part) {
    __shared__ double sh[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long per = (N + gridDim.x - 1) / gridDim.x;
    const long lo = (long)blockIdx.x * per;
    const long hi = lo + per < N ? lo + per : N;
    double* out = part + (long)blockIdx.x * (D + 1);
    for (int f0 = 0; f0 < D; f0 += 64) {
        const int f = f0 + lane;
        const bool v = f < D;
        const int fc = v ? f : 0;                        // (a lane beyond the row reads feature 0 and drops it)
        const float p = pivot[fc];
        double a = 0.0;
#pragma unroll 16
        for (long row = lo + wave; row < hi; row += 4) {      // (sixteen rows' loads in flight per wave: the pass is memory-bound)
            float w = 1.0f;
            if constexpr (WEIGHTED) w = wgt[row];
            const float x = X[row * D + fc];
            const float d = w != 0.0f ? x - p : 0.0f;    // a row of weight 0 is selected out, not multiplied by 0
            a += (double)w * (double)d;                  // (float x float: exact in double)
        }
        sh[wave][lane] = a;
        __syncthreads();
        if (wave == 0 && v) out[f] = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
        __syncthreads();
    }
    double ws = 0.0;
    for (long row = lo + wave; row < hi; row += 4) {
        if constexpr (WEIGHTED) ws += (double)wgt[row]; else ws += 1.0;
    }
    if (lane == 0) sh[wave][0] = ws;
    __syncthreads();
    if (threadIdx.x == 0) out[D] = (sh[0][0] + sh[1][0]) + (sh[2][0] + sh[3][0]);
}

// The reductions: a workgroup of MOM_RED_WAVES waves per 64 outputs.  Wave q adds the partials q, q + 16, ... of its lane's output in
// ascending order (independent loads, so many are in flight), and wave 0 joins the sixteen run sums in a fixed binary tree: one
// order for a given number of partials.
__device__ __forceinline__ double mom_join_runs(const double (*sh)[64], int lane) {
    double v[MOM_RED_WAVES];
#pragma unroll
    for (int q = 0; q < MOM_RED_WAVES; ++q) v[q] = sh[q][lane];
#pragma unroll
    for (int o = 1; o < MOM_RED_WAVES; o <<= 1)
#pragma unroll
        for (int q = 0; q < MOM_RED_WAVES; q += 2 * o) v[q] += v[q + o];
    return v[0];
}

// sums[f] = the workgroups' partials of feature f (f == D: wsum); grid ceil((D + 1) / 64)
__global__ __launch_bounds__(64 * MOM_RED_WAVES) void moments_sums_reduce_kernel(const double* __restrict__ part, int n_parts, int D,
                                                                                 double* __restrict__ sums) {
    __shared__ double sh[MOM_RED_WAVES][64];
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int f = blockIdx.x * 64 + lane;
    const bool v = f <= D;
    double a = 0.0;
    if (v) {
#pragma unroll 8
        for (int g = q; g < n_parts; g += MOM_RED_WAVES) a += part[(long)g * (D + 1) + f];
    }
    sh[q][lane] = a;
    __syncthreads();
    if (q == 0 && v) sums[f] = mom_join_runs(sh, lane);
}

// the MFMA steps of one chunk (rows r0 ... r0 + MOM_R) into acc; FULL: every row of the chunk exists
template <bool WEIGHTED, bool FULL>
__device__ __forceinline__ void moments_gram_chunk(const float* __restrict__ X, const float* __restrict__ wgt, long N, int D,
                                                   long r0, int half, int fa, int fb, bool va, bool vb, float pa, float pb,
                                                   f32x16& acc) {
#pragma unroll 8
    for (int k = 0; k < MOM_R; k += 2) {
        const long row = r0 + k + half;
        bool live = FULL || row < N;
        const long rc = live ? row : r0;                 // (r0 < N: a chunk has a first row)
        float w = 1.0f;
        if constexpr (WEIGHTED) { w = wgt[rc]; live = live && w != 0.0f; }
        const float xa = X[rc * D + fa], xb = X[rc * D + fb];
        const float a = live && va ? w * (xa - pa) : 0.0f;
        const float b = live && vb ? xb - pb : 0.0f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
}

// grid (tile groups, splits); part [split][tile][16 registers][64 lanes] doubles
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void moments_gram_kernel(const float* __restrict__ X, const float* __restrict__ wgt,
                                                           const float* __restrict__ pivot, long N, int D,
                                                           double* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, col = lane & 31;
    const long T = mom_tiles(D), S = gridDim.y;
    const long t = (long)blockIdx.x * 4 + wave;
    if (t >= T) return;                                  // (a whole wave; the kernel has no barrier)
    int ab, bb;
    mom_tile_blocks(t, D, &ab, &bb);
    const bool va = ab * 32 + col < D, vb = bb * 32 + col < D;
    const int fa = va ? ab * 32 + col : 0, fb = vb ? bb * 32 + col : 0;   // (a lane beyond the row reads feature 0 and drops it)
    const float pa = pivot[fa], pb = pivot[fb];
    double dacc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) dacc[r] = 0.0;
    const long chunks = mom_chunks(N);
    for (long c = blockIdx.y; c < chunks; c += S) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        const long r0 = c * MOM_R;
        if (r0 + MOM_R <= N) moments_gram_chunk<WEIGHTED, true>(X, wgt, N, D, r0, half, fa, fb, va, vb, pa, pb, acc);
        else moments_gram_chunk<WEIGHTED, false>(X, wgt, N, D, r0, half, fa, fb, va, vb, pa, pb, acc);
#pragma unroll
        for (int r = 0; r < 16; ++r) dacc[r] += (double)acc[r];
    }
    double* out = part + ((long)blockIdx.y * T + t) * MOM_TILE;
#pragma unroll
    for (int r = 0; r < 16; ++r) out[r * 64 + lane] = dacc[r];
}

// grid (tiles, 16 registers); element e = register * 64 + lane of the tile: row i = mfma32_row(register, lane >> 5) is the a feature,
// column lane & 31 the b feature
__global__ __launch_bounds__(64 * MOM_RED_WAVES) void moments_gram_reduce_kernel(const double* __restrict__ part, long S, int D,
                                                                                 double* __restrict__ gram) {
    __shared__ double sh[MOM_RED_WAVES][64];
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const long T = gridDim.x, t = blockIdx.x;
    int ab, bb;
    mom_tile_blocks(t, D, &ab, &bb);
    const int e = (int)blockIdx.y * 64 + lane;
    const int i = mfma32_row((int)blockIdx.y, lane >> 5), j = lane & 31;
    const long a = ab * 32 + i, b = bb * 32 + j;
    const bool valid = a < D && b < D && !(ab == bb && i > j);
    double v = 0.0;
    if (valid) {
#pragma unroll 8
        for (long s = q; s < S; s += MOM_RED_WAVES) v += part[(s * T + t) * MOM_TILE + e];
    }
    sh[q][lane] = v;
    __syncthreads();
    if (q == 0 && valid) {
        v = mom_join_runs(sh, lane);
        gram[a * D + b] = v;
        gram[b * D + a] = v;
    }
}

// rows idx[i] of a device block, dense: out[i][f] = X[idx[i]][f]
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ X, const long long* __restrict__ idx, long k,
                                                          int D, float* __restrict__ out) {
    const long total = k * D;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long i = e / D;
        out[e] = X[idx[i] * D + (e - i * D)];
    }
}

}  // namespace somhip
