// Training monitor: what one epoch did, measured from what the epoch itself left on the device (som_epoch_measure_rows /
// som_epoch_measure_shift / som_epoch_metrics, include/somhip.h).
//   monitor_rows_kernel     sum_n w_n d_n, sum_n w_n, the rows measured and the rows whose BMU differs from last epoch's, as one
//                           partial per workgroup.  d_n is bmu_dist_kernel's float32 (diag.hpp) bit for bit: lane l takes features
//                           l, l + 64, ... in one fma chain, wave_sum, sqrtf.  That lane assignment is part of the value, so the
//                           row is read once with one dword per lane -- every load instruction of a wave is one contiguous 256 bytes.
//                           The same launch moves this epoch's ids into `prev` (lane 0 of the row's wave reads, then writes, its entry).
//   monitor_shift_kernel    sum (W' - W)^2 and max |W' - W| over the K x D elements, W' = the float32 the merge is about to write
//                           (num / den where den != 0, else W), formed from the final accumulator: one partial per workgroup
//   monitor_*_reduce_kernel one workgroup adds the partials, runs of them in index order and the runs in a fixed tree, into the
//                           handle's metrics struct
// No floating-point atomics.  The grids are functions of N (rows) and K x D (shift) alone and every sum has a fixed tree, so the
// results are a function of the rows, the ids, the weights and the accumulator: two monitored runs return the same bits (the update
// path's reproducibility rule).
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/somhip.h"
#include "som_common.hpp"

namespace somhip {

struct MonitorRowPartial { double wd, w; long long rows, changed; };
struct MonitorShiftPartial { double sumsq; float mx; float pad; };

constexpr int MON_REDUCE_THREADS = 256;
constexpr int MON_ROWS_UNROLL = 4;
constexpr int MON_MAX_CHUNK = 16;          // partials per thread of a reduction at most: 4096 / 256

// launch geometry, host and device agree on it: workgroups of the row kernel (qe_kernel's rule) and of the shift kernel (four
// elements per thread at least), and the run of partials thread t of the reduction adds
__host__ __device__ inline long monitor_rows_grid(long N) { const long g = (N + 3) / 4; return g < 4096 ? g : 4096; }
__host__ __device__ inline long monitor_shift_grid(long elems) { const long g = (elems + 1023) / 1024; return g < 2048 ? g : 2048; }
__host__ __device__ inline int monitor_reduce_chunk(int n_parts) { return (n_parts + MON_REDUCE_THREADS - 1) / MON_REDUCE_THREADS; }

// the fma chains of one turn's rows (rows row0 + j waves, units b[j]): lane l adds features l, l + 64, ... of each, bmu_dist_kernel's
// chain.  ALL: every row of the turn is live, and the loads of all of them stand in one basic block.
template <bool MASKED, bool ALL>
__device__ __forceinline__ void monitor_row_chains(const float* __restrict__ X, const float* __restrict__ W, long row0, long waves,
                                                   const int (&b)[MON_ROWS_UNROLL], const bool (&live)[MON_ROWS_UNROLL], int lane,
                                                   int D, float (&s)[MON_ROWS_UNROLL]) {
    for (int k = lane; k < D; k += 64) {
#pragma unroll
        for (int j = 0; j < MON_ROWS_UNROLL; ++j) {
            if (!ALL && !live[j]) continue;
            const float xv = X[(row0 + j * waves) * D + k];
            const float wv = W[(long)b[j] * D + k];
            if constexpr (MASKED) {
                if (xv == xv) { const float df = xv - wv; s[j] = __builtin_fmaf(df, df, s[j]); }
            } else {
                const float df = xv - wv; s[j] = __builtin_fmaf(df, df, s[j]);
            }
        }
    }
}

// prev == nullptr (streamed chunks): no last epoch to compare with.  have_prev == 0: prev is only written.
template <bool MASKED, bool WEIGHTED>
__global__ __launch_bounds__(256) void monitor_rows_kernel(const float* __restrict__ X, const int* __restrict__ bmu,
                                                           const float* __restrict__ W, const float* __restrict__ wgt,
                                                           int* __restrict__ prev, int have_prev, long N, int D,
                                                           MonitorRowPartial* __restrict__ part) {
    __shared__ double s_wd[4], s_w[4];
    __shared__ long long s_rows[4], s_changed[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long waves = (long)gridDim.x * 4;
    double a_wd = 0.0, a_w = 0.0;
    long long a_rows = 0, a_changed = 0;                 // (a_changed: lane 0's only)
    // MON_ROWS_UNROLL of the wave's rows per turn -- rows r, r + waves, ... -- so that their loads are in flight together (one row's
    // two dependent loads, id then unit, leave the memory system idle); they are added in that same order, which is the order
    // of a wave that took them one by one
    for (long row0 = (long)blockIdx.x * 4 + wave; row0 < N; row0 += waves * MON_ROWS_UNROLL) {
        int b[MON_ROWS_UNROLL];
        float wt[MON_ROWS_UNROLL];
        bool live[MON_ROWS_UNROLL];
#pragma unroll
        for (int j = 0; j < MON_ROWS_UNROLL; ++j) {
            const long row = row0 + j * waves;
            live[j] = row < N;
            b[j] = 0;
            wt[j] = 1.0f;
            if (live[j]) {
                b[j] = bmu[row];
                if constexpr (WEIGHTED) wt[j] = wgt[row];
            }
        }
        if (prev != nullptr && lane == 0) {
#pragma unroll
            for (int j = 0; j < MON_ROWS_UNROLL; ++j) {
                const long row = row0 + j * waves;
                if (row < N) {
                    const int p = prev[row];
                    prev[row] = b[j];
                    a_changed += (have_prev != 0 && p != b[j]) ? 1 : 0;
                }
            }
        }
        float s[MON_ROWS_UNROLL];
#pragma unroll
        for (int j = 0; j < MON_ROWS_UNROLL; ++j) {
            if constexpr (WEIGHTED) live[j] = live[j] && wt[j] != 0.0f;   // a row of weight 0 is not read (the update's rule)
            s[j] = 0.0f;
        }
        // (all rows of the turn live -- every turn but a wave's last, and rows of weight 0 aside: no branch between the loads)
        bool all = true;
#pragma unroll
        for (int j = 0; j < MON_ROWS_UNROLL; ++j) all = all && live[j];
        if (all) monitor_row_chains<MASKED, true>(X, W, row0, waves, b, live, lane, D, s);
        else monitor_row_chains<MASKED, false>(X, W, row0, waves, b, live, lane, D, s);
#pragma unroll
        for (int j = 0; j < MON_ROWS_UNROLL; ++j) {
            if (!live[j]) continue;                      // (uniform over the wave: a row is the whole wave's)
            const double d = (double)__builtin_sqrtf(wave_sum(s[j]));
            if constexpr (WEIGHTED) { a_wd += (double)wt[j] * d; a_w += (double)wt[j]; }    // (float x float: exact in double)
            else { a_wd += d; a_w += 1.0; }
            ++a_rows;
        }
    }
    if (lane == 0) { s_wd[wave] = a_wd; s_w[wave] = a_w; s_rows[wave] = a_rows; s_changed[wave] = a_changed; }
    __syncthreads();
    if (threadIdx.x == 0) {
        MonitorRowPartial p;
        p.wd = (s_wd[0] + s_wd[1]) + (s_wd[2] + s_wd[3]);
        p.w = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
        p.rows = s_rows[0] + s_rows[1] + s_rows[2] + s_rows[3];
        p.changed = s_changed[0] + s_changed[1] + s_changed[2] + s_changed[3];
        part[blockIdx.x] = p;
    }
}

// One workgroup.  Thread t adds the partials [t c, (t + 1) c) in ascending order, c = monitor_reduce_chunk(n_parts); lane l of wave 0
// adds the run sums 4 l ... 4 l + 3 in ascending order and a fixed xor butterfly joins the 64 lanes: one tree for a given n_parts.  add != 0 (streamed chunks): onto what the struct holds -- chunk order is launch order.
// changed_known == 0: changed = -1.  n_parts == 0 writes the zeros of an empty row set.
__global__ __launch_bounds__(MON_REDUCE_THREADS) void monitor_rows_reduce_kernel(const MonitorRowPartial* __restrict__ part,
                                                                                 int n_parts, int add, int changed_known,
                                                                                 som_epoch_metrics_t* __restrict__ m) {
    __shared__ double s_wd[MON_REDUCE_THREADS], s_w[MON_REDUCE_THREADS];
    __shared__ long long s_rows[MON_REDUCE_THREADS], s_changed[MON_REDUCE_THREADS];
    const int t = threadIdx.x, c = monitor_reduce_chunk(n_parts);
    double wd = 0.0, w = 0.0;
    long long rows = 0, changed = 0;
    const int i1 = (t + 1) * c < n_parts ? (t + 1) * c : n_parts;
    MonitorRowPartial run[MON_MAX_CHUNK];                // (all of a run's loads first: sixteen dependent round trips otherwise)
#pragma unroll
    for (int j = 0; j < MON_MAX_CHUNK; ++j) {
        run[j] = MonitorRowPartial{0.0, 0.0, 0, 0};
        if (t * c + j < i1) run[j] = part[t * c + j];
    }
#pragma unroll
    for (int j = 0; j < MON_MAX_CHUNK; ++j)
        if (t * c + j < i1) { wd += run[j].wd; w += run[j].w; rows += run[j].rows; changed += run[j].changed; }
    s_wd[t] = wd; s_w[t] = w; s_rows[t] = rows; s_changed[t] = changed;
    __syncthreads();
    if (t >= 64) return;
    // wave 0: lane l adds the run sums 4 l ... 4 l + 3 in ascending order, the xor butterfly joins the lanes
    wd = ((s_wd[4 * t] + s_wd[4 * t + 1]) + s_wd[4 * t + 2]) + s_wd[4 * t + 3];
    w = ((s_w[4 * t] + s_w[4 * t + 1]) + s_w[4 * t + 2]) + s_w[4 * t + 3];
    rows = s_rows[4 * t] + s_rows[4 * t + 1] + s_rows[4 * t + 2] + s_rows[4 * t + 3];
    changed = s_changed[4 * t] + s_changed[4 * t + 1] + s_changed[4 * t + 2] + s_changed[4 * t + 3];
    wd = wave_sum_d(wd);
    w = wave_sum_d(w);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { rows += __shfl_xor(rows, o, 64); changed += __shfl_xor(changed, o, 64); }
    if (t != 0) return;
    if (add) { wd = m->sum_wd + wd; w = m->sum_w + w; rows += m->rows; }
    m->sum_wd = wd; m->sum_w = w; m->rows = rows;
    m->changed = changed_known ? changed : -1;
}

// W'[k][d] = den != 0 ? num / den : W[k][d] -- the merge kernels' expression, so the float32 they will write --, MASKED: with the
// feature's own denominator ACC[k][D + d].  The difference is squared and added in double (fma: one rounding per term); the
// maximum is float32's |W' - W|.  A NaN difference is ignored by the maximum (fmaxf) and poisons the sum.
template <bool MASKED>
__global__ __launch_bounds__(256) void monitor_shift_kernel(const float* __restrict__ ACC, const float* __restrict__ W, long K,
                                                            int D, int D1p, MonitorShiftPartial* __restrict__ part) {
    __shared__ double s_sq[4];
    __shared__ float s_mx[4];
    const long total = K * D, stride = (long)gridDim.x * 256;
    double sq = 0.0;
    float mx = 0.0f;
    // (k, d) of element i walk with it: two divisions per thread, none per element
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    long k = i / D;
    int d = (int)(i - k * D);
    const long sk = stride / D;
    const int sd = (int)(stride - sk * D);
    for (; i < total; i += stride, k += sk, d += sd) {
        if (d >= D) { d -= D; ++k; }
        const float old = W[i];
        const float den = ACC[k * D1p + D + (MASKED ? d : 0)];
        const float nw = den != 0.0f ? ACC[k * D1p + d] / den : old;
        const double df = (double)nw - (double)old;
        sq = __builtin_fma(df, df, sq);
        mx = __builtin_fmaxf(mx, __builtin_fabsf(nw - old));
    }
    sq = wave_sum_d(sq);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = __builtin_fmaxf(mx, __shfl_xor(mx, o, 64));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s_sq[wave] = sq; s_mx[wave] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        MonitorShiftPartial p;
        p.sumsq = (s_sq[0] + s_sq[1]) + (s_sq[2] + s_sq[3]);
        p.mx = __builtin_fmaxf(__builtin_fmaxf(s_mx[0], s_mx[1]), __builtin_fmaxf(s_mx[2], s_mx[3]));
        p.pad = 0.0f;
        part[blockIdx.x] = p;
    }
}

__global__ __launch_bounds__(MON_REDUCE_THREADS) void monitor_shift_reduce_kernel(const MonitorShiftPartial* __restrict__ part,
                                                                                  int n_parts, som_epoch_metrics_t* __restrict__ m) {
    __shared__ double s_sq[MON_REDUCE_THREADS];
    __shared__ float s_mx[MON_REDUCE_THREADS];
    const int t = threadIdx.x, c = monitor_reduce_chunk(n_parts);
    double sq = 0.0;
    float mx = 0.0f;
    const int i1 = (t + 1) * c < n_parts ? (t + 1) * c : n_parts;
    MonitorShiftPartial run[MON_MAX_CHUNK];
#pragma unroll
    for (int j = 0; j < MON_MAX_CHUNK; ++j) {
        run[j] = MonitorShiftPartial{0.0, 0.0f, 0.0f};
        if (t * c + j < i1) run[j] = part[t * c + j];
    }
#pragma unroll
    for (int j = 0; j < MON_MAX_CHUNK; ++j)
        if (t * c + j < i1) { sq += run[j].sumsq; mx = __builtin_fmaxf(mx, run[j].mx); }
    s_sq[t] = sq; s_mx[t] = mx;
    __syncthreads();
    if (t >= 64) return;
    sq = ((s_sq[4 * t] + s_sq[4 * t + 1]) + s_sq[4 * t + 2]) + s_sq[4 * t + 3];
    mx = __builtin_fmaxf(__builtin_fmaxf(s_mx[4 * t], s_mx[4 * t + 1]), __builtin_fmaxf(s_mx[4 * t + 2], s_mx[4 * t + 3]));
    sq = wave_sum_d(sq);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = __builtin_fmaxf(mx, __shfl_xor(mx, o, 64));
    if (t != 0) return;
    m->shift_sumsq = sq;
    m->shift_max = mx;
}

}  // namespace somhip
