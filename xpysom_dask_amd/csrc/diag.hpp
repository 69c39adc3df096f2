// Map diagnostics on the device: every row's distance to its BMU (som_bmu_distances*) and, per unit, how many rows it won and the
// sum, the sum of squares and the maximum of their distances (som_unit_stats*).
//   bmu_dist_kernel    qe_kernel (update.hpp) / qe_masked_kernel (bmu_masked_f32.hpp) with the per-row value KEPT: dist[row] is the
//                      float32 those kernels widen and add, bit for bit -- the same lanes, the same fma chain, wave_sum, sqrtf
//   unit_heads_kernel  where every unit's segment of the rows sorted by unit begins (update.hpp's stable sort: by unit, rows
//                      ascending inside a unit), read off the sorted keys
//   unit_stats_kernel  a wave per unit over its segment
// No atomics at all: lane l of a unit's wave adds the segment's entries l, l + 64, ... in ascending row order and a fixed
// xor butterfly joins the lanes, so the sums are a function of the ids and the distances alone -- two calls, or the host and the
// device entry point on the same rows, return the same bits (the update path's rule, extended to this query).
#pragma once

#include <hip/hip_runtime.h>

#include "som_common.hpp"

namespace somhip {

// dist[n] = sqrt(sum_d (x_nd - W[bmu_n][d])^2); MASKED (missing values): over the observed (non-NaN) features only, a row with
// nothing observed gets 0.  Persistent waves as qe_kernel's: grid = min(cdiv(N, 4), 4096) workgroups of four waves.
template <bool MASKED>
__global__ __launch_bounds__(256) void bmu_dist_kernel(const float* __restrict__ X, const int* __restrict__ bmu,
                                                       const float* __restrict__ W, long N, int D, float* __restrict__ dist) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long waves = (long)gridDim.x * 4;
    for (long row = (long)blockIdx.x * 4 + wave; row < N; row += waves) {
        const float* x = X + row * D;
        const float* w = W + (long)bmu[row] * D;
        float s = 0.0f;
        for (int k = lane; k < D; k += 64) {
            const float xv = x[k];
            if constexpr (MASKED) {
                if (xv == xv) { const float df = xv - w[k]; s = __builtin_fmaf(df, df, s); }
            } else {
                float df = xv - w[k]; s = __builtin_fmaf(df, df, s);
            }
        }
        s = wave_sum(s);
        if (lane == 0) dist[row] = __builtin_sqrtf(s);
    }
}

// start[k] = the first sorted position of unit k, for every unit that has rows (start preset to -1 by the caller): position i
// heads a segment where its key differs from the one before it.  The sort's own output says where the segments are -- no
// histogram, no scan, no atomic.
__global__ __launch_bounds__(256) void unit_heads_kernel(const int* __restrict__ skey, long N, int K, int* __restrict__ start) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int k = skey[i];
    if ((i == 0 || skey[i - 1] != k) && (unsigned)k < (unsigned)K) start[k] = (int)i;
}

// unit k's rows are order[start[k] ...] for as long as the sorted key stays k: their number, the sum and the sum of squares of
// their distances in double (a float32 squared is exact in double), their maximum (fmaxf: a NaN distance is ignored by the
// maximum and poisons the sums).  A unit without rows (start[k] < 0) writes zeros; a segment of any length walks the same loop.
__global__ __launch_bounds__(256) void unit_stats_kernel(const int* __restrict__ start, const int* __restrict__ skey,
                                                         const int* __restrict__ order, const float* __restrict__ dist, long N,
                                                         int K, long long* __restrict__ count, double* __restrict__ sum,
                                                         double* __restrict__ sumsq, float* __restrict__ mx) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;
    const int s0 = start[k];
    double s = 0.0, q = 0.0;
    float m = 0.0f;
    int c = 0;
    if (s0 >= 0)
        for (long i = (long)s0 + lane; i < N && skey[i] == k; i += 64) {
            const float d = dist[order[i]];
            const double dd = (double)d;
            s += dd;
            q += dd * dd;
            m = __builtin_fmaxf(m, d);
            ++c;
        }
    s = wave_sum_d(s);
    q = wave_sum_d(q);
    long long n = c;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m = __builtin_fmaxf(m, __shfl_xor(m, o, 64));
        n += __shfl_xor(n, o, 64);
    }
    if (lane == 0) { count[k] = n; sum[k] = s; sumsq[k] = q; mx[k] = m; }
}

}  // namespace somhip
