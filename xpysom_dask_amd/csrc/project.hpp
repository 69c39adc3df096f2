// Label and value maps on the device: what the rows a unit wins SAY -- how many carry each class label (som_unit_label_counts*)
// and, per column of numbers the map was not trained on, how many values the unit saw, their sum and the sum of their squares
// (som_unit_value_sums*).  Both run behind the ACTIVATION BMU search of the query row set (the ids som_bmu / predict / labels_map
// use), update.hpp's stable sort by unit and diag.hpp's unit_heads_kernel: unit k's rows are order[start[k] ...] for as long as
// the sorted key stays k, rows ascending inside a unit.
//   unit_label_counts_kernel   a wave per unit, a column block of 64 classes at a time: the wave's own 64 integers of LDS, every
//                              lane adds 1 at its row's label (integer LDS atomics), lane l writes class c0 + l.  A sum of integers:
//                              order-free, so the atomics' order changes nothing.  No global atomics, no floating point.
//   unit_value_sums_kernel     a wave per unit, a column block of 64 columns at a time; the 64 lanes are R row slots x Cp column
//                              slots (Cp = the next power of two >= the block's columns, R = 64 / Cp; lane = r * Cp + col).  Row
//                              slot r adds the segment's entries r, r + R, ... in ascending sorted position, then a fixed xor
//                              butterfly (offsets 32 ... Cp) joins the row slots.  No atomics: the order of the additions is a
//                              function of the segment's length and the column count alone, so two calls -- or the host and the
//                              device entry point -- on the same rows return the same bits.  One column: 64 row slots, a segment
//                              of n rows costs n / 64 steps (unit_stats_kernel's walk).
// A unit without rows (start[k] < 0) writes zeros; a segment of any length walks the same loop.
#pragma once

#include <hip/hip_runtime.h>

#include "som_common.hpp"

namespace somhip {

constexpr int PROJ_CB = 64;        // classes / columns per block: one per lane

// counts[k][c] = #{rows n of unit k : labels[n] == c}, 0 <= c < C; a label outside [0, C) -- "unlabelled" -- is counted nowhere.
// Four waves a workgroup, a unit each; every workgroup walks all column blocks, so the barriers are uniform (a wave whose unit
// is past the map, or has no rows, walks nothing and still meets them).
__global__ __launch_bounds__(256) void unit_label_counts_kernel(const int* __restrict__ start, const int* __restrict__ skey,
                                                                const int* __restrict__ order, const int* __restrict__ labels,
                                                                long N, int K, int C, long long* __restrict__ counts) {
    __shared__ unsigned hist[4][PROJ_CB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = blockIdx.x * 4 + wave;
    const int s0 = k < K ? start[k] : -1;
    for (int c0 = 0; c0 < C; c0 += PROJ_CB) {
        hist[wave][lane] = 0u;
        __syncthreads();
        if (s0 >= 0)
            for (long i = (long)s0 + lane; i < N && skey[i] == k; i += 64) {
                const unsigned c = (unsigned)labels[order[i]] - (unsigned)c0;      // (a negative label wraps beyond every block)
                if (c < (unsigned)PROJ_CB) atomicAdd(&hist[wave][c], 1u);
            }
        __syncthreads();
        if (k < K && c0 + lane < C) counts[(long)k * C + c0 + lane] = (long long)hist[wave][lane];
        // (lane l alone reads and re-zeroes hist[wave][l]: program order; the next block's atomics wait behind its first barrier)
    }
}

// per unit k and column c of values [N][C]: count[k][c] = the unit's rows whose value in the column is not NaN ("not observed",
// for that column only), sum[k][c] and sumsq[k][c] over those values in double (a float32 and its square are exact in double);
// +-Inf is a value and goes into the sums.  Cp consecutive lanes read Cp consecutive floats of one row.
__global__ __launch_bounds__(256) void unit_value_sums_kernel(const int* __restrict__ start, const int* __restrict__ skey,
                                                              const int* __restrict__ order, const float* __restrict__ values,
                                                              long N, int K, int C, long long* __restrict__ count,
                                                              double* __restrict__ sum, double* __restrict__ sumsq) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;
    const int s0 = start[k];
    for (int c0 = 0; c0 < C; c0 += PROJ_CB) {
        const int cols = min(PROJ_CB, C - c0);
        int lg = 0;
        while ((1 << lg) < cols) ++lg;
        const int Cp = 1 << lg, R = 64 >> lg;                  // column slots, row slots
        const int col = lane & (Cp - 1), r = lane >> lg;
        const bool live = col < cols;
        double s = 0.0, q = 0.0;
        long long n = 0;
        if (s0 >= 0 && live)
            for (long i = (long)s0 + r; i < N && skey[i] == k; i += R) {
                const float v = values[(long)order[i] * C + c0 + col];
                if (v == v) {
                    const double d = (double)v;
                    s += d;
                    q += d * d;
                    ++n;
                }
            }
        for (int o = 32; o >= Cp; o >>= 1) {                   // the row slots of a column: lanes col, col + Cp, ...
            s += __shfl_xor(s, o, 64);
            q += __shfl_xor(q, o, 64);
            n += __shfl_xor(n, o, 64);
        }
        if (r == 0 && live) {
            const long at = (long)k * C + c0 + col;
            count[at] = n; sum[at] = s; sumsq[at] = q;
        }
    }
}

}  // namespace somhip
