// Sparse rows (som_set_data_csr, som_bmu_csr, som_quantization_error_csr; include/somhip.h): CSR rows -- indptr int64 [n + 1], indices
// int32 [nnz] strictly ascending inside a row, values float32 [nnz] -- searched and summed without ever being made dense.  The rows
// mean what their dense form means; everything is float32.
//
// Matrix instructions do not fit: the contraction x . w_k over a row's nnz entries is a gather, and a codebook element is used once
// per (entry, unit).  What can be arranged is that this one read is a full line and that nothing else touches memory.
//
//   sparse_transpose_kernel     WT[D][Kp] = W[K][D] transposed through a 64 x 65 LDS tile, Kp = K rounded up to 64, the padding
//                               columns zero.  Rebuilt in front of every search: 8 K D bytes against the search's 4 nnz K.
//   sparse_rownorm_kernel       |x|^2 per row, a wave per row (lanes stride the entries, one butterfly)
//   sparse_bmu_kernel<MODE, U>  grid = row tiles x parts.  A workgroup of 4 waves shares one tile of SP_ROWS consecutive rows, whose
//                               entries are ONE contiguous span of the CSR arrays: the span goes through LDS in chunks of SP_CHUNK
//                               (col, val) pairs, 16 bytes a lane from a 16-byte aligned base (the arrays are padded to whole
//                               int4s), so a row longer than a chunk only costs more chunks -- its accumulators stay in registers
//                               across the chunk barrier.  The waves divide the UNITS: of a slab of 256 U units wave w owns the U
//                               64-unit groups from w U on, lane l unit 64 g + l of each.  Per entry col and val are wave-uniform LDS
//                               broadcasts and acc[u] = fma(val, WT[col][k_u], acc[u]) reads one 256-byte line per u: U independent
//                               chains.  At the end of a row the score is score_f32<MODE> (bmu_f32.hpp: the dense kernels'
//                               formulas) of acc, |w_k|^2 and |x|^2; a lane keeps the first minimum over its u (ascending ids), one
//                               butterfly by (score, id) gives the wave's, lane 0 folds it into the wave's LDS slot of the row (its
//                               slabs ascend, so `<` keeps the lower id), and after the last slab 32 threads join the four waves by
//                               (score, id).  A part whose range is longer than a slab walks the slabs in turn and stages the span
//                               again for each.  parts == 1: the ids are written; else (score, id) per (part, row) and
//   sparse_merge_kernel         a thread per row: the minimum by (score, id) over the parts.
//                               No atomics anywhere: every unit's score is one fixed fma chain over the row's entries in CSR
//                               order, whatever the tile, the slab or the part -- the ids are identical for every geometry.
//                               A row without entries: acc = 0, so euclidean picks the unit of least |w|^2 (first on a tie) and
//                               cosine scores 1 everywhere (0 / 0 -> NaN -> 0: unit 0).  An id that no finite score named
//                               (non-finite values: outside the contract) is written as 0, never out of range.
//   sparse_unit_bounds_kernel   first sorted position of every unit (and N behind the last): a lower bound per thread
//   sparse_segsum_kernel        level 0 of the run sum for CSR rows, behind sort_rows_by_unit.  A wave owns one (unit, slab of
//                               SP_SLAB columns): it zeroes its 8 KiB of LDS, walks the unit's rows in sorted order -- per row the
//                               entries inside the slab (a binary search on the row's ascending columns; a short row is scanned
//                               and masked instead: no dependent loads), lanes on distinct entries of ONE row at a time, columns
//                               unique in a row: no two lanes meet on an address -- and stores the slab to SC[unit] with plain
//                               stores.  The slab that holds column D stores the row count there and in the dense count array, as
//                               the run sum does.  Every (unit, slab) is written once, zeros where a unit has no rows; the order of
//                               every sum is the sorted order of the unit's rows: a function of the ids alone.
//   sparse_qe_kernel            a wave per row walks W[bmu] in 64-column steps; a cursor moves through the row's entries, those of
//                               the step are scattered into the wave's 64-float LDS line (zeroed per step), each lane adds
//                               (x_d - w_d)^2 from the difference itself; wave sum, sqrtf: dist[row]
//   sparse_dsum_kernel          one workgroup: the rows' distances added in double in a fixed tree
//
// Traffic: the search reads 4 nnz K bytes of WT through the caches (2 nnz K flop), the staged span once per slab of a part; the
// segment sum reads a row's entries once per slab it touches (a short row: once per slab) and writes 4 K D1p bytes; the distance
// reads 4 D bytes of the codebook per row.  Offsets into the CSR arrays, WT, SC and W are 64-bit.
#pragma once
#include "bmu_f32.hpp"

namespace somhip {

// Every kernel of this file is compiled without the packed float32 instructions (two fmas of independent chains in one operation):
// the scan's U chains and the norms' squares are what the compiler would pair, and each chain is meant to be a plain float32 fma chain.
#define SOM_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))

constexpr int SP_ROWS = 32;        // rows per tile of the search
constexpr int SP_CHUNK = 1024;     // (col, val) pairs per staging chunk: 256 lanes x 16 bytes, twice
constexpr int SP_SLAB = 2048;      // columns per slab of the segment sum: 8 KiB of LDS per wave
constexpr int SP_SCAN_MAX = 128;   // a row of at most this many entries is scanned, not searched, by the segment sum

// Launch geometry of the search: pure host arithmetic.  wanted: the part count choose_parts (or SOM_SPARSE_PARTS) asks for; the
// 64-unit groups are cut into that many parts, never more than there are groups, and a count that would leave parts without a
// group is lowered.  U: groups per wave of a slab -- the widest that still gives every wave of a part's first slab a group.
struct SparsePlan { long row_tiles; int groups, per, parts, U; };
inline SparsePlan sparse_plan(long n_rows, int K, long wanted) {
    SparsePlan p;
    p.row_tiles = (n_rows + SP_ROWS - 1) / SP_ROWS;
    p.groups = (K + 63) / 64;
    long s = wanted < 1 ? 1 : (wanted > p.groups ? p.groups : wanted);
    p.per = (int)((p.groups + s - 1) / s);
    p.parts = (p.groups + p.per - 1) / p.per;
    p.U = p.per > 8 ? 4 : p.per > 4 ? 2 : 1;
    return p;
}

__global__ SOM_NO_PK_F32 __launch_bounds__(256) void sparse_transpose_kernel(const float* __restrict__ W, int K, int D, int Kp, float* __restrict__ WT) {
    __shared__ float tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int k0 = blockIdx.x * 64, d0 = blockIdx.y * 64;
    for (int i = ty; i < 64; i += 4) {
        const int k = k0 + i, d = d0 + tx;
        tile[i][tx] = (k < K && d < D) ? W[(size_t)k * D + d] : 0.0f;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int d = d0 + i, k = k0 + tx;
        if (d < D && k < Kp) WT[(size_t)d * Kp + k] = tile[tx][i];
    }
}

__global__ SOM_NO_PK_F32 __launch_bounds__(256) void sparse_rownorm_kernel(const long long* __restrict__ indptr, const float* __restrict__ values, long N,
                                                             float* __restrict__ xsq) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= N) return;
    const long long rs = indptr[row], re = indptr[row + 1];
    float a = 0.0f;
    for (long long e = rs + lane; e < re; e += 64) { const float v = values[e]; a = __builtin_fmaf(v, v, a); }
    a = wave_sum(a);
    if (lane == 0) xsq[row] = a;
}

// (score, id) strictly before (score, id)
__device__ __forceinline__ bool sparse_before(float sa, int ia, float sb, int ib) { return sa < sb || (sa == sb && ia < ib); }

// n_alloc: entries the index and value arrays hold, a multiple of 4 (>= nnz): what a 16-byte load may touch
template <int MODE, int U>
__global__ SOM_NO_PK_F32 __launch_bounds__(256) void sparse_bmu_kernel(const long long* __restrict__ indptr, const int* __restrict__ indices,
                                                         const float* __restrict__ values, long N, long long n_alloc,
                                                         const float* __restrict__ xsq, const float* __restrict__ WT,
                                                         const float* __restrict__ wsq, int K, int Kp, int per, int parts,
                                                         float* __restrict__ part_sc, int* __restrict__ part_id, int* __restrict__ out) {
    __shared__ int4 s_col4[SP_CHUNK / 4];
    __shared__ float4 s_val4[SP_CHUNK / 4];
    __shared__ long long s_ptr[SP_ROWS + 1];
    __shared__ float s_bs[4][SP_ROWS];
    __shared__ int s_bi[4][SP_ROWS];
    const int* s_col = (const int*)s_col4;
    const float* s_val = (const float*)s_val4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long r0 = (long)blockIdx.x * SP_ROWS;
    const int nr = (int)(N - r0 < SP_ROWS ? N - r0 : SP_ROWS);
    const int groups = Kp >> 6;
    const int g_begin = blockIdx.y * per, g_end = g_begin + per < groups ? g_begin + per : groups;
    if (tid <= nr) s_ptr[tid] = indptr[r0 + tid];
    if (tid < 4 * SP_ROWS) { s_bs[tid / SP_ROWS][tid % SP_ROWS] = __builtin_inff(); s_bi[tid / SP_ROWS][tid % SP_ROWS] = 0x7fffffff; }
    __syncthreads();
    const long long e_begin = s_ptr[0];
    for (int gs = g_begin; gs < g_end; gs += 4 * U) {          // a slab of 256 U units
        const int g0 = gs + wave * U;
        const bool active = g0 < g_end;
        int unit[U]; bool valid[U]; float wq[U]; const float* wt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int g = g0 + u;
            unit[u] = 64 * g + lane;
            valid[u] = g < g_end && unit[u] < K;
            wq[u] = valid[u] ? wsq[unit[u]] : 0.0f;
            wt[u] = WT + 64 * (g < groups ? g : groups - 1) + lane;      // (a group past the end: any column that exists)
        }
        float acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = 0.0f;
        long long base = e_begin & ~3LL;
        int r = 0;
        while (r < nr) {                                       // one staging chunk [base, base + SP_CHUNK) a turn
            __syncthreads();                                   // (the last chunk's readers are done)
            {
                const long long i = base + 4 * tid;
                int4 c = make_int4(0, 0, 0, 0); float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (i < n_alloc) { c = *(const int4*)(indices + i); v = *(const float4*)(values + i); }
                s_col4[tid] = c; s_val4[tid] = v;
            }
            __syncthreads();
            const long long lim = base + SP_CHUNK;
            while (r < nr) {                                   // the rows with entries in this chunk (all of this is workgroup-uniform)
                const long long rs = s_ptr[r], re = s_ptr[r + 1];
                const int a = (int)((rs > base ? rs : base) - base), b = (int)((re < lim ? re : lim) - base);
                if (active) {
#pragma unroll 4
                    for (int j = a; j < b; ++j) {
                        const size_t off = (size_t)s_col[j] * Kp;
                        const float v = s_val[j];
#pragma unroll
                        for (int u = 0; u < U; ++u) acc[u] = __builtin_fmaf(v, wt[u][off], acc[u]);
                    }
                }
                if (re > lim) break;                           // the row goes on in the next chunk
                if (active) {
                    const float xs = MODE == SCORE_EUCLID_PART ? 0.0f : xsq[r0 + r];
                    float best = __builtin_inff(); int bid = 0x7fffffff;
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const float s = score_f32<MODE>(acc[u], wq[u], xs);
                        if (valid[u] && s < best) { best = s; bid = unit[u]; }
                        acc[u] = 0.0f;
                    }
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const float os = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bid, o, 64);
                        if (sparse_before(os, oi, best, bid)) { best = os; bid = oi; }
                    }
                    if (lane == 0 && best < s_bs[wave][r]) { s_bs[wave][r] = best; s_bi[wave][r] = bid; }
                }
                ++r;
            }
            base = lim;
        }
    }
    __syncthreads();
    if (tid < nr) {
        float best = s_bs[0][tid]; int bid = s_bi[0][tid];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (sparse_before(s_bs[w][tid], s_bi[w][tid], best, bid)) { best = s_bs[w][tid]; bid = s_bi[w][tid]; }
        if (parts == 1) out[r0 + tid] = bid < K ? bid : 0;
        else { part_sc[(size_t)blockIdx.y * N + r0 + tid] = best; part_id[(size_t)blockIdx.y * N + r0 + tid] = bid; }
    }
}

__global__ SOM_NO_PK_F32 __launch_bounds__(256) void sparse_merge_kernel(const float* __restrict__ part_sc, const int* __restrict__ part_id, long N, int parts,
                                                           int K, int* __restrict__ out) {
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    if (row >= N) return;
    float best = part_sc[row]; int bid = part_id[row];
    for (int p = 1; p < parts; ++p) {
        const float s = part_sc[(size_t)p * N + row]; const int i = part_id[(size_t)p * N + row];
        if (sparse_before(s, i, best, bid)) { best = s; bid = i; }
    }
    out[row] = bid < K ? bid : 0;
}

// first i in [lo, hi) with a[i] >= key (hi: none)
template <class I>
__device__ __forceinline__ long long sparse_lower_bound(const I* __restrict__ a, long long lo, long long hi, long long key) {
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if ((long long)a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ustart[k] = first sorted position whose unit is >= k, k = 0 .. K (ustart[K] = N)
__global__ SOM_NO_PK_F32 __launch_bounds__(256) void sparse_unit_bounds_kernel(const int* __restrict__ skey, long N, int K, int* __restrict__ ustart) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k <= K) ustart[k] = (int)sparse_lower_bound(skey, 0, N, k);
}

__global__ SOM_NO_PK_F32 __launch_bounds__(256) void sparse_segsum_kernel(const long long* __restrict__ indptr, const int* __restrict__ indices,
                                                            const float* __restrict__ values, const int* __restrict__ srow,
                                                            const int* __restrict__ ustart, int K, int D, int D1p, int nslabs,
                                                            float* __restrict__ SC, float* __restrict__ cnt_dense) {
    __shared__ float s_slab[4][SP_SLAB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long item = (long)blockIdx.x * 4 + wave;             // (unit, slab); no workgroup barrier below: a wave may leave
    if (item >= (long)K * nslabs) return;
    const int unit = (int)(item / nslabs), slab = (int)(item % nslabs);
    const int c0 = slab * SP_SLAB, c1 = c0 + SP_SLAB < D1p ? c0 + SP_SLAB : D1p;
    float* s = s_slab[wave];
    for (int i = lane; i < SP_SLAB; i += 64) s[i] = 0.0f;
    const int lo = ustart[unit], hi = ustart[unit + 1];
    for (int p = lo; p < hi; ++p) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the last row's adds (other lanes') before this row's
        const long row = srow[p];
        const long long rs = indptr[row], re = indptr[row + 1];
        if (re - rs <= SP_SCAN_MAX) {
            for (long long e = rs + lane; e < re; e += 64) {
                const int c = indices[e];
                if (c >= c0 && c < c1) s[c - c0] += values[e];
            }
        } else {
            const long long a = sparse_lower_bound(indices, rs, re, c0), b = sparse_lower_bound(indices, a, re, c1);
            for (long long e = a + lane; e < b; e += 64) {
                const int c = indices[e];
                if (c >= c0 && c < c1) s[c - c0] += values[e];   // (true for ascending columns; never an address outside the slab)
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (lane == 0 && D >= c0 && D < c1) {                        // the count column, and the counts once more, densely
        s[D - c0] = (float)(hi - lo);
        cnt_dense[unit] = (float)(hi - lo);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    float* dst = SC + (size_t)unit * D1p + c0;
    for (int i = lane; i < c1 - c0; i += 64) dst[i] = s[i];
}

__global__ SOM_NO_PK_F32 __launch_bounds__(256) void sparse_qe_kernel(const long long* __restrict__ indptr, const int* __restrict__ indices,
                                                        const float* __restrict__ values, const int* __restrict__ bmu,
                                                        const float* __restrict__ W, long N, int D, float* __restrict__ dist) {
    __shared__ float s_line[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* line = s_line[wave];
    for (long row = (long)blockIdx.x * 4 + wave; row < N; row += (long)gridDim.x * 4) {
        const float* w = W + (size_t)bmu[row] * D;
        long long cur = indptr[row];
        const long long re = indptr[row + 1];
        float acc = 0.0f;
        for (int d0 = 0; d0 < D; d0 += 64) {
            line[lane] = 0.0f;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            // the entries of this step: at most 64 (ascending, unique columns), so one turn of the lanes takes them all
            const long long e = cur + lane;
            const int c = e < re ? indices[e] : 0x7fffffff;
            const bool in = c >= d0 && c < d0 + 64;
            if (in) line[c - d0] = values[e];
            cur += __builtin_popcountll(__ballot(c < d0 + 64));
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if (d0 + lane < D) { const float t = line[lane] - w[d0 + lane]; acc = __builtin_fmaf(t, t, acc); }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
        acc = wave_sum(acc);
        if (lane == 0) dist[row] = __builtin_sqrtf(acc);
    }
}

// *out = sum_n dist[n] in double: thread t adds rows t, t + 1024, ... in order, then a fixed tree
__global__ SOM_NO_PK_F32 __launch_bounds__(1024) void sparse_dsum_kernel(const float* __restrict__ dist, long N, double* __restrict__ out) {
    __shared__ double s[1024];
    double a = 0.0;
    for (long i = threadIdx.x; i < N; i += 1024) a += (double)dist[i];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s[0];
}

}  // namespace somhip
