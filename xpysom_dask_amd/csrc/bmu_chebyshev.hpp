// Fused Chebyshev (L-infinity) distance + first-minimum argmin: 'chebyshev' (MiniSom's fourth activation distance)
//   ids[n] = argmin_k max_d | fl32(x_nd - w_kd) |
// without the (n, K) matrix.  fl32(x - w) is correctly rounded and max is exact, so the distance has the same bits under
// every tiling, feature order and lane layout: nothing here follows a summation order, and the ids equal a NumPy model's.
//
// Work split.  A workgroup of 256 lanes (16 x 16) owns 128 rows x 128 units; a lane holds 8 rows x 8 units = 64 running
// maxima in registers (rows 4 ty .. +3 and 64 + 4 ty .. +3, units 4 tx .. +3 and 64 + 4 tx .. +3).  The workgroup keeps its
// rows and walks the unit blocks of its part of the codebook (gridDim.y parts; they merge by atomicMin on
// (distance bits << 32 | unit) -- a distance is >= 0, so its bits order as the value does -- and bmu_finalize_kernel).
//
// Operands.  Both go through LDS feature-major, [feature][row] and [feature][unit], 32 features a chunk, pitch 132 floats.
// A lane reads 16 bytes along the feature axis from global memory (four lanes a row: 64 bytes) and stores the four values
// to four feature lines: the bank is 16 a + b (a = feature quad 0..3, b = 16 consecutive rows) -- no two lanes of a wave
// on one of 64 banks.  Per feature a lane fetches its 8 rows and 8 units with two ds_read_b128 each: the row reads are
// four addresses a wave (broadcast), the unit reads 256 contiguous bytes.  Chunks are double-buffered: chunk t+1 is in
// flight from global memory to registers while chunk t is folded, and one barrier a chunk separates the two buffers.
//   RES (input_len <= 64):  the 128 rows stay in LDS for the whole scan ([<= 64][132] floats), only unit chunks stream.
//   else:                   the rows are re-staged with every unit block (from L2), chunk by chunk beside the units'.
// Either way a workgroup holds at most 2 x 2 x 32 x 132 floats = 66 KB, so two workgroups -- two waves a SIMD -- share a CU.
// (Rows resident up to 128 features would take 66 KB + 33 KB of unit chunks: one workgroup a CU, one wave a SIMD.)
//
// Inner loop.  Two features at a time: d0 = x_f - w_f, d1 = x_f+1 - w_f+1 (v_sub_f32), acc = max(acc, |d0|, |d1|)
// (one v_max3_f32 with both abs modifiers): 1.5 VALU instructions a pair.  The packed-FP32 subtract (two pairs an
// instruction) is deliberately NOT used: the kernel is compiled with the packed FP32 operations off (SOM_NO_PK_F32).
//
// Padding.  Features beyond input_len are zero on both sides (|0 - 0| = 0 never raises a maximum); units beyond K are
// skipped by the fold; rows beyond N are zero and never written.  A row holding a NaN or an infinity gets unit 0 (NumPy's
// argmin over an all-NaN row; every distance +inf): v_max drops NaNs, so the staging flags such rows.
#pragma once
#include "sparse.hpp"      // SOM_NO_PK_F32

namespace somhip {

constexpr int CH_BM = 128;                   // rows of a workgroup
constexpr int CH_BN = 128;                   // units of a unit block
constexpr int CH_KC = 32;                    // features of a chunk
constexpr int CH_PITCH = 132;                // floats of a feature line: 128 + 4 (16-byte aligned lines, 16 a + b banks)
constexpr int CH_CHUNK = CH_KC * CH_PITCH;   // floats of one operand chunk
constexpr int CH_RES_D = 64;                 // rows stay in LDS up to this many features

// dynamic LDS: the flags, the rows (RES: every chunk; else two buffers), two buffers of unit chunks
inline size_t ch_lds_bytes(int D) {
    const int x_chunks = D <= CH_RES_D ? (D + CH_KC - 1) / CH_KC : 2;
    return (size_t)CH_BM * sizeof(int) + (size_t)(x_chunks + 2) * CH_CHUNK * sizeof(float);
}

// 128 lines x 32 features of a row-major [R][D] matrix from (r0, f0) into registers: lane (a = tid & 3, b = tid >> 2)
// takes lines b and b + 64, features f0 + 4 a .. +3 and f0 + 16 + 4 a .. +3; zeros beyond R and beyond D
__device__ __forceinline__ void ch_load(const float* __restrict__ M, long R, int D, long r0, int f0, bool vec, int tid,
                                        float4 (&v)[4]) {
    const int a = tid & 3, b = tid >> 2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long line = r0 + b + 64 * (i >> 1);
        const int f = f0 + 4 * a + 16 * (i & 1);
        float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (line < R && f < D) {
            const float* p = M + line * (long)D + f;
            if (vec) t = *reinterpret_cast<const float4*>(p);    // (D % 4 == 0 and a 16-byte aligned base: f + 3 < D)
            else {
                t.x = p[0];
                if (f + 1 < D) t.y = p[1];
                if (f + 2 < D) t.z = p[2];
                if (f + 3 < D) t.w = p[3];
            }
        }
        v[i] = t;
    }
}

// the transposing store of ch_load's registers into a chunk [32][CH_PITCH]
__device__ __forceinline__ void ch_store(float* __restrict__ S, int tid, const float4 (&v)[4]) {
    const int a = tid & 3, b = tid >> 2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float* s = S + (4 * a + 16 * (i & 1)) * CH_PITCH + b + 64 * (i >> 1);
        s[0] = v[i].x; s[CH_PITCH] = v[i].y; s[2 * CH_PITCH] = v[i].z; s[3 * CH_PITCH] = v[i].w;
    }
}

__device__ __forceinline__ bool ch_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// rows of ch_load's registers that hold a NaN or an infinity -> flag[line] = 1 (every writer writes the same value)
__device__ __forceinline__ void ch_flag(int* __restrict__ flag, int tid, const float4 (&v)[4]) {
    const int b = tid >> 2;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (ch_nonfinite(v[i].x) || ch_nonfinite(v[i].y) || ch_nonfinite(v[i].z) || ch_nonfinite(v[i].w)) flag[b + 64 * (i >> 1)] = 1;
}

// one chunk: acc[i][j] = max(acc[i][j], |x_i - w_j| over the chunk's 32 features), two features an iteration
__device__ __forceinline__ void ch_fold(const float* __restrict__ Xs, const float* __restrict__ Ws, int ty, int tx, float (&acc)[8][8]) {
#pragma unroll 2
    for (int f = 0; f < CH_KC; f += 2) {
        float x[2][8], w[2][8];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const f32x4 xa = *reinterpret_cast<const f32x4*>(Xs + (f + g) * CH_PITCH + 4 * ty);
            const f32x4 xb = *reinterpret_cast<const f32x4*>(Xs + (f + g) * CH_PITCH + 64 + 4 * ty);
            const f32x4 wa = *reinterpret_cast<const f32x4*>(Ws + (f + g) * CH_PITCH + 4 * tx);
            const f32x4 wb = *reinterpret_cast<const f32x4*>(Ws + (f + g) * CH_PITCH + 64 + 4 * tx);
#pragma unroll
            for (int e = 0; e < 4; ++e) { x[g][e] = xa[e]; x[g][4 + e] = xb[e]; w[g][e] = wa[e]; w[g][4 + e] = wb[e]; }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d0 = __fsub_rn(x[0][i], w[0][j]);
                const float d1 = __fsub_rn(x[1][i], w[1][j]);
                acc[i][j] = __builtin_fmaxf(__builtin_fmaxf(acc[i][j], __builtin_fabsf(d0)), __builtin_fabsf(d1));
            }
    }
}

__global__ __launch_bounds__(256) void ch_fill_kernel(unsigned long long* __restrict__ p, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = ~0ull;
}

// grid (row blocks, parts).  out64 == nullptr (one part): the ids go straight to `out`.
template <bool RES>
__global__ SOM_NO_PK_F32 __launch_bounds__(256)
void bmu_chebyshev_kernel(const float* __restrict__ X, long N, int D, const float* __restrict__ W, int K, int x_vec, int w_vec,
                          int* __restrict__ out, unsigned long long* __restrict__ out64) {
    extern __shared__ __attribute__((aligned(16))) float smem_ch[];
    const int n_chunks = (D + CH_KC - 1) / CH_KC;
    int* flag = reinterpret_cast<int*>(smem_ch);
    float* Xs = smem_ch + CH_BM;                                   // RES: [n_chunks] chunks; else two buffers
    float* Ws = Xs + (RES ? n_chunks : 2) * CH_CHUNK;              // two buffers
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const long r0 = (long)blockIdx.x * CH_BM;
    const int n_ub = (K + CH_BN - 1) / CH_BN;
    const int ub0 = (int)((long)n_ub * blockIdx.y / gridDim.y), ub1 = (int)((long)n_ub * (blockIdx.y + 1) / gridDim.y);
    const int steps = (ub1 - ub0) * n_chunks;                      // (a part holds a unit block: the host keeps parts <= n_ub)

    if (tid < CH_BM) flag[tid] = 0;
    __syncthreads();
    float4 xr[4], wr[4];
    if (RES) {
        for (int c = 0; c < n_chunks; ++c) {
            ch_load(X, N, D, r0, c * CH_KC, x_vec != 0, tid, xr);
            ch_flag(flag, tid, xr);
            ch_store(Xs + c * CH_CHUNK, tid, xr);
        }
    } else {
        ch_load(X, N, D, r0, 0, x_vec != 0, tid, xr);
        ch_flag(flag, tid, xr);
        ch_store(Xs, tid, xr);
    }
    ch_load(W, K, D, (long)ub0 * CH_BN, 0, w_vec != 0, tid, wr);
    ch_store(Ws, tid, wr);
    __syncthreads();

    float acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.0f;
    float best[8];
    int bidx[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { best[i] = __builtin_inff(); bidx[i] = ub0 * CH_BN; }   // (all-infinite part: its first unit)

    int ub = ub0, c = 0;
    for (int t = 0; t < steps; ++t) {
        // the next step's operands leave global memory now and reach the other buffer after this chunk's fold
        int nub = ub, nc = c + 1;
        if (nc == n_chunks) { nc = 0; nub = ub + 1; }
        const bool more = t + 1 < steps;
        if (more) {
            ch_load(W, K, D, (long)nub * CH_BN, nc * CH_KC, w_vec != 0, tid, wr);
            if (!RES) {
                ch_load(X, N, D, r0, nc * CH_KC, x_vec != 0, tid, xr);
                if (nub == ub0) ch_flag(flag, tid, xr);            // (the first unit block sees every feature once)
            }
        }
        ch_fold(RES ? Xs + c * CH_CHUNK : Xs + (t & 1) * CH_CHUNK, Ws + (t & 1) * CH_CHUNK, ty, tx, acc);
        if (c == n_chunks - 1) {
            // this unit block's 8 units per row, ascending: the first minimum stays
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int u = ub * CH_BN + 64 * (j >> 2) + 4 * tx + (j & 3);
                    if (u < K && acc[i][j] < best[i]) { best[i] = acc[i][j]; bidx[i] = u; }
                    acc[i][j] = 0.0f;
                }
        }
        if (more) {
            ch_store(Ws + ((t + 1) & 1) * CH_CHUNK, tid, wr);
            if (!RES) ch_store(Xs + ((t + 1) & 1) * CH_CHUNK, tid, xr);
        }
        __syncthreads();
        ub = nub; c = nc;
    }

    // across the 16 lanes of a row (consecutive lanes of one wave): the smaller (distance bits, unit)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        unsigned long long key = ((unsigned long long)__float_as_uint(best[i]) << 32) | (uint32_t)bidx[i];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const unsigned long long other = __shfl_xor(key, o, 64);
            if (other < key) key = other;
        }
        const int line = 64 * (i >> 2) + 4 * ty + (i & 3);
        const long row = r0 + line;
        if (tx == 0 && row < N) {
            if (flag[line]) key = 0ull;                            // NaN / infinite row: unit 0
            if (out64 == nullptr) out[row] = (int)(uint32_t)key;
            else atomicMin(out64 + row, key);
        }
    }
}

}  // namespace somhip
