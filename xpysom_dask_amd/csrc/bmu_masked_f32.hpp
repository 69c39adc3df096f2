// Fused masked distance + BMU argmin, float32: the search of a handle created with SOM_MISSING_NAN.
//
// A NaN in a row means "not observed".  With m_d = 1 where x_d is observed and 0 otherwise, and x~_d = x_d where observed
// and 0 otherwise, the masked squared distance of row x to unit w is
//     sum_d m_d (x_d - w_d)^2  =  sum_d m_d x_d^2  -  2 sum_d x~_d w_d  +  sum_d m_d w_d^2 .
// The first sum does not depend on the unit, so the BMU is the first minimum of
//     s_k = fmaf(-2, c1_k, c2_k),    c1_k = sum_d x~_d w_kd,    c2_k = sum_d m_d (w_kd w_kd),
// TWO contractions per unit where the unmasked search has one and a per-unit constant |w|^2: which features of a unit
// count depends on the row.
//
// Arithmetic: both chains run on v_mfma_f32_32x32x2_f32 with the operand mapping of bmu_f32.hpp -- A operand = units,
// B operand = samples, a lane owns one sample and its accumulator registers are 16 units, the running first minimum is
// f32_tile_argmin -- so each chain is a k-ordered float32 fma chain.  The second chain's A operand is w * w rounded once to
// float32, formed when the A fragment is read from LDS (no pass of its own over the codebook); x~ and m are formed in
// registers from the rows as they are, NaNs included (no augmented copy of the data).  Any NaN bit pattern counts
// (x != x); +-inf is a value.  On complete rows c2 is the k-ordered sum of the rounded squares: the same ids as the
// unmasked kernel wherever every product and sum is exact, not bit-identical scores in general (|w|^2 there is NumPy's
// pairwise sum).  A row with nothing observed scores 0 on every unit and takes unit 0.
//
// Tiling: dist_matrix_f32_kernel's -- a workgroup = 4 waves x 32 samples scans the codebook in tiles of 128 units, both
// operands staged through LDS in chunks of 32 features (+1 padded rows: conflict-free fragment reads), each chunk fetched into
// registers one chunk ahead.  The rows' chunk is staged again for every unit tile: it comes from L2, under a chunk's 128 MFMAs
// per wave (8192 cycles).  Tails on all
// three axes: padding units are staged as zeros and never compete (f32_tile_argmin<.., TAIL>), padding features are staged
// as zeros on both sides (an observed 0 against a unit value 0: nothing to either chain), padding samples are not written.
// Any K >= 1, N >= 1, D >= 1.
#pragma once
#include "bmu_f32.hpp"

namespace somhip {

// bytes of dynamic LDS bmu_masked_f32_kernel needs
constexpr size_t MSK_LDS_BYTES = (size_t)(F32_UB + F32_SB) * (F32_KC + 1) * sizeof(float);

// (two waves per SIMD asked for: 128 accumulator registers, 32 of the chunk in flight and a chunk's unrolled fragment reads come to
//  238 VGPRs, no AGPRs, no scratch -- two workgroups per CU, the barriers of one under the MFMAs of the other)
__global__ __launch_bounds__(256, 2) void bmu_masked_f32_kernel(const float* __restrict__ X, long N, int D, int Dp,
                                                             const float* __restrict__ W, int K,
                                                             int* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float msk_lds[];
    constexpr int LD = F32_KC + 1;
    float* Ws = msk_lds;
    float* Xs = Ws + F32_UB * LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, col = lane & 31;
    const long s0 = (long)blockIdx.x * F32_SB;
    const long my_sample = s0 + wave * 32 + col;
    float best = __builtin_inff();
    int bkey = 0;
    // staging: thread t holds feature t & 31 of rows (t >> 5) + 8 i, i = 0 .. 15, of both tiles.  A chunk's 32 values are loaded
    // into registers BEFORE the MFMAs of the chunk ahead of it and written to LDS after them, so the loads' latency lies under
    // 128 MFMAs (loaded in the staging loop itself -- 16 dependent round trips per chunk -- the kernel ran at half this rate)
    constexpr int ST = F32_UB * F32_KC / 256;             // 16
    const int sk = tid & 31, sr = tid >> 5;
    float wreg[ST], xreg[ST];
    auto fetch = [&](int u0, int kc) {
        const bool kin = kc + sk < D;
#pragma unroll
        for (int i = 0; i < ST; ++i) {
            const int r = sr + 8 * i;
            wreg[i] = (kin && u0 + r < K) ? W[(long)(u0 + r) * D + kc + sk] : 0.0f;
            xreg[i] = (kin && s0 + r < N) ? X[(s0 + r) * (long)D + kc + sk] : 0.0f;
        }
    };
    fetch(0, 0);
    for (int u0 = 0; u0 < K; u0 += F32_UB) {
        f32x16 c1[4], c2[4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) { c1[rb][r] = 0.0f; c2[rb][r] = 0.0f; }
        for (int kc = 0; kc < Dp; kc += F32_KC) {
            __syncthreads();                             // (the chunk before has been read)
#pragma unroll
            for (int i = 0; i < ST; ++i) {
                Ws[(sr + 8 * i) * LD + sk] = wreg[i];
                Xs[(sr + 8 * i) * LD + sk] = xreg[i];
            }
            __syncthreads();
            {                                            // the next chunk, or the next unit tile's first one
                const bool more_k = kc + F32_KC < Dp;
                const int nu = more_k ? u0 : u0 + F32_UB, nk = more_k ? kc + F32_KC : 0;
                if (nu < K) fetch(nu, nk);
            }
            const float* xrow = Xs + (wave * 32 + col) * LD + half;
            const float* wrow = Ws + col * LD + half;
#pragma unroll
            for (int k = 0; k < F32_KC; k += 2) {
                const float b = xrow[k];
                const bool seen = b == b;
                const float xt = seen ? b : 0.0f;
                const float m = seen ? 1.0f : 0.0f;
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) {
                    const float a = wrow[rb * 32 * LD + k];
                    c1[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xt, c1[rb], 0, 0, 0);
                    c2[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(__fmul_rn(a, a), m, c2[rb], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
            f32x4 wv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j) wv[q][j] = c2[rb][4 * q + j];
            const int tile = (u0 >> 5) + rb;
            if ((tile + 1) * 32 > K) f32_tile_argmin<SCORE_EUCLID_PART, true>(c1[rb], wv, 0.0f, tile, half, K, best, bkey);
            else f32_tile_argmin<SCORE_EUCLID_PART, false>(c1[rb], wv, 0.0f, tile, half, K, best, bkey);
        }
    }
    int bidx = f32_key_unit(bkey, half);
    const float ob = __shfl_xor(best, 32, 64);
    const int oi = __shfl_xor(bidx, 32, 64);
    if (ob < best || (ob == best && oi < bidx)) bidx = oi;
    if (half == 0 && my_sample < N) out[my_sample] = bidx;
}

// sum_n sqrt(sum_d m_nd (x_nd - W[bmu_n][d])^2): qe_kernel over the observed features only -- the differences formed
// directly, a row with nothing observed adds 0 (and is counted by the caller's mean)
__global__ __launch_bounds__(256) void qe_masked_kernel(const float* __restrict__ X, const int* __restrict__ bmu,
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
        for (int k = lane; k < D; k += 64) {
            const float xv = x[k];
            if (xv == xv) { const float df = xv - w[k]; s = __builtin_fmaf(df, df, s); }
        }
        s = wave_sum(s);
        acc += (double)__builtin_sqrtf(s);
    }
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sum_out, (part[0] + part[1]) + (part[2] + part[3]));
}

}  // namespace somhip
