// Fused continuous Tanimoto (Jaccard) distance + first-minimum argmin: activation_distance='tanimoto'
//   s(n, k) = 1 - p / (a + b - p),   p = x_n . w_k,  a = |x_n|^2,  b = |w_k|^2      (float32; a + b - p <= 0: s = 0)
//   ids[n]  = the first k with the smallest s(n, k)
// without the (n, K) matrix.  For 0/1 rows against a 0/1 codebook p, a, b are exact integers and s is the Jaccard distance.
// The kernel reads the rows and the codebook as they are: no operand image of the rows, no prep pass over N x D.  (The
// handle still rebuilds the float32 parity image of the CODEBOOK with every codebook change, as it does for every
// float32 handle, 'chebyshev' included; this kernel does not read it.)
//
// a and b come from the existing row_sq_f32_kernel (NumPy's pairwise order): once per row set (RowSet::xsq, as for 'cosine')
// and once per codebook (som_handle::wsq).  A row whose a is not finite -- it holds a NaN or an infinity, or its squares
// overflow float32 -- gets unit 0, the rule of the Chebyshev and Manhattan searches.
//
// Work split.  A workgroup of 4 waves (2 x 2) owns 128 rows x 128 units and walks the features in chunks of 32; a wave owns
// 64 rows x 64 units = 2 x 2 accumulators of v_mfma_f32_32x32x2_f32 (A = units, B = rows: a lane owns the row `lane & 31` of
// each row tile and 16 units per accumulator), 64 accumulator registers that live through the whole feature walk.  The
// workgroup keeps its rows and walks the 128-unit blocks of its part of the codebook (gridDim.y parts).
//
// The order of p.  One chain of fused multiply-adds from 0 per (row, unit): chunks of 32 features ascending; inside a chunk the
// groups of 8 features g = 0..3; inside a group the steps j = 0..3, and step j adds feature 8 g + j, then feature 8 g + 4 + j
// (the two k of one instruction: lanes 0..31 hold the first, lanes 32..63 the second).  So a group's features enter as
// 0, 4, 1, 5, 2, 6, 3, 7.  Features beyond input_len are zeros on both sides.  The order does not depend on the part count.
//
// Operands.  Both go through LDS in FRAGMENT order: a chunk of 128 lines x 32 features is 16 pieces of 1 KiB, piece
// (t = line / 32, g) = 64 slots of 16 bytes, and the slot of lane (half, col) holds features 8 g + 4 half .. + 3 of line
// 32 t + col -- the lane's operand of the group's four steps, one ds_read_b128.  The slot sits at half * 32 + (col ^ 8 half):
//   reads:  the 64 lanes of a wave read the 64 slots of one piece, a permutation that keeps every aligned 16 lanes on 16
//           different slots (64 banks): conflict-free IF ds_read_b128 serves a wave as four groups of 16 consecutive lanes
//           -- derived from that assumption, not measured (no counter run was made);
//   writes: lane (q = tid & 7, b = tid >> 3) loads 16 bytes of line b + 32 i, features 4 q .. + 3, from global memory (eight
//           lanes a line: 128 contiguous bytes) -- exactly the slot of (t = i, g = q / 2, half = q & 1, col = b) -- and
//           stores it with one ds_write_b128; a wave's 8 lines x 2 halves fall on 16 different slots mod 16 (the ^ 8 half),
//           four lanes a slot (g): the minimum for 1 KiB.
// Chunks are double-buffered: chunk t + 1 travels global memory -> registers while chunk t is multiplied, is stored behind
// it into the other buffer, and one barrier a chunk separates the two.  2 operands x 2 buffers x 16 KiB = 64 KiB a
// workgroup: two workgroups, two waves a SIMD, share a CU.
//
// Epilogue, in registers, after a unit block's last chunk: s from p, a and b, '<' in ascending unit order keeps the lane's
// first minimum per row.  At the end the two lane halves of a row join by a shuffle, the two unit-half waves through LDS,
// and the parts by atomicMin on out64[row] -- everywhere the smaller packed key (order-preserving score bits << 32 | unit),
// so ties go to the lower unit under every tile and part count.  One part writes the ids itself.
//
// Registers (hipcc 7.2, gfx950): 160 VGPRs (64 of them accumulators, 32 the chunk in flight), no AGPRs, no scratch; the
// registers would allow 3 waves a SIMD, the 64 KiB of LDS allow 2 workgroups a CU: occupancy 2 waves a SIMD.
#pragma once
#include "som_common.hpp"      // f32x4, f32x16, mfma32_row
#include "bmu_chebyshev.hpp"   // ch_fill_kernel, ch_nonfinite

namespace somhip {

constexpr int TN_BM = 128;                   // rows of a workgroup
constexpr int TN_BN = 128;                   // units of a unit block
constexpr int TN_KC = 32;                    // features of a chunk
constexpr int TN_CHUNK = TN_BM * TN_KC;      // floats of one operand chunk (16 KiB)
constexpr int TN_MAX_D = 4096;               // the longest row served (the chain the tests' bound was checked for)
constexpr size_t TN_LDS_BYTES = (size_t)4 * TN_CHUNK * sizeof(float);   // rows and units, two buffers each

// 128 lines x 32 features of a row-major [R][D] matrix from (r0, f0) into registers: lane (q = tid & 7, b = tid >> 3) takes
// lines b + 32 i, features f0 + 4 q .. + 3; zeros beyond R and beyond D
__device__ __forceinline__ void tn_load(const float* __restrict__ M, long R, int D, long r0, int f0, bool vec, int tid, f32x4 (&v)[4]) {
    const int q = tid & 7, b = tid >> 3;
    const int f = f0 + 4 * q;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long line = r0 + b + 32 * i;
        f32x4 t = {0.0f, 0.0f, 0.0f, 0.0f};
        if (line < R && f < D) {
            const float* p = M + line * (long)D + f;
            if (vec) t = *reinterpret_cast<const f32x4*>(p);     // (D % 4 == 0 and a 16-byte aligned base: f + 3 < D)
            else {
                t[0] = p[0];
                if (f + 1 < D) t[1] = p[1];
                if (f + 2 < D) t[2] = p[2];
                if (f + 3 < D) t[3] = p[3];
            }
        }
        v[i] = t;
    }
}

// float offset of the slot of (piece t * 4 + g, half, col) in a chunk
__device__ __forceinline__ int tn_slot(int piece, int half, int col) { return (piece * 64 + half * 32 + (col ^ (half << 3))) * 4; }

// tn_load's registers into a chunk, in fragment order
__device__ __forceinline__ void tn_store(float* __restrict__ S, int tid, const f32x4 (&v)[4]) {
    const int q = tid & 7, b = tid >> 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(S + tn_slot(i * 4 + (q >> 1), q & 1, b)) = v[i];
}

// float bits -> unsigned, ascending as the values ascend (a score is slightly negative where p rounds above (a + b) / 2)
__device__ __forceinline__ uint32_t tn_order_bits(float s) {
    const uint32_t u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// grid (row blocks, parts).  out64 == nullptr (one part): the ids go straight to `out`.
__global__ __launch_bounds__(256, 2)
void bmu_tanimoto_kernel(const float* __restrict__ X, long N, int D, const float* __restrict__ xsq, const float* __restrict__ W,
                         const float* __restrict__ wsq, int K, int x_vec, int w_vec, int* __restrict__ out,
                         unsigned long long* __restrict__ out64) {
    extern __shared__ __attribute__((aligned(16))) float smem_tn[];
    float* Xs = smem_tn;                                           // two buffers
    float* Ws = smem_tn + 2 * TN_CHUNK;                            // two buffers
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;                       // row half, unit half
    const int half = lane >> 5, col = lane & 31;
    const long r0 = (long)blockIdx.x * TN_BM;
    const int n_chunks = (D + TN_KC - 1) / TN_KC;
    const int n_ub = (K + TN_BN - 1) / TN_BN;
    const int ub0 = (int)((long)n_ub * blockIdx.y / gridDim.y), ub1 = (int)((long)n_ub * (blockIdx.y + 1) / gridDim.y);
    const int steps = (ub1 - ub0) * n_chunks;                      // (a part holds a unit block: the host keeps parts <= n_ub)

    float a[2];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
        const long row = r0 + wr * 64 + sb * 32 + col;
        a[sb] = row < N ? xsq[row] : 0.0f;
    }
    float best[2];
    int bidx[2];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) { best[sb] = __builtin_inff(); bidx[sb] = ub0 * TN_BN; }   // (no score below +inf: the part's first unit)

    f32x4 xr[4], wv[4];
    tn_load(X, N, D, r0, 0, x_vec != 0, tid, xr);
    tn_load(W, K, D, (long)ub0 * TN_BN, 0, w_vec != 0, tid, wv);
    tn_store(Xs, tid, xr);
    tn_store(Ws, tid, wv);
    __syncthreads();

    f32x16 acc[2][2];                                              // [unit tile][row tile]
#pragma unroll
    for (int tu = 0; tu < 2; ++tu)
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tu][sb][r] = 0.0f;

    const int a_off = tn_slot(wc * 2 * 4, half, col);              // + (tu * 4 + g) * 256 floats
    const int b_off = tn_slot(wr * 2 * 4, half, col);              // + (sb * 4 + g) * 256 floats

    int ub = ub0, c = 0;
    for (int t = 0; t < steps; ++t) {
        // the next step's operands leave global memory now and reach the other buffer after this chunk's products
        int nub = ub, nc = c + 1;
        if (nc == n_chunks) { nc = 0; nub = ub + 1; }
        const bool more = t + 1 < steps;
        if (more) {
            tn_load(X, N, D, r0, nc * TN_KC, x_vec != 0, tid, xr);
            tn_load(W, K, D, (long)nub * TN_BN, nc * TN_KC, w_vec != 0, tid, wv);
        }
        const float* xs = Xs + (t & 1) * TN_CHUNK + b_off;
        const float* ws = Ws + (t & 1) * TN_CHUNK + a_off;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 fa[2], fb[2];
#pragma unroll
            for (int tu = 0; tu < 2; ++tu) fa[tu] = *reinterpret_cast<const f32x4*>(ws + (tu * 4 + g) * 256);
#pragma unroll
            for (int sb = 0; sb < 2; ++sb) fb[sb] = *reinterpret_cast<const f32x4*>(xs + (sb * 4 + g) * 256);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int tu = 0; tu < 2; ++tu)
#pragma unroll
                    for (int sb = 0; sb < 2; ++sb)
                        acc[tu][sb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[tu][j], fb[sb][j], acc[tu][sb], 0, 0, 0);
        }
        if (c == n_chunks - 1) {
            // this unit block's 32 units per row of the lane, ascending: the first minimum stays
#pragma unroll
            for (int tu = 0; tu < 2; ++tu)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int u = ub * TN_BN + wc * 64 + tu * 32 + mfma32_row(r, half);
                    const float b = u < K ? wsq[u] : 0.0f;
#pragma unroll
                    for (int sb = 0; sb < 2; ++sb) {
                        const float p = acc[tu][sb][r];
                        const float den = __fsub_rn(__fadd_rn(a[sb], b), p);
                        const float s = den > 0.0f ? __fsub_rn(1.0f, __fdiv_rn(p, den)) : 0.0f;
                        if (u < K && s < best[sb]) { best[sb] = s; bidx[sb] = u; }
                        acc[tu][sb][r] = 0.0f;
                    }
                }
        }
        if (more) {
            tn_store(Xs + ((t + 1) & 1) * TN_CHUNK, tid, xr);
            tn_store(Ws + ((t + 1) & 1) * TN_CHUNK, tid, wv);
        }
        __syncthreads();
        ub = nub; c = nc;
    }

    // a row's four holders -- two lane halves, two unit-half waves -- then the parts: the smaller (score, unit) key
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem_tn);   // [128] (the chunks are no longer read: the loop's last barrier)
    unsigned long long key[2];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
        key[sb] = ((unsigned long long)tn_order_bits(best[sb]) << 32) | (uint32_t)bidx[sb];
        const unsigned long long other = __shfl_xor(key[sb], 32, 64);
        if (other < key[sb]) key[sb] = other;
        if (wc == 1 && half == 0) keys[wr * 64 + sb * 32 + col] = key[sb];
    }
    __syncthreads();
    if (wc == 0 && half == 0) {
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) {
            const int line = wr * 64 + sb * 32 + col;
            const long row = r0 + line;
            if (row >= N) continue;
            if (keys[line] < key[sb]) key[sb] = keys[line];
            if (ch_nonfinite(a[sb])) key[sb] = 0ull;                // NaN / infinite row: unit 0
            if (out64 == nullptr) out[row] = (int)(uint32_t)key[sb];
            else atomicMin(out64 + row, key[sb]);
        }
    }
}

}  // namespace somhip
