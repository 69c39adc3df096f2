// Fused masked distance + BMU argmin on the 16-bit matrix pipe: the search of a handle created with SOM_MISSING_NAN once
// som_set_masked_search picked SOM_PREC_BF16 or SOM_PREC_F16 (XPySom(..., missing='nan', missing_search='bf16' | 'f16')).
//
// With m_d = 1 where x_d is observed (x == x) and 0 otherwise, x~ the row rounded to the operand type (cvt<> of som_common.hpp)
// with 0 at the holes and w~ the codebook rounded the same way, the masked squared distance in the rounded space is
//     sum_d m_d (x~_d - w~_kd)^2  =  sum_d m_d x~_d^2  +  2 s_k,       s_k = 1/2 sum_d m_d q_kd  -  sum_d x~_d w~_kd,    q = w~ w~.
// The first sum does not depend on the unit: the BMU is the first minimum of s_k.  Both contractions of s_k are GEMMs against the
// SAME row fragment pair (x~, m), so they share one float32 accumulator of v_mfma_f32_16x16x32:
//     acc += (-w~) . x~          on the mode's own instruction (bf16 or f16 operands)
//     acc += (q_hi/2) . m        on the bf16 instruction in BOTH modes
//     acc += (q_lo/2) . m        likewise
// q/2 is carried as two bf16 images: h = fl32(w~ w~) / 2 is exact (a square of a 16-bit value has at most 22 significant bits, a
// halving is exact), q_hi/2 = bf16(h), q_lo/2 = bf16(h - q_hi/2).  For bf16 operands (8 significant bits: 16 in the square) the pair
// is exact; for half operands (11: 22) it is within 2^-17 of h.  bf16 has float32's range: no scaling, no overflow up to 65504^2.
// m is 1.0 or 0: exact.  Three MFMAs per (16 units, 32 features, 16 rows) where the unmasked 16-bit kernels issue one.
//
// Geometry (bmu_bf16_k16.hpp's): A = 16 units x 32 features (lane l: unit l & 15, features 8 (l >> 4) + j), B = 32 features x 16
// rows (lane l: row l & 15), C: lane l holds row l & 15, units 4 (l >> 4) + reg.  A workgroup = MH_NW waves x MH_SB blocks of 16
// rows = MH_WG_SAMPLES rows; the codebook goes by in STAGES of MH_STAGE_UNITS units.
//
// The codebook images are written by prep_masked_half_kernel in front of every search (the codebook may have changed: 6 Kp Dp
// bytes, nothing beside the scan) into scratch the masked path owns, in MFMA fragment order:
//     chunk g = stage * KS + ks  (KS = ceil(D / 32)):  [tile t16 0..3][image 0..2: -w~, q_hi/2, q_lo/2][lane 0..63][8 x 16 bit]
// MH_CHUNK_BYTES = 12 KiB each; a stage is KS consecutive chunks.  Padding units and padding features are zeros in all three.
//
// Two kernels:
//   bmu_masked_half_kernel<KS32>     up to 128 features.  The rows are read ONCE, float32 with their NaNs, as they are (no 16-bit or
//                                    augmented copy of the data): every wave forms the x~ and m fragments of its 64 rows in
//                                    registers and keeps them across the whole codebook.  Only the images stream: whole stages by
//                                    LDS-DMA (global_load_lds) into a ring of two slots, the next stage in flight under this one's
//                                    MFMAs, one barrier a stage.  One A-fragment triple read from LDS feeds 12 MFMAs.
//   bmu_masked_half_stream_kernel    beyond 128 features: both sides stream in 32-feature chunks.  A stage's 16 accumulators stay in
//                                    registers while the feature chunks pass: the image chunk by LDS-DMA into a ring of two slots,
//                                    the rows' next 32 features as float32 in registers, both one chunk ahead; x~ and m are formed
//                                    per chunk from those.
// Argmin: plain (float, id) compares, strict `<` in ascending unit order inside a lane, (score, id) across the four lane
// quads: the first minimum.  A padding unit (images all zero: it would score 0) is set to +inf in the stage that holds the tail.  A
// row with nothing observed has x~ = m = 0, scores 0 on every unit and takes unit 0.  Padding rows and padding features are loaded
// as NaN, i.e. "not observed".  NaN scores (rows holding +-inf: outside the 16-bit modes' contract) never win; a row of only such
// scores takes unit 0.
// Grid = (row blocks) x (codebook parts): a part scans its share of the stages and, where there are several, leaves (score, id)
// per row; sparse.hpp's merge kernel takes the minimum by (score, id).  No atomics.  A unit's score is one fixed chain of MFMAs in
// feature order whatever the part count, so the ids do not depend on it.
#pragma once
#include "bmu_bf16.hpp"
#include "sparse.hpp"      // SOM_NO_PK_F32, sparse_before, sparse_merge_kernel

namespace somhip {

// (a lambda is not always_inline by itself, and a kernel whose target features differ from the default -- SOM_NO_PK_F32 -- inlines
//  nothing else: its captured arrays would live in scratch)
#define SOM_MH_INLINE __attribute__((always_inline))

constexpr int MH_SB = 4;                                 // 16-row blocks per wave
constexpr int MH_NW = 4;                                 // waves per workgroup (they share the LDS ring)
constexpr int MH_WG_SAMPLES = MH_NW * 16 * MH_SB;        // 256
constexpr int MH_T = 4;                                  // 16-unit tiles per stage
constexpr int MH_STAGE_UNITS = 16 * MH_T;                // 64
constexpr int MH_IMGS = 3;                               // -w~, q_hi / 2, q_lo / 2
constexpr int MH_CHUNK_BYTES = MH_T * MH_IMGS * 1024;    // one (stage, 32-feature step) of the images
constexpr int MH_RES_KS = 4;                             // 32-feature steps the register-resident kernel serves (128 features)

// the kernels are templates on a flag, not on the operand tag: HALF = IEEE half operands for x~ and w~ ('f16'), else bfloat16
template <bool HALF> struct MhOperand { typedef __bf16 T; };
template <> struct MhOperand<true> { typedef _Float16 T; };

__host__ __device__ constexpr size_t mh_lds_bytes(int ks32) { return 2 * (size_t)ks32 * MH_CHUNK_BYTES; }

// one workgroup per chunk: thread = (tile, lane) = (unit, 8 features); three 16-byte fragments each
template <bool HALF>
__global__ SOM_NO_PK_F32 __launch_bounds__(256) void prep_masked_half_kernel(const float* __restrict__ W, int K, int D, int KS,
                                                                             char* __restrict__ Wimg) {
    using E = typename MhOperand<HALF>::T;
    using ex8 = typename V8<E>::t;
    const long g = blockIdx.x;
    const long stage = g / KS;
    const int ks = (int)(g - stage * KS);
    const int t16 = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long u = stage * MH_STAGE_UNITS + t16 * 16 + (lane & 15);
    const int k0 = ks * 32 + (lane >> 4) * 8;
    ex8 a;
    bf16x8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float f = (u < K && k0 + j < D) ? W[u * D + k0 + j] : 0.0f;
        a[j] = cvt<E>(-f);                                 // (rounding is sign-symmetric: -w~)
        const float wt = (float)cvt<E>(f);
        const float h = 0.5f * __fmul_rn(wt, wt);          // exact
        const __bf16 hb = (__bf16)h;
        const float r = h - (float)hb;                     // exact
        hi[j] = hb;
        lo[j] = (__bf16)(r == r ? r : 0.0f);               // (h overflowed: bf16 units beyond 1.8e19)
    }
    char* dst = Wimg + g * MH_CHUNK_BYTES + (long)(t16 * MH_IMGS) * 1024 + lane * 16;
    *(ex8*)dst = a;
    *(bf16x8*)(dst + 1024) = hi;
    *(bf16x8*)(dst + 2048) = lo;
}

// features k0 .. k0 + 7 of a row as they are; NaN ("not observed") beyond the row's end and beyond the last row
__device__ __forceinline__ void mh_row_load(const float* __restrict__ X, long N, int D, long row, int k0, bool vec, float (&v)[8]) {
    if (row < N && vec && k0 + 8 <= D) {
        const f32x4 p = *(const f32x4*)(X + row * D + k0), q = *(const f32x4*)(X + row * D + k0 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] = p[j]; v[4 + j] = q[j]; }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (row < N && k0 + j < D) ? X[row * D + k0 + j] : __builtin_nanf("");
    }
}
template <class E>
__device__ __forceinline__ void mh_row_fragment(const float (&v)[8], typename V8<E>::t& xf, bf16x8& mf) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const bool seen = v[j] == v[j];
        xf[j] = cvt<E>(seen ? v[j] : 0.0f);
        mf[j] = (__bf16)(seen ? 1.0f : 0.0f);
    }
}

// the running first minimum of one lane: the tile's units u0 .. u0 + 3 of its MH_SB rows, in ascending order
__device__ __forceinline__ void mh_fold(const f32x4 (&acc)[MH_SB], int u0, bool tail, int K, float (&best)[MH_SB], int (&bid)[MH_SB]) {
#pragma unroll
    for (int sb = 0; sb < MH_SB; ++sb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = acc[sb][r];
            if (tail && u0 + r >= K) v = __builtin_inff();
            if (v < best[sb]) { best[sb] = v; bid[sb] = u0 + r; }
        }
}

// the four lane quads of a row joined by (score, id); quad 0 writes the id, or -- several parts -- the part's (score, id)
__device__ __forceinline__ void mh_write(const float (&best)[MH_SB], const int (&bid)[MH_SB], long wave_s0, int lane, long N,
                                         int* __restrict__ out, float* __restrict__ part_sc, int* __restrict__ part_id) {
    const int by = blockIdx.y, ny = gridDim.y;
#pragma unroll
    for (int sb = 0; sb < MH_SB; ++sb) {
        float b = best[sb];
        int i = bid[sb];
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float ob = __shfl_xor(b, o, 64);
            const int oi = __shfl_xor(i, o, 64);
            if (sparse_before(ob, oi, b, i)) { b = ob; i = oi; }
        }
        const long row = wave_s0 + sb * 16 + (lane & 15);
        if ((lane >> 4) == 0 && row < N) {
            if (ny == 1) out[row] = i;
            else { part_sc[(size_t)by * N + row] = b; part_id[(size_t)by * N + row] = i; }
        }
    }
}

// (KS32 = 4: 32 row fragments + a tile's 12 image fragments + their successors = 250 registers and 96 KiB of LDS: one workgroup a
//  CU on the unified 512-register file; up to 96 features two fit)
template <int KS32, bool HALF>
__global__ SOM_NO_PK_F32 __launch_bounds__(64 * MH_NW, KS32 <= 3 ? 2 : 1) void bmu_masked_half_kernel(
    const float* __restrict__ X, long N, int D, const char* __restrict__ Wimg, int n_stages, int K, int* __restrict__ out,
    float* __restrict__ part_sc, int* __restrict__ part_id) {
    using E = typename MhOperand<HALF>::T;
    using ex8 = typename V8<E>::t;
    constexpr int STAGE = KS32 * MH_CHUNK_BYTES;
    constexpr int PIECES = KS32 * MH_T * MH_IMGS;
    extern __shared__ __attribute__((aligned(16))) char mh_smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int quad = lane >> 4, col = lane & 15;
    const long wave_s0 = (long)blockIdx.x * MH_WG_SAMPLES + wave * (16 * MH_SB);
    const bool vec = (D & 3) == 0 && ((uintptr_t)X & 15) == 0;

    ex8 xf[MH_SB][KS32];
    bf16x8 mf[MH_SB][KS32];
#pragma unroll
    for (int sb = 0; sb < MH_SB; ++sb)
#pragma unroll
        for (int ks = 0; ks < KS32; ++ks) {
            float v[8];
            mh_row_load(X, N, D, wave_s0 + sb * 16 + col, ks * 32 + quad * 8, vec, v);
            mh_row_fragment<E>(v, xf[sb][ks], mf[sb][ks]);
        }
    float best[MH_SB];
    int bid[MH_SB];
#pragma unroll
    for (int sb = 0; sb < MH_SB; ++sb) { best[sb] = __builtin_inff(); bid[sb] = 0; }

    const int s_begin = (int)((long)n_stages * blockIdx.y / gridDim.y);
    const int s_end = (int)((long)n_stages * (blockIdx.y + 1) / gridDim.y);
    auto dma_stage = [&](int s, char* dst) SOM_MH_INLINE {
        const char* src = Wimg + (long)s * STAGE;
        for (int p = wave; p < PIECES; p += MH_NW) lds_dma_16(src + (long)p * 1024 + lane * 16, dst + p * 1024);
    };
    if (s_begin < s_end) dma_stage(s_begin, mh_smem);
    for (int s = s_begin; s < s_end; ++s) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                      // stage s has landed; everyone has read stage s - 1
        asm volatile("" ::: "memory");
        if (s + 1 < s_end) dma_stage(s + 1, mh_smem + ((s + 1 - s_begin) & 1) * STAGE);
        const char* st = mh_smem + ((s - s_begin) & 1) * STAGE + lane * 16;
        const bool tail = (s + 1) * MH_STAGE_UNITS > K;
        auto load_tile = [&](int t16, ex8 (&aw)[KS32], bf16x8 (&ah)[KS32], bf16x8 (&al)[KS32]) SOM_MH_INLINE {
#pragma unroll
            for (int ks = 0; ks < KS32; ++ks) {
                const char* p = st + ((ks * MH_T + t16) * MH_IMGS) * 1024;
                aw[ks] = *(const ex8*)p;
                ah[ks] = *(const bf16x8*)(p + 1024);
                al[ks] = *(const bf16x8*)(p + 2048);
            }
        };
        ex8 aw[KS32];
        bf16x8 ah[KS32], al[KS32];
        load_tile(0, aw, ah, al);
#pragma unroll
        for (int t16 = 0; t16 < MH_T; ++t16) {
            ex8 awN[KS32];
            bf16x8 ahN[KS32], alN[KS32];
            if (t16 + 1 < MH_T) load_tile(t16 + 1, awN, ahN, alN);   // (read under this tile's MFMAs)
            f32x4 acc[MH_SB];
#pragma unroll
            for (int sb = 0; sb < MH_SB; ++sb) acc[sb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int ks = 0; ks < KS32; ++ks) {
#pragma unroll
                for (int sb = 0; sb < MH_SB; ++sb) acc[sb] = mfma16(aw[ks], xf[sb][ks], acc[sb]);
#pragma unroll
                for (int sb = 0; sb < MH_SB; ++sb) acc[sb] = mfma16(ah[ks], mf[sb][ks], acc[sb]);
#pragma unroll
                for (int sb = 0; sb < MH_SB; ++sb) acc[sb] = mfma16(al[ks], mf[sb][ks], acc[sb]);
            }
            mh_fold(acc, s * MH_STAGE_UNITS + t16 * 16 + quad * 4, tail, K, best, bid);
            if (t16 + 1 < MH_T) {
#pragma unroll
                for (int ks = 0; ks < KS32; ++ks) { aw[ks] = awN[ks]; ah[ks] = ahN[ks]; al[ks] = alN[ks]; }
            }
        }
    }
    mh_write(best, bid, wave_s0, lane, N, out, part_sc, part_id);
}

// (a stage's 16 accumulators, a chunk's 12 image fragments and the rows' next 32 float32 features: 170 registers, 24 KiB of LDS)
template <bool HALF>
__global__ SOM_NO_PK_F32 __launch_bounds__(64 * MH_NW, 2) void bmu_masked_half_stream_kernel(
    const float* __restrict__ X, long N, int D, const char* __restrict__ Wimg, int n_stages, int KS, int K, int* __restrict__ out,
    float* __restrict__ part_sc, int* __restrict__ part_id) {
    using E = typename MhOperand<HALF>::T;
    using ex8 = typename V8<E>::t;
    constexpr int PIECES = MH_T * MH_IMGS;
    extern __shared__ __attribute__((aligned(16))) char mh_smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int quad = lane >> 4, col = lane & 15;
    const long wave_s0 = (long)blockIdx.x * MH_WG_SAMPLES + wave * (16 * MH_SB);
    const bool vec = (D & 3) == 0 && ((uintptr_t)X & 15) == 0;

    float best[MH_SB];
    int bid[MH_SB];
#pragma unroll
    for (int sb = 0; sb < MH_SB; ++sb) { best[sb] = __builtin_inff(); bid[sb] = 0; }

    const int s_begin = (int)((long)n_stages * blockIdx.y / gridDim.y);
    const int s_end = (int)((long)n_stages * (blockIdx.y + 1) / gridDim.y);
    auto dma_chunk = [&](long g, char* dst) SOM_MH_INLINE {
        const char* src = Wimg + g * MH_CHUNK_BYTES;
        for (int p = wave; p < PIECES; p += MH_NW) lds_dma_16(src + (long)p * 1024 + lane * 16, dst + p * 1024);
    };
    float xraw[MH_SB][8];
    auto fetch_rows = [&](int ks) SOM_MH_INLINE {
#pragma unroll
        for (int sb = 0; sb < MH_SB; ++sb) mh_row_load(X, N, D, wave_s0 + sb * 16 + col, ks * 32 + quad * 8, vec, xraw[sb]);
    };
    if (s_begin < s_end) { dma_chunk((long)s_begin * KS, mh_smem); fetch_rows(0); }
    int slot = 0;
    for (int s = s_begin; s < s_end; ++s) {
        f32x4 acc[MH_T][MH_SB];
#pragma unroll
        for (int t16 = 0; t16 < MH_T; ++t16)
#pragma unroll
            for (int sb = 0; sb < MH_SB; ++sb) acc[t16][sb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int ks = 0; ks < KS; ++ks, slot ^= 1) {
            ex8 xf[MH_SB];
            bf16x8 mf[MH_SB];
#pragma unroll
            for (int sb = 0; sb < MH_SB; ++sb) mh_row_fragment<E>(xraw[sb], xf[sb], mf[sb]);
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                  // this chunk has landed; everyone has read the one before
            asm volatile("" ::: "memory");
            {                                              // the next chunk, or the next stage's first one
                const bool more_k = ks + 1 < KS;
                if (more_k || s + 1 < s_end) {
                    dma_chunk((long)s * KS + ks + 1, mh_smem + (slot ^ 1) * MH_CHUNK_BYTES);
                    fetch_rows(more_k ? ks + 1 : 0);
                }
            }
            const char* st = mh_smem + slot * MH_CHUNK_BYTES + lane * 16;
#pragma unroll
            for (int t16 = 0; t16 < MH_T; ++t16) {
                const char* p = st + (t16 * MH_IMGS) * 1024;
                const ex8 aw = *(const ex8*)p;
                const bf16x8 ah = *(const bf16x8*)(p + 1024), al = *(const bf16x8*)(p + 2048);
#pragma unroll
                for (int sb = 0; sb < MH_SB; ++sb) acc[t16][sb] = mfma16(aw, xf[sb], acc[t16][sb]);
#pragma unroll
                for (int sb = 0; sb < MH_SB; ++sb) acc[t16][sb] = mfma16(ah, mf[sb], acc[t16][sb]);
#pragma unroll
                for (int sb = 0; sb < MH_SB; ++sb) acc[t16][sb] = mfma16(al, mf[sb], acc[t16][sb]);
            }
        }
        const bool tail = (s + 1) * MH_STAGE_UNITS > K;
#pragma unroll
        for (int t16 = 0; t16 < MH_T; ++t16) mh_fold(acc[t16], s * MH_STAGE_UNITS + t16 * 16 + quad * 4, tail, K, best, bid);
    }
    mh_write(best, bid, wave_s0, lane, N, out, part_sc, part_id);
}

}  // namespace somhip
