// precision 'exact', euclidean, input_len <= 128, maps of >= 4096 units: BLOCK SKIPPING in the screen -- resident rows from their
// second epoch on (bound: last epoch's BMU) and, through the SCOUT at the end of this file, every other large row set.
//
// The screen (bmu_bf16_k16_kernel<.., GM>) is the exact epoch; what is left is not to run it where no BMU can be.  Two facts:
//   * last epoch's BMU u of a row x gives an upper bound on the distance to this epoch's BMU k*: the float32 kernel picks
//     k* with fl(tau(k*)) <= fl(tau(u)), so  |x - w_k*|^2 <= U(x) := |x|^2 + tau_up(u) + share,  tau_up an upper bound of
//     u's real score tau(u) = |w_u|^2 - 2 x.w_u under the CURRENT codebook, share the float32 kernel's error window;
//   * a block of units (a patch of the map) with centroid c and radius r = max |w - c| has  |x - w| >= |x - c| - r  for
//     each of its units.
// So a block holds no candidate of row x if  |x - c| > sqrt(U(x)) + r.
//
// ROWS stay resident in the order of their last BMU's patch (somhip.hip: a sorted copy of the operand image, the float32
// rows, the norms; re-sorted only when the order has gone stale -- most rows move to a neighbouring patch at most from
// one epoch to the next, and a 256-row tile of neighbours shares its blocks either way), so the 256 rows of a workgroup
// tile lie in one region of the map.
// BLOCKS come at two levels: the 64-unit GROUPS of the screen (one stage of its image = an 8 x 8 patch of the map) and
// their four 16-unit SUB-BLOCKS (the stage's four MFMA tiles = 4 x 4 squares of the patch where both map sides are multiples
// of 8 -- som_patch_order --, 2 x 8 strips elsewhere).  Late in a schedule the units of a patch spread out (its radius grows
// to the scale of the data) and the group bound alone keeps a quarter of all blocks; the sub-blocks' own centroids and radii
// cut that to a third.  The PLAN kernel below is the screen's MFMA loop
// on centroids with the test as its epilogue and an OR over the tile's rows: level 1 over the group centroids (1/64 of
// the units), level 2 over the sub-block centroids of the groups level 1 kept.  The screen then walks, per tile, the list
// of (group, 4-bit sub-block mask) items some row of it needs.
// A skipped (row, block) stores no minimum: to the select kernel it is a block outside the window, which is what the test
// proved.  The row minimum m(n) is over the blocks run: never below the true one, and the float32 winner's block is
// among them, so the selection argument of bmu_exact.hpp holds unchanged (the re-score evaluates whole groups).
// SEED: tau_up(u) comes from the operands the plan holds anyway -- the row's half image and unit u's fragments of the
// screen's stage image, a vector-ALU dot product in the plan's prologue: v_u = S (B + tau(u) / 2) up to the screen's
// one-unit error (measured operand rounding + accumulation), which is charged.  The same v_u caps what the screen
// stores at all (bmu_exact.hpp, seed).
// Rigour: |x - c|^2 = |x|^2 + tau_c is taken from the plan's screen value d'_c = S'(B' + tau_c / 2) less the screen's
// error bound for the centroid image (E_c / 2 of ex_row_bound on the centroids' scales), norms and radii are rounded
// outwards; a row whose quantities are not finite needs every block.
#pragma once
#include "bmu_bf16_k16.hpp"
#include "bmu_f32_res.hpp"

namespace somhip {

static_assert(SK_TILE == K16_WG_SAMPLES, "block skipping: a plan / screen tile (exact_scratch.hpp) is the resident screen's workgroup of rows");
static_assert(K16_STAGE_UNITS == 64 && K16_T == 4, "block skipping: a stage of the resident screen is one 64-unit group of four 16-unit tiles");

// Centroids and radii of the blocks of W (patch order), both levels in one launch: workgroup g holds group g's 64
// units in registers (thread <-> a feature of a sub-block; rows read whole: coalesced) and forms the centroid of the group and of each of
// its four 16-unit sub-blocks, their |c|^2, and the radii r = max |w - c| (a unit's |w - c|^2 is a wave reduction).
// Level 1: slot g = group g.  Level 2: slot 16 (g >> 2) + 4 (g & 3) + b = sub-block b of group g -- sixteen consecutive slots are
// the sub-blocks of four consecutive groups, one 16-row MFMA tile of the level-2 centroid image.  A slot without units:
// centroid 0, radius -1 (never needed).  The grid covers whole level-2 tiles (n_groups rounded up to four).
// cmax2 (per level {max |c|^2, max rounding error^2}): a centroid is a mean of units, |c| <= max |w|: the images take the
// codebook's own scale (no reduction over the centroids); the error slot is reset here and filled by the image kernel.
struct CentroidLevel { float* C; float* rg; float* csq; float* cmax2; int n_slots; };
// (eight waves: thread (feature d, quarter q) holds the sixteen units of sub-block q -- a group's 32 KB are in flight at once)
struct CentroidShared {
    float qsum[4][128];                                       // the sub-blocks' feature sums
    float part[2][64][2];                                     // [feature half][unit][group / sub-block]: partial |w - c|^2
    float csq_s[2][5];
};
// The arithmetic itself, on the sixteen units a thread holds (w[k] = 0 beyond the group's units and the features): shared by
// exact_centroids_kernel and the fused merge below, so that both write the same bits.  Every thread of the 512 calls it.
__device__ __forceinline__ void group_centroids(const float (&w)[16], int g, int K, int D, const CentroidLevel& l1,
                                                const CentroidLevel& l2, CentroidShared& sh) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int d = tid & 127, q = tid >> 7, fh = (tid >> 6) & 1;   // feature, sub-block, which 64 features of the 128
    const int cnt = (int)max(0L, min(64L, (long)K - (long)g * 64));
    const int cb = max(0, min(16, cnt - 16 * q));
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k) sum += w[k];
    sh.qsum[q][d] = sum;
    __syncthreads();
    const float cs = cb > 0 ? sum / (float)cb : 0.0f;
    const float cg = cnt > 0 ? ((sh.qsum[0][d] + sh.qsum[1][d]) + (sh.qsum[2][d] + sh.qsum[3][d])) / (float)cnt : 0.0f;
    if (d < D) {
        if (q == 0 && g < l1.n_slots) l1.C[(long)g * D + d] = cg;
        const int j = 16 * (g >> 2) + 4 * (g & 3) + q;
        if (j < l2.n_slots) l2.C[(long)j * D + d] = cs;
    }
    // |c|^2 of the five centroids (float32, any order: the plan's margin covers it)
    {
        const float a = wave_sum(cs * cs);
        if (lane == 0) sh.csq_s[fh][1 + q] = a;
        if (q == 0) { const float bq = wave_sum(cg * cg); if (lane == 0) sh.csq_s[fh][0] = bq; }
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (k < cb) {                                         // (uniform over the wave)
            const float dg = w[k] - cg, ds = w[k] - cs;
            const float qg = wave_sum(d < D ? dg * dg : 0.0f);    // (a NaN anywhere in the unit: NaN)
            const float qs = wave_sum(d < D ? ds * ds : 0.0f);
            if (lane == 0) { sh.part[fh][16 * q + k][0] = qg; sh.part[fh][16 * q + k][1] = qs; }
        }
    }
    __syncthreads();
    if (tid < 5) {
        // thread 0: the group; threads 1..4: its sub-blocks
        const int b = tid - 1;
        const int k0 = tid == 0 ? 0 : 16 * b, k1 = tid == 0 ? cnt : min(cnt, 16 * b + 16);
        float m = 0.0f;
        for (int k = k0; k < k1; ++k) {
            const float d2 = sh.part[0][k][tid == 0 ? 0 : 1] + sh.part[1][k][tid == 0 ? 0 : 1];
            m = (d2 > m || !(d2 == d2)) ? d2 : m;             // (a NaN unit: a NaN radius, the block is never skipped)
        }
        // (the sum of squares in float32, any order: relative error <= 128 * 2^-24; the margin covers it many times over)
        const float r = k1 > k0 ? __builtin_sqrtf(m) * (1.0f + 1.0f / 512.0f) + 1.0e-30f : -1.0f;
        const float sq = sh.csq_s[0][tid] + sh.csq_s[1][tid];
        if (tid == 0) { if (g < l1.n_slots) { l1.rg[g] = r; l1.csq[g] = sq; } }
        else {
            const int j = 16 * (g >> 2) + 4 * (g & 3) + b;
            if (j < l2.n_slots) { l2.rg[j] = r; l2.csq[j] = sq; }
        }
    }
}

__global__ __launch_bounds__(512) void exact_centroids_kernel(const float* __restrict__ W, int K, int D, int n_groups,
                                                              CentroidLevel l1, CentroidLevel l2, const float* __restrict__ wmax2) {
    __shared__ CentroidShared sh;
    const int g = blockIdx.x, tid = threadIdx.x;
    const int d = tid & 127, q = tid >> 7;
    const long u0 = (long)g * 64 + 16 * q;
    const int cnt = (int)max(0L, min(64L, (long)K - (long)g * 64));
    const int cb = max(0, min(16, cnt - 16 * q));
    if (g == 0 && tid == 0) { l1.cmax2[0] = *wmax2; l1.cmax2[1] = 0.0f; l2.cmax2[0] = *wmax2; l2.cmax2[1] = 0.0f; }
    float w[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k] = (d < D && k < cb) ? W[(u0 + k) * D + d] : 0.0f;
    group_centroids(w, g, K, D, l1, l2, sh);
}

// THE FUSED MERGE of the exact mode (euclidean, input_len <= 128; som_epoch_merge): one read of the accumulator writes what
// the next epoch's first launch needs of the new codebook, each bit for bit what the separate kernels write --
//   merge_kernel            W (unit order) and Wp (patch order): den != 0 ? num / den : the old row;
//   row_sq_f32_kernel       wsq, wsq_p: np_pairwise_sq_sum's own leaf over a padded copy of the group in LDS, a thread per unit;
//   exact_copy_wsq_kernel   wn and the maximum of |w|^2 into wmax2[0] (the host zeroed the pair in front of this launch);
//   prep_w_f32_res_kernel   the group's stage of the float32 image Wfst (FR_STAGE_UNITS = one group) in the image order;
//   exact_centroids_kernel  centroids, radii, |c|^2 of both levels (l1.C != null; cmax2 waits for the final maximum: the 16-bit
//                           image's kernel resets it, prep_w_exact_k16_kernel).
// Workgroup g <-> group g of the IMAGE ORDER (perm[position] = unit, or null: the units' own order): thread (feature d,
// quarter q) holds sixteen units as exact_centroids_kernel does, so every load and store of a row is one contiguous piece.
constexpr int MPX_STRIDE = 129;       // floats between two units of the LDS copy: a thread per unit walks its row without bank conflicts
static_assert(FR_STAGE_UNITS == 64, "the fused merge writes one float32 stage per 64-unit group");
struct MergePrepOut {
    float* W; float* Wp; const int* perm;
    float* wsq; float* wsq_p; float* wn; float* wmax2;
    char* Wfst; int fr_kg;                                     // (Wfst null: the float32 image is left to its own kernel)
};
__global__ __launch_bounds__(512) void exact_merge_prep_kernel(const float* __restrict__ ACC, int K, int D, int D1p, int n_groups,
                                                               MergePrepOut o, CentroidLevel l1, CentroidLevel l2) {
    __shared__ CentroidShared sh;
    __shared__ float ws[64 * MPX_STRIDE];
    __shared__ int u_s[64];
    __shared__ float den_s[64];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int d = tid & 127, q = tid >> 7;
    const int cnt = (int)max(0L, min(64L, (long)K - (long)g * 64));
    const int cb = max(0, min(16, cnt - 16 * q));
    if (tid < cnt) {
        const int pos = g * 64 + tid;
        const int u = o.perm != nullptr ? o.perm[pos] : pos;
        u_s[tid] = u;
        den_s[tid] = ACC[(long)u * D1p + D];
    }
    __syncthreads();
    // (w[] is written by selects only: a store into the array under a branch makes the compiler copy all sixteen registers)
    float w[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {                            // every load of the thread's sixteen units first
        const bool on = d < D && k < cb;
        const long u = on ? u_s[16 * q + k] : 0;
        // (no row in reach of a unit: the old weights stay; a thread without an element reads a valid address and drops it)
        const float* src = !on ? ACC : den_s[16 * q + k] != 0.0f ? ACC + u * D1p + d : o.W + u * D + d;
        const float v = *src;
        w[k] = on ? v : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const bool on = d < D && k < cb;
        const int i = 16 * q + k;
        const float den = on ? den_s[i] : 0.0f;
        const float v = w[k] / den;
        w[k] = den != 0.0f ? v : w[k];
        if (on) {
            const long u = u_s[i];
            if (den != 0.0f) o.W[u * D + d] = w[k];
            if (o.Wp != nullptr) o.Wp[((long)g * 64 + i) * D + d] = w[k];
            ws[i * MPX_STRIDE + d] = w[k];
        }
    }
    // (the centroid levels' error maxima start from zero for the image kernel that follows: exact_prep_images_kernel)
    if (l1.C != nullptr && g == 0 && tid == 0) { l1.cmax2[1] = 0.0f; l2.cmax2[1] = 0.0f; }
    if (l1.C != nullptr) group_centroids(w, g, K, D, l1, l2, sh);   // (its barriers order the LDS copy as well)
    else __syncthreads();
    if (g >= n_groups) return;                                // (the grid covers whole level-2 tiles: groups without units)
    if (o.Wfst != nullptr) {
        char* base = o.Wfst + (long)g * fr_stage_bytes(o.fr_kg);
        for (int r = tid; r < FR_UT * o.fr_kg * 64; r += 512) {   // prep_w_f32_res_kernel's chunk r of the stage
            const int lane = r & 63, t = r >> 6;
            const int gk = t % o.fr_kg, i = (t / o.fr_kg) * 32 + (lane & 31);
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = 8 * gk + 2 * j + (lane >> 5);
                v[j] = (i < cnt && k < D) ? ws[i * MPX_STRIDE + k] : 0.0f;
            }
            *(f32x4*)(base + (long)r * 16) = v;
        }
    }
    if (tid < 64) {                                           // a thread per unit: |w|^2 in NumPy's order
        float qv = __builtin_inff(), m = 0.0f;
        if (tid < cnt) {
            const int pos = g * 64 + tid;
            qv = np_pairwise_sq_sum_leaf((const float*)(ws + tid * MPX_STRIDE), D);
            o.wsq[u_s[tid]] = qv;
            if (o.wsq_p != nullptr) o.wsq_p[pos] = qv;
            o.wn[pos] = qv;
            m = (qv == qv) ? qv : 0.0f;
        }
        if (o.Wfst != nullptr) ((float*)(o.Wfst + (long)g * fr_stage_bytes(o.fr_kg) + (long)FR_UT * o.fr_kg * 1024))[tid] = qv;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
        if (tid == 0) atomic_max_pos_f32(o.wmax2, m);
    }
}

// sort key of row n: the group (patch) of its last BMU; value: n
__global__ __launch_bounds__(256) void exact_sortkey_kernel(const int* __restrict__ prev, const int* __restrict__ inv, long n,
                                                            int K, int* __restrict__ keys, int* __restrict__ vals) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int u = prev[i];
    u = u < 0 ? 0 : u >= K ? K - 1 : u;
    keys[i] = (inv != nullptr ? inv[u] : u) >> 6;
    vals[i] = (int)i;
}

// position (patch order) of every sorted row's last BMU: what the plan's prologue reads instead of three dependent loads
__global__ __launch_bounds__(256) void exact_lastpos_kernel(const int* __restrict__ prev, const int* __restrict__ order,
                                                            const int* __restrict__ inv, long n, int K, int* __restrict__ lastpos) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    int u = prev[order[p]];
    u = u < 0 ? 0 : u >= K ? K - 1 : u;                      // (any unit gives a valid bound)
    lastpos[p] = inv != nullptr ? inv[u] : u;
}

// The pass in sorted order: image rows (DP halves), the float32 rows themselves (what the re-score reads: a candidate
// group's rows are then neighbours in memory; input_len a multiple of 8: even features first, then the odd ones), |x|^2, rounding error -- and the rows' SECOND half image for the refinement
// pass (bmu_exact.hpp): lo = half(2^11 (x^ - hi)), x^ = sx x.  Positions behind the pass's rows (up to the tile multiple) get
// zero rows and NaN norms (they keep nothing, need nothing).  Sixteen lanes per row.
template <class EL>
__global__ __launch_bounds__(256) void exact_gather_sorted_kernel(const int* __restrict__ order, long n, long np, int dp, int D,
                                                                  const __bf16* __restrict__ Xb, const float* __restrict__ X,
                                                                  const float* __restrict__ xsq, const float* __restrict__ xerr,
                                                                  const float* __restrict__ xmax2,
                                                                  __bf16* __restrict__ Xb_s, __bf16* __restrict__ Xl_s,
                                                                  float* __restrict__ Xf_s,
                                                                  float* __restrict__ xsq_s, float* __restrict__ xerr_s) {
    using E = typename EL::T;
    using bf16x8 = typename V8<E>::t;
    // (sixteen lanes per row -- dp <= 128 halves = at most sixteen 16-byte pieces --, four rows per wave: a wave per row left
    //  three quarters of its lanes idle and the kernel at a third of the fabric's rate)
    const int lane = threadIdx.x & 15;
    const long p = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (p >= np) return;
    const long r = p < n ? (long)order[p] : -1;
    const float sx = ex_scale(*xmax2);
    const bool vec = (D & 7) == 0;
    for (int c = lane; c < dp / 8; c += 16) {                 // 16-byte pieces of the half images = 8 features
        bf16x8 v, vl;
#pragma unroll
        for (int j = 0; j < 8; ++j) { v[j] = (E)0.0f; vl[j] = (E)0.0f; }
        if (r >= 0) {
            v = *(const bf16x8*)((const char*)Xb + (r * dp + c * 8) * 2);
            float f[8];
            if (vec && c * 8 < D) {                           // (one read of the float32 row: its copy and its second half)
                // (the float32 copy DE-INTERLEAVED: the row's even features, then its odd ones -- a lane of the re-score's 32x32x2 MFMA
                //  feeds one parity of the features, and reads its half of the row in whole 16-byte pieces: exact_rescore_mfma_kernel)
                const f32x4 a = *(const f32x4*)(X + r * D + c * 8), b = *(const f32x4*)(X + r * D + c * 8 + 4);
                const f32x4 ev = {a[0], a[2], b[0], b[2]}, od = {a[1], a[3], b[1], b[3]};
                *(f32x4*)(Xf_s + p * D + c * 4) = ev;
                *(f32x4*)(Xf_s + p * D + D / 2 + c * 4) = od;
#pragma unroll
                for (int j = 0; j < 4; ++j) { f[j] = a[j]; f[4 + j] = b[j]; }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    f[j] = c * 8 + j < D ? X[r * D + c * 8 + j] : 0.0f;
                    if (c * 8 + j < D) Xf_s[p * D + c * 8 + j] = f[j];
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = (f[j] * sx - (float)v[j]) * 2048.0f;
                vl[j] = cvt<E>(d == d && __builtin_fabsf(d) < 3.0e38f ? d : 0.0f);
            }
        }
        *(bf16x8*)((char*)Xb_s + (p * dp + c * 8) * 2) = v;
        if (Xl_s != nullptr) *(bf16x8*)((char*)Xl_s + (p * dp + c * 8) * 2) = vl;   // (allocated when the refinement first engages)
    }
    if (lane == 0) {
        const float nanv = __builtin_nanf("");
        xsq_s[p] = r >= 0 ? xsq[r] : nanv;
        xerr_s[p] = r >= 0 ? xerr[r] : nanv;
    }
}

// a positive float32 rounded UP to a NORMAL IEEE half (what one MFMA operand can carry of it without ever reading less):
// at least 2^-14 (an MFMA that flushes subnormal inputs would read 0 below that), +inf beyond 65504, NaN stays NaN
__device__ __forceinline__ float up_to_half(float v) {
    if (!(v == v)) return v;
    if (v > 65504.0f) return __builtin_inff();
    if (v < 0x1p-14f) return 0x1p-14f;
    const _Float16 hv = (_Float16)v;                         // round to nearest even
    float f = (float)hv;
    if (f < v) f = (float)__builtin_bit_cast(_Float16, (unsigned short)(__builtin_bit_cast(unsigned short, hv) + 1));   // next half up
    return f;
}

// ---- the plan's threshold P as three MFMA operands (SOM_EXACT_PLAN_FOLD) -----------------------------------------------------
// The rows' side of the extra feature step carries P beside bx: three values p1, p2, p3 of the operand type and ONE power of two c
// per launch and level on the centroids' side (-c in three slots), so that the step subtracts P~ = c (p1 + p2 + p3) from every
// accumulator and the tile's test is the SIGN of what is left.  Each product -c p_i is exact (c a power of two), and
//   P~ >= nextup(P) > P   in real arithmetic:  t = nextup(P) / c exactly, p1 = rn(t), p2 = rn(t - p1), p3 = up(t - p1 - p2)
// (both differences are exact: a float32 less its rounding to fewer bits), a part that would be subnormal in the operand type is
// left out of its rounding step and the LAST part rounds the whole remainder UP -- to the smallest normal value where that
// remainder is positive and below it (an MFMA that flushes subnormal operands would read 0).  P~ <= P + |P| 2^-19 + c MINN.
// nextup: an accumulator EQUAL to P reads "needed" in the test against P (!(acc > P)); acc - P~ is then negative.
// P = +inf (the row needs everything) and a NaN: p1 = +inf; P = -inf (a row behind the pass): p1 = -inf; t beyond the operand
// type's range: p1 = +inf above it (see plan_fold_scale: such a P is above every accumulator), the largest negative value below.
struct PlanParts { float p1, p2, p3; };
template <class EL> struct PlanPartFmt;
template <> struct PlanPartFmt<F16> {                       // IEEE half: 11 significant bits, normal from 2^-14, c within its normal powers of two
    static constexpr int M = 10, CMIN = -14, CMAX = 15;
    static constexpr float MINN = 0x1p-14f, MAXV = 65504.0f;
};
// (no kernel behind this one: the plan kernels are built for ExactEl = F16 alone; som_debug_plan_split runs the split on the host)
template <> struct PlanPartFmt<Bf16> {                      // bfloat16: 8 significant bits, float32's exponents
    static constexpr int M = 7, CMIN = -100, CMAX = 100;
    static constexpr float MINN = 0x1p-126f, MAXV = 0x1.FEp127f;
};
// a float32 rounded to M + 1 significant bits: to nearest even, or UP (towards +inf); v normal in the narrower type or zero
__host__ __device__ inline float plan_part_round(float v, int M, bool up) {
    uint32_t b = __builtin_bit_cast(uint32_t, v);
    const int sh = 23 - M;
    const uint32_t low = (1u << sh) - 1u;
    if (up) { if ((b >> 31) == 0u) b += low; }               // (a negative value is cut towards zero: up)
    else b += (low >> 1) + ((b >> sh) & 1u);
    b &= ~low;
    return __builtin_bit_cast(float, b);
}
// c, once per launch and level, from the level's scales: the power of two with 65504 c >= 1.01 S'Bm' (< 2.02 S'Bm'; clamped to the
// operand type's powers of two).  Every accumulator is at most S'Bm' (d'_c <= S'(2 B' + |c|^2 / 2), less positive terms), so a finite P
// beyond 65504 c keeps every block whatever it is compared with: +inf says the same.  ANY power of two is safe (P~ >= P).
template <class EL>
__host__ __device__ inline float plan_fold_scale(float s_bmag) {
    using F = PlanPartFmt<EL>;
    const float m = s_bmag * (1.01f / 65504.0f);
    if (!(m > 0.0f) || !(m < 3.0e38f)) return 1.0f;
    const uint32_t b = __builtin_bit_cast(uint32_t, m);
    int e = (int)(b >> 23) - 127 + ((b & 0x7FFFFFu) != 0u ? 1 : 0);
    e = e > F::CMAX ? F::CMAX : e < F::CMIN ? F::CMIN : e;
    return __builtin_bit_cast(float, (uint32_t)(e + 127) << 23);
}
template <class EL>
__host__ __device__ inline PlanParts plan_split_threshold(float P, float c) {
    using F = PlanPartFmt<EL>;
    const float inf = __builtin_inff();
    if (!(P == P) || P == inf) return PlanParts{inf, 0.0f, 0.0f};
    if (P == -inf) return PlanParts{-inf, 0.0f, 0.0f};
    {                                                        // one float32 step up
        uint32_t b = __builtin_bit_cast(uint32_t, P);
        if ((b << 1) == 0u) b = 1u; else b = (b >> 31) == 0u ? b + 1u : b - 1u;
        P = __builtin_bit_cast(float, b);
        if (P == inf) return PlanParts{inf, 0.0f, 0.0f};
    }
    const float rc = __builtin_bit_cast(float, (uint32_t)(254 - (int)(__builtin_bit_cast(uint32_t, c) >> 23)) << 23);   // 1 / c
    const float t = P * rc;                                  // (exact unless it leaves float32's normal range: the two lines below)
    if (P > 0.0f && !(t >= F::MINN)) return PlanParts{0.0f, 0.0f, F::MINN};
    if (P <= 0.0f && !(t <= -F::MINN)) return PlanParts{0.0f, 0.0f, 0.0f};
    if (!(t < 3.0e38f)) return PlanParts{inf, 0.0f, 0.0f};
    PlanParts o;
    o.p1 = plan_part_round(t, F::M, false);
    if (o.p1 > F::MAXV) return PlanParts{inf, 0.0f, 0.0f};
    if (o.p1 < -F::MAXV) return PlanParts{-F::MAXV, 0.0f, 0.0f};
    const float r1 = t - o.p1;
    o.p2 = plan_part_round(r1, F::M, false);
    if (__builtin_fabsf(o.p2) < F::MINN) o.p2 = 0.0f;
    const float r2 = r1 - o.p2;
    if (r2 > 0.0f) o.p3 = r2 < F::MINN ? F::MINN : plan_part_round(r2, F::M, true);
    else {
        o.p3 = plan_part_round(r2, F::M, true);
        if (__builtin_fabsf(o.p3) < F::MINN) o.p3 = 0.0f;
    }
    return o;
}

// OR of a value over the sixteen lanes of its DPP row (a quad of the MFMA layout: lanes 16 q .. 16 q + 15), in every lane of the
// row: four rotations inside the row, no LDS, no scalar unit
__device__ __forceinline__ uint32_t row16_or(uint32_t v) {
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xF, 0xF, false);   // row_ror:1
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xF, 0xF, false);   // row_ror:2
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false);   // row_ror:4
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);   // row_ror:8
    return v;
}

// The test of the plan, arranged so that the MFMA evaluates all of it but one comparison per (row, centroid):
//   skip  <=>  d'_c > A(row) + hS (sU(row) + r_c)^2  =  [A + hS sU^2] + hS r_c^2 + 2 hS sU r_c
//         <=>  (d'_c - hS r_c^2) - (sx sU (1 + 2^-10)) (sw r_c)  >  P(row) := A + hS sU^2,        2 hS = S (1 + 2^-10), S = sx sw.
// hS r_c^2 leaves the initial accumulator, the cross term is ONE more feature: the rows carry up_to_half(sx sU (1 + 2^-10)), the
// centroids -up_to_half(sw r_c) -- both rounded up, so the product the MFMA forms is never below the real one (the test errs
// towards "needed") -- in the first slot of an extra 32-feature step.
// The centroid stage images of both levels in one launch (a wave per 16-slot MFMA tile; the tiles of level 1 first): the
// fragments of -c~ as prep_w_exact_k16_kernel lays out the units' (scaled by the codebook's power of two; the measured rounding
// error's maximum into cmax2[1]), and the stage's tail: [0, 64) floats: initial accumulators S'(B' + |c|^2 / 2) - hS r^2,
// [64, 128): -up_to_half(sw r) (an empty slot: +inf and 0: never needed; a NaN radius: NaN: always needed).
// (the body, for block `bid` of 256 threads: shared with exact_prep_images_kernel below)
template <int KS32, class EL>
__device__ __forceinline__ void exact_centroid_image_body(const unsigned bid, const CentroidLevel& l1, char* __restrict__ Cst1, int n_cstages1,
                                                          const CentroidLevel& l2, char* __restrict__ Cst2, int n_cstages2, int D,
                                                          const float* __restrict__ xmax2, const float* __restrict__ wmax2,
                                                          char* __restrict__ Cst1_plain) {
    using E = typename EL::T;
    using bf16x8 = typename V8<E>::t;
    constexpr int STAGE = k16_stage_bytes(KS32);
    const int lane = threadIdx.x & 63;
    long tile = (long)bid * 4 + (threadIdx.x >> 6);
    const long t1 = (long)n_cstages1 * K16_T;
    const bool second = tile >= t1;
    if (second) tile -= t1;
    if (tile >= (long)(second ? n_cstages2 : n_cstages1) * K16_T) return;
    const CentroidLevel& lv = second ? l2 : l1;
    char* Cst = second ? Cst2 : Cst1;
    const long stage = tile / K16_T;
    const int t16 = (int)(tile - stage * K16_T);
    const long slot = stage * K16_STAGE_UNITS + t16 * 16 + (lane & 15);
    const float sw = ex_scale(*wmax2), sx = ex_scale(*xmax2);
    float er = 0.0f;
#pragma unroll
    for (int ks = 0; ks < KS32; ++ks) {
        const int k0 = ks * 32 + (lane >> 4) * 8;
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float f = (slot < lv.n_slots && k0 + j < D) ? lv.C[slot * D + k0 + j] * sw : 0.0f;
            const E hb = cvt<E>(-f);
            v[j] = hb;
            const float e = half_operand_error(-f, (float)hb);
            er = __builtin_fmaf(e, e, er);
        }
        *(bf16x8*)(Cst + stage * STAGE + ((long)(t16 * KS32 + ks) * 64 + lane) * 16) = v;
        if (!second && Cst1_plain != nullptr) *(bf16x8*)(Cst1_plain + stage * STAGE + ((long)(t16 * KS32 + ks) * 64 + lane) * 16) = v;
    }
    er += __shfl_xor(er, 16, 64);                            // the centroid's four feature quarters
    er += __shfl_xor(er, 32, 64);
    float m = (er == er) ? er : 0.0f;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) atomic_max_pos_f32(lv.cmax2 + 1, m);
    if (lane < 16) {
        float* tail = (float*)(Cst + (stage + 1) * (long)STAGE - 1024);
        const int within = t16 * 16 + lane;
        const float rad = slot < lv.n_slots ? lv.rg[slot] : -1.0f;
        // (the scout's copy of the level-1 image: the plain screen value of the centroid, S'(B' + |c|^2 / 2) -- nearest centroid)
        float* ptail = (!second && Cst1_plain != nullptr) ? (float*)(Cst1_plain + (stage + 1) * (long)STAGE - 1024) : nullptr;
        if (rad < 0.0f) { tail[within] = __builtin_inff(); tail[64 + within] = 0.0f; if (ptail) ptail[within] = __builtin_inff(); }
        else {
            const float big = __builtin_sqrtf(*wmax2) * __builtin_sqrtf(*xmax2) * (1.0f + 1.0f / 1024.0f);   // (ex_scales: B')
            const float S = sx * sw, hS = 0.5f * S * (1.0f + 1.0f / 1024.0f);
            const float s0 = __builtin_fmaf(0.5f * S, lv.csq[slot], S * big);
            tail[within] = s0 - hS * rad * rad * (1.0f + 0x1p-20f);
            tail[64 + within] = -up_to_half(sw * rad);
            if (ptail) ptail[within] = (s0 == s0 && s0 < 3.0e38f) ? s0 : __builtin_inff();
        }
    }
}
template <int KS32, class EL>
__global__ __launch_bounds__(256) void exact_centroid_image_kernel(CentroidLevel l1, char* __restrict__ Cst1, int n_cstages1,
                                                                   CentroidLevel l2, char* __restrict__ Cst2, int n_cstages2, int D,
                                                                   const float* __restrict__ xmax2, const float* __restrict__ wmax2,
                                                                   char* __restrict__ Cst1_plain = nullptr) {
    exact_centroid_image_body<KS32, EL>(blockIdx.x, l1, Cst1, n_cstages1, l2, Cst2, n_cstages2, D, xmax2, wmax2, Cst1_plain);
}

// The preparations a planned launch starts with, in ONE grid: the codebook's 16-bit stage image (prep_w_exact_k16_kernel: the
// first w_blocks blocks), the centroid images of both levels (c_blocks blocks behind them), and the stages' initial
// accumulators with the launch's merge keys (prep_wsqh_kernel, scaled: the blocks behind those).  All read what the merge left
// -- the codebook, its norms and their maximum, the centroids -- and none reads what another writes (the stage image's
// fragments and its last KiB are different bytes).  The one word two of them shared, the centroid levels' error maximum cm[1],
// is zeroed by the fused merge that wrote the centroids (exact_merge_prep_kernel), not here: the centroid blocks add to it
// from their first wave on.
template <int KS32, class EL>
__global__ __launch_bounds__(256) void exact_prep_images_kernel(unsigned w_blocks, unsigned c_blocks, const float* __restrict__ W, int K, int D,
                                                                char* __restrict__ Wst, int n_stages, float* __restrict__ werr2,
                                                                char* __restrict__ Wst_lo, float* __restrict__ cm1, float* __restrict__ cm2,
                                                                CentroidLevel l1, char* __restrict__ Cst1, int n_cstages1,
                                                                CentroidLevel l2, char* __restrict__ Cst2, int n_cstages2,
                                                                const float* __restrict__ xmax2, const float* __restrict__ wmax2,
                                                                char* __restrict__ Cst1_plain, const float* __restrict__ wn,
                                                                int stage_units, unsigned long long* __restrict__ best64, long n_rows) {
    if (blockIdx.x < w_blocks) prep_w_exact_k16_body<KS32, EL>(blockIdx.x, W, K, D, Wst, n_stages, wmax2, werr2, Wst_lo, cm1, cm2, false);
    else if (blockIdx.x < w_blocks + c_blocks)
        exact_centroid_image_body<KS32, EL>(blockIdx.x - w_blocks, l1, Cst1, n_cstages1, l2, Cst2, n_cstages2, D, xmax2, wmax2, Cst1_plain);
    else prep_wsqh_body(blockIdx.x - w_blocks - c_blocks, wn, K, wmax2, xmax2, Wst, n_stages, k16_stage_bytes(KS32), stage_units, best64, n_rows, 1);
}

// The pieces below are shared by exact_plan_kernel (one level a launch) and exact_plan_fused_kernel (both levels and the lists in
// one launch): the prologue's arithmetic, the two walks and the lists are written once, so that both paths issue the same tests
// on the same operands.
//
// PROLOGUE, level 1's part for one row of the pass: the screen's value v_u of the row's last BMU on the operands the screen reads,
// from it the screen's seed (seed_s, stored by the quad's first lanes) and sqrt(U) (returned; +inf: the row needs everything).
template <int KS32, class EL>
__device__ __forceinline__ float plan_row_seed(const typename V8<typename EL::T>::t (&xrow)[KS32], long row, float q, float xe,
                                               const ExactBound& eb, const ExactScales& sw, const char* __restrict__ Wst,
                                               const int* __restrict__ lastpos, const int* __restrict__ lastpos2,
                                               int* __restrict__ scout_wins, float* __restrict__ seed_s, int force_all) {
    using bf16x8 = typename V8<typename EL::T>::t;
    constexpr int STAGE = k16_stage_bytes(KS32);
    const int lane = threadIdx.x & 63, quad = lane >> 4;
    // v_u: the screen's value of unit u = the row's last BMU on the operands the screen reads (-w~ fragments of
    // the stage image, the row's x~), a float32 fma chain: every product of two halves is exact, the chain and
    // the two cross-quad adds err by < 40 ulps of the largest accumulator magnitude (charged: e_valu)
    // (lastpos2: a second unit per row -- the scout's pick beside the real last BMU --: the smaller value bounds as well)
    auto value_of = [&](int pos) -> float {           // (a position below K: exact_lastpos_kernel, exact_scout_pos_kernel)
        const char* stg = Wst + (long)(pos >> 6) * STAGE;
        const int t16 = (pos >> 4) & 3, c = pos & 15;
        float d = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS32; ++ks) {
            const bf16x8 a = *(const bf16x8*)(stg + ((t16 * KS32 + ks) * 64 + quad * 16 + c) * 16);
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) d = __builtin_fmaf((float)a[jj], (float)xrow[ks][jj], d);
        }
        d += __shfl_xor(d, 16, 64);
        d += __shfl_xor(d, 32, 64);
        return *(const float*)(stg + K16_T * KS32 * 1024 + (t16 * 16 + c) * 4) + d;
    };
    float vu = value_of(lastpos[row]);
    if (lastpos2 != nullptr) {
        // (lastpos: the scout's pick, lastpos2: the real last BMU.  A WIN of the scout: its unit's squared distance --
        //  |x|^2 + tau(v), tau(v) = 2 (v / S - B) -- is a tenth or more below the last BMU's: counted, so that the host
        //  knows whether the scout is still worth its launches next epoch)
        const float v2 = value_of(lastpos2[row]);
        const float Sq = sw.sx * sw.sw;
        const float ua = q + 2.0f * (vu / Sq - sw.big), ub = q + 2.0f * (v2 / Sq - sw.big);
        const bool win = ua < 0.9f * ub;
        const unsigned long long wm = __ballot(win && quad == 0);
        if (scout_wins != nullptr && lane == __builtin_ctzll(__ballot(true)) && wm != 0ull) atomicAdd(scout_wins, (int)__popcll(wm));
        vu = (v2 < vu || !(vu == vu)) ? v2 : vu;      // (a NaN value -- a NaN unit -- gives way to the other unit's)
    }
    const float Sw = sw.sx * sw.sw;
    const float e = ex_row_bound(eb, sw, q, xe);          // two-unit window E of the screen (d' units)
    const float f32s = ex_f32_share(eb, sw, q);           // its float32 share (two evaluations)
    const float e_valu = 48.0f * 0x1p-24f * Sw * sw.bmag;
    // seed: whatever beats u in the float32 kernel has a screen value of at most v_u + E + e_valu = seed + f32s
    const float sd = vu + (e - f32s) * (1.0f + 1.0f / 1024.0f) + e_valu + Sw * sw.bmag * 0x1p-21f;
    if (quad == 0) seed_s[row] = (sd > 0.0f && sd < 3.0e38f) ? sd : __builtin_inff();
    // tau_up >= u's real score: d'_real(u) <= v_u + (one-unit screen error) + e_valu,  tau = 2 (d' / S - B)
    const float e_one = 0.5f * (e - f32s) * (1.0f + 1.0f / 1024.0f) + e_valu;
    const float tau_up = 2.0f * (((vu + e_one) - Sw * sw.big) / Sw) + 0x1p-20f * (sw.big + __builtin_fabsf(vu) / Sw);
    const float xn = __builtin_sqrtf(q) * (1.0f + 1.0f / 1024.0f);
    const float share = 2.0f * (eb.cA * xn * sw.wm + eb.cW * sw.wm * sw.wm);      // tau units, one float32 window
    // (no fmax here: it would swallow the NaN of a row whose last BMU is a NaN unit, and bound that row by zero)
    const float U0 = q * (1.0f + 1.0f / 1024.0f) + tau_up + share * (1.0f + 1.0f / 1024.0f) + 0x1p-18f * (q + __builtin_fabsf(tau_up));
    const float U = U0 < 0.0f ? 0.0f : U0;
    float su = __builtin_sqrtf(U) * (1.0f + 1.0f / 1024.0f);
    if (force_all || !(su == su) || !(su < 3.0e38f) || !(e == e)) su = __builtin_inff();
    return su;
}

// PROLOGUE, one level's part for one row: the right-hand side P of the level's test and the rows' side bx of the extra feature
// step, from |x|^2, the row's rounding error, sqrt(U) and the level's scales (sc: ex_scales on the level's centroid image).
// in_pass == false (a row behind the pass) needs nothing: P = -inf; a row whose numbers are not finite needs everything: P = +inf.
// FOLD: P enters the accumulator in the extra step (plan_extra_step, plan_run_tile): that step's sum then reaches 2 S'Bm' + |P~|,
// |P~| <= 65504 c < 2.02 S'Bm' for every P that can decide a test (plan_fold_scale), 2.01 times what the charge below assumes for
// ONE of the KS32 + 1 MFMAs (24 ulps of S'Bm' each): + 24.3 ulps, rounded up to + 28.
template <int KS32, bool FOLD>
__device__ __forceinline__ void plan_row_threshold(const ExactBound& eb, const ExactScales& sc, bool in_pass, float q, float xe, float su,
                                                   float& P, float& bx) {
    const float S = sc.sx * sc.sw;
    float A = -__builtin_inff(), sU = 0.0f;
    if (in_pass) {
        const float ec = 0.5f * ex_row_bound(eb, sc, q, xe) * (1.0f + 1.0f / 1024.0f);
        sU = su;
        // d'_c > S' (B' + ((sU + r)^2 - |x|^2_lo) / 2) + e_c   <=>   skip
        // (+ margins: the float32 rounding of this line, and |c|^2 as float32 summed it against the real |c|^2)
        A = S * sc.big + ec - 0.5f * S * q * (1.0f - 1.0f / 1024.0f) + 0x1p-12f * S * (sc.big + q) + 0x1p-16f * S * sc.wm * sc.wm;
        if (!(A == A) || !(A < 3.0e38f) || !(su < 3.0e38f)) {
            A = __builtin_inff(); sU = 0.0f;                                                 // need everything
        }
    }
    // P = A + hS sU^2 (+ the extra feature step's and the larger accumulators' share of the MFMA rounding: the cross term
    // can double the accumulator's magnitude, and there is one more MFMA in the chain: 4 (KS32 + 1) x 6 ulps of S' Bm')
    bx = up_to_half(sc.sx * sU * (1.0f + 1.0f / 1024.0f));
    P = A + 0.5f * S * (1.0f + 1.0f / 1024.0f) * sU * sU * (1.0f + 0x1p-20f) + (float)(24 * (KS32 + 1) + (FOLD ? 28 : 0)) * 0x1p-23f * S * sc.bmag;
    if (!(bx < 3.0e38f) || !(P == P)) P = __builtin_inff();                                  // (sU beyond the half range: need everything)
    if (A == -__builtin_inff()) P = -__builtin_inff();                                       // (rows behind the pass)
}
// the rows' operand of the extra feature step: slot 0 of the first quad = bx, FOLD: its slots 1..3 = the parts of P under the
// level's scale c (plan_split_threshold), else 0
template <class EL, bool FOLD>
__device__ __forceinline__ typename V8<typename EL::T>::t plan_extra_step(float bx, float P, float c) {
    using E = typename EL::T;
    typename V8<E>::t v;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) v[jj] = (E)0.0f;
    if (((threadIdx.x & 63) >> 4) == 0) {
        if (bx < 3.0e38f) v[0] = (E)bx;
        if constexpr (FOLD) {
            const PlanParts pp = plan_split_threshold<EL>(P, c);
            v[1] = (E)pp.p1; v[2] = (E)pp.p2; v[3] = (E)pp.p3;      // (exact: the parts are values of the operand type)
        }
    }
    return v;
}
// what the walks hand every tile beside its operands: the thresholds of the wave's four sample blocks (FOLD: unused, the
// registers are free) and -c of the level (FOLD: the centroids' side of slots 1..3)
template <class EL>
struct PlanTest {
    float P[K16_SB];
    typename EL::T negc;
};

// MFMAs + test of one 16-centroid tile (either level; its operands in (a, wv, rneg): the KS32 fragments, the initial
// accumulators, the centroids' side of the extra step, slot 0 = -up_to_half(sw r)): lane (quad, col) sets bit 4 j + r of
// lane_bits where one of its rows needs the centroid behind accumulator register r of tile j.
// FOLD: the extra step also subtracts P~ >= P (the rows' slots 1..3 times -c), and a row needs the centroid iff what is left is
// not above zero: negative, or a NaN (a NaN centroid, a row that needs everything and an empty slot: +inf - inf).  Read on the
// accumulators' BIT PATTERNS, as unsigned integers: exactly the patterns above +inf's -- every value with the sign bit set and
// every positive NaN -- say "needed", so one unsigned maximum over the four sample blocks (v_max3_u32 + v_max_u32) and one
// compare serve a register, with no NaN rule of a floating-point minimum to rely on (and none of the canonicalising
// instructions the compiler puts in front of one).  +0 (acc == P~ > P) is not needed; -0 would read "needed": the safe side.
template <int KS32, class EL, bool FOLD>
__device__ __forceinline__ void plan_run_tile(int j, const typename V8<typename EL::T>::t (&a)[KS32], const f32x4& wv, float rneg,
                                              const typename V8<typename EL::T>::t (&xf)[K16_SB][KS32],
                                              const typename V8<typename EL::T>::t (&xe)[K16_SB], const PlanTest<EL>& pt,
                                              uint32_t& lane_bits) {
    using E = typename EL::T;
    using bf16x8 = typename V8<E>::t;
    const float (&P)[K16_SB] = pt.P;
    bf16x8 ae;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) ae[jj] = (E)0.0f;
    if (((threadIdx.x & 63) >> 4) == 0) {
        ae[0] = (E)rneg;
        if constexpr (FOLD) { ae[1] = pt.negc; ae[2] = pt.negc; ae[3] = pt.negc; }
    }
    f32x4 acc[K16_SB];
#pragma unroll
    for (int sb = 0; sb < K16_SB; ++sb) acc[sb] = wv;
#pragma unroll
    for (int ks = 0; ks < KS32; ++ks)
#pragma unroll
        for (int sb = 0; sb < K16_SB; ++sb) acc[sb] = mfma16(a[ks], xf[sb][ks], acc[sb]);
#pragma unroll
    for (int sb = 0; sb < K16_SB; ++sb) acc[sb] = mfma16(ae, xe[sb], acc[sb]);
    // (gathered over the rows once per stage / chunk by the caller -- a ballot and four scalar tests per accumulator register
    //  kept the scalar unit busier than the matrix pipe)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if constexpr (FOLD) {
            // (__float_as_uint takes the element BY VALUE: a bit cast of the vector element expression itself read element 0)
            uint32_t m = __float_as_uint(acc[0][r]);
#pragma unroll
            for (int sb = 1; sb < K16_SB; ++sb) { const uint32_t u = __float_as_uint(acc[sb][r]); m = u > m ? u : m; }
            lane_bits |= m > 0x7F800000u ? (1u << (4 * j + r)) : 0u;
        } else {
            bool nd = false;
#pragma unroll
            for (int sb = 0; sb < K16_SB; ++sb) nd = nd || !(acc[sb][r] > P[sb]);
            lane_bits |= nd ? (1u << (4 * j + r)) : 0u;
        }
    }
}
// a tile's operands out of its stage slot in LDS (st; wq: the slot's tail)
template <int KS32, class EL>
__device__ __forceinline__ void plan_load_tile(const char* st, int t, typename V8<typename EL::T>::t (&a)[KS32], f32x4& wv, float& rneg) {
    using bf16x8 = typename V8<typename EL::T>::t;
    const int lane = threadIdx.x & 63;
    const float* wq = (const float*)(st + K16_T * KS32 * 1024);
#pragma unroll
    for (int ks = 0; ks < KS32; ++ks) a[ks] = *(const bf16x8*)(st + ((t * KS32 + ks) * 64 + lane) * 16);
    wv = *(const f32x4*)(wq + t * 16 + 4 * (lane >> 4));
    rneg = wq[64 + t * 16 + (lane & 15)];
}

// LEVEL 1's WALK over the centroid stages [s_begin, s_end) of Cst, double-buffered in the two stage slots at smem: word
// nl[s - s_begin] (LDS, zero on entry -- the first barrier of the walk orders the clearing) collects the tile's need bits of stage s
// (bit i <-> centroid slot 64 s + i).  The caller's barrier behind the walk completes the words.
template <int KS32, class EL, bool FOLD>
__device__ __forceinline__ void plan_walk_level1(const char* __restrict__ Cst, int s_begin, int s_end, char* smem, unsigned long long* nl,
                                                 const typename V8<typename EL::T>::t (&xf)[K16_SB][KS32],
                                                 const typename V8<typename EL::T>::t (&xe)[K16_SB], const PlanTest<EL>& P) {
    using bf16x8 = typename V8<typename EL::T>::t;
    constexpr int STAGE = k16_stage_bytes(KS32);
    constexpr int PIECES = K16_T * KS32 + 1;
    const int lane = threadIdx.x & 63, quad = lane >> 4, col = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    auto dma_stage = [&](int s, char* dst) {
        const char* src = Cst + (long)s * STAGE;
        for (int p = wave; p < PIECES; p += K16_NW) lds_dma_16(src + (long)p * 1024 + lane * 16, dst + p * 1024);
    };
    if (s_begin < s_end) dma_stage(s_begin, smem);
    for (int i = s_begin; i < s_end; ++i) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (i + 1 < s_end) dma_stage(i + 1, smem + ((i + 1 - s_begin) & 1) * STAGE);
        const char* st = smem + ((i - s_begin) & 1) * STAGE;
        uint32_t lane_bits = 0u;                              // (the word's bit 16 t16 + 4 quad + r <-> centroid slot of that place in the stage)
        // the stage's four tiles, their operands alternating between two register sets (no copies): the next tile's are read
        // under this tile's MFMAs and test
        bf16x8 aA[KS32], aB[KS32];
        f32x4 wvA, wvB;
        float rnA, rnB;
        plan_load_tile<KS32, EL>(st, 0, aA, wvA, rnA);
        plan_load_tile<KS32, EL>(st, 1, aB, wvB, rnB);
        plan_run_tile<KS32, EL, FOLD>(0, aA, wvA, rnA, xf, xe, P, lane_bits);
        plan_load_tile<KS32, EL>(st, 2, aA, wvA, rnA);
        plan_run_tile<KS32, EL, FOLD>(1, aB, wvB, rnB, xf, xe, P, lane_bits);
        plan_load_tile<KS32, EL>(st, 3, aB, wvB, rnB);
        plan_run_tile<KS32, EL, FOLD>(2, aA, wvA, rnA, xf, xe, P, lane_bits);
        plan_run_tile<KS32, EL, FOLD>(3, aB, wvB, rnB, xf, xe, P, lane_bits);
        // OR over the sixteen rows of every quad; the quad's first lane spreads its four nibbles (one per tile) to their places
        const uint32_t any_row = row16_or(lane_bits);
        if (col == 0 && any_row != 0u) {
            const uint32_t lo = ((any_row & 15u) | (((any_row >> 4) & 15u) << 16)) << (4 * quad);
            const uint32_t hi = (((any_row >> 8) & 15u) | (((any_row >> 12) & 15u) << 16)) << (4 * quad);
            atomicOr(nl + (i - s_begin), ((unsigned long long)hi << 32) | lo);
        }
    }
}

// LEVEL 2's LIST: the groups level 1 kept for this tile (need1: the tile's n_cstages1 level-1 words, in LDS or in memory), dense and
// ascending in act[]; their number in *act_n.  Called by one wave; the caller's barrier publishes the list.
// (n_slots2: the slots of the level-2 image -- a group behind them has no sub-blocks to test)
__device__ __forceinline__ void plan_level2_list(const unsigned long long* need1, int n_cstages1, int n_slots2, int* act, int* act_n) {
    const int lane = threadIdx.x & 63;
    int cnt = 0;
    for (int s1 = 0; s1 < n_cstages1; ++s1) {
        const unsigned long long w = need1[s1];
        const int g = s1 * 64 + lane;
        const bool on = ((w >> lane) & 1ull) && 4 * (g >> 2) * 4 < n_slots2;
        const unsigned long long mk = __ballot(on);
        if (on) act[cnt + __popcll(mk & ((1ull << lane) - 1ull))] = g;
        cnt += __popcll(mk);
    }
    if (lane == 0) *act_n = cnt;
}

// LEVEL 2's WALK over the entries [b0, e0) of the DENSE list act[] of kept groups, sixteen to a barrier: four MFMA tiles of four
// groups' sub-blocks each, GATHERED -- late in a schedule a quarter of the groups is kept, spread so evenly that nearly every tile
// of four consecutive groups holds one: walking image tiles ran four times level 1's work to test a quarter of it.
// A tile's fragments come by LDS-DMA with per-lane addresses (lane (quad, c) <-> sub-block c & 3 of the tile's
// (c >> 2)-th group), its initial accumulators and radii by plain loads one chunk ahead (a wave per tile), written
// into the slot's tail (laid out like a stage's) before the next barrier.
// nl (LDS, zero on entry, ordered by a barrier of the caller's): word g >> 4 collects a nibble per group (bit 4 (g & 15) + sub <->
// sub-block `sub` of group g), filed by LDS atomics.  The caller's barrier behind the walk completes the words.
template <int KS32, class EL, bool FOLD>
__device__ __forceinline__ void plan_walk_level2(const char* __restrict__ Cst, const int* act, int b0, int e0, char* smem,
                                                 unsigned long long* nl, const typename V8<typename EL::T>::t (&xf)[K16_SB][KS32],
                                                 const typename V8<typename EL::T>::t (&xe)[K16_SB], const PlanTest<EL>& P) {
    using bf16x8 = typename V8<typename EL::T>::t;
    constexpr int STAGE = k16_stage_bytes(KS32);
    static_assert(K16_NW == 4, "a wave per tile fills the slot's tail");
    const int lane = threadIdx.x & 63, quad = lane >> 4, col = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int TQ = K16_T * KS32 * 1024;              // the slot's tail: [0, 64) initial accumulators, [64, 128) -up_to_half(sw r)
    // where sub-block `sub` of group g sits in the level-2 image: stage g >> 4, tile (g >> 2) & 3, row 4 (g & 3) + sub
    auto frag_of = [&](int g, int sub, int ks, int q) -> const char* {
        return Cst + (long)(g >> 4) * STAGE + (((((g >> 2) & 3) * KS32 + ks) * 64 + q * 16 + 4 * (g & 3) + sub) * 16);
    };
    auto dma_chunk = [&](int c0, char* dst) {
        for (int p = wave; p < K16_T * KS32; p += K16_NW) {
            const int j = p / KS32, ks = p - j * KS32;
            if (c0 + 4 * j < e0) {                        // (wave-uniform)
                const int gi = c0 + 4 * j + (col >> 2);
                const int g = gi < e0 ? act[gi] : act[c0 + 4 * j];   // (a slot behind the list: any valid address; its bits are dropped)
                lds_dma_16(frag_of(g, col & 3, ks, quad), dst + p * 1024);
            }
        }
    };
    // wave w <-> the chunk's tile w: lanes 0..15 its initial accumulators, lanes 16..31 its radii (row i <-> sub-block i & 3 of
    // the tile's (i >> 2)-th group)
    auto load_tail = [&](int c0) -> float {
        const int i = lane & 15, gi = c0 + 4 * wave + (i >> 2);
        if (lane >= 32 || gi >= e0) return lane < 16 ? __builtin_inff() : 0.0f;     // (an empty slot: never needed)
        const int g = act[gi];
        return *(const float*)(Cst + (long)(g >> 4) * STAGE + TQ + (((lane >> 4) * 64) + ((g >> 2) & 3) * 16 + 4 * (g & 3) + (i & 3)) * 4);
    };
    auto store_tail = [&](char* dst, float v) {
        if (lane < 32) *(float*)(dst + TQ + (((lane >> 4) * 64) + wave * 16 + (lane & 15)) * 4) = v;
    };
    if (b0 < e0) { dma_chunk(b0, smem); store_tail(smem, load_tail(b0)); }
    int k = 0;
    for (int c0 = b0; c0 < e0; c0 += 16, ++k) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        char* sn = smem + ((k + 1) & 1) * STAGE;
        float tail_n = 0.0f;
        if (c0 + 16 < e0) { dma_chunk(c0 + 16, sn); tail_n = load_tail(c0 + 16); }
        const char* st = smem + (k & 1) * STAGE;
        uint32_t lane_bits = 0u;                           // bit 4 j + r: tile j of the chunk, accumulator register r
        // (lane (quad, col): bit r <-> its row needs sub-block r of the tile's quad-th group; gathered over the rows
        //  once per chunk, below)
        bf16x8 aA[KS32], aB[KS32];
        f32x4 wvA, wvB;
        float rnA, rnB;
        const bool h1 = c0 + 4 < e0, h2 = c0 + 8 < e0, h3 = c0 + 12 < e0;
        plan_load_tile<KS32, EL>(st, 0, aA, wvA, rnA);
        if (h1) plan_load_tile<KS32, EL>(st, 1, aB, wvB, rnB);
        plan_run_tile<KS32, EL, FOLD>(0, aA, wvA, rnA, xf, xe, P, lane_bits);
        if (h1) {
            if (h2) plan_load_tile<KS32, EL>(st, 2, aA, wvA, rnA);
            plan_run_tile<KS32, EL, FOLD>(1, aB, wvB, rnB, xf, xe, P, lane_bits);
            if (h2) {
                if (h3) plan_load_tile<KS32, EL>(st, 3, aB, wvB, rnB);
                plan_run_tile<KS32, EL, FOLD>(2, aA, wvA, rnA, xf, xe, P, lane_bits);
                if (h3) plan_run_tile<KS32, EL, FOLD>(3, aB, wvB, rnB, xf, xe, P, lane_bits);
            }
        }
        // the chunk's sixteen groups: OR over the sixteen rows of every quad (lanes of one DPP row), then the quad's first lane
        // files tile j's nibble under the tile's quad-th group
        const uint32_t any_row = row16_or(lane_bits);
        if (col == 0 && any_row != 0u) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t nib = (any_row >> (4 * j)) & 15u;
                const int gi = c0 + 4 * j + quad;
                if (nib != 0u && gi < e0) {
                    const int g = act[gi];
                    atomicOr(nl + (g >> 4), (unsigned long long)nib << (4 * (g & 15)));
                }
            }
        }
        if (c0 + 16 < e0) store_tail(sn, tail_n);
    }
}

// The plan: which blocks does a tile of SK_TILE (sorted) rows need?  The resident kernel's MFMA loop over a centroid
// stage image (64 centroids per stage), epilogue: need(row, j) = not (d'_c > A(row) + (S'/2) (sU(row) + r_j)^2), OR over
// the tile's rows into need[tile][stage] (bit i <-> centroid slot 64 stage + i).
//   LEVEL2 == false: the centroids of the groups.  The prologue also forms, per row, the screen value v_u of the row's last
//     BMU u (vector ALU, from the row's half image and u's fragments of the screen's stage image Wst), from it the seed of
//     the screen (seed_s) and sqrt(U) (sU_s: kept for the level-2 LAUNCH -- exact_plan_fused_kernel keeps it in registers and writes
//     no sU_s --; +inf: the row needs everything).  need2_clear (or null): level 2's
//     bitmap [tile][4 n_cstages], whose words of this workgroup's stages are zeroed for the level-2 launch that follows.
//   LEVEL2 == true: the centroids of the 16-unit sub-blocks, slot order as exact_centroid_kernel's (a 16-slot MFMA tile =
//     the sub-blocks of four consecutive groups); only the tiles whose groups level 1 kept (need1) are loaded and run.
// eb / scales: the centroid image's (cmax2 = {max |c|^2, max rounding error^2}); wmax2 / werr2: the codebook's.
// FOLD (SOM_EXACT_PLAN_FOLD, default): the threshold rides in the extra MFMA step and the test is a sign (plan_run_tile); false:
// the compare against P of before, for A/B runs on the same data.
template <int KS32, class EL, bool LEVEL2, bool FOLD>
__global__ __launch_bounds__(64 * K16_NW, LEVEL2 ? 3 : 2) void exact_plan_kernel(const __bf16* __restrict__ Xb, long N,
                                                                    const char* __restrict__ Cst, int n_cstages,
                                                                    const float* __restrict__ rg, int n_slots,
                                                                    const float* __restrict__ xsq, const float* __restrict__ xerr,
                                                                    float* __restrict__ sU_s,
                                                                    const float* __restrict__ xmax2, const float* __restrict__ cmax2,
                                                                    const float* __restrict__ wmax2, const float* __restrict__ werr2,
                                                                    ExactBound eb, unsigned long long* __restrict__ need,
                                                                    const int* __restrict__ lastpos, const char* __restrict__ Wst,
                                                                    float* __restrict__ seed_s,
                                                                    const unsigned long long* __restrict__ need1, int n_cstages1,
                                                                    int force_all, const int* __restrict__ lastpos2 = nullptr,
                                                                    int* __restrict__ scout_wins = nullptr,
                                                                    unsigned long long* __restrict__ need2_clear = nullptr) {
    using bf16x8 = typename V8<typename EL::T>::t;
    constexpr int DP = 32 * KS32;
    constexpr int STAGE = k16_stage_bytes(KS32);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int act_n;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int quad = lane >> 4, col = lane & 15;
    const long wave_s0 = (long)blockIdx.x * K16_WG_SAMPLES + wave * (16 * K16_SB);

    bf16x8 xf[K16_SB][KS32];
    bf16x8 xe[K16_SB];                                       // the extra feature step: slot 0 = up_to_half(sx sU (1 + 2^-10)), FOLD: 1..3 = P's parts, else 0
    PlanTest<EL> pt;
    const ExactScales sc = ex_scales(xmax2, cmax2, cmax2 + 1);
    const ExactScales sw = ex_scales(xmax2, wmax2, werr2);
    const float cf = plan_fold_scale<EL>(sc.sx * sc.sw * sc.bmag);
    pt.negc = (typename EL::T)(-cf);
#pragma unroll
    for (int sb = 0; sb < K16_SB; ++sb) {
        const long row = wave_s0 + sb * 16 + col;
#pragma unroll
        for (int ks = 0; ks < KS32; ++ks) xf[sb][ks] = *(const bf16x8*)(Xb + row * DP + ks * 32 + quad * 8);
        // rows behind the pass need nothing (A = -inf: d' > rhs always); a row whose numbers are not finite needs everything
        float q = 0.0f, xer = 0.0f, su = 0.0f;
        if (row < N) {
            q = xsq[row]; xer = xerr[row];
            if constexpr (!LEVEL2) {
                su = plan_row_seed<KS32, EL>(xf[sb], row, q, xer, eb, sw, Wst, lastpos, lastpos2, scout_wins, seed_s, force_all);
                if (quad == 0) sU_s[row] = su;
            } else {
                su = sU_s[row];
            }
        }
        float bx;
        plan_row_threshold<KS32, FOLD>(eb, sc, row < N, q, xer, su, pt.P[sb], bx);
        xe[sb] = plan_extra_step<EL, FOLD>(bx, pt.P[sb], cf);
    }

    // the words this workgroup produces (one per stage), gathered in LDS with LDS atomics (a global atomic per wave and stage
    // sat in front of the next stage's barrier)
    int* act = (int*)(smem + 2 * STAGE);
    unsigned long long* nl = (unsigned long long*)(smem + 2 * STAGE + (LEVEL2 ? (size_t)n_cstages1 * 64 * sizeof(int) : 0));
    for (int i = tid; i < n_cstages; i += 64 * K16_NW) nl[i] = 0ull;
    if constexpr (LEVEL2) {
        if (wave == 0) plan_level2_list(need1 + (long)blockIdx.x * n_cstages1, n_cstages1, n_slots, act, &act_n);
        __syncthreads();
        const int n_act = act_n;
        const int c_all = (n_act + 15) / 16;
        const int b0 = 16 * (int)((long)c_all * blockIdx.y / gridDim.y);
        const int e0 = min(n_act, 16 * (int)((long)c_all * (blockIdx.y + 1) / gridDim.y));
        plan_walk_level2<KS32, EL, FOLD>(Cst, act, b0, e0, smem, nl, xf, xe, pt);
        __syncthreads();
        // (two parts of a tile's walk may share a stage: OR into words that start from zero -- cleared by the level-1 workgroups, or by the host's fill)
        for (int i = tid; i < n_cstages; i += 64 * K16_NW)
            if (nl[i] != 0ull) atomicOr(need + (long)blockIdx.x * n_cstages + i, nl[i]);
        return;
    }
    // (gridDim.y workgroups share a tile's centroid stages: few tiles -- a batch of 65 536 rows is 256 -- would otherwise be
    //  one workgroup per CU walking all the stages alone)
    const int s_begin = (int)((long)n_cstages * blockIdx.y / gridDim.y);
    const int s_end = (int)((long)n_cstages * (blockIdx.y + 1) / gridDim.y);
    plan_walk_level1<KS32, EL, FOLD>(Cst, s_begin, s_end, smem, nl, xf, xe, pt);
    __syncthreads();
    for (int i = s_begin + tid; i < s_end; i += 64 * K16_NW) need[(long)blockIdx.x * n_cstages + i] = nl[i - s_begin];
    // (level 2 ORs into words that start from zero: the four level-2 words of every stage this workgroup walked are cleared
    //  here, by the workgroup that owns them, instead of by a fill of their own in front of level 2)
    if (need2_clear != nullptr)
        for (int i = 4 * s_begin + tid; i < 4 * s_end; i += 64 * K16_NW) need2_clear[(long)blockIdx.x * 4 * n_cstages + i] = 0ull;
}

// need bitmaps -> per tile the ascending list of items (group << 4 | mask of the group's 16-unit sub-blocks to run), and its
// length.  need1: bit j of word s <-> group 64 s + j (level 1).  need2 (or null: every sub-block of a kept group runs):
// word 4 s + k holds, for the groups 64 s + 16 k .. + 15, a nibble each (bit 4 (g & 15) + sub <-> sub-block `sub` of group g).
// ... and the same blocks as the tile's dense list of 16-unit tiles (tlist / tcnt: what the screen walks; glist / gcnt: what
// the select kernel walks).  One wave per tile; tile_counts[tile] = (16-unit blocks listed, groups level 1 kept).
// tile_ticket[tile] = 0: the arrivals of the tile's parts in the listed screen's select tail (bmu_bf16_k16.hpp) start from zero in
// every pass -- here, where every tile of the pass is visited anyway, not by a fill of their own.
// (PUBLISH: tile_counts[tile] leaves as one 8-byte agent-scope store, written through to memory: another workgroup of the same
//  launch reads it -- exact_lists_totals_kernel)
template <bool PUBLISH>
__device__ __forceinline__ void exact_lists_tile(const long tile, const int lane, const unsigned long long* __restrict__ need1, int n_cstages,
                                                 const unsigned long long* __restrict__ need2, int n_groups,   // (the TILE's own words, in memory or in LDS)
                                                 int* __restrict__ glist, int* __restrict__ gcnt,
                                                 int2* tile_counts, int* __restrict__ tlist,
                                                 int* __restrict__ tcnt, int* __restrict__ tile_ticket) {
    const unsigned long long below = (1ull << lane) - 1ull;
    int base = 0, blk = 0, kept = 0;
    for (int s0 = 0; s0 < n_cstages; s0 += 64) {
        // (the tile's level-1 words in one load, lane <-> stage; then stage by stage out of registers)
        const unsigned long long mine = s0 + lane < n_cstages ? need1[s0 + lane] : 0ull;
        const uint32_t lo = (uint32_t)mine, hi = (uint32_t)(mine >> 32);
        unsigned long long todo = __ballot(mine != 0ull);
        for (; todo != 0ull; todo &= todo - 1ull) {
            const int sl = (int)__builtin_ctzll(todo), s = s0 + sl;
            const unsigned long long w = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)hi, sl) << 32) |
                                         (uint32_t)__builtin_amdgcn_readlane((int)lo, sl);
            uint32_t nib = 15u;
            if (need2 != nullptr) nib = (uint32_t)(need2[4 * s + (lane >> 4)] >> (4 * (lane & 15))) & 15u;
            const int g = s * 64 + lane;
            const bool l1 = ((w >> lane) & 1ull) && g < n_groups;
            const bool on = l1 && nib != 0u;
            const unsigned long long mk = __ballot(on);
            if (on) glist[tile * n_groups + base + __popcll(mk & ((1ull << lane) - 1ull))] = (g << 4) | (int)nib;
            base += __popcll(mk);
            kept += __popcll(__ballot(l1));
            // the same blocks as a DENSE list of 16-unit tiles (group << 2 | sub-block), ascending: what the screen walks, four
            // to a barrier, whatever group they belong to
            int before = 0, total = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const unsigned long long mb = __ballot(on && ((nib >> b) & 1u));
                before += __popcll(mb & below);
                total += __popcll(mb);
            }
            if (on) {
                int o = blk + before;
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if ((nib >> b) & 1u) tlist[tile * 4 * n_groups + o++] = (g << 2) | b;
            }
            blk += total;
        }
    }
    // (per tile: 4 096 waves adding into two words of one cache line took as long as the rest of this kernel)
    if (lane == 0) {
        gcnt[tile] = base; tcnt[tile] = blk;
        tile_ticket[tile] = 0;
        if (PUBLISH)
            __hip_atomic_store((unsigned long long*)(tile_counts + tile), ((unsigned long long)(uint32_t)kept << 32) | (uint32_t)blk,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else tile_counts[tile] = make_int2(blk, kept);
    }
}
__global__ __launch_bounds__(64) void exact_lists_kernel(const unsigned long long* __restrict__ need1, int n_cstages,
                                                         const unsigned long long* __restrict__ need2, int n_groups,
                                                         int* __restrict__ glist, int* __restrict__ gcnt,
                                                         int2* __restrict__ tile_counts, int* __restrict__ tlist,
                                                         int* __restrict__ tcnt, int* __restrict__ tile_ticket) {
    exact_lists_tile<false>(blockIdx.x, threadIdx.x, need1 + (long)blockIdx.x * n_cstages, n_cstages,
                            need2 != nullptr ? need2 + (long)blockIdx.x * 4 * n_cstages : nullptr, n_groups, glist, gcnt, tile_counts, tlist, tcnt, tile_ticket);
}

// sum of the tiles' (16-unit blocks listed, groups level 1 kept) into the pass's counters.  One workgroup.
// items != nullptr: ... and the listed screen's WORK ITEMS (bmu_bf16_k16_kernel<.., GM, TL>): every tile's list cut into parts of
// about L blocks -- L = len_pct % of the mean list (1.25 x), or what gives every slot of the chip two items where the tiles are few; never below
// 32 blocks (a part re-reads its tile's 64 KB of rows) --, item = (tile, part | parts << 16) in tile order; the queue's counter reset.
// At most tiles + max(100 / len_pct tiles, 2.1 slots) items (the three cases of L): with len_pct >= 25, within 5 tiles + 4 slots.
// (the body, for a workgroup of NT threads -- what it writes does not depend on NT: integer sums, and items in tile order --;
//  sb, sk: NT / 64 ints of LDS each, tot_b: one)
template <int NT>
__device__ __forceinline__ void exact_list_totals_body(const int2* tile_counts, long tiles, int* __restrict__ blocks_run,
                                                       int* __restrict__ groups_run, int slots, int2* __restrict__ items,
                                                       int* __restrict__ n_items, int* __restrict__ item_ctr, int len_pct,
                                                       int* sb, int* sk, int& tot_b) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b = 0, k = 0;
    for (long t = tid; t < tiles; t += NT) { const int2 c = tile_counts[t]; b += c.x; k += c.y; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { b += __shfl_xor(b, o, 64); k += __shfl_xor(k, o, 64); }
    if (lane == 0) { sb[wave] = b; sk[wave] = k; }
    __syncthreads();
    if (tid == 0) {
        b = 0; k = 0;
        for (int w = 0; w < NT / 64; ++w) { b += sb[w]; k += sk[w]; }
        *blocks_run = b; *groups_run = k;
        tot_b = b;
    }
    if (items == nullptr) return;
    __syncthreads();
    const long total = tot_b;
    const long by_mean = (len_pct * total) / (100 * (tiles > 0 ? tiles : 1)) + 1, by_slots = total / (2 * (long)(slots > 0 ? slots : 1));
    const int L = (int)max(32L, min(by_mean, by_slots));
    auto parts_of = [&](int cnt) -> int { return cnt <= L ? 1 : (cnt + L - 1) / L; };
    // a contiguous run of tiles per thread; exclusive scan of the runs' item counts over the NT threads
    const long per = (tiles + NT - 1) / NT, t_b = min((long)tid * per, tiles), t_e = min(t_b + per, tiles);
    int mine = 0;
    for (long t = t_b; t < t_e; ++t) mine += parts_of(tile_counts[t].x);
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
    __syncthreads();                                         // (sb is read above by thread 0)
    if (lane == 63) sb[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) { if (w < wave) before += sb[w]; all += sb[w]; }
    int o = before + incl - mine;
    for (long t = t_b; t < t_e; ++t) {
        const int np = parts_of(tile_counts[t].x);
        for (int q = 0; q < np; ++q) items[o++] = make_int2((int)t, q | (np << 16));
    }
    if (tid == 0) { *n_items = all; *item_ctr = 0; }
}
__global__ __launch_bounds__(1024) void exact_list_totals_kernel(const int2* __restrict__ tile_counts, long tiles, int* __restrict__ blocks_run,
                                                                 int* __restrict__ groups_run, int slots = 0, int2* __restrict__ items = nullptr,
                                                                 int* __restrict__ n_items = nullptr, int* __restrict__ item_ctr = nullptr,
                                                                 int len_pct = 125) {
    __shared__ int sb[16], sk[16];
    __shared__ int tot_b;
    exact_list_totals_body<1024>(tile_counts, tiles, blocks_run, groups_run, slots, items, n_items, item_ctr, len_pct, sb, sk, tot_b);
}

// Both in ONE launch: sixteen tiles a workgroup (a wave each), and the workgroup that finishes LAST does the totals and cuts the
// items -- the single workgroup of exact_list_totals_kernel otherwise starts only when the whole lists grid has drained, and
// costs a launch of its own.  Last is whoever draws the final ticket of `done` (the pass's counter block: zero at the pass's
// start; the last workgroup leaves it zero again for the pass's next plan).  What crosses workgroups inside the launch is
// tile_counts alone (the lists themselves are read by later launches): every wave writes its tile's pair through to memory
// with one agent-scope store and waits for it, the workgroup's barrier stands between those waits and its ticket, and the last
// workgroup acquires (agent scope) before it reads the pairs.  With a release fence per workgroup instead (__threadfence()
// before the ticket: a write-back of all the lists the workgroup has just written) the launch measured 27.4 us against 22.5 us
// for the two launches it replaces, this way 23.4 us: profiles/exact_chain_summary.md.  No workgroup waits for another.
constexpr int LISTS_WG_TILES = 16;
// the ticket: every thread of the workgroup calls it behind its tiles' lists; true in the workgroup that arrives last (*last_s: LDS)
__device__ __forceinline__ bool exact_lists_last(int* __restrict__ done, int* last_s) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const int ticket = __hip_atomic_fetch_add(done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *last_s = ticket == (int)gridDim.x - 1 ? 1 : 0;
        if (*last_s) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    return *last_s != 0;
}
// where the lists, the counts and the work items of a pass go (exact_plan_fused_kernel: the arguments of exact_lists_totals_kernel)
struct PlanListsOut {
    int n_groups;
    int* glist; int* gcnt; int2* tile_counts; int* tlist; int* tcnt; int* tile_ticket;
    int* done; int* blocks_run; int* groups_run;
    int slots; int2* items; int* n_items; int* item_ctr; int len_pct;
};
__global__ __launch_bounds__(64 * LISTS_WG_TILES) void exact_lists_totals_kernel(const unsigned long long* __restrict__ need1, int n_cstages,
                                                                                const unsigned long long* __restrict__ need2, int n_groups,
                                                                                int* __restrict__ glist, int* __restrict__ gcnt,
                                                                                int2* tile_counts, int* __restrict__ tlist,
                                                                                int* __restrict__ tcnt, long tiles, int* __restrict__ done,
                                                                                int* __restrict__ blocks_run, int* __restrict__ groups_run,
                                                                                int slots, int2* __restrict__ items, int* __restrict__ n_items,
                                                                                int* __restrict__ item_ctr, int len_pct,
                                                                                int* __restrict__ tile_ticket) {
    static_assert(LISTS_WG_TILES == 16, "the totals' scan is written for sixteen waves");
    __shared__ int sb[16], sk[16];
    __shared__ int tot_b;
    __shared__ int last;
    const int tid = threadIdx.x;
    const long tile = (long)blockIdx.x * LISTS_WG_TILES + (tid >> 6);
    if (tile < tiles)
        exact_lists_tile<true>(tile, tid & 63, need1 + tile * n_cstages, n_cstages, need2 != nullptr ? need2 + tile * 4 * n_cstages : nullptr, n_groups,
                               glist, gcnt, tile_counts, tlist, tcnt, tile_ticket);
    if (!exact_lists_last(done, &last)) return;
    exact_list_totals_body<64 * LISTS_WG_TILES>(tile_counts, tiles, blocks_run, groups_run, slots, items, n_items, item_ctr, len_pct, sb, sk, tot_b);
}

// BOTH LEVELS AND THE LISTS IN ONE LAUNCH, one workgroup per 256-row tile (a pass of many tiles: the split kernels' gridDim.y == 1),
// three phases on the tile's rows, which stay in registers throughout:
//   A  level 1 as exact_plan_kernel<.., false> runs it: prologue, walk over all centroid stages, the need words in LDS (nl1);
//   B  level 2 as exact_plan_kernel<.., true> runs it: the dense list of the groups kept, from nl1; the gathered walk; the nibbles
//      filed into the workgroup's own words in LDS (nl2: no global atomics, nothing to clear);
//   C  exact_lists_tile from the two sets of LDS words (one wave), then exact_lists_totals_kernel's ticket: the workgroup that
//      finishes last sums the tiles' counts and cuts the screen's work items.
// Nothing but the lists, the counts and seed_s leaves the workgroup: the need bitmaps and sqrt(U) (sU_s) have no other reader.
// The two levels' thresholds differ (the centroid images' measured rounding errors: ec in plan_row_threshold): both are formed in
// the prologue, level 2's waits in LDS (p2s) while level 1 walks.  The extra step's row operand bx is sx sqrt(U) rounded up in both
// levels unless the level's A is not finite, where it is up_to_half(0) and P = +inf: every test of that level then says "needed"
// whatever the accumulator holds, so one operand serves both levels -- level 1's, or level 2's where level 1's P is +inf.
// FOLD: a level's threshold is part of the rows' extra-step operand, so level 2's parts (under level 2's scale c) wait in LDS
// instead of its P, four operand values a row, and replace level 1's in xe between the walks.
template <int KS32, class EL, bool FOLD>
__global__ __launch_bounds__(64 * K16_NW, 3) void exact_plan_fused_kernel(const __bf16* __restrict__ Xb, long N,
                                                                    const char* __restrict__ Cst1, int n_cstages1, const float* __restrict__ cmax2_1,
                                                                    const char* __restrict__ Cst2, int n_slots2, const float* __restrict__ cmax2_2,
                                                                    const float* __restrict__ xsq, const float* __restrict__ xerr,
                                                                    const float* __restrict__ xmax2,
                                                                    const float* __restrict__ wmax2, const float* __restrict__ werr2,
                                                                    ExactBound eb, const int* __restrict__ lastpos, const char* __restrict__ Wst,
                                                                    float* __restrict__ seed_s, int force_all, PlanListsOut lo) {
    using E = typename EL::T;
    using bf16x8 = typename V8<E>::t;
    constexpr int DP = 32 * KS32;
    constexpr int STAGE = k16_stage_bytes(KS32);
    constexpr int NT = 64 * K16_NW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int act_n;
    __shared__ int sb_s[NT / 64], sk_s[NT / 64];
    __shared__ int tot_b;
    __shared__ int last;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int quad = lane >> 4, col = lane & 15;
    const long wave_s0 = (long)blockIdx.x * K16_WG_SAMPLES + wave * (16 * K16_SB);
    // LDS behind the two stage slots: the list of kept groups, level 2's words, level 1's words, level 2's thresholds
    const int n_cstages2 = 4 * n_cstages1;
    int* act = (int*)(smem + 2 * STAGE);
    unsigned long long* nl2 = (unsigned long long*)(smem + 2 * STAGE + (size_t)n_cstages1 * 64 * sizeof(int));
    unsigned long long* nl1 = nl2 + n_cstages2;
    float* p2s = (float*)(nl1 + n_cstages1);               // (8 bytes a row: FOLD: (-, p1, p2, p3) of the operand type, else P as a float)
    E* p2e = (E*)p2s;

    bf16x8 xf[K16_SB][KS32];
    bf16x8 xe[K16_SB];
    PlanTest<EL> pt;
    float (&P)[K16_SB] = pt.P;
    E negc2;
    {
        const ExactScales sc1 = ex_scales(xmax2, cmax2_1, cmax2_1 + 1);
        const ExactScales sc2 = ex_scales(xmax2, cmax2_2, cmax2_2 + 1);
        const ExactScales sw = ex_scales(xmax2, wmax2, werr2);
        const float cf1 = plan_fold_scale<EL>(sc1.sx * sc1.sw * sc1.bmag), cf2 = plan_fold_scale<EL>(sc2.sx * sc2.sw * sc2.bmag);
        pt.negc = (E)(-cf1);
        negc2 = (E)(-cf2);
#pragma unroll
        for (int sb = 0; sb < K16_SB; ++sb) {
            const long row = wave_s0 + sb * 16 + col;
#pragma unroll
            for (int ks = 0; ks < KS32; ++ks) xf[sb][ks] = *(const bf16x8*)(Xb + row * DP + ks * 32 + quad * 8);
            float q = 0.0f, xer = 0.0f, su = 0.0f;
            if (row < N) {
                q = xsq[row]; xer = xerr[row];
                su = plan_row_seed<KS32, EL>(xf[sb], row, q, xer, eb, sw, Wst, lastpos, nullptr, nullptr, seed_s, force_all);
            }
            float bx1, bx2, P2;
            plan_row_threshold<KS32, FOLD>(eb, sc1, row < N, q, xer, su, P[sb], bx1);
            plan_row_threshold<KS32, FOLD>(eb, sc2, row < N, q, xer, su, P2, bx2);
            xe[sb] = plan_extra_step<EL, FOLD>(P[sb] == __builtin_inff() ? bx2 : bx1, P[sb], cf1);
            if (quad == 0) {
                const int at = wave * (16 * K16_SB) + sb * 16 + col;
                if constexpr (FOLD) {
                    const PlanParts pp = plan_split_threshold<EL>(P2, cf2);
                    p2e[4 * at + 1] = (E)pp.p1; p2e[4 * at + 2] = (E)pp.p2; p2e[4 * at + 3] = (E)pp.p3;
                } else p2s[2 * at] = P2;
            }
        }
    }
    for (int i = tid; i < n_cstages1 + n_cstages2; i += NT) nl2[i] = 0ull;   // (nl2, then nl1: one run of words)

    // A
    plan_walk_level1<KS32, EL, FOLD>(Cst1, 0, n_cstages1, smem, nl1, xf, xe, pt);
    __syncthreads();
    // B
    if (wave == 0) plan_level2_list(nl1, n_cstages1, n_slots2, act, &act_n);
#pragma unroll
    for (int sb = 0; sb < K16_SB; ++sb) {
        const int at = wave * (16 * K16_SB) + sb * 16 + col;
        if constexpr (FOLD) {
            if (quad == 0) { xe[sb][1] = p2e[4 * at + 1]; xe[sb][2] = p2e[4 * at + 2]; xe[sb][3] = p2e[4 * at + 3]; }
        } else P[sb] = p2s[2 * at];
    }
    pt.negc = negc2;
    __syncthreads();
    plan_walk_level2<KS32, EL, FOLD>(Cst2, act, 0, act_n, smem, nl2, xf, xe, pt);
    __syncthreads();
    // C
    if (wave == 0)
        exact_lists_tile<true>(blockIdx.x, lane, nl1, n_cstages1, nl2, lo.n_groups, lo.glist, lo.gcnt, lo.tile_counts, lo.tlist, lo.tcnt, lo.tile_ticket);
    if (!exact_lists_last(lo.done, &last)) return;
    exact_list_totals_body<NT>(lo.tile_counts, gridDim.x, lo.blocks_run, lo.groups_run, lo.slots, lo.items, lo.n_items, lo.item_ctr, lo.len_pct,
                               sb_s, sk_s, tot_b);
}

// ---- the SCOUT: a bound for rows WITHOUT a last BMU (query rows, streamed chunks, a row set's first epoch) and for the
// epochs in which last epoch's BMU says little (a schedule's first epochs: rows still travel across the map).
//   1. every row's nearest GROUP centroid g*: the plain resident kernel (bmu_bf16_k16_kernel<.., false, false>) on the plain
//      copy of the level-1 centroid image -- 1/64 of a full scan.
//   2. the rows sorted by g* (the radix sort of update.hpp), their operands gathered in that order: the 256 rows of a tile
//      then share one or two groups.
//   3. per tile the set of its rows' groups (+, where last epoch's BMUs exist, those units' groups) as a tile list
//      (exact_scout_lists_kernel), and the resident kernel once more over those few groups, unit indices kept
//      (bmu_bf16_k16_kernel<.., GM = false, TL = true>): the best unit among them is the row's PSEUDO last BMU.
// Every unit of g* is within r of the centroid, so that unit is no farther than |x - c_g*| + r_g*: the centroid-only bound
// U_c of tools/ucent_probe.py, and usually much nearer.  Any unit gives a valid bound: the plan's prologue (exact_plan_kernel)
// evaluates the unit it is handed rigorously, whatever picked it -- the scout runs in half precision and owes nothing.
__global__ __launch_bounds__(256) void exact_groupkey_kernel(const int* __restrict__ g, long n, int n_groups, int* __restrict__ keys,
                                                             int* __restrict__ vals) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int v = g[i];
    keys[i] = v < 0 ? 0 : v >= n_groups ? n_groups - 1 : v;
    vals[i] = (int)i;
}

// per 256-row tile of the sorted pass: the distinct groups of its rows' keys (gkey[p]: ascending over the pass) and, where
// lastpos is given, of their last BMUs (lastpos[p] >> 6) -- a bitmap of the groups in LDS -- as the tile's dense list of
// 16-unit tiles (all four of every group, ascending: what bmu_bf16_k16_kernel<.., TL> walks).  One wave per tile.
// group_items: the list as (group << 4 | 15) items, one per group (what the wide kernel walks), tcnt = groups listed.
__global__ __launch_bounds__(64) void exact_scout_lists_kernel(const int* __restrict__ gkey, const int* __restrict__ lastpos, long n,
                                                               int n_groups, int* __restrict__ tlist, int* __restrict__ tcnt,
                                                               int group_items = 0) {
    extern __shared__ unsigned long long sbm[];
    const long tile = blockIdx.x;
    const int lane = threadIdx.x;
    const int nw = (n_groups + 63) / 64;
    for (int w = lane; w < nw; w += 64) sbm[w] = 0ull;
    __syncthreads();
    for (int i = 0; i < SK_TILE / 64; ++i) {
        const long p = tile * SK_TILE + i * 64 + lane;
        if (p < n) {
            int g = gkey[p];
            g = g < 0 ? 0 : g >= n_groups ? n_groups - 1 : g;
            atomicOr(sbm + (g >> 6), 1ull << (g & 63));
            if (lastpos != nullptr) {
                int g2 = lastpos[p] >> 6;
                g2 = g2 < 0 ? 0 : g2 >= n_groups ? n_groups - 1 : g2;
                atomicOr(sbm + (g2 >> 6), 1ull << (g2 & 63));
            }
        }
    }
    __syncthreads();
    int base = 0;
    int* out = tlist + tile * (group_items ? 1 : 4) * (long)n_groups;
    for (int w0 = 0; w0 < nw; w0 += 64) {
        unsigned long long word = w0 + lane < nw ? sbm[w0 + lane] : 0ull;
        const int c = __popcll(word);
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
        int at = base + incl - c;
        for (; word != 0ull; word &= word - 1ull) {
            const int g = (w0 + lane) * 64 + (int)__builtin_ctzll(word);
            if (group_items) out[at] = (g << 4) | 15;
            else {
#pragma unroll
                for (int b = 0; b < 4; ++b) out[4 * at + b] = (g << 2) | b;
            }
            ++at;
        }
        base += __shfl(incl, 63, 64);
    }
    if (lane == 0) tcnt[tile] = group_items ? base : 4 * base;
}

// Is a plan from the scout worth its launches at all?  First the cheap question: how much of the map does a ROW need?  A sample of
// the rows (one workgroup each, strided through the row set) against every group centroid in float32: with sqrt(U) = min_g (|x -
// c_g| + r_g) -- the centroid-only bound -- how many groups pass level 1's test |x - c_g| - r_g <= sqrt(U)?  counts[0] += groups
// needed, counts[1] += rows sampled.  A tile needs the union over its 256 rows: where a row alone needs nearly every group (a
// random codebook, rows without structure) there is nothing to plan, and the launch is spared the scout altogether.
__global__ __launch_bounds__(256) void exact_scout_rowneed_kernel(const float* __restrict__ X, long N, int D, int n_samples,
                                                                  const float* __restrict__ Cc, const float* __restrict__ rg,
                                                                  int n_groups, int* __restrict__ counts) {
    extern __shared__ float xs[];                            // the row, then four wave minima / counts
    __shared__ float wmin[4];
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long step = N / n_samples;
    const float* x = X + ((long)blockIdx.x * step + step / 2) * D;
    for (int k = tid; k < D; k += 256) xs[k] = x[k];
    __syncthreads();
    auto dist = [&](int g) -> float {
        const float* c = Cc + (long)g * D;
        float q = 0.0f;
        if ((D & 3) == 0) {
            for (int k = 0; k < D; k += 4) {
                const f32x4 v = *(const f32x4*)(c + k);
#pragma unroll
                for (int j = 0; j < 4; ++j) { const float t = xs[k + j] - v[j]; q = __builtin_fmaf(t, t, q); }
            }
        } else {
            for (int k = 0; k < D; ++k) { const float t = xs[k] - c[k]; q = __builtin_fmaf(t, t, q); }
        }
        return __builtin_sqrtf(q);
    };
    float m = __builtin_inff();
    for (int g = tid; g < n_groups; g += 256) {
        const float r = rg[g];
        if (r >= 0.0f) m = __builtin_fminf(m, dist(g) + r);  // (a slot without units: r < 0)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = __builtin_fminf(m, __shfl_xor(m, o, 64));
    if (lane == 0) wmin[wave] = m;
    __syncthreads();
    m = __builtin_fminf(__builtin_fminf(wmin[0], wmin[1]), __builtin_fminf(wmin[2], wmin[3]));
    int need = 0;
    for (int g = tid; g < n_groups; g += 256) {
        const float r = rg[g];
        if (r >= 0.0f) need += !(dist(g) - r > m) ? 1 : 0;   // (NaN distances: needed)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) need += __shfl_xor(need, o, 64);
    if (lane == 0) wcnt[wave] = need;
    __syncthreads();
    if (tid == 0) { atomicAdd(counts, wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3]); atomicAdd(counts + 1, 1); }
}

// ... then the exact one, on SAMPLE TILES: every stride-th 256-row tile of the pass in its sorted
// order -- the very tiles the plan would see -- copied out (their rows' ids and sort keys) as a small pass of its own; the host
// gathers, picks and plans that sample exactly as it would the pass and reads the executed share back before committing the
// whole pass to the gather, the pick and the plan (somhip.hip, launch_bmu_exact).
__global__ __launch_bounds__(256) void exact_sample_tiles_kernel(const int* __restrict__ order, const int* __restrict__ keys, long stride_tiles,
                                                                 int* __restrict__ order_out, int* __restrict__ keys_out) {
    const long src = (long)blockIdx.x * stride_tiles * SK_TILE + threadIdx.x;
    const long dst = (long)blockIdx.x * SK_TILE + threadIdx.x;
    static_assert(SK_TILE == 256, "one thread per row of a tile");
    order_out[dst] = order[src];
    keys_out[dst] = keys[src];
}

// the scout's pick per sorted position -> lastpos (a position below K: what the plan's prologue evaluates), and the merge
// keys back to all ones for the screen proper
// (perm: positions -> UNIT ids, where the consumer wants units -- the wide plan's float32 seed)
__global__ __launch_bounds__(256) void exact_scout_pos_kernel(unsigned long long* __restrict__ best64, long n, int K,
                                                              int* __restrict__ lastpos, const int* __restrict__ perm = nullptr) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint32_t u = (uint32_t)best64[p];
    const int pos = u < (uint32_t)K ? (int)u : 0;            // (a NaN row: any unit gives a valid bound)
    lastpos[p] = perm != nullptr ? perm[pos] : pos;
    best64[p] = ~0ull;
}

}  // namespace somhip
