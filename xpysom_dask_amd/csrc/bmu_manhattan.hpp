// Fused Manhattan (L1) distance + first-minimum argmin: 'manhattan' / 'manhattan_no_opt'
//   ids[n] = argmin_k S(0, input_len),  the float32 sum of t_d = | fl32(x_nd - w_kd) | in NumPy's pairwise order
// without the (n, K) matrix.  The order is np_pairwise_absdiff_pow's (bmu_pairwise.hpp, p = 1), bit for bit:
//   n < 8:    t_off + t_off+1 + ... left to right
//   n <= 128: m = n - n % 8; eight chains r_j = t_off+j + t_off+8+j + ... (j = 0..7), res = ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)),
//             then the n % 8 remaining terms added to res one by one
//   n > 128:  n2 = n/2 - (n/2) % 8;  S(off, n) = S(off, n2) + S(off + n2, n - n2)
// Every add and subtract is one correctly rounded float32 operation (no fma, no reassociation, no packed FP32).
//
// The schedule.  Every term is >= +0, so a chain may START from its first term (0 + t = t) and LDS is feature-major, so the
// order in which a lane consumes features is free.  The host (mn_schedule) turns input_len into a list of chunks.  A chunk is
// four or eight whole chains of one leaf (a leaf is a range of <= 128 features summed by the second rule), walked CHAIN BY
// CHAIN: a chain of `cl` steps sums into one register, and the eight chains of a leaf land as
//   c0 -> a | c1 -> run, a += run | c2 -> b | c3 -> run, a += b + run | c4 -> b | c5 -> run, b += run | c6 -> c |
//   c7 -> run, run = a + (b + (c + run))                      (the tree above; a float32 add is commutative)
// and the leaf's tail terms follow in `run`: four live values a pair, not eight.  A leaf with chains of <= 8 steps is one chunk,
// a longer one two (chains 0..3, then 4..7 and the tail): a chunk holds at most 64 + 7 feature lines.  The split tree is walked
// in post-order: the end of a leaf pops pending left sums (run = left + run) and pushes its own where it ends a left subtree;
// the stack is L registers a pair, L = the tree's depth (0 up to 128 features, 6 covers every input_len <= 4096).
//
// Work split.  A workgroup of 256 lanes (16 x 16) owns 64 RT rows x 64 units; a lane holds 4 RT rows x 4 units (rows
// 4 ty .. +3, with RT = 2 also 64 + 4 ty .. +3; units 4 tx .. +3) at 4 + L registers a pair: 8 x 4 pairs without a stack,
// 4 x 4 pairs with the stack of six -- 128 and 160 accumulators a lane.  The workgroup keeps its rows and walks the
// 64-unit blocks of its part of the codebook (gridDim.y parts; they merge by atomicMin on (distance bits << 32 | unit) -- a
// sum of terms >= 0 is >= 0, so its bits order as the value does -- and bmu_finalize_kernel).
//
// Operands.  Both go through LDS feature-major: line (chain jj, step s) of a chunk is feature off + 8 s + jj, so four
// neighbouring chains at one step are 16 contiguous bytes of a row: a lane reads them with one 16-byte load and stores them
// to four lines (64 consecutive rows a wave: 64 different banks).  Chunks are double-buffered through registers as in
// bmu_chebyshev.hpp: chunk t+1 leaves global memory while chunk t is folded, one barrier a chunk.
//   instance <RES = true, L = 0, RT = 2>   input_len <= 128: the 128 rows stay in LDS for the whole scan, only unit chunks stream
//   instance <RES = false, L = 6, RT = 1>  else: the 64 rows are re-staged with every unit block (from L2) beside the units'
// Per feature line a lane issues RT + 1 ds_read_b128 (its rows, its 4 units) and 2 x 16 RT VALU instructions: v_sub_f32, then
// v_add_f32 with the |.| source modifier (the first step of a chain: a move of |d|).
//
// Padding.  Units beyond K are skipped by the fold; rows beyond N are zero and never written.  A row holding a NaN or an
// infinity gets unit 0 (NumPy's argmin over an all-NaN row; every distance +inf), flagged by the staging as in the Chebyshev
// kernel; a NaN distance (a NaN in the codebook) never wins: `d < best` is false.
#pragma once
#include <vector>
#include "bmu_chebyshev.hpp"   // ch_nonfinite, ch_fill_kernel, SOM_NO_PK_F32

namespace somhip {

constexpr int MN_BN = 64;           // units of a unit block
constexpr int MN_WP = 68;           // floats of a feature line of units: 64 + 4 (16-byte aligned lines)
constexpr int MN_RT_RES = 2;        // row quads a lane: the resident instance (8 rows a lane, 128 a workgroup)
constexpr int MN_RT_DEEP = 1;       // ... the streamed one (4 rows a lane, 64 a workgroup)
constexpr int mn_bm(int rt) { return 64 * rt; }          // rows of a workgroup
constexpr int mn_xp(int rt) { return 64 * rt + 4; }      // floats of a feature line of rows
constexpr int MN_RES_D = 128;       // rows stay in LDS up to this many features (= one leaf: no stack)
constexpr int MN_STACK = 6;         // pending left sums of the streamed instance
constexpr int MN_MAX_D = 4096;      // every input_len up to here has a split tree of depth <= MN_STACK (mn_schedule checks)

enum { MN_END_ROOT = 1, MN_END_PUSH = 2, MN_TAIL_FIRST = 4, MN_POPS_SHIFT = 8 };

struct MnChunk {
    int off;     // feature of (chain j0, step 0): the leaf's first feature + j0
    int cl;      // steps of each chain
    int nj;      // chains in the chunk: 0 (a leaf of < 8 features), 4 or 8
    int j0;      // the first chain: 0 or 4
    int toff;    // the first tail feature
    int nt;      // tail terms after the chains: 0..7 (only where the chunk ends its leaf)
    int xline;   // the chunk's first line among the resident rows' lines (the lines before it)
    int end;     // MN_TAIL_FIRST: the tail starts the sum | where the chunk ends a leaf: pops << MN_POPS_SHIFT, MN_END_PUSH
};

// ---- host: the schedule ---------------------------------------------------------------------------------------------------
inline void mn_leaf(int off, int n, std::vector<MnChunk>& out) {
    const int m = n - n % 8, cl = m / 8;
    if (n < 8) out.push_back({off, 0, 0, 0, off, n, 0, MN_TAIL_FIRST});
    else if (cl <= 8) out.push_back({off, cl, 8, 0, off + m, n % 8, 0, 0});
    else {
        out.push_back({off, cl, 4, 0, off + m, 0, 0, 0});
        out.push_back({off + 4, cl, 4, 4, off + m, n % 8, 0, 0});
    }
}

inline void mn_tree(int off, int n, std::vector<MnChunk>& out) {
    if (n <= 128) { mn_leaf(off, n, out); return; }
    int n2 = n / 2;
    n2 -= n2 % 8;
    mn_tree(off, n2, out);
    out.back().end |= MN_END_PUSH;                      // the left sum waits on the stack ...
    mn_tree(off + n2, n - n2, out);
    out.back().end += 1 << MN_POPS_SHIFT;               // ... for the right one
}

// the chunks of input_len D; *max_lines: the feature lines of the longest chunk, *depth: the stack the walk needs
inline std::vector<MnChunk> mn_schedule(int D, int* max_lines, int* depth) {
    std::vector<MnChunk> s;
    mn_tree(0, D, s);
    int line = 0, ml = 0, sp = 0, dp = 0;
    for (auto& c : s) {
        const int lines = c.nj * c.cl + c.nt;
        c.xline = line;
        line += lines;
        ml = std::max(ml, lines);
        sp -= c.end >> MN_POPS_SHIFT;
        if (c.end & MN_END_PUSH) dp = std::max(dp, ++sp);
    }
    s.back().end |= MN_END_ROOT;
    *max_lines = ml;
    *depth = dp;
    return s;
}

// dynamic LDS: the flags, the rows (RES: every line; else two buffers of the longest chunk), two buffers of unit chunks
inline size_t mn_lds_bytes(int D, int max_lines) {
    const bool res = D <= MN_RES_D;
    const int x_lines = res ? D : 2 * max_lines, rt = res ? MN_RT_RES : MN_RT_DEEP;
    return (size_t)mn_bm(rt) * sizeof(int) + ((size_t)x_lines * mn_xp(rt) + (size_t)2 * max_lines * MN_WP) * sizeof(float);
}

// ---- device: staging ------------------------------------------------------------------------------------------------------
// A chunk's lines of 2^LG lines-of-the-matrix (rows: LG = 7 or 6, units: LG = 6) of a row-major [R][D] matrix into registers.
// Item id = 256 i + tid: matrix line id & (2^LG - 1), slot id >> LG = 0..15: (step, quad of chains) of the chain part -- one
// 16-byte read: features off + 8 step + 4 quad .. +3 -- and the tail term of the tail.  Zeros beyond R.
template <int LG>
struct MnRegs { float4 v[8 >> (7 - LG)]; float t[4 >> (7 - LG)]; };

template <int LG>
__device__ __forceinline__ void mn_load(const float* __restrict__ M, long R, int D, long r0, const MnChunk& c, bool vec, int tid, MnRegs<LG>& g) {
    constexpr int NV = 8 >> (7 - LG), NT = 4 >> (7 - LG), MASK = (1 << LG) - 1;
    const int qs = c.nj >> 3;                                      // 8 chains: slot = 2 step + quad; 4 chains: slot = step
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int id = 256 * i + tid, slot = id >> LG;
        const long line = r0 + (id & MASK);
        const int s = slot >> qs, q = slot & qs;
        float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (s < c.cl && line < R) {
            const float* p = M + line * (long)D + c.off + 8 * s + 4 * q;   // (inside the leaf's chain part: p + 3 is a feature)
            if (vec) t = *reinterpret_cast<const float4*>(p);              // (D % 4 == 0 and a 16-byte aligned base; off % 4 == 0)
            else { t.x = p[0]; t.y = p[1]; t.z = p[2]; t.w = p[3]; }
        }
        g.v[i] = t;
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int id = 256 * i + tid, slot = id >> LG;
        const long line = r0 + (id & MASK);
        g.t[i] = slot < c.nt && line < R ? M[line * (long)D + c.toff + slot] : 0.0f;
    }
}

// the transposing store of mn_load's registers into a chunk's lines [nj cl + nt][PITCH]
template <int LG, int PITCH>
__device__ __forceinline__ void mn_store(float* __restrict__ S, const MnChunk& c, int tid, const MnRegs<LG>& g) {
    constexpr int NV = 8 >> (7 - LG), NT = 4 >> (7 - LG), MASK = (1 << LG) - 1;
    const int qs = c.nj >> 3;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int id = 256 * i + tid, slot = id >> LG;
        const int s = slot >> qs, q = slot & qs;
        if (s < c.cl) {
            float* p = S + (4 * q * c.cl + s) * PITCH + (id & MASK);
            const int step = c.cl * PITCH;
            p[0] = g.v[i].x; p[step] = g.v[i].y; p[2 * step] = g.v[i].z; p[3 * step] = g.v[i].w;
        }
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int id = 256 * i + tid, slot = id >> LG;
        if (slot < c.nt) S[(c.nj * c.cl + slot) * PITCH + (id & MASK)] = g.t[i];
    }
}

// rows of mn_load's registers that hold a NaN or an infinity -> flag[line] = 1 (every writer writes the same value)
template <int LG>
__device__ __forceinline__ void mn_flag(int* __restrict__ flag, int tid, const MnRegs<LG>& g) {
    bool bad = false;
#pragma unroll
    for (int i = 0; i < (8 >> (7 - LG)); ++i) bad = bad || ch_nonfinite(g.v[i].x) || ch_nonfinite(g.v[i].y) || ch_nonfinite(g.v[i].z) || ch_nonfinite(g.v[i].w);
#pragma unroll
    for (int i = 0; i < (4 >> (7 - LG)); ++i) bad = bad || ch_nonfinite(g.t[i]);
    if (bad) flag[tid & ((1 << LG) - 1)] = 1;                      // (every item of a lane is of one row)
}

// ---- device: the fold -----------------------------------------------------------------------------------------------------
// one feature line: acc[i][j] (+)= |x_i - w_j|;  FIRST: the term starts the sum
template <bool FIRST, int RT>
__device__ __forceinline__ void mn_step(const float* __restrict__ xs, const float* __restrict__ ws, int ty, int tx, float (&acc)[4 * RT][4]) {
    const f32x4 xa = *reinterpret_cast<const f32x4*>(xs + 4 * ty);
    f32x4 xb = xa;
    if constexpr (RT > 1) xb = *reinterpret_cast<const f32x4*>(xs + 64 + 4 * ty);   // (the second row quad: only where there is one)
    const f32x4 wv = *reinterpret_cast<const f32x4*>(ws + 4 * tx);
#pragma unroll
    for (int i = 0; i < 4 * RT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = __builtin_fabsf(__fsub_rn(i < 4 ? xa[i & 3] : xb[i & 3], wv[j]));
            acc[i][j] = FIRST ? d : __fadd_rn(acc[i][j], d);
        }
}

// one chain of cl >= 1 steps into acc, left to right
template <int RT>
__device__ __forceinline__ void mn_chain(const float* __restrict__ xs, const float* __restrict__ ws, int cl, int ty, int tx, float (&acc)[4 * RT][4]) {
    mn_step<true, RT>(xs, ws, ty, tx, acc);
#pragma unroll 2
    for (int s = 1; s < cl; ++s) mn_step<false, RT>(xs + s * mn_xp(RT), ws + s * MN_WP, ty, tx, acc);
}

#define MN_PAIRS(expr) _Pragma("unroll") for (int i = 0; i < 4 * RT; ++i) _Pragma("unroll") for (int j = 0; j < 4; ++j) { expr; }

// one chunk: its chains, each into the register its place in the 8-way combine asks for, then its tail terms into `run`
template <int RT>
__device__ __forceinline__ void mn_fold(const float* __restrict__ Xs, const float* __restrict__ Ws, const MnChunk& c, int ty, int tx,
                                        float (&a)[4 * RT][4], float (&b)[4 * RT][4], float (&cc)[4 * RT][4], float (&run)[4 * RT][4]) {
    constexpr int MN_XP = mn_xp(RT);
    for (int jj = 0; jj < c.nj; ++jj) {
        const float* xs = Xs + jj * c.cl * MN_XP;
        const float* ws = Ws + jj * c.cl * MN_WP;
        switch (c.j0 + jj) {
        case 0: mn_chain<RT>(xs, ws, c.cl, ty, tx, a); break;
        case 1: mn_chain<RT>(xs, ws, c.cl, ty, tx, run); MN_PAIRS(a[i][j] = __fadd_rn(a[i][j], run[i][j])) break;
        case 2: mn_chain<RT>(xs, ws, c.cl, ty, tx, b); break;
        case 3: mn_chain<RT>(xs, ws, c.cl, ty, tx, run); MN_PAIRS(a[i][j] = __fadd_rn(a[i][j], __fadd_rn(b[i][j], run[i][j]))) break;
        case 4: mn_chain<RT>(xs, ws, c.cl, ty, tx, b); break;
        case 5: mn_chain<RT>(xs, ws, c.cl, ty, tx, run); MN_PAIRS(b[i][j] = __fadd_rn(b[i][j], run[i][j])) break;
        case 6: mn_chain<RT>(xs, ws, c.cl, ty, tx, cc); break;
        default: mn_chain<RT>(xs, ws, c.cl, ty, tx, run);
            MN_PAIRS(run[i][j] = __fadd_rn(a[i][j], __fadd_rn(b[i][j], __fadd_rn(cc[i][j], run[i][j])))) break;
        }
    }
    const float* xs = Xs + c.nj * c.cl * MN_XP;
    const float* ws = Ws + c.nj * c.cl * MN_WP;
    int t = 0;
    if ((c.end & MN_TAIL_FIRST) && c.nt > 0) { mn_step<true, RT>(xs, ws, ty, tx, run); t = 1; }
    for (; t < c.nt; ++t) mn_step<false, RT>(xs + t * MN_XP, ws + t * MN_WP, ty, tx, run);
}

// grid (row blocks, parts).  out64 == nullptr (one part): the ids go straight to `out`.  sched: n_chunks chunks of at most
// max_lines lines (mn_schedule).  L: the registers of the pending-sum stack (>= the schedule's depth; the host checks).
template <bool RES, int L, int RT>
__global__ SOM_NO_PK_F32 __launch_bounds__(256)
void bmu_manhattan_kernel(const float* __restrict__ X, long N, int D, const float* __restrict__ W, int K,
                          const MnChunk* __restrict__ sched, int n_chunks, int max_lines, int x_vec, int w_vec,
                          int* __restrict__ out, unsigned long long* __restrict__ out64) {
    extern __shared__ __attribute__((aligned(16))) float smem_mn[];
    constexpr int MN_BM = mn_bm(RT), MN_XP = mn_xp(RT), XLG = 5 + RT;   // (RT = 1, 2: 2^XLG rows)
    int* flag = reinterpret_cast<int*>(smem_mn);
    float* Xs = smem_mn + MN_BM;                                   // RES: [D] lines; else two buffers of max_lines lines
    float* Ws = Xs + (RES ? D : 2 * max_lines) * MN_XP;            // two buffers of max_lines lines
    const int x_buf = max_lines * MN_XP, w_buf = max_lines * MN_WP;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const long r0 = (long)blockIdx.x * MN_BM;
    const int n_ub = (K + MN_BN - 1) / MN_BN;
    const int ub0 = (int)((long)n_ub * blockIdx.y / gridDim.y), ub1 = (int)((long)n_ub * (blockIdx.y + 1) / gridDim.y);
    const int steps = (ub1 - ub0) * n_chunks;                      // (a part holds a unit block: the host keeps parts <= n_ub)

    if (tid < MN_BM) flag[tid] = 0;
    __syncthreads();
    MnRegs<XLG> xr;
    MnRegs<6> wr;
    if (RES) {
        for (int c = 0; c < n_chunks; ++c) {
            const MnChunk ck = sched[c];
            mn_load<XLG>(X, N, D, r0, ck, x_vec != 0, tid, xr);
            mn_flag(flag, tid, xr);
            mn_store<XLG, MN_XP>(Xs + ck.xline * MN_XP, ck, tid, xr);
        }
    } else {
        const MnChunk ck = sched[0];
        mn_load<XLG>(X, N, D, r0, ck, x_vec != 0, tid, xr);
        mn_flag(flag, tid, xr);
        mn_store<XLG, MN_XP>(Xs, ck, tid, xr);
    }
    {
        const MnChunk ck = sched[0];
        mn_load<6>(W, K, D, (long)ub0 * MN_BN, ck, w_vec != 0, tid, wr);
        mn_store<6, MN_WP>(Ws, ck, tid, wr);
    }
    __syncthreads();

    float a[4 * RT][4], b[4 * RT][4], cc[4 * RT][4], run[4 * RT][4], st[L > 0 ? L : 1][4 * RT][4];
    float best[4 * RT];
    int bidx[4 * RT];
#pragma unroll
    for (int i = 0; i < 4 * RT; ++i) { best[i] = __builtin_inff(); bidx[i] = ub0 * MN_BN; }   // (all-infinite part: its first unit)

    int ub = ub0, c = 0, sp = 0;
    for (int t = 0; t < steps; ++t) {
        // the next step's operands leave global memory now and reach the other buffer after this chunk's fold
        int nub = ub, nc = c + 1;
        if (nc == n_chunks) { nc = 0; nub = ub + 1; }
        const bool more = t + 1 < steps;
        const MnChunk ck = sched[c], nk = sched[more ? nc : c];
        if (more) {
            mn_load<6>(W, K, D, (long)nub * MN_BN, nk, w_vec != 0, tid, wr);
            if (!RES) {
                mn_load<XLG>(X, N, D, r0, nk, x_vec != 0, tid, xr);
                if (nub == ub0) mn_flag(flag, tid, xr);            // (the first unit block sees every feature once)
            }
        }
        mn_fold<RT>(RES ? Xs + ck.xline * MN_XP : Xs + (t & 1) * x_buf, Ws + (t & 1) * w_buf, ck, ty, tx, a, b, cc, run);
        if (L > 0) {
            // the end of a leaf: run = (pending left sum) + run for every subtree that ends here, then run waits itself
            for (int p = ck.end >> MN_POPS_SHIFT; p > 0; --p) {
                --sp;
#pragma unroll
                for (int l = 0; l < L; ++l)
                    if (sp == l) MN_PAIRS(run[i][j] = __fadd_rn(st[l][i][j], run[i][j]))
            }
            if (ck.end & MN_END_PUSH) {
#pragma unroll
                for (int l = 0; l < L; ++l)
                    if (sp == l) MN_PAIRS(st[l][i][j] = run[i][j])
                ++sp;
            }
        }
        if (ck.end & MN_END_ROOT) {
            // this unit block's 4 units per row, ascending: the first minimum stays
#pragma unroll
            for (int i = 0; i < 4 * RT; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int u = ub * MN_BN + 4 * tx + j;
                    if (u < K && run[i][j] < best[i]) { best[i] = run[i][j]; bidx[i] = u; }
                }
        }
        if (more) {
            mn_store<6, MN_WP>(Ws + ((t + 1) & 1) * w_buf, nk, tid, wr);
            if (!RES) mn_store<XLG, MN_XP>(Xs + ((t + 1) & 1) * x_buf, nk, tid, xr);
        }
        __syncthreads();
        ub = nub; c = nc;
    }

    // across the 16 lanes of a row (consecutive lanes of one wave): the smaller (distance bits, unit)
#pragma unroll
    for (int i = 0; i < 4 * RT; ++i) {
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
