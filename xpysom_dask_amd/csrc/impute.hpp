// Missing values, the completed rows (som_impute*): out[n][d] = x[n][d] where it is observed and W[ids[n]][d] where it is a
// NaN, bit for bit -- no arithmetic on a value, only the test x == x.
//   impute_rows_kernel<V>   V = 4: 16 bytes a lane (the launcher has seen D % 4 == 0 and X, out, W on 16-byte addresses);
//                           V = 1: a float a lane, for every other D and for a view that starts at any float
// A memory-bound pass: X is read once and (out of place) written once; of the codebook only the holes' values are read.
// Rows are dealt out in TILES of whole rows, about IMP_TILE lane-accesses each, and a workgroup walks its tile as one flat
// run of V-float pieces: lane t takes pieces t, t + 256, ... of the tile, whichever rows they fall in.  So D = 4 puts 256
// rows into one sweep of the workgroup, D = 132 puts 31 rows into four, and no lane idles except in a tile's last sweep;
// consecutive lanes read consecutive addresses whatever D is.  A row longer than a tile is a tile of its own.
// The tile's ids are read once per row, by the tile's first lanes into LDS, before the sweep.
// In place (out == X) only the holes are stored, as single floats.  Every piece is read by the one lane that may write it,
// before it writes it, and no lane reads another lane's piece: no order between lanes is needed.
#pragma once

#include <hip/hip_runtime.h>

#include "som_common.hpp"

namespace somhip {

constexpr int IMP_TILE = 1024;       // pieces a tile aims at: four sweeps of the 256 lanes

// rows per tile for rows of `pieces` pieces: whole rows, at least one, at most IMP_TILE (the LDS array of ids)
__host__ __device__ inline int impute_tile_rows(int pieces) { return pieces >= IMP_TILE ? 1 : IMP_TILE / pieces; }

template <int V> struct ImputePiece;
template <> struct ImputePiece<1> { using type = float; };
template <> struct ImputePiece<4> { using type = float4; };

// X and out are the same array or disjoint ones (the caller has refused everything else), so neither is __restrict__.
// N rows of D floats, D % V == 0; ids[n] in [0, K) names the row of W.  Element offsets are 64-bit: N * D passes 2^31.
template <int V>
__global__ __launch_bounds__(256) void impute_rows_kernel(const float* X, const int* __restrict__ ids,
                                                          const float* __restrict__ W, long N, int D, float* out) {
    using piece_t = typename ImputePiece<V>::type;
    __shared__ int unit[IMP_TILE];
    const unsigned P = (unsigned)(D / V);                   // pieces per row
    const int R = impute_tile_rows((int)P);
    const long tiles = (N + R - 1) / R;
    const bool in_place = (const float*)out == X;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long row0 = tile * R;
        const int rows = (int)(N - row0 < R ? N - row0 : R);
        __syncthreads();                                    // (the sweep before has read `unit`)
        for (int r = threadIdx.x; r < rows; r += 256) unit[r] = ids[row0 + r];
        __syncthreads();
        const long base = row0 * D;                         // first element of the tile
        const unsigned n = (unsigned)rows * P;              // (rows > 1 only where rows * P <= IMP_TILE)
        for (unsigned i = threadIdx.x; i < n; i += 256) {
            const unsigned r = i / P, c = (i - r * P) * V;  // row inside the tile, first feature of the piece
            const long at = base + (long)i * V;
            const piece_t x = *reinterpret_cast<const piece_t*>(X + at);
            const float* w = W + (long)unit[r] * D + c;
            if constexpr (V == 1) {
                if (x == x) { if (!in_place) out[at] = x; }
                else out[at] = w[0];
            } else {
                const bool h0 = x.x != x.x, h1 = x.y != x.y, h2 = x.z != x.z, h3 = x.w != x.w;
                if (in_place) {
                    if (h0) out[at] = w[0];
                    if (h1) out[at + 1] = w[1];
                    if (h2) out[at + 2] = w[2];
                    if (h3) out[at + 3] = w[3];
                } else {
                    piece_t y = x;
                    if (h0) y.x = w[0];
                    if (h1) y.y = w[1];
                    if (h2) y.z = w[2];
                    if (h3) y.w = w[3];
                    *reinterpret_cast<piece_t*>(out + at) = y;
                }
            }
        }
    }
}

}  // namespace somhip
