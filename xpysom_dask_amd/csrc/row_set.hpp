// A ROW SET is a batch of float32 rows on the device with the buffers derived from it: |x|^2 (exact mode: the rows' measured
// operand errors behind it), the 16-bit operand image, the ids a search writes.  The engine holds three kinds -- the resident
// training rows, the query scratch (which also serves pageable streamed chunks), the two pinned-chunk slots -- and this header
// owns HOW LARGE their buffers are: one rule, pure host arithmetic (no HIP, no handle), in the manner of codebook_operands.hpp.
// somhip.hip's RowSet allocates what sizes() says; som_debug_row_set_sizes exposes it to the CPU suite (tests/test_row_sets_cpu.py).
#pragma once

#include <cstddef>

namespace somhip {
namespace rowset {

enum class Kind { Resident = 0, Query = 1, Slot = 2 };
struct Flags {                // fixed at som_create
    bool f32 = true;          // precision f32: no 16-bit image
    bool exact = false;       // precision 'exact': |x|^2 holds twice its rows -- the errors live in its second half
    bool needs_xsq = false;   // the configured search reads |x|^2 (exact; f32 with euclidean_no_opt or cosine)
    bool cos_tiled = false;   // 16-bit image, cosine, beyond 128 features: |x|^2 as scratch of the image's preparation
};
constexpr long ROW_PAD = 3072;     // the 16-bit row image is padded to a multiple of every kernel's workgroup tile
constexpr long QUERY_PAD = 1024;   // the query scratch grows in steps of 1 024 rows

// cap: the rows the derived buffers hold (the error half starts at xsq + cap).  X, xsq, Xb, ids: elements; 0 = no such buffer, and a
// buffer that exists holds at least one element (an allocation of none is one of one).  X counts only where the set owns its rows.
struct Sizes { long cap = 0; size_t X = 0, xsq = 0, Xb = 0, ids = 0; };
inline Sizes sizes(Kind kind, long n, int D, int dp, const Flags& f) {
    const auto up = [](long a, long b) { return (a + b - 1) / b * b; };
    const auto some = [](long a) { return (size_t)(a > 0 ? a : 1); };
    Sizes z;
    if (kind == Kind::Resident) {
        // exactly the rows: rebuilt for every row set the handle adopts; |x|^2 only where something reads it
        z.cap = n;
        z.X = some(n * D);
        z.ids = some(n);
        if (f.needs_xsq || (!f.f32 && f.cos_tiled)) z.xsq = some(n * (f.exact ? 2 : 1));
        if (!f.f32 && n > 0) z.Xb = (size_t)(up(n, ROW_PAD) * dp);
        return z;
    }
    if (n <= 0) return z;                                // (a transient set of no rows is never reserved)
    // the query scratch in steps of 1 024 rows (its image padded from there); a slot straight to the image's padding
    z.cap = kind == Kind::Query ? up(n, QUERY_PAD) : up(n, ROW_PAD);
    z.X = (size_t)(z.cap * D);
    z.ids = (size_t)z.cap;
    z.xsq = (size_t)(z.cap * (f.exact ? 2 : 1));
    if (!f.f32) z.Xb = (size_t)(up(z.cap, ROW_PAD) * dp);
    return z;
}
}  // namespace rowset
}  // namespace somhip
