// THE SORT BY UNIT: a row set's rows ordered by their BMU, stably, into (skey, srow) -- what the update's segment sum (resident rows,
// streamed chunks), som_unit_stats*, som_unit_label_counts* and som_unit_value_sums* all start from.  Two implementations give the
// same order (update.hpp): the counting sort for maps of at most CS_MAX_K units, the radix sort for everything else.  This header
// owns HOW LARGE the sort's buffers are and WHICH of the two runs: one rule, pure host arithmetic (no HIP, no handle), in the
// manner of row_set.hpp.  somhip.hip's UnitSort allocates what sizes() says and sorts as counting() says;
// som_debug_unit_sort_sizes exposes both to the CPU suite (tests/test_unit_sort_cpu.py).
#pragma once

#include <cstddef>

namespace somhip {

constexpr int RS_BLOCK = 2048;        // radix sort: items per block
constexpr int CS_MAX_K = 8192;        // counting sort: units (LDS: 4 bytes per unit)
constexpr int CS_BLOCK = 1024;        // counting sort: rows per block
constexpr long CS_MAX_TABLE = 1L << 21;   // counting sort: (blocks x units) counts at the most: 8 MiB of table, a scan of a few microseconds

namespace unitsort {

// key bits of a sort over K keys (at least one)
inline int key_bits(long K) {
    int bits = 1;
    while ((1L << bits) < K) ++bits;
    return bits;
}

// the radix sort's scratch for n items, in ints: two (key, value) ping-pong pairs of n + the 256 x blocks table + its 256 totals
inline size_t radix_scratch_ints(long n) {
    const long blocks = ((n > 1 ? n : 1) + RS_BLOCK - 1) / RS_BLOCK;
    return 4 * (size_t)n + 256 * (size_t)blocks + 256;
}

// elements of the buffers that sort up to rows_cap rows.  table: the counting sort's [K][B] counts of a sort over B <= cs_blocks
// blocks of rows, and the units' [K] totals behind them; cs_blocks == 0: no table -- the map is too large, the capacity under two blocks, the table past its
// ceiling, or the switch (SOM_COUNTING_SORT=0) off -- and every sort in these buffers is the radix sort
struct Sizes { size_t skey = 0, srow = 0, scratch = 0, table = 0; long cs_blocks = 0; };
inline Sizes sizes(long rows_cap, int K, bool counting_on) {
    Sizes z;
    z.skey = z.srow = (size_t)rows_cap;
    z.scratch = radix_scratch_ints(rows_cap);
    const long csb = (rows_cap + CS_BLOCK - 1) / CS_BLOCK;
    if (counting_on && K <= CS_MAX_K && rows_cap >= 2 * CS_BLOCK && csb * K <= CS_MAX_TABLE) {
        z.table = (size_t)(csb + 1) * K;
        z.cs_blocks = csb;
    }
    return z;
}

// the run-time half: N rows take the counting sort where a table is held, their blocks fit it and they fill two of them
inline bool counting(long cs_blocks, long N) {
    return cs_blocks > 0 && (N + CS_BLOCK - 1) / CS_BLOCK <= cs_blocks && N >= 2 * CS_BLOCK;
}
inline bool counting(const Sizes& z, long N) { return counting(z.cs_blocks, N); }

}  // namespace unitsort
using unitsort::radix_scratch_ints;
}  // namespace somhip
