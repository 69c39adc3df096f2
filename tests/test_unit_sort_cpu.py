"""The sort by unit's rule (csrc/unit_sort.hpp: unitsort::sizes and unitsort::counting) without a GPU, through the library's
test hook som_debug_unit_sort_sizes (include/somhip_test.h).

The formulas here are the ones seg_reserve and diag_reserve_stats each carried before they shared the rule:
  skey, srow     the capacity
  radix scratch  4 n + 256 * cdiv(max(n, 1), RS_BLOCK = 2 048) + 256
  table          (csb + 1) * K with csb = cdiv(capacity, CS_BLOCK = 1 024), held iff the switch is on, K <= CS_MAX_K = 8 192,
                 capacity >= 2 CS_BLOCK and csb * K <= 2^21
  counting sort  of n rows: a table is held, cdiv(n, CS_BLOCK) <= csb, n >= 2 CS_BLOCK
and update_ref.sort_path, the suite's one restatement of the path (every sort.* label and every case list leans on it), is
pinned against the hook: a threshold that drifts in the C++ fails here, on the CPU."""
import ctypes as C

import pytest

from tests import diag_ref
from tests import test_gpu_project
from tests import test_gpu_update_ref
from tests import update_ref as U
from xpysom_dask_amd import _lib

ROWS = (0, 1, 1023, 1024, 2047, 2048, 2049, 5120, 262144, 262145, 2 ** 24 + 3, 2 ** 31 - 1)
UNITS = (1, 64, 8191, 8192, 8193, 65536)


def cdiv(a, b):
    return -(-a // b)


def up(a, b):
    return cdiv(a, b) * b


def hook(rows_cap, K, on, n):
    """(skey, srow, scratch, table, cs_blocks, n rows take the counting sort)"""
    out = (C.c_int64 * 6)()
    assert _lib.load().som_debug_unit_sort_sizes(rows_cap, K, 1 if on else 0, n, out) == 0
    return list(out)


def want(rows_cap, K, on, n):
    csb = cdiv(rows_cap, 1024)
    held = on and K <= 8192 and rows_cap >= 2048 and csb * K <= 2 ** 21
    counting = held and cdiv(n, 1024) <= csb and n >= 2048
    return [rows_cap, rows_cap, 4 * rows_cap + 256 * cdiv(max(rows_cap, 1), 2048) + 256, (csb + 1) * K if held else 0,
            csb if held else 0, 1 if counting else 0]


@pytest.mark.parametrize("on", [True, False], ids=["counting-on", "counting-off"])
def test_sizes_match_the_formulas(on):
    for cap in ROWS:
        for K in UNITS:
            for n in sorted({0, 1, 2047, 2048, cap // 2, max(cap - 1, 0), cap}):
                got = hook(cap, K, on, n)
                assert got == want(cap, K, on, n), (cap, K, on, n, got)
                skey, srow, scratch, table, csb, counting = got
                # what the host code leans on: the totals row at B * K for every B <= cs_blocks lies inside the table, the radix
                # sort's four lists, its 256 x blocks table and its 256 totals inside the scratch
                assert table == 0 or table >= (csb + 1) * K
                assert scratch >= 4 * cap + 256 * cdiv(cap, 2048) + 256
                assert (table > 0) == (csb > 0) and (not counting or table > 0)


def test_both_sides_of_every_clause():
    held = lambda cap, K, on=True: hook(cap, K, on, cap)[4] > 0
    path = lambda cap, K, n, on=True: hook(cap, K, on, n)[5]
    # the map: CS_MAX_K units and one more
    assert held(5120, 8192) and not held(5120, 8193)
    assert path(5120, 8192, 5000) == 1 and path(5120, 8193, 5000) == 0
    # the capacity: two blocks and one row under
    assert held(2048, 64) and not held(2047, 64)
    assert hook(2048, 64, True, 2048)[3:] == [3 * 64, 2, 1]
    # the table's ceiling: csb * K exactly 2^21, and one row (a 257th block) past it
    assert 256 * 8192 == 2 ** 21
    assert hook(262144, 8192, True, 262144)[3:] == [257 * 8192, 256, 1]
    assert hook(262145, 8192, True, 262145)[3:] == [0, 0, 0]
    # the switch
    assert not held(5120, 64, on=False) and path(5120, 64, 5000, on=False) == 0
    # under a table: two blocks of rows and one row under
    assert path(5120, 64, 2048) == 1 and path(5120, 64, 2047) == 0
    # more blocks of rows than the table was sized for: 5 blocks held, 5 120 rows fit, 5 121 need a sixth
    assert hook(5120, 64, True, 5120)[4:] == [5, 1] and path(5120, 64, 5121) == 0
    # (and fewer: three blocks inside the five-block table)
    assert path(5120, 64, 3000) == 1


def _case_pairs():
    pairs = {(c["X"] * c["Y"], c["N"]) for c in test_gpu_update_ref.CASES}
    pairs |= {(c["X"] * c["Y"], c["n"]) for c in diag_ref.CASES}
    pairs |= {(c["X"] * c["Y"], c["n"]) for c in test_gpu_project.CASES}
    pairs |= {(K, n) for K in UNITS for n in ROWS}
    return sorted(pairs)


def test_the_python_restatement_agrees_with_the_rule():
    """update_ref.sort_path(K, n) is the sort n rows take where the scratch was sized for them: a fresh resident set (capacity
    n, seg_reserve) and a first query or first streamed chunk (capacity round_up(n, 1 024): rowset::QUERY_PAD, stream_rows)."""
    pairs = _case_pairs()
    assert len(pairs) > 80
    seen = set()
    for K, n in pairs:
        for cap in (n, up(n, 1024)):
            got = "counting" if hook(cap, K, True, n)[5] else "radix"
            assert U.sort_path(K, n) == got, (K, n, cap)
            assert hook(cap, K, False, n)[5] == 0
        seen.add(U.sort_path(K, n))
        assert "sort." + U.sort_path(K, n) in U.update_paths(K, 1, 3, "gaussian", "rectangular", False, n) or n == 0
        assert diag_ref.sort_path(dict(X=K, Y=1, n=n)) == U.sort_path(K, n)
    assert seen == {"counting", "radix"}


def test_bad_arguments():
    lib = _lib.load()
    out = (C.c_int64 * 6)()
    assert lib.som_debug_unit_sort_sizes(2048, 64, 1, 2048, out) == 0
    assert lib.som_debug_unit_sort_sizes(2048, 64, 1, 2048, None) != 0
    assert lib.som_debug_unit_sort_sizes(-1, 64, 1, 0, out) != 0
    assert lib.som_debug_unit_sort_sizes(2048, 64, 1, -1, out) != 0
    assert lib.som_debug_unit_sort_sizes(2048, 0, 1, 2048, out) != 0
    assert lib.som_debug_unit_sort_sizes(2048, -5, 1, 2048, out) != 0
