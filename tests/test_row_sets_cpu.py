"""The row sets' size rule (csrc/row_set.hpp, rowset::sizes) without a GPU, through the library's test hook
som_debug_row_set_sizes (include/somhip_test.h).

The oracle restates, one function per kind, what the three allocation sites did before they shared the rule -- the resident rows
(exactly the rows; |x|^2 only where something reads it), the query scratch (steps of 1 024 rows, its image padded again to 3 072)
and a pinned-chunk slot (3 072 straight away) -- for every configuration som_create can produce.  A buffer that exists holds at
least one element (an allocation of none is one of one); 0 says the set holds no such buffer."""
import ctypes as C

import pytest

from xpysom_dask_amd import _lib

RESIDENT, QUERY, SLOT = range(3)
F32, BF16, F16, EXACT = 0, 1, 3, 5                       # som_config.precision
EUCLIDEAN, EUCLIDEAN_NO_OPT, COSINE, MANHATTAN, NORM_P, NORM_P_NO_OPT = range(6)
ROWS = (0, 1, 1023, 1024, 1025, 3071, 3072, 3073, 100000)
FEATURES = (3, 128, 130, 260)


def up(a, b):
    return (a + b - 1) // b * b


def handle_flags(precision, distance, D, big_map):
    """(f32, exact, needs |x|^2, cosine + tiled, dp) as som_create settles them, or None where it refuses the configuration."""
    exact = False
    if precision in (BF16, F16) and distance not in (EUCLIDEAN, COSINE):
        return None
    if precision == EXACT:
        n_kchunks = up(D, 64) // 64
        wide = D > 128 and big_map and n_kchunks <= 25
        exact = (distance == EUCLIDEAN and D <= 128) or (distance in (EUCLIDEAN, COSINE) and wide)
        if not exact:
            precision = F32                              # the float32 kernels ARE the exact mode there
    f32 = precision == F32
    tiled = not f32 and D > 128
    dp = up(D, 64) if tiled else up(D, 32)
    needs_xsq = exact or (f32 and distance in (EUCLIDEAN_NO_OPT, COSINE))
    return f32, exact, needs_xsq, distance == COSINE and tiled, dp


CONFIGS = {}
for _p, _pn in ((F32, "f32"), (BF16, "bf16"), (F16, "f16"), (EXACT, "exact")):
    for _d in range(6):
        for _big in (False, True):
            if handle_flags(_p, _d, 3, _big) is not None and (_big or _p == EXACT):
                CONFIGS["%s-d%d%s" % (_pn, _d, "-big" if _big and _p == EXACT else "")] = (_p, _d, _big)


def some(n):
    return max(n, 1)


def resident_then(n, D, dp, f32, exact, needs_xsq, cos_tiled):
    xsq = some(n * (2 if exact else 1)) if needs_xsq or (not f32 and cos_tiled) else 0
    Xb = up(n, 3072) * dp if not f32 and n > 0 else 0
    return [n, some(n * D), xsq, Xb, some(n)]


def query_then(n, D, dp, f32, exact, needs_xsq, cos_tiled):
    if n == 0:
        return [0] * 5
    cap = up(n, 1024)
    return [cap, up(n * D, 1024 * D), cap * (2 if exact else 1), 0 if f32 else up(cap, 3072) * dp, cap]


def slot_then(n, D, dp, f32, exact, needs_xsq, cos_tiled):
    if n == 0:
        return [0] * 5
    cap = up(n, 3072)
    return [cap, cap * D, cap * (2 if exact else 1), 0 if f32 else cap * dp, cap]


THEN = {RESIDENT: resident_then, QUERY: query_then, SLOT: slot_then}


def sizes(kind, n, D, dp, f32, exact, needs_xsq, cos_tiled):
    out = (C.c_int64 * 5)()
    flags = (1 if f32 else 0) | (2 if exact else 0) | (4 if needs_xsq else 0) | (8 if cos_tiled else 0)
    assert _lib.load().som_debug_row_set_sizes(kind, n, D, dp, flags, out) == 0
    return list(out)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_sizes_match_the_three_sites(name):
    precision, distance, big = CONFIGS[name]
    for D in FEATURES:
        f32, exact, needs_xsq, cos_tiled, dp = handle_flags(precision, distance, D, big)
        for kind in (RESIDENT, QUERY, SLOT):
            for n in ROWS:
                got = sizes(kind, n, D, dp, f32, exact, needs_xsq, cos_tiled)
                want = THEN[kind](n, D, dp, f32, exact, needs_xsq, cos_tiled)
                assert got == want, (name, kind, n, D, got, want)
                cap, X, xsq, Xb, ids = got
                # the invariants the host code leans on
                assert cap >= n and ids >= cap
                if exact:
                    assert xsq >= 2 * cap and (cap == 0 or xsq == 2 * cap)    # xerr() = xsq + cap is in bounds
                assert Xb % (3072 * dp) == 0 and (f32 or n == 0 or Xb >= up(n, 3072) * dp)
                if kind == RESIDENT:
                    assert cap == n
                    assert (xsq > 0) == (needs_xsq or (not f32 and cos_tiled))


def test_every_flag_combination_appears():
    seen = set()
    for precision, distance, big in CONFIGS.values():
        for D in FEATURES:
            seen.add(handle_flags(precision, distance, D, big)[:4])
    # f32 with and without |x|^2; 16-bit with and without the cosine scratch; exact, and exact + cosine beyond 128 features
    assert seen == {(True, False, False, False), (True, False, True, False), (False, False, False, False),
                    (False, False, False, True), (False, True, True, False), (False, True, True, True)}


def test_bad_arguments():
    lib = _lib.load()
    out = (C.c_int64 * 5)()
    assert lib.som_debug_row_set_sizes(RESIDENT, 10, 8, 32, 1, out) == 0
    assert lib.som_debug_row_set_sizes(3, 10, 8, 32, 1, out) != 0
    assert lib.som_debug_row_set_sizes(-1, 10, 8, 32, 1, out) != 0
    assert lib.som_debug_row_set_sizes(RESIDENT, -1, 8, 32, 1, out) != 0
    assert lib.som_debug_row_set_sizes(RESIDENT, 10, 0, 32, 1, out) != 0
    assert lib.som_debug_row_set_sizes(RESIDENT, 10, 8, 32, 1, None) != 0
