"""tests/topk_ref.py itself -- the oracle, the admissibility check, the pinned share, the plan mirror, the histogram weights -- and
the host-side pieces of the k nearest units that need no GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import query_ref as Q
from tests import topk_ref as T

F32, F64 = np.float32, np.float64
INF, NAN = np.inf, np.nan


def test_oracle_on_hand_made_rows():
    s = np.array([
        [3.0, 1.0, 2.0, 1.0, 5.0],            # a tie: the lower id first
        [0.0, -0.0, 1.0, -0.0, 0.0],          # -0.0 == +0.0: ids in order
        [NAN, 2.0, INF, 1.0, NAN],            # NaN and +inf never enter: two filled slots
        [-INF, 4.0, -INF, 0.0, INF],          # -inf enters, and ties with itself
        [NAN, NAN, NAN, NAN, NAN],            # nothing enters
        [INF, INF, 7.0, INF, INF],            # one score below +inf
    ], F32)
    got = T.topk_lowest(s, 3)
    want = np.array([[1, 3, 2], [0, 1, 3], [3, 1, -1], [0, 2, 3], [-1, -1, -1], [2, -1, -1]])
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(T.topk_lowest(s, 1), want[:, :1])
    # k beyond the units: the spare slots are -1
    assert np.array_equal(T.topk_lowest(s[:, :2], 3), np.array([[1, 0, -1], [0, 1, -1], [1, -1, -1], [0, 1, -1], [-1, -1, -1], [-1, -1, -1]]))
    # the gathered scores: NaN where nothing was listed
    g = T.gather(s, got)
    assert np.array_equal(np.isnan(g), got < 0) and g[0].tolist() == [1.0, 1.0, 2.0] and g[3].tolist() == [-INF, -INF, 0.0]
    # the first k of a longer list are the shorter list
    assert np.array_equal(T.topk_lowest(s, 5)[:, :3], got)


def test_bit_comparisons():
    a = np.array([[0.0, 1.0, NAN]], F32)
    assert T.same_bits(a, a.copy()) and not T.same_bits(a, np.array([[-0.0, 1.0, NAN]], F32))
    assert T.same_bits_or_nan(a, a.copy()) and not T.same_bits_or_nan(a, np.array([[0.0, NAN, NAN]], F32))
    assert not T.same_bits_or_nan(a, np.array([[-0.0, 1.0, NAN]], F32))


def _case(c, mode):
    x, w = T.case_data(c)
    return Q.scores(x, w, mode)


def test_check_topk_accepts_the_float64_order_and_rejects_a_wrong_list():
    c = T.CASES[2]
    s, E = _case(c, "part")
    for k in T.KS:
        ids = T.topk_lowest(s, k)
        assert T.check_topk(ids, s, E, k, "float64 order") == 0.0
    k = 5
    ids = T.topk_lowest(s, k)
    pinned = np.flatnonzero(T.pinned_rows(s, E, k))
    i = int(pinned[0])
    swapped = ids.copy()
    swapped[i, [1, 3]] = swapped[i, [3, 1]]
    with pytest.raises(AssertionError, match="row %d " % i):
        T.check_topk(swapped, s, E, k, "swapped")
    dup = ids.copy()
    dup[i, 4] = dup[i, 0]
    with pytest.raises(AssertionError, match="twice"):
        T.check_topk(dup, s, E, k, "duplicated")
    far = ids.copy()
    far[i, 4] = int(np.argmax(s[i]))                        # the farthest unit in the last slot
    with pytest.raises(AssertionError, match="row %d " % i):
        T.check_topk(far, s, E, k, "a far unit")
    out = ids.copy()
    out[i, 2] = s.shape[1]
    with pytest.raises(AssertionError, match="out of range"):
        T.check_topk(out, s, E, k, "out of range")
    with pytest.raises(AssertionError, match="out of range"):
        T.check_topk(np.where(ids == ids[i, 0], -1, ids), s, E, k, "unfilled")
    # a list that is in order but misses the nearest unit
    shifted = T.topk_lowest(s, k + 1)[:, 1:]
    with pytest.raises(AssertionError):
        T.check_topk(shifted, s, E, k, "shifted")


def test_check_topk_with_k_equal_to_the_units():
    c = T.CASES[1]
    s, E = _case(c, "sq")
    assert T.check_topk(T.topk_lowest(s, 8), s, E, 8, "k = K") == 0.0
    assert T.pinned_share(s, E, 8) == 1.0                   # (nothing behind the eighth: only the neighbours count)


@pytest.mark.parametrize("c", T.BLOB_CASES, ids=[c["id"] for c in T.BLOB_CASES])
def test_pinned_shares_are_a_condition(c):
    """At least 90 % of every blobs case's rows admit ONE list of k = 8 (of k = K on the smaller maps): the admissibility check
    cannot hide a wrong list behind its bounds on them.  Measured here: 91.4 % (9x37, d130, cosine) to 100 %."""
    K = c["X"] * c["Y"]
    for mode in ("part", "sq", "cosine"):
        s, E = _case(c, mode)
        share = T.pinned_share(s, E, min(8, K))
        print("%s %s: %.1f %% of the rows pinned" % (c["id"], mode, 100 * share))
        assert share >= 0.90, "%s %s: only %.1f %% of the rows pinned" % (c["id"], mode, 100 * share)


def test_pinned_rows_on_a_hand_made_matrix():
    s = np.array([[0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 1.05, 3.0], [0.0, 1.0, 2.0, 2.05], [0.0, 1.0, 3.0, 0.95]])
    E = np.full_like(s, 0.04)
    # gaps must exceed 0.08.  Row 1: the second and third are 0.05 apart; row 2: the third and fourth; row 3: units 3 and 1
    assert T.pinned_rows(s, E, 1).tolist() == [True, True, True, True]
    assert T.pinned_rows(s, E, 2).tolist() == [True, False, True, False]
    assert T.pinned_rows(s, E, 3).tolist() == [True, False, False, False]
    assert T.pinned_share(s, E, 2) == 0.5


def test_plan_mirror_is_the_library_and_leaves_no_part_empty():
    from xpysom_dask_amd import _lib
    lib = _lib.load()
    out = (C.c_int64 * 4)()
    rs = np.random.RandomState(7)
    cases = [(1, 1, 512, 0), (260, 8, 512, 0), (1000, 200, 512, 64), (128, 65536, 512, 0), (262144, 65536, 512, 0),
             (129, 129, 1, 3), (5000, 65536, 512, 7), (300, 16384, 1024, 1000)]
    cases += [(int(rs.randint(1, 1 << 19)), int(rs.randint(1, 1 << 17)), int(rs.randint(1, 2048)), int(rs.choice([0, 0, 1, 3, 64, 5000])))
              for _ in range(300)]
    for n, K, slots, forced in cases:
        assert lib.som_debug_topk_plan(n, K, slots, forced, out) == 0
        row_tiles, stages, parts, per = list(out)
        assert (row_tiles, stages, parts, per) == T.plan(n, K, slots, forced), (n, K, slots, forced)
        assert row_tiles == -(-n // 128) and stages == -(-K // 128)
        assert 1 <= parts <= stages and per >= 1
        assert (parts - 1) * per < stages <= parts * per          # every part holds a stage, every stage has a part
        if forced == 0 and row_tiles >= slots:
            assert parts == 1                                     # the rows fill the chip on their own
    for bad in ((0, 8, 512, 0), (10, 0, 512, 0), (10, 8, 0, 0), (10, 8, 512, -1), (1 << 31, 8, 512, 0)):
        assert lib.som_debug_topk_plan(*bad, out) != 0
    assert lib.som_debug_topk_plan(10, 8, 512, 0, None) != 0


def test_sdh_weights_and_the_host_formula():
    from xpysom_dask_amd.xpysom import _sdh
    for s in range(1, 9):
        wgt = T.sdh_weights(s)
        assert abs(wgt.sum() - 1.0) < 1e-15 and (np.diff(wgt) < 0).all() and wgt[-1] == 1 / (s * (s + 1) / 2.0)
    rs = np.random.RandomState(1)
    counts = rs.randint(0, 50, (5, 6, 7)).astype(np.int64)
    assert np.array_equal(_sdh(counts), T.sdh(counts, 5))
    assert _sdh(counts).shape == (6, 7) and _sdh(counts).dtype == F64
    # every sample with a full list adds one point in all: columns of equal sums n
    full = np.zeros((3, 4), np.int64)
    full[0, 1] = full[1, 2] = full[2, 0] = 10
    assert abs(T.sdh(full, 3).sum() - 10.0) < 1e-12
    assert np.array_equal(_sdh(counts[:1]), counts[0].astype(F64))           # s = 1: the hit histogram


def test_k_is_checked_before_any_engine_exists():
    from xpysom_dask_amd.engine import TOPK_MAX, check_topk
    assert TOPK_MAX == T.TOPK_MAX == 8
    assert check_topk(1) == 1 and check_topk(np.int64(8)) == 8
    for bad in (0, 9, -1, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="k must be"):
            check_topk(bad)


def test_xpysom_refuses_by_name_without_an_engine():
    from xpysom_dask_amd import XPySom
    x = np.zeros((4, 3), F32)
    som = XPySom(2, 3, 3, random_seed=1)
    for call in (lambda: som.nearest_units(x, 0), lambda: som.rank_hits(x, 9), lambda: som.smoothed_hits(x, 0)):
        with pytest.raises(ValueError, match="k must be between 1 and 8"):
            call()
    with pytest.raises(ValueError, match="k = 7 exceeds the map's 6 units"):
        som.nearest_units(x, 7)
    with pytest.raises(NotImplementedError, match="nearest_units.*missing='nan'"):
        XPySom(2, 3, 3, random_seed=1, missing="nan").nearest_units(x, 2)
    with pytest.raises(NotImplementedError, match="rank_hits.*GEMM-form.*manhattan"):
        XPySom(2, 3, 3, random_seed=1, activation_distance="manhattan").rank_hits(x, 2)
