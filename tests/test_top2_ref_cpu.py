"""The exact mode's top-2 path restated on the CPU (tests/top2_ref.py): the tie test that lets the float32 top-2 of
q = |w|^2 - 2 x.w stand for the top-2 of the sqrt'd distance, the second-smallest window of the screen, and the C surface.
No GPU: the device side of the same rules is tests/test_gpu_top2.py."""
import re

import numpy as np
import pytest

from tests import top2_ref as T
from tests.conftest import REPO

F32 = np.float32


def _step(q, k):
    """q moved up by k float32 steps, elementwise (k >= 0)."""
    q = np.asarray(q, F32).copy()
    for _ in range(int(np.max(k))):
        q = np.where(k > 0, np.nextafter(q, F32(np.inf)), q).astype(F32)
        k = k - 1
    return q


def _cases(rs):
    """(name, q, xs, built_to_tie) -- float32 score vectors without NaN and the row's |x|^2."""
    K = 40
    for i in range(300):
        xs = F32(rs.uniform(0.1, 50.0))
        yield "random", (rs.normal(0, 5, K) - xs * rs.uniform(0, 1)).astype(F32), xs, False
    for i in range(300):
        # adjacent floats: every score within a few steps of one value
        q0 = F32(rs.uniform(-30, 30))
        yield "adjacent", _step(np.full(K, q0, F32), rs.randint(0, 4, K)), F32(rs.uniform(31, 60)), False
    for i in range(200):
        # exact ties in first and second place (duplicated values, any ids)
        q = rs.normal(0, 3, K).astype(F32)
        lo = np.sort(q)[:2]
        q[rs.randint(0, K, 3)] = lo[0]
        q[rs.randint(0, K, 3)] = lo[1] if i % 2 else lo[0]
        yield "ties", q, F32(rs.uniform(20, 40)), False
    for i in range(300):
        # negative and zero radicands: q + |x|^2 straddles 0 (the sqrt of a negative one is NaN -> 0)
        xs = F32(rs.uniform(1, 100))
        q = (-xs + rs.uniform(-1, 1, K) * xs * F32(2.0 ** -rs.randint(0, 24))).astype(F32)
        if i % 3 == 0:
            q[rs.randint(0, K, 4)] = -xs                     # radicand exactly 0
        yield "radicand<=0", q, xs, True
    for i in range(100):
        q = rs.normal(0, 1, K).astype(F32) ** 2
        q[rs.randint(0, K, 5)] = F32(-0.0)
        q[rs.randint(0, K, 5)] = F32(0.0)
        yield "-0", q, F32(0.0) if i % 2 else F32(rs.uniform(0, 1e-30)), False
    for i in range(300):
        # |x|^2 a million times the distances: the radicand rounds, units at different distances tie under the sqrt
        xs = F32(rs.uniform(1e5, 1e7))
        d = rs.uniform(0.0, 4.0, K)
        yield "offset", (d - np.float64(xs)).astype(F32), xs, True
    for i in range(100):
        q = rs.normal(0, 5, K).astype(F32)
        q[rs.randint(0, K, 3)] = F32(np.inf)
        if i % 4 == 1:
            q[rs.randint(0, K)] = F32(-np.inf)
        xs = F32(np.inf) if i % 4 == 2 else F32(3.0e38) if i % 4 == 3 else F32(rs.uniform(30, 60))
        yield "inf", q, xs, i % 4 != 0


def test_settled_pair_is_the_top2_of_the_sqrt_distance():
    rs = np.random.RandomState(7)
    seen, settled_n, unsettled_tie = {}, 0, 0
    for name, q, xs, tie in _cases(rs):
        assert not np.isnan(q).any()
        b1, b2, ok = T.pair_settled(q, xs)
        seen[name] = seen.get(name, 0) + 1
        if tie and not ok:
            unsettled_tie += 1
        if not ok:
            continue
        settled_n += 1
        want = T.top2_lowest(T.sqrt_distance(q, xs))
        assert (b1, b2) == want, "%s: q-order pair (%d, %d) is settled, the sqrt'd distance names %r (|x|^2 = %r)" % (name, b1, b2, want, xs)
    assert set(seen) == {"random", "adjacent", "ties", "radicand<=0", "-0", "offset", "inf"}
    assert settled_n >= 500                                # (the rule is not vacuous)
    assert unsettled_tie >= 100                            # ... and says "unsettled" on the inputs built to tie


def test_unsettled_where_the_sqrt_ties():
    """Hand-made: two scores one float32 step apart whose radicands round to the same float32 -- the lower one is not settled."""
    xs = F32(1.0e6)
    q = np.array([3.0, np.nextafter(F32(3.0), F32(np.inf)), 5.0], F32)
    assert T.sqrt_distance(q[0], xs) == T.sqrt_distance(q[1], xs)
    assert not T.settled(q[0], xs)
    # (a unit near the row: |q| well above the radicand, one step of q is several steps of the sum)
    assert T.settled(F32(-9.0), F32(10.0)) and not T.settled(F32(np.inf), F32(1.0)) and not T.settled(F32(1.0), F32(np.inf))
    assert not T.settled(F32(-3.0), F32(1.0))              # radicand < 0 on both sides of the step: 0 == 0
    assert T.settled(F32(-0.0), F32(0.0))                  # the step from -0 is the least positive float


def _window_rows(rs, n, K, scenario):
    """float32 scores s (n, K), the row bounds E (n,), screen values within E / 2 of the scores."""
    s = rs.normal(0.0, 1.0, (n, K)).astype(F32)
    if scenario == "quantized":                             # exact ties everywhere
        s = np.round(s * 4).astype(F32) / 4
    r = np.arange(n)
    k1 = rs.randint(0, K, n)
    if scenario == "far":                                   # a best unit far below the rest
        s[r, k1] -= F32(100.0)
    if scenario == "own_group":                             # the second-best unit in the winner's own group
        s[r, k1] -= F32(50.0)
        g0 = k1 // T.EX_GROUP * T.EX_GROUP
        k2 = g0 + (k1 - g0 + 1 + rs.randint(0, min(T.EX_GROUP, K) - 1, n)) % np.minimum(T.EX_GROUP, K - g0)
        s[r, k2] = s[r, k1] + F32(0.5) * (k2 != k1)
    E = (10.0 ** rs.uniform(-4, 0.5, n)).astype(np.float64)
    screen = s.astype(np.float64) + rs.uniform(-0.5, 0.5, (n, K)) * E[:, None]
    return s, E, screen


@pytest.mark.parametrize("K", [64, 100, 192, 1000, 4096])
def test_second_smallest_window_holds_both_units(K):
    rs = np.random.RandomState(K)
    total = 0
    for scenario in ("plain", "quantized", "far", "own_group"):
        n = 700 if K >= 1000 else 1200
        s, E, screen = _window_rows(rs, n, K, scenario)
        order = np.argsort(s, axis=1, kind="stable")        # float32's top-2, lowest ids first
        k1, k2 = order[:, 0], order[:, 1]
        cand = T.window_candidates(screen, E)
        r = np.arange(n)
        assert cand[r, k1 // T.EX_GROUP].all(), "%s: the best unit's group is outside the window" % scenario
        miss = np.flatnonzero(~cand[r, k2 // T.EX_GROUP])
        assert len(miss) == 0, "%s: row %d: the second-best unit's group is outside the window" % (scenario, miss[0])
        # every unit that TIES the second-best is a candidate too (the lowest id is then decided by the re-score)
        tie = s == s[r, k2][:, None]
        gm_tie = np.zeros_like(cand)
        for g in range(cand.shape[1]):
            gm_tie[:, g] = tie[:, g * T.EX_GROUP:(g + 1) * T.EX_GROUP].any(axis=1)
        assert not (gm_tie & ~cand).any()
        # ... and what the select takes, the screen has stored (whatever the number of codebook parts)
        for parts in (1, 3):
            if parts <= cand.shape[1]:
                assert not (cand & ~T.stored_mask(screen, E, parts)).any(), "%s: a candidate the screen did not store (%d parts)" % (scenario, parts)
        total += n
    assert total >= 2800                                    # (five K: 14 000 rows and more in all)


def test_window_on_the_minimum_alone_would_miss_the_second():
    """Why the window moved: within E of the row MINIMUM the second-best unit's group is usually absent."""
    rs = np.random.RandomState(3)
    s, E, screen = _window_rows(rs, 500, 1024, "far")
    gm = T.group_minima(screen)
    old = gm <= (gm.min(axis=1) + E)[:, None]
    k2 = np.argsort(s, axis=1, kind="stable")[:, 1]
    assert (~old[np.arange(500), k2 // T.EX_GROUP]).mean() > 0.9


def test_fast_path_predicate_and_labels():
    assert T.top2_fast_path(64, 64, 32, "exact", "euclidean")
    assert T.top2_fast_path(4, 16, 3, "exact", "euclidean")
    assert not T.top2_fast_path(64, 64, 32, "exact", "euclidean", {"SOM_EXACT_TOP2": "0"})
    assert not T.top2_fast_path(64, 64, 32, "exact", "cosine")
    assert not T.top2_fast_path(64, 64, 130, "exact", "euclidean")
    assert not T.top2_fast_path(64, 64, 32, "f32", "euclidean")
    assert not T.top2_fast_path(64, 64, 32, "bf16", "euclidean")
    assert not T.top2_fast_path(1, 1, 32, "exact", "euclidean")
    assert T.top2_paths(64, 64, 32, 100, "exact", "euclidean") == {"exact.top2", "f32.res.kg4.top2"}
    assert T.top2_paths(64, 64, 32, 100, "f32", "euclidean") == {"f32.res.kg4.top2"}


def _prototype_args(header, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert m, "include/somhip.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_and_binding_declare_the_top2_surface():
    """include/somhip.h declares som_bmu_top2_device and som_exact_top2_stats; _lib.py binds both with matching argument lists."""
    import ctypes as C

    from xpysom_dask_amd import _lib
    header = open(REPO + "/include/somhip.h").read()
    want = {"som_bmu_top2_device": ["som_handle*", "const void*", "int64_t", "int32_t*", "int32_t*"],
            "som_exact_top2_stats": ["som_handle*", "int64_t*", "int64_t*"]}
    ctype_of = {"som_handle*": C.c_void_p, "const void*": C.c_void_p, "int64_t": C.c_int64, "int32_t*": C.POINTER(C.c_int32),
                "int64_t*": C.POINTER(C.c_int64)}
    for name, types in want.items():
        args = _prototype_args(header, name)
        assert [re.sub(r"\s*\w+$", "", a).replace(" *", "*") for a in args] == types, (name, args)
        assert name in _lib.SIGNATURES, "%s is not bound in _lib.py" % name
        res, argtypes = _lib.SIGNATURES[name]
        assert res is C.c_int and argtypes == [ctype_of[t] for t in types], (name, argtypes)
    from xpysom_dask_amd.engine import HipEngine
    assert hasattr(HipEngine, "bmu_top2_device") and hasattr(HipEngine, "exact_top2_stats")
