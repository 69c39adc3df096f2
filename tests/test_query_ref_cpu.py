"""The float64 query reference (tests/query_ref.py) itself: it agrees with the oracle within its bounds, its checks reject
plausible wrong answers, and the GPU module's case list reaches every label of the host's query dispatch.  No GPU needed."""
import numpy as np
import pytest

from oracle import som_oracle as O
from tests import test_gpu_query_ref as G
from tests.query_ref import (ALL_LABELS, F32, F64, check_matrix, check_picks, check_qe, check_ties, check_top2, is_exact,
                             make_rows, make_units, query_paths, scores)


def _f32_scores(x, w, mode):
    """The float32 evaluation the GEMM kernels do, emulated in NumPy float32 (a different summation order: still inside
    the bound)."""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    if mode == "part":
        return O.dist_euclid_part(x, w)
    if mode == "sq":
        return O.dist_euclid_sq(x, w)
    if mode == "sqrt":
        return O.dist_euclid(x, w)
    return O.dist_cosine(x, w)


@pytest.fixture(scope="module", params=["blobs", "offset30", "offset300", "int"])
def data(request):
    x = make_rows(request.param, 300, 37, 5)
    w = make_units(request.param, x, 150, 37, 5, dup=3)
    return request.param, x, w


# ------------------------------------------------------------------------------------------------ reference vs the oracle
@pytest.mark.parametrize("mode", ["part", "sq", "sqrt", "cosine"])
def test_gemm_forms_agree_with_the_oracle(data, mode):
    kind, x, w = data
    s, E = scores(x, w, mode)
    got = _f32_scores(x, w, mode)
    check_matrix(got, s, E, mode)
    ids = np.argmin(got, axis=1)
    check_picks(ids, s, E, mode)
    if mode in ("part", "sq"):
        assert (ids == O.bmu_ids(x, w, {"part": "euclidean", "sq": "euclidean_no_opt"}[mode])).all()
    if kind == "int" and mode != "cosine":
        check_ties(ids, s, mode)


def test_quantization_top2_and_qe_agree_with_the_oracle(data):
    kind, x, w = data
    s, E = scores(x, w, "sqrt")
    ids = O.quantization_ids(x, w.reshape(1, -1, w.shape[1]))
    check_picks(ids, s, E, "quantization")
    t = O.top2_ids(x, w.reshape(1, -1, w.shape[1]))
    # the oracle's argsort is not stable: on exact ties its pair may come in either order -- compare values
    if kind == "int":
        srt = np.sort(s, axis=1)
        assert (s[np.arange(len(x)), t[:, 0]] == srt[:, 0]).all() and (s[np.arange(len(x)), t[:, 1]] == srt[:, 1]).all()
    else:
        check_top2(t[:, 0], t[:, 1], s, E, "top2")
    check_qe(O.quantization_error(x, w.reshape(1, -1, w.shape[1])), x, w, ids, "qe")


@pytest.mark.parametrize("p", [1, 2, 3, 4, 16])
def test_pairwise_forms_agree_with_the_oracle(p):
    x = make_rows("blobs", 40, 11, 2) / 3
    w = make_units("blobs", x, 20, 11, 2)
    even = p % 2 == 0
    s, E = scores(x, w, "even" if even else "generic", p=p)
    ref = O.dist_norm_p(x.astype(F64), w.astype(F64), p) if even else O.dist_norm_p_generic(x, w, p)
    check_matrix(ref, s, E, "p=%d" % p)
    check_picks(O.bmu_ids_pairwise(x, w, "norm_p", p), s, E, "p=%d" % p)
    if p == 1:
        check_picks(O.bmu_ids_pairwise(x, w, "manhattan"), s, E, "manhattan")


def test_real_p_and_float64_rows():
    x = make_rows("blobs", 40, 9, 3)
    w = make_units("blobs", x, 25, 9, 3)
    s, E = scores(x, w, "generic", p_real=2.5)
    check_matrix(np.power(np.abs(x[:, None, :] - w[None]), F32(2.5)).sum(-1), s, E, "p=2.5")
    x64 = x.astype(F64) * (1 + 2.0 ** -40)
    s, E = scores(x64, w, "f64")
    wsq = O.row_sq(w).astype(F64)
    check_matrix(-2 * x64 @ w.astype(F64).T + wsq.T, s, E, "f64")


def test_cosine_zero_rows_and_units():
    x = make_rows("blobs", 20, 5, 4)
    w = make_units("blobs", x, 9, 5, 4)
    x[3] = 0
    w[2] = 0
    s, E = scores(x, w, "cosine")
    assert (s[3] == 1).all() and (s[:, 2] == 1).all() and (E[3] == 0).all() and (E[:, 2] == 0).all()
    check_matrix(O.dist_cosine(x, w), s, E, "cosine")


# ------------------------------------------------------------------------------------------------ the checks have teeth
@pytest.fixture(scope="module")
def case():
    """blobs with a last feature of large variance and a map whose last partial 128-unit tile holds the BMUs of rows"""
    rs = np.random.RandomState(7)
    x = make_rows("blobs", 400, 20, 7)
    x[:, -1] *= 30
    w = make_units("blobs", x, 200, 20, 7)
    w[150:] = x[rs.randint(0, 400, 50)]                  # the last 72 units sit on rows: they are BMUs
    return x, w


def test_unmutated_answers_pass(case):
    x, w = case
    s, E = scores(x, w, "sqrt")
    ids = np.argmin(_f32_scores(x, w, "sqrt"), axis=1)
    check_picks(ids, s, E)
    d = _f32_scores(x, w, "sqrt")
    o = np.argsort(d, axis=1, kind="stable")
    check_top2(o[:, 0], o[:, 1], s, E)
    check_qe(np.linalg.norm(x.astype(F64) - w[ids].astype(F64), axis=1).mean(), x, w, ids)


def test_rejects_a_dropped_last_feature(case):
    x, w = case
    s, E = scores(x, w, "part")
    bad = _f32_scores(x[:, :-1], w[:, :-1], "part")
    with pytest.raises(AssertionError):
        check_matrix(bad, s, E)
    with pytest.raises(AssertionError):
        check_picks(np.argmin(bad, axis=1), s, E)


def test_rejects_a_skipped_last_unit_tile(case):
    x, w = case
    s, E = scores(x, w, "part")
    d = _f32_scores(x, w, "part")
    with pytest.raises(AssertionError):
        check_picks(np.argmin(d[:, :128], axis=1), s, E)


def test_rejects_the_second_best_as_best(case):
    x, w = case
    s, E = scores(x, w, "sqrt")
    o = np.argsort(_f32_scores(x, w, "sqrt"), axis=1, kind="stable")
    with pytest.raises(AssertionError):
        check_picks(o[:, 1], s, E)


def test_rejects_a_swapped_pair(case):
    x, w = case
    s, E = scores(x, w, "sqrt")
    o = np.argsort(_f32_scores(x, w, "sqrt"), axis=1, kind="stable")
    with pytest.raises(AssertionError):
        check_top2(o[:, 1], o[:, 0], s, E)


def test_rejects_a_tie_won_by_the_higher_index():
    x = make_rows("int", 200, 6, 9)
    w = make_units("int", x, 40, 6, 9, dup=10)
    for mode in ("part", "sqrt"):
        s, E = scores(x, w, mode)
        ids = np.argmin(s, axis=1)
        check_ties(ids, s, mode)
        rev = w.shape[0] - 1 - np.argmin(s[:, ::-1], axis=1)      # the last of the equal minima
        assert (rev != ids).any()
        check_picks(rev, s, E)                                    # (admissible: the same value ...)
        with pytest.raises(AssertionError):                       # ... but not the lowest id
            check_ties(rev, s, mode)
    s, E = scores(x, w, "sqrt")
    o = np.argsort(s, axis=1, kind="stable")
    check_top2(o[:, 0], o[:, 1], s, E, exact=True)
    twin = (o[:, 0] < 10) & (s[np.arange(200), o[:, 0]] == s[np.arange(200), o[:, 1]])
    assert twin.any()
    a, b = o[:, 0].copy(), o[:, 1].copy()
    a[twin], b[twin] = b[twin], a[twin]
    with pytest.raises(AssertionError):
        check_top2(a, b, s, E, exact=True)


def test_rejects_one_bmu_off_by_one(case):
    x, w = case
    s, E = scores(x, w, "sqrt")
    ids = np.argmin(_f32_scores(x, w, "sqrt"), axis=1)
    bad = ids.copy()
    bad[17] = (bad[17] + 1) % w.shape[0]
    with pytest.raises(AssertionError):
        check_picks(bad, s, E)


def test_rejects_a_qe_from_other_ids(case):
    x, w = case
    ids = np.argmin(_f32_scores(x, w, "sqrt"), axis=1)
    other = np.argmin(_f32_scores(x, w, "part")[:, ::-1], axis=1)
    other = w.shape[0] - 1 - other
    other[::7] = (ids[::7] + 3) % w.shape[0]
    qe_other = np.linalg.norm(x.astype(F64) - w[other].astype(F64), axis=1).mean()
    with pytest.raises(AssertionError):
        check_qe(qe_other, x, w, ids)


def test_the_square_root_rule_and_the_part_rule_differ_on_offset_data():
    """what the exact mode's value-only search must not do: float32's argmin of |w|^2 - 2 x.w is not float32's argmin of
    the sqrt'd distance on un-centred data, and the QE of the two id sets differs"""
    rs = np.random.RandomState(0)
    w = (50.0 + rs.normal(0.0, 1e-2, (256, 32))).astype(F32)
    x = w.copy()
    part = np.argmin(_f32_scores(x, w, "part"), axis=1)
    sqrt = np.argmin(_f32_scores(x, w, "sqrt"), axis=1)
    assert (part != sqrt).mean() > 0.5
    q_part = np.linalg.norm(x.astype(F64) - w[part].astype(F64), axis=1).mean()
    with pytest.raises(AssertionError):
        check_qe(q_part, x, w, sqrt)


# ------------------------------------------------------------------------------------------------ the grid's coverage
def _reached():
    reached = set()
    for c in G.CASES:
        for call in c["calls"]:
            reached |= query_paths(c["X"], c["Y"], c["D"], c["n"], c["prec"], c["dist"], call, c["env"], c["p"], c["p_real"])
    return reached


def test_grid_reaches_every_query_path():
    reached = _reached()
    assert ALL_LABELS - reached == set()
    assert reached <= ALL_LABELS


def test_grid_covers_the_edges():
    assert {c["D"] for c in G.CASES} >= {1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 265, 266, 784, 800}
    Ks = {c["X"] * c["Y"] for c in G.CASES}
    assert Ks >= {1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129} and max(Ks) >= 2000
    ns = {c["n"] for c in G.CASES}
    assert ns >= {1, 127, 128, 129, 255, 256, 257} and max(ns) > 16384
    assert {c["data"] for c in G.CASES} >= {"blobs", "offset30", "offset300", "int"}
    assert {(c["dist"], c["p"], c["p_real"]) for c in G.CASES if c["dist"].startswith("norm_p")} >= {
        ("norm_p", 2, 0.0), ("norm_p", 3, 0.0), ("norm_p", 4, 0.0), ("norm_p", 16, 0.0), ("norm_p", 2, 2.5),
        ("norm_p_no_opt", 2, 0.0)}
    assert {"manhattan", "euclidean_no_opt", "cosine"} <= {c["dist"] for c in G.CASES}
    calls = {call for c in G.CASES for call in c["calls"]}
    assert calls == {"bmu", "quant", "top2", "dist", "dist_q", "f64", "qe", "qe_dev"}


def test_query_paths_follows_the_dispatch_rules():
    assert query_paths(1, 1, 8, 1, "f32", "euclidean", "bmu") == {"f32.res.kg1", "f32.res.kg1.single"}
    assert query_paths(3, 43, 64, 5, "f32", "euclidean", "bmu") == {"f32.res.kg8"}            # (occupancy decides)
    assert "f32.res.kg8.multi" in query_paths(3, 43, 64, 5, "f32", "euclidean", "bmu", {"SOM_F32_PARTS": "2"})
    assert "f32.res.kg16.top2" in query_paths(3, 43, 65, 5, "f32", "euclidean", "top2")
    assert query_paths(3, 43, 129, 5, "bf16", "euclidean", "top2") == {"f32.tiled.top2"}
    assert query_paths(1, 2, 265, 5, "f32", "norm_p", "bmu", p=4) == {"pairwise.even.lds"}
    assert query_paths(1, 2, 266, 5, "f32", "norm_p", "bmu", p=4) == {"pairwise.even.global"}
    assert query_paths(1, 2, 26, 5, "f32", "norm_p", "bmu", p=3) == {"pairwise.generic.lds"}
    assert query_paths(1, 2, 26, 5, "f32", "norm_p", "bmu", p=2, p_real=2.5) == {"pairwise.real.lds"}
    assert query_paths(4, 16, 32, 16384, "exact", "euclidean", "qe") == {"qe.exact_screen", "qe.one_pass"}
    assert query_paths(4, 16, 32, 16385, "exact", "euclidean", "qe") == {"qe.exact_screen", "qe.stride"}
    assert "f32.res.kg4" in query_paths(4, 16, 32, 10, "exact", "euclidean", "quant")
    assert query_paths(3, 43, 32, 129, "f32", "cosine", "dist") == {"dist.cosine", "dist.rowtiles2+", "dist.unittiles2+"}
    # 'exact' beyond 128 features: the wide screen on >= 4096 units, else the float32 kernels
    assert is_exact(64, 64, 200, "exact", "euclidean") and not is_exact(8, 8, 200, "exact", "euclidean")
    assert not is_exact(8, 8, 20, "exact", "cosine") and is_exact(64, 64, 200, "exact", "cosine")
    assert "f32.tiled" in query_paths(8, 8, 200, 10, "exact", "euclidean", "qe")
