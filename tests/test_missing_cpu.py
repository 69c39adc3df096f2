"""Missing values (`missing='nan'`), the part that needs no GPU: what the constructor accepts and refuses, the calls a
masked model refuses before any engine exists, pickling, the float64 model of tests/missing_ref.py against the definition,
and its error bound against a float32 evaluation of the kernel's two fma chains."""
import pickle

import numpy as np
import pytest

from oracle import som_oracle as O
from tests import missing_ref as M
from tests import query_ref as Q
from tests import update_ref as U
from tests import weights_ref as R
from xpysom_dask_amd import _lib
from xpysom_dask_amd.xpysom import XPySom

F32, F64 = np.float32, np.float64


class NoEngine:
    def __call__(self):
        raise AssertionError("the engine was asked for before the call was refused")


def holes(n=30, d=4, seed=0):
    x = np.random.RandomState(seed).rand(n, d).astype(F32)
    x[3, 1] = np.nan
    return x


# ------------------------------------------------------------------------------------------------------ the constructor
def test_missing_is_keyword_only_and_defaults_to_none():
    assert XPySom(4, 4, 3)._missing is None
    assert XPySom(4, 4, 3, missing='nan')._missing == 'nan'
    with pytest.raises(TypeError):
        XPySom(4, 4, 3, 0, 1, 0.5, 0.01, 'exponential', 'gaussian', 0.5, 'rectangular', 'euclidean', {}, None, 0, False, None,
               False, 'auto', 'nan')


@pytest.mark.parametrize("precision", ["exact", "f32"])
@pytest.mark.parametrize("topology, neighbourhood", [("rectangular", "gaussian"), ("rectangular", "mexican_hat"),
                                                     ("rectangular", "bubble"), ("rectangular", "triangle"),
                                                     ("hexagonal", "gaussian"), ("toroidal", "gaussian")])
def test_constructor_accepts_the_scope(precision, topology, neighbourhood):
    s = XPySom(6, 6, 3, missing='nan', precision=precision, topology=topology, neighborhood_function=neighbourhood)
    assert s._missing == 'nan'


@pytest.mark.parametrize("kw, what", [
    (dict(missing='NaN'), "missing must be None or 'nan'"),
    (dict(missing=True), "missing must be None or 'nan'"),
    (dict(missing='nan', precision='bf16'), "precision 'exact' or 'f32', not 'bf16'"),
    (dict(missing='nan', precision='f16'), "precision 'exact' or 'f32', not 'f16'"),
    (dict(missing='nan', activation_distance='cosine'), "'euclidean' only, got 'cosine'"),
    (dict(missing='nan', activation_distance='euclidean_no_opt'), "'euclidean' only"),
    (dict(missing='nan', activation_distance='manhattan'), "'euclidean' only"),
    (dict(missing='nan', activation_distance='norm_p'), "'euclidean' only"),
])
def test_constructor_refuses(kw, what):
    with pytest.raises(ValueError, match=what):
        XPySom(4, 4, 3, **kw)


def test_engine_wrapper_refuses_an_unknown_mode_before_loading_anything():
    from xpysom_dask_amd.engine import HipEngine
    with pytest.raises(ValueError, match="missing must be None or 'nan'"):
        HipEngine(4, 4, 3, missing='zero')


def test_the_keyword_reaches_the_engine(monkeypatch):
    from xpysom_dask_amd import engine as eng_mod
    seen = {}

    class Recorder:
        def __init__(self, *a, **kw):
            seen.update(kw)

    monkeypatch.setattr(eng_mod, "HipEngine", Recorder)
    XPySom(4, 4, 3, missing='nan')._engine()
    assert seen["missing"] == 'nan'
    seen.clear()
    XPySom(4, 4, 3)._engine()
    assert "missing" not in seen


def test_config_struct_ends_with_the_mode():
    assert _lib.SomConfig._fields_[-1][0] == "missing"
    assert _lib.SOM_MISSING == {None: 0, "nan": 1}
    cfg = _lib.SomConfig(4, 4, 3, 0, 0, 0, 0, 0, 0.5, None, 0, 0, 0.0)
    assert cfg.missing == 0                                 # thirteen positional fields, as before: the mode stays off
    assert "som_epoch_fetch_masked" in _lib.SIGNATURES


# ------------------------------------------------------------------------------------------------------ refused calls
@pytest.mark.parametrize("call", ["topographic_error", "activate", "distance_from_weights"])
def test_analysis_calls_without_a_masked_definition_raise(monkeypatch, call):
    s = XPySom(4, 4, 4, missing='nan', random_seed=1)
    monkeypatch.setattr(s, "_engine", NoEngine())
    with pytest.raises(NotImplementedError, match="missing='nan'"):
        getattr(s, call)(holes())


@pytest.mark.parametrize("call", ["random_weights_init", "pca_weights_init"])
def test_initialisers_refuse_data_with_a_nan(call):
    s = XPySom(4, 4, 4, missing='nan', random_seed=1)
    before = s.get_weights().copy()
    with pytest.raises(ValueError, match="NaN"):
        getattr(s, call)(holes())
    assert np.array_equal(before, s.get_weights())
    getattr(s, call)(np.nan_to_num(holes()))                # complete rows are taken as ever
    assert np.isfinite(s.get_weights()).all()


# ------------------------------------------------------------------------------------------------------ pickling
def test_pickle_round_trip_carries_the_keyword():
    s = XPySom(5, 4, 3, missing='nan', random_seed=2)
    t = pickle.loads(pickle.dumps(s))
    assert t._missing == 'nan' and t._engine_obj is None
    assert np.array_equal(t.get_weights(), s.get_weights())
    with pytest.raises(NotImplementedError):
        t.topographic_error(holes(d=3))
    u = pickle.loads(pickle.dumps(XPySom(5, 4, 3, random_seed=2)))
    assert u._missing is None


def test_a_pickle_from_before_the_keyword_loads_unmasked():
    s = XPySom(5, 4, 3, random_seed=2)
    state = s.__getstate__()
    del state['_missing']
    t = XPySom.__new__(XPySom)
    t.__setstate__(state)
    assert t._missing is None


# ------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("X, Y, D", [(5, 7, 3), (12, 11, 6)])
@pytest.mark.parametrize("pattern", M.PATTERNS)
@pytest.mark.parametrize("family", ["gaussian", "mexican_hat", "bubble", "triangle", "hex_gaussian"])
def test_update_model_against_brute_force(X, Y, D, pattern, family):
    neigh, topo, compact = U.FAMILIES[family]
    N = 150
    rs = np.random.RandomState(X + D)
    bmu = U.make_bmu("skewed", X, Y, N, rs)
    x = M.punch(U.make_data(N, D, 1.0, 5), pattern, 3, bmu)
    kw = dict(wide=True, neighbourhood=neigh, topology=topo, compact=compact)
    num, den, mnum, mden = M.reference_update_masked(x, bmu, X, Y, 0.5, 2.0, **kw)
    bnum, bden = M.brute_force_update(x, bmu, X, Y, 0.5, 2.0, **kw)
    assert np.allclose(num, bnum, rtol=1e-12, atol=1e-12 * max(1.0, mnum.max()))
    assert np.allclose(den, bden, rtol=1e-12, atol=1e-12 * max(1.0, mden.max()))
    assert (mnum >= np.abs(num) - 1e-12).all() and (mden >= np.abs(den) - 1e-12).all()
    assert np.isfinite(num).all() and np.isfinite(den).all()
    if pattern == "feature":
        assert (den[:, D // 2] == 0).all() and (num[:, D // 2] == 0).all()
    if pattern == "none":                                   # complete rows: every column of den is the unmasked den
        unum, uden, _, _ = U.reference_update(x, bmu, X, Y, 0.5, 2.0, **kw)
        assert np.allclose(num, unum, rtol=1e-12, atol=1e-300) and np.allclose(den, uden[:, None], rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("X, Y, D", [(5, 7, 3), (12, 11, 6)])
def test_weighted_update_model_against_brute_force(X, Y, D):
    N = 150
    rs = np.random.RandomState(X)
    bmu = U.make_bmu("spread", X, Y, N, rs)
    x = M.punch(U.make_data(N, D, 1.0, 6), "random30", 4)
    w = R.make_weights(N, 7)
    x[np.flatnonzero(w == 0)[0]] = np.inf                   # a row of weight 0 is not read
    num, den, mnum, mden = M.reference_update_masked(x, bmu, X, Y, 0.5, 2.0, wide=False, weights=w)
    bnum, bden = M.brute_force_update(x, bmu, X, Y, 0.5, 2.0, wide=False, weights=w)
    assert np.isfinite(num).all()
    assert np.allclose(num, bnum, rtol=1e-12, atol=1e-12 * mnum.max()) and np.allclose(den, bden, rtol=1e-12, atol=1e-12 * mden.max())


@pytest.mark.parametrize("X, Y, D", [(5, 7, 3), (12, 11, 6)])
@pytest.mark.parametrize("pattern", M.PATTERNS)
def test_score_model_against_the_definition(X, Y, D, pattern):
    K, N = X * Y, 200
    x = M.punch(Q.make_rows("blobs", N, D, 1), pattern, 2)
    w = Q.make_units("blobs", np.nan_to_num(x), K, D, 1)
    s, E = M.masked_scores(x, w)
    xt, m = M.split(x)
    full = M.masked_sq_dist(x, w)
    brute = np.zeros((N, K))
    for n in range(N):
        for k in range(K):
            brute[n, k] = sum((float(x[n, d]) - float(w[k, d])) ** 2 for d in range(D) if x[n, d] == x[n, d])
    assert np.allclose(full, brute, rtol=1e-13, atol=1e-13)
    assert np.allclose(s + (xt * xt).sum(1)[:, None], full, rtol=1e-12, atol=1e-10)
    assert (E >= 0).all() and np.isfinite(E).all()
    none = np.flatnonzero(m.sum(1) == 0)
    assert (s[none] == 0).all() and (E[none] == 0).all() and (M.masked_bmu(x, w)[none] == 0).all()
    assert Q.check_picks(M.masked_bmu(x, w), s, E, pattern) == 0.0


# ------------------------------------------------------------------------------------------------------ the large grid
def test_masked_grid_reaches_every_update_branch():
    """The rows of tests/test_gpu_missing_large.py reach, with UD = 2 D wide rows, every transform tile, both stage-2
    forms, the bands, the swapped order, the hexagonal class copies, the toroidal wrap kernels, the run sum's 16-, 4-,
    2- and 1-wave workgroups (8 waves: tests/test_gpu_missing.py at D = 260), both parities and both sorts; and on every
    row the merge check covers at least MIN_MERGE_SHARE of the (unit, feature) elements -- from the reference alone."""
    reached = set()
    for row in M.LARGE_FORCED:
        fam, X, Y, D, N = row[:5]
        neigh, topo, compact = M.family_of(fam)
        reached |= U.update_paths(X, Y, D, neigh, topo, compact, N, masked=True)
    want = ({"%s.%s" % (s, b) for s in ("s1", "s2")
             for b in ("tile64", "tile128", "narrow2", "narrow4", "narrow_none", "rows1", "rows2", "rows3+", "last1", "wrap")}
            | {"s2.per_column", "s2.whole_rows", "bands.on", "bands.off", "swapped.on", "swapped.off", "hex.classes0",
               "hex.classes3", "hex.classes4", "seg.waves16", "seg.waves4", "seg.waves2", "seg.waves1", "seg.vec2", "seg.vec1",
               "sort.counting", "sort.radix", "runsum.upper", "runsum.single"})
    assert want - reached == set()
    assert reached <= U.ALL_LABELS | U.TORUS_LABELS
    assert len(set(M.LARGE_FORCED)) == len(M.LARGE_FORCED)
    for row in M.LARGE_FORCED:
        c = M.large_forced_case(row)
        share = M.merge_share(c["ref"], c["mexican"])
        print("%s: the merge check covers %.4f of the elements" % (M.large_id(row), share))
        assert share >= M.MIN_MERGE_SHARE, M.large_id(row)
        assert np.isnan(c["data"]).any() and all(np.isfinite(a).all() for a in c["ref"])


def _f32_case(row):
    """(case, num, den): a LARGE_FORCED row and its reference rounded to float32 -- what a correct kernel may return."""
    c = M.large_forced_case(row)
    return c, c["ref"][0].astype(F32), c["ref"][1].astype(F32)


def _row(X, Y, D):
    return next(r for r in M.LARGE_FORCED if r[1:4] == (X, Y, D))


def test_large_grid_control_the_model_from_the_unit_rows_passes():
    """the control of the two mutants below: the true per-unit rows give the reference, and its float32 rounding passes"""
    for row in (_row(5, 7, 600), _row(129, 5, 64)):
        fam, X, Y, D, N, _, _, sigma, wide = row
        c, num, den = _f32_case(row)
        assert M.check_accumulators(num, den, c["ref"]) < 0.1
        assert M.check_merge(c["w0"], M.merge(c["w0"], num, den), num, den, c["ref"]) < 0.1
        sc = M.unit_rows(c["data"], c["bmu"], X * Y)
        assert (sc[:, -1] == np.bincount(c["bmu"], minlength=X * Y)).all()
        mnum, mden = M.update_from_unit_rows(sc[:, :-1], X, Y, M.LARGE_ETA, sigma, wide=wide, std_coeff=M.LARGE_STD)
        assert M.check_accumulators(mnum.astype(F32), mden.astype(F32), c["ref"]) < 0.1


def test_checker_rejects_rows_laid_out_with_the_unmasked_row_pitch():
    """The per-unit rows [S | C | count] of a masked handle written D1p = round_up(D + 1, 4) floats apart -- the pitch of
    a handle without missing values -- instead of round_up(2 D + 1, 4): every row's counts are overwritten by the next
    row's sums before the transform reads them."""
    row = _row(5, 7, 600)
    fam, X, Y, D, N, _, _, sigma, wide = row
    c = M.large_forced_case(row)
    K, width = X * Y, 2 * D + 1
    sc = M.unit_rows(c["data"], c["bmu"], K)
    for pitch, good in ((-(-(2 * D + 1) // 4) * 4, True), (-(-(D + 1) // 4) * 4, False)):
        flat = np.zeros(K * pitch + width)
        for k in range(K):                                   # unit by unit, as the run sum stores them
            flat[k * pitch:k * pitch + width] = sc[k]
        read = np.stack([flat[k * pitch:k * pitch + width] for k in range(K)])
        num, den = M.update_from_unit_rows(read[:, :-1], X, Y, M.LARGE_ETA, sigma, wide=wide, std_coeff=M.LARGE_STD)
        if good:
            M.check_accumulators(num.astype(F32), den.astype(F32), c["ref"])
        else:
            with pytest.raises(AssertionError):
                M.check_accumulators(num.astype(F32), den.astype(F32), c["ref"])


def test_checker_rejects_a_second_block_without_its_count_columns():
    """Stage 2 of the second 128-row block (one map row at 129 x 5) leaves the counts C -- the columns a masked handle
    divides by -- as the accumulator was zeroed: five units out of 645.  The accumulator check sees the denominators; the
    merge check sees the rows that kept their old values."""
    row = _row(129, 5, 64)
    fam, X, Y, D, N = row[:5]
    c, num, den = _f32_case(row)
    bad = den.copy()
    bad[128 * Y:] = 0
    assert (den[128 * Y:] != 0).all() and (bad != den).sum() == Y * D
    with pytest.raises(AssertionError, match="den"):
        M.check_accumulators(num, bad, c["ref"])
    with pytest.raises(AssertionError, match="merge vs reference"):
        M.check_merge(c["w0"], M.merge(c["w0"], num, bad), num, bad, c["ref"])


def test_exact_case_is_exact_in_float32_and_has_ties():
    x, w = M.exact_case(300, 77, 33, seed=1)
    s, _ = M.masked_scores(x, w)
    assert np.array_equal(s, s.astype(F32).astype(F64))
    assert np.array_equal(s * 64, np.round(s * 64))
    ids = np.argmin(s, axis=1)
    assert ((s == s.min(axis=1, keepdims=True)).sum(axis=1) > 1).mean() > 0.2, "hardly a tie: the construction lost its point"
    assert ids[150] == 0 and np.isnan(x[150]).all()


def fma32(a, b, c):
    """float32 fma on arrays: the product of two float32 values is exact in float64."""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


@pytest.mark.parametrize("D", [1, 3, 32, 33, 130, 260])
@pytest.mark.parametrize("kind", ["blobs", "offset30"])
def test_bound_holds_for_a_float32_evaluation_of_the_two_chains(D, kind):
    """2 000 random (row, unit) pairs: c1 and c2 as k-ordered float32 fma chains, the squares rounded once, one fma to
    join them -- the kernel's arithmetic in NumPy -- against the float64 score."""
    P = 2000
    rs = np.random.RandomState(D)
    rows = M.punch(Q.make_rows(kind, 500, D, 3), "random30", 4)
    units = Q.make_units(kind, np.nan_to_num(rows), 300, D, 3)
    x, w = rows[rs.randint(0, 500, P)], units[rs.randint(0, 300, P)]
    seen = ~np.isnan(x)
    xt, m = np.where(seen, x, F32(0)), seen.astype(F32)
    c1, c2 = np.zeros(P, F32), np.zeros(P, F32)
    for d in range(D):
        c1 = fma32(w[:, d], xt[:, d], c1)
        c2 = fma32((w[:, d] * w[:, d]).astype(F32), m[:, d], c2)
    got = fma32(np.full(P, -2, F32), c1, c2).astype(F64)
    xt64, m64 = M.split(x)
    w64 = w.astype(F64)
    ref = (m64 * w64 * w64).sum(1) - 2 * (xt64 * w64).sum(1)
    E = Q.gamma(D + 3) * (2 * (np.abs(xt64 * w64)).sum(1) + (m64 * w64 * w64).sum(1))
    s, Efull = M.masked_scores(x[:5], w[:5])
    assert np.allclose(np.diag(s), ref[:5], rtol=1e-13, atol=1e-13) and np.allclose(np.diag(Efull), E[:5], rtol=1e-13)
    err = np.abs(got - ref)
    assert (err <= E).all(), "worst err / bound %.3g" % (err / np.where(E > 0, E, 1)).max()
    assert err.max() > 0 or D == 1
