"""Missing values on the device (`XPySom(..., missing='nan')`, som_config.missing = SOM_MISSING_NAN).  GPU only (`-m gpu`).

The float64 model and its bounds are tests/missing_ref.py's.  Shapes are the smallest that cross every boundary of the
kernels: maps 5 x 7, 12 x 11 (a second 128-unit tile of the masked search) and 16 x 16; input_len 1, 3 (odd: the scalar
lanes of the run sum), 32 (one whole 32-feature chunk; 2 D = 64), 33 (a chunk tail), 130 (beyond 128) and 260 (a second
256-feature sweep of the run sum); 1, 127, 129, 300 and 5 000 rows (one lane, both sides of a 128-row workgroup of the
search, several run-sum chunks, the counting sort and more than one run-sum workgroup).

  1  BMUs against the model        query_ref.check_picks with E = gamma(D + 3) (2 sum |x~ w| + sum m w^2); som_bmu, som_bmu_device
  2  BMUs in exact arithmetic      integers / 8: every float32 operation is exact, the ids ARE NumPy's first argmin
  3  forced update against the model   every neighbourhood, hexagonal, toroidal, float32 and float64 tables
  4  complete rows                 num bitwise the unmasked num; den and the merged codebook within the model's bound of the unmasked
  5  structure                     a feature nobody observes stays bit for bit; an all-missing row changes nothing; no NaN ever
  6  sample weights                1.0 = none, integer = repeated, 0 = absent (bitwise); the weighted model
  7  determinism and paths         graph = eager, device = host, streamed = resident, two shards add up, the accumulator's size
  8  quantization error            query_ref.check_qe's form on the masked definition
  9  end to end through XPySom
  10 refusals of the C ABI
"""
import numpy as np
import pytest

from oracle import som_oracle as O
from tests import missing_ref as M
from tests import query_ref as Q
from tests import update_ref as U
from tests import weights_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def engine(*a, **kw):
    from xpysom_dask_amd.engine import HipEngine
    kw.setdefault("missing", "nan")
    kw.setdefault("precision", "f32")
    return HipEngine(*a, **kw)


def som(*a, **kw):
    from xpysom_dask_amd import XPySom
    kw.setdefault("missing", "nan")
    return XPySom(*a, **kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def codebook(X, Y, D, seed=3):
    return O.default_codebook(X, Y, D, seed).astype(F32).reshape(X * Y, D)


def device_ids(e, x):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(x, dtype=F32), device="cuda")
    torch.cuda.synchronize()
    return e.bmu_device(t.data_ptr(), len(x))


# ----------------------------------------------------------------------------- 1: BMUs against the model
BMU_CASES = [   # X, Y, D, N, pattern, precision
    (5, 7, 1, 1, "none", "f32"),
    (5, 7, 1, 300, "row", "exact"),
    (5, 7, 3, 127, "random30", "f32"),
    (12, 11, 32, 129, "feature", "exact"),
    (12, 11, 33, 300, "payload", "f32"),
    (12, 11, 6, 300, "none", "exact"),
    (16, 16, 130, 5000, "random30", "f32"),
    (16, 16, 260, 300, "halves", "exact"),
    (16, 16, 3, 5000, "row", "f32"),
]


@pytest.mark.parametrize("X, Y, D, N, pattern, precision", BMU_CASES, ids=["%dx%dx%d-n%d-%s-%s" % c for c in BMU_CASES])
def test_bmus_against_the_model(X, Y, D, N, pattern, precision):
    x = M.punch(Q.make_rows("blobs", N, D, 11 + D), pattern, 5)
    w = Q.make_units("blobs", np.nan_to_num(Q.make_rows("blobs", 400, D, 11 + D)), X * Y, D, 7, dup=3)
    s, E = M.masked_scores(x, w)
    e = engine(X, Y, D, precision=precision)
    try:
        e.set_weights(w)
        host = e.bmu(x)
        dev = device_ids(e, x)
        quant = e.bmu(x, quantization=True)
    finally:
        e.close()
    what = "%dx%dx%d n%d %s" % (X, Y, D, N, pattern)
    worst = Q.check_picks(host, s, E, what + " som_bmu")
    print("%s: worst err / bound %.3g" % (what, worst))
    assert np.array_equal(host, dev), what + ": som_bmu_device differs from som_bmu"
    assert np.array_equal(host, quant), what + ": the QUANTIZATION mode differs"
    none = np.flatnonzero(np.isnan(x).all(axis=1))
    assert (host[none] == 0).all()


# ----------------------------------------------------------------------------- 2: BMUs in exact arithmetic
@pytest.mark.parametrize("X, Y, D, N", [(5, 7, 3, 127), (12, 11, 33, 300), (16, 16, 130, 129), (16, 16, 32, 5000), (5, 7, 1, 300)])
def test_bmus_in_exact_arithmetic(X, Y, D, N):
    x, w = M.exact_case(N, X * Y, D, seed=D + N)
    s, _ = M.masked_scores(x, w)
    want = np.argmin(s, axis=1)
    e = engine(X, Y, D)
    try:
        e.set_weights(w)
        ids = e.bmu(x)
        dev = device_ids(e, x)
    finally:
        e.close()
    Q.check_ties(ids, s, "exact %dx%dx%d" % (X, Y, D))
    assert np.array_equal(dev, want)
    assert ids[N // 2] == 0 and np.isnan(x[N // 2]).all()
    # the same data without holes: the unmasked float32 handle's ids
    xc, _ = M.exact_case(N, X * Y, D, seed=D + N, holes=False)
    assert not np.isnan(xc).any()
    e, u = engine(X, Y, D), engine(X, Y, D, missing=None)
    try:
        e.set_weights(w)
        u.set_weights(w)
        a, b = e.bmu(xc), u.bmu(xc)
    finally:
        e.close()
        u.close()
    assert np.array_equal(a, b)
    Q.check_ties(a, M.masked_scores(xc, w)[0], "complete rows")


# ----------------------------------------------------------------------------- 3: forced update against the model
FORCED = [   # family (update_ref.FAMILIES or "torus_gaussian"), X, Y, D, N, BMU pattern, missing pattern, sigma, wide
    ("gaussian", 5, 7, 3, 127, "spread", "random30", 2.0, False),
    ("gaussian", 12, 11, 33, 300, "edges", "payload", 2.0, True),
    ("gaussian", 16, 16, 32, 5000, "skewed", "halves", 3.0, False),
    ("gaussian", 16, 16, 130, 300, "sparse", "feature", 2.0, True),
    ("gaussian", 12, 11, 260, 129, "spread", "random30", 2.0, False),
    ("gaussian", 5, 7, 1, 5000, "skewed", "row", 1.5, True),
    ("gaussian", 5, 7, 3, 1, "sparse", "none", 2.0, True),
    ("mexican_hat", 12, 11, 6, 300, "spread", "random30", 2.0, True),
    ("bubble", 12, 11, 3, 300, "edges", "row", 2.0, False),
    ("triangle", 16, 16, 6, 5000, "skewed", "random30", 3.0, False),
    ("hex_gaussian", 12, 11, 6, 300, "spread", "random30", 2.0, True),
    ("torus_gaussian", 12, 11, 6, 300, "edges", "random30", 2.0, False),
]
_forced_cache = {}


def forced_case(case):
    """(data, bmu, w0, reference) of a FORCED row, computed once."""
    if case not in _forced_cache:
        fam, X, Y, D, N, bpat, mpat, sigma, wide = case
        neigh, topo, compact = ("gaussian", "toroidal", False) if fam == "torus_gaussian" else U.FAMILIES[fam]
        rs = np.random.RandomState(X * Y + D + N)
        bmu = U.make_bmu(bpat, X, Y, N, rs)
        data = M.punch(U.make_data(N, D, 1.0, 70 + D), mpat, 9, bmu)
        ref = M.reference_update_masked(data, bmu, X, Y, 0.5, sigma, wide=wide, neighbourhood=neigh, topology=topo, compact=compact)
        _forced_cache[case] = (data, bmu, codebook(X, Y, D), ref, dict(neighborhood=neigh, topology=topo, compact_support=compact))
    return _forced_cache[case]


@pytest.mark.parametrize("case", FORCED, ids=["%s-%dx%dx%d-n%d-%s-%s" % c[:7] for c in FORCED])
def test_forced_update_against_the_model(case):
    fam, X, Y, D, N, bpat, mpat, sigma, wide = case
    data, bmu, w0, ref, kw = forced_case(case)
    e = engine(X, Y, D, **kw)
    try:
        e.set_weights(w0)
        e.set_data(data)
        e.epoch_accumulate_forced(bmu, sigma, 0.5, wide)
        num, den, _ = e.epoch_fetch_masked(want_bmu=False)
        e.epoch_merge()
        w1 = e.get_weights()
    finally:
        e.close()
    what = "%s %dx%dx%d n%d %s" % (fam, X, Y, D, N, mpat)
    assert np.isfinite(num).all() and np.isfinite(den).all() and np.isfinite(w1).all()
    a = M.check_accumulators(num, den, ref, what)
    m = M.check_merge(w0, w1, num, den, ref, fam == "mexican_hat", what)
    print("%s: accumulators %.3g, merge %.3g of the bound" % (what, a, m))
    if mpat == "feature":
        d = D // 2
        assert (den[:, d] == 0).all() and same_bits(w1[:, d], w0[:, d]) and not same_bits(w1[:, 0], w0[:, 0])


# ----------------------------------------------------------------------------- 4: complete rows
@pytest.mark.parametrize("X, Y, D, N, sigma", [(12, 11, 6, 300, 2.0), (16, 16, 33, 5000, 3.0), (16, 16, 64, 300, 2.0)])
def test_complete_rows_reproduce_the_unmasked_update(X, Y, D, N, sigma):
    rs = np.random.RandomState(D)
    bmu = U.make_bmu("spread", X, Y, N, rs)
    data = U.make_data(N, D, 1.0, 12)
    w0 = codebook(X, Y, D)
    out = {}
    for mode in ("nan", None):
        e = engine(X, Y, D, missing=mode)
        try:
            e.set_weights(w0)
            e.set_data(data)
            e.epoch_accumulate_forced(bmu, sigma, 0.5, True)
            acc = e.epoch_fetch_masked(want_bmu=False) if mode else e.epoch_fetch(want_bmu=False)
            e.epoch_merge()
            out[mode] = (acc[0], acc[1], e.get_weights())
        finally:
            e.close()
    (mnum, mden, mw), (unum, uden, uw) = out["nan"], out[None]
    assert same_bits(mnum, unum)
    ref = M.reference_update_masked(data, bmu, X, Y, 0.5, sigma, wide=True)
    err = np.abs(mden.astype(F64) - uden.astype(F64)[:, None])
    assert (err <= U.accum_bound(ref[3])).all()
    ok, _, bound = M.merge_bound(ref)
    assert ok.any() and (np.abs(mw.astype(F64) - uw.astype(F64))[ok] <= bound[ok]).all()
    M.check_merge(w0, mw, mnum, mden, ref, False, "complete rows")


# ----------------------------------------------------------------------------- 5: structure
def test_a_feature_nobody_observes_is_left_bit_for_bit():
    X, Y, D, N = 12, 11, 6, 300
    x = O.gaussian_blobs(N, D, seed=3)
    x[:, 4] = np.nan
    w0 = codebook(X, Y, D)
    e = engine(X, Y, D, precision="exact")
    try:
        e.set_weights(w0)
        e.set_data(x)
        e.epoch(2.0, 0.5, True)
        w1 = e.get_weights()
    finally:
        e.close()
    assert same_bits(w1[:, 4], w0[:, 4])
    assert all((bits(w1[:, d]) != bits(w0[:, d])).any() for d in (0, 1, 2, 3, 5))
    assert np.isfinite(w1).all()


def integer_rows(N, D, seed):
    """Small integers with 30 % holes: every sum of the update's level 0 is exact in float32, so the order of the rows does not
    show in a bitwise comparison."""
    rs = np.random.RandomState(seed)
    x = rs.randint(-3, 4, size=(N, D)).astype(F32)
    x[rs.rand(N, D) < 0.3] = np.nan
    return x


def test_an_all_missing_row_changes_nothing():
    X, Y, D, N = 12, 11, 6, 300
    x = integer_rows(N, D, 4)
    x = x[~np.isnan(x).all(axis=1)]
    with_row = np.insert(x, 100, np.nan, axis=0)
    a = som(X, Y, D, random_seed=9, precision="f32").train(x, 3).get_weights()
    b = som(X, Y, D, random_seed=9, precision="f32").train(with_row, 3).get_weights()
    assert np.isfinite(a).all() and same_bits(a, b)


@pytest.mark.parametrize("precision", ["f32", "exact"])
def test_no_nan_reaches_the_codebook(precision):
    X, Y, D, N = 16, 16, 33, 5000
    x = M.punch(O.gaussian_blobs(N, D, seed=8), "payload", 2)
    x[17] = np.nan
    s = som(X, Y, D, random_seed=1, precision=precision).train(x, 5)
    assert np.isfinite(s.get_weights()).all()
    assert np.isfinite(s.quantization_error(x))


# ----------------------------------------------------------------------------- 6: sample weights
def test_unit_weights_equal_no_weights_bit_for_bit():
    X, Y, D, N = 16, 16, 12, 5000
    x = M.punch(O.gaussian_blobs(N, D, seed=21), "random30", 6)
    ones = np.ones(N, F32)
    plain = som(X, Y, D, random_seed=4).train(x, 3).get_weights()
    weighted = som(X, Y, D, random_seed=4).train(x, 3, sample_weight=ones).get_weights()
    assert np.isfinite(plain).all() and same_bits(plain, weighted)
    cuts = [(0, 700), (700, 3333), (3333, N)]
    s_plain = som(X, Y, D, random_seed=4).train_streaming(lambda: [x[a:b] for a, b in cuts], 3)
    s_weighted = som(X, Y, D, random_seed=4).train_streaming(lambda: [(x[a:b], ones[a:b]) for a, b in cuts], 3)
    assert same_bits(s_plain.get_weights(), s_weighted.get_weights())


@pytest.mark.parametrize("X, Y, D, N", [(16, 16, 8, 2000), (12, 11, 3, 300)])
def test_integer_weight_equals_the_row_repeated_and_zero_equals_absent(X, Y, D, N):
    x = integer_rows(N, D, X + N)
    w = np.random.RandomState(N).randint(0, 5, size=N).astype(F32)
    zero = np.flatnonzero(w == 0)
    assert len(zero) > 10 and (w == 4).any()
    x[zero[3], 0] = np.inf                                    # a row of weight 0 is not read
    repeated = np.repeat(x, w.astype(np.int64), axis=0)
    assert not np.isinf(repeated).any()
    a = som(X, Y, D, random_seed=9, precision="f32").train(x, 3, sample_weight=w).get_weights()
    b = som(X, Y, D, random_seed=9, precision="f32").train(repeated, 3).get_weights()
    c = som(X, Y, D, random_seed=9, precision="f32").train(x[w != 0], 3, sample_weight=w[w != 0]).get_weights()
    assert np.isfinite(a).all()
    assert same_bits(a, b) and same_bits(a, c)
    assert not same_bits(a, som(X, Y, D, random_seed=9, precision="f32").train(x[w != 0], 3).get_weights()), \
        "the weights changed nothing: the test is blind"


@pytest.mark.parametrize("X, Y, D, N, bpat", [(5, 7, 3, 300, "spread"), (16, 16, 130, 5000, "skewed"), (12, 11, 32, 129, "edges")])
def test_forced_weighted_update_against_the_model(X, Y, D, N, bpat):
    rs = np.random.RandomState(N + D)
    bmu = U.make_bmu(bpat, X, Y, N, rs)
    data = M.punch(U.make_data(N, D, 1.0, 71), "random30", 10)
    w = R.make_weights(N, 5 + D)
    data[np.flatnonzero(w == 0)[0]] = np.inf
    e = engine(X, Y, D)
    try:
        e.set_weights(codebook(X, Y, D))
        e.set_data(data)
        e.set_sample_weights(w)
        e.epoch_accumulate_forced(bmu, 2.0, 0.5, True)
        num, den, _ = e.epoch_fetch_masked(want_bmu=False)
    finally:
        e.close()
    ref = M.reference_update_masked(data, bmu, X, Y, 0.5, 2.0, wide=True, weights=w)
    print("weighted %dx%dx%d: %.3g of the bound" % (X, Y, D, M.check_accumulators(num, den, ref, "weighted")))


# ----------------------------------------------------------------------------- 7: determinism and paths
def test_two_runs_are_bitwise_equal_and_the_graph_path_equals_the_eager_one(monkeypatch):
    """Four epochs under SOM_GRAPH=0 and =1 (the second captures, the later ones replay the masked launches), each twice:
    every epoch's BMUs and accumulators are bitwise those of the eager handle -- a second epoch on the same handle is a
    fresh handle's second epoch."""
    X, Y, D, N = 12, 11, 7, 1500
    x = M.punch(O.gaussian_blobs(N, D, seed=11), "random30", 12)
    w0 = codebook(X, Y, D)
    outs = []
    for mode in ("0", "1", "1"):
        monkeypatch.setenv("SOM_GRAPH", mode)
        e = engine(X, Y, D)
        try:
            e.set_data(x)
            e.set_weights(w0)
            res = []
            for t in range(4):
                e.epoch_accumulate(3.0 - 0.4 * t, 0.5 - 0.05 * t, t % 2 == 0)
                res.append(tuple(a.copy() for a in e.epoch_fetch_masked()))
                e.epoch_merge()
            res.append(e.get_weights())
        finally:
            e.close()
        outs.append(res)
    for other in outs[1:]:
        for t in range(4):
            assert np.array_equal(outs[0][t][2], other[t][2]), "epoch %d: BMUs" % t
            assert same_bits(outs[0][t][0], other[t][0]) and same_bits(outs[0][t][1], other[t][1]), "epoch %d" % t
        assert same_bits(outs[0][4], other[4])
    assert not same_bits(outs[0][0][0], outs[0][1][0])


def test_device_rows_equal_host_rows():
    import torch
    X, Y, D, N = 16, 16, 8, 2000
    x = M.punch(O.gaussian_blobs(N, D, seed=51), "random30", 13)
    host = som(X, Y, D, random_seed=9).train(x, 3)
    xd = torch.as_tensor(x, device="cuda")
    dev = som(X, Y, D, random_seed=9).train(xd, 3)
    assert np.isfinite(host.get_weights()).all() and same_bits(host.get_weights(), dev.get_weights())
    assert host.winner(x) == dev.winner(xd)
    assert host.quantization_error(x) == dev.quantization_error(xd)


def test_streamed_equals_resident_and_shards_add_up():
    X, Y, D, N = 12, 11, 6, 3000
    x = M.punch(O.gaussian_blobs(N, D, seed=61), "random30", 14)
    w0 = codebook(X, Y, D)
    e = engine(X, Y, D)
    try:
        ptr, n_floats = e.accum_device_ptr()
        assert n_floats == X * Y * 16 and ptr                 # K rows of round_up(2 D + 1, 4) floats: [num | den | count | pad]
        e.set_weights(w0)
        e.set_data(x)
        e.epoch_accumulate(2.0, 0.5, True)
        rnum, rden, bmu = e.epoch_fetch_masked()
        e.stream_epoch_accumulate([x], 2.0, 0.5, True)
        num1, den1, _ = e.epoch_fetch_masked(want_bmu=False)
        e.stream_epoch_accumulate([x[:1], x[1:1700], x[1700:]], 2.0, 0.5, True)
        num3, den3, _ = e.epoch_fetch_masked(want_bmu=False)
        halves = []
        for part in (x[:N // 2], x[N // 2:]):
            e.set_data(part)
            e.epoch_accumulate(2.0, 0.5, True)
            halves.append(e.epoch_fetch_masked())
    finally:
        e.close()
    assert same_bits(rnum, num1) and same_bits(rden, den1)
    ref = M.reference_update_masked(x, bmu, X, Y, 0.5, 2.0, wide=True)
    M.check_accumulators(rnum, rden, ref, "resident")
    M.check_accumulators(num3, den3, ref, "three chunks")
    assert np.array_equal(np.r_[halves[0][2], halves[1][2]], bmu)
    M.check_accumulators(halves[0][0].astype(F64) + halves[1][0], halves[0][1].astype(F64) + halves[1][1], ref, "two shards")


def test_staged_blocks_equal_the_monolithic_accumulate():
    X, Y, D, N = 12, 11, 6, 300
    x = M.punch(O.gaussian_blobs(N, D, seed=62), "random30", 15)
    e = engine(X, Y, D)
    try:
        e.set_weights(codebook(X, Y, D))
        e.set_data(x)
        e.epoch_accumulate(2.0, 0.5, True)
        a = e.epoch_fetch_masked()
        e.epoch_accumulate_begin(2.0, 0.5, True)
        total = 0
        for b in range(e.epoch_block_count()):
            off, n = e.epoch_accumulate_block(b)
            assert off == total
            total += n
        c = e.epoch_fetch_masked()
    finally:
        e.close()
    assert total == X * Y * 16
    assert same_bits(a[0], c[0]) and same_bits(a[1], c[1]) and np.array_equal(a[2], c[2])


# ----------------------------------------------------------------------------- 8: quantization error
@pytest.mark.parametrize("X, Y, D, N, pattern", [(5, 7, 3, 127, "random30"), (12, 11, 33, 300, "row"), (16, 16, 130, 5000, "payload"),
                                                 (16, 16, 260, 129, "halves")])
def test_quantization_error_against_the_definition(X, Y, D, N, pattern):
    x = M.punch(Q.make_rows("blobs", N, D, 3), pattern, 16)
    w = Q.make_units("blobs", np.nan_to_num(x), X * Y, D, 4)
    e = engine(X, Y, D)
    try:
        e.set_weights(w)
        ids = e.bmu(x)
        qe = e.quantization_error(x)
    finally:
        e.close()
    s, E = M.masked_scores(x, w)
    Q.check_picks(ids, s, E, "qe ids")
    print("QE %dx%dx%d: %.3g of the bound" % (X, Y, D, M.check_qe(qe, x, w, ids, "qe")))
    assert np.isfinite(qe)


# ----------------------------------------------------------------------------- 9: end to end
def test_training_through_xpysom_lowers_the_masked_quantization_error():
    X, Y, D, N = 12, 11, 6, 2000
    x = M.punch(O.gaussian_blobs(N, D, seed=5, centres=8), "random30", 17)
    s = som(X, Y, D, sigma=3.0, random_seed=2)
    before = s.quantization_error(x)
    s.train(x, 10)
    after = s.quantization_error(x)
    w = np.asarray(s.get_weights(), F32).reshape(X * Y, D)
    assert np.isfinite(w).all() and after < before
    e = engine(X, Y, D, precision="exact")
    try:
        e.set_weights(w)
        ids = e.bmu(x)
    finally:
        e.close()
    assert s.winner(x) == [tuple(divmod(int(i), Y)) for i in ids]
    assert np.array_equal(s.predict(x), ids)
    assert s.activation_response(x).sum() == N
    M.check_qe(after, x, w, ids, "trained map")
    Q.check_picks(ids, *M.masked_scores(x, w), "trained map")
    assert s.winner(x.astype(F64))[:5] == s.winner(x)[:5]     # float64 rows take the same masked path


# ----------------------------------------------------------------------------- 10: refusals
def test_c_abi_refusals():
    from xpysom_dask_amd.engine import HipEngine, SomHipError
    X, Y, D, N = 5, 7, 3, 50
    x = M.punch(O.gaussian_blobs(N, D, seed=1), "random30", 1)
    e = engine(X, Y, D)
    try:
        e.set_weights(codebook(X, Y, D))
        e.set_data(x)
        with pytest.raises(SomHipError, match="som_epoch_accumulate_faithful: .*SOM_MISSING_NAN"):
            e.epoch_accumulate_faithful(2.0, 0.5, True)
        with pytest.raises(SomHipError, match="som_set_verify: .*SOM_MISSING_NAN"):
            e.set_verify(4)
        e.set_verify(0)
        with pytest.raises(SomHipError, match="som_bmu_top2: .*SOM_MISSING_NAN"):
            e.bmu_top2(x)
        with pytest.raises(SomHipError, match="som_epoch_fetch: .*som_epoch_fetch_masked"):
            e.epoch_fetch()
        with pytest.raises(SomHipError, match="som_distance_matrix: .*SOM_MISSING_NAN"):
            e.distance_matrix(x)
        with pytest.raises(SomHipError, match="som_bmu_f64: .*SOM_MISSING_NAN"):
            e.bmu_f64(x.astype(F64))
        e.epoch(2.0, 0.5, True)                               # the handle is still good
        assert np.isfinite(e.get_weights()).all()
    finally:
        e.close()
    u = HipEngine(X, Y, D, precision="f32")
    try:
        with pytest.raises(SomHipError, match="som_epoch_fetch_masked: .*not created with SOM_MISSING_NAN"):
            u.epoch_fetch_masked()
    finally:
        u.close()
    for kw, what in ((dict(precision="bf16"), "not 'bf16' / 'f16'"), (dict(precision="f16"), "not 'bf16' / 'f16'"),
                     (dict(distance="cosine"), "'euclidean' activation distance only"),
                     (dict(distance="manhattan"), "'euclidean' activation distance only")):
        with pytest.raises(SomHipError, match="som_create: missing values.*" + what):
            HipEngine(X, Y, D, missing="nan", **kw)
