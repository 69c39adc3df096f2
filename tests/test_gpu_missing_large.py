"""Missing values on the device at size: the update chain and the search of a handle created with SOM_MISSING_NAN on
large maps and wide rows.  GPU only (`-m gpu`).

A masked handle sends rows [S | C | count] of width UD = 2 D through the whole update chain, so every width the host's
dispatch decides on is doubled: tests/test_gpu_missing.py stays on maps of at most 16 x 16 and 260 features, where one
128-row block, the 64-row tile without bands and the 16- and 8-wave run sum are all there is.  The rows here
(tests/missing_ref.py, LARGE_FORCED) are the smallest shapes that cross each boundary with UD-wide rows;
tests/test_missing_cpu.py shows from update_ref.update_paths(..., masked=True) that they reach every branch, and that the
merge check covers at least 95 % of the (unit, feature) elements on each of them.

  1  forced update against the model   one epoch_accumulate_forced + epoch_fetch_masked + epoch_merge per row; the model is
                                       missing_ref.reference_update_masked (float64, the augmented rows [x~ | m]):
                                       accumulators within update_ref.TOL of the magnitude, the merge bit for bit
                                       float32(num / den) (the old value where den == 0) and within merge_bound of the
                                       model; a second accumulate bitwise equal; with more than one map-row block, begin +
                                       every block bitwise the monolithic accumulate; no NaN anywhere
  2  weighted twins                    three of the rows with sample weights (several blocks, one wave, three levels)
  3  streaming                         chunks of 1, 700 and 299 rows: the run sum's accumulate mode on UD-wide rows
  4  complete rows                     num bitwise the unmasked handle's, den within the model's bound of its denominator
  5  the search at size                thousands of units, tail tiles of 1, 33, 40 and 127 units, 64 feature chunks, ties
                                       between distant tiles in exact arithmetic
  6  one unforced epoch                'f32' and 'exact': the accumulators against the model from the engine's own BMUs
"""
import numpy as np
import pytest

from tests import missing_ref as M
from tests import query_ref as Q
from tests import test_gpu_missing as G
from tests import update_ref as U

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
ETA = M.LARGE_ETA
WORST = {}      # test id -> the worst err / bound it saw (printed by the last test of the module)


def row_of(X, Y, D):
    return next(r for r in M.LARGE_FORCED if r[1:4] == (X, Y, D))


def fetch(e):
    num, den, _ = e.epoch_fetch_masked(want_bmu=False)
    return num, den


def staged_equals_monolithic(e, w0, sigma, wide, what):
    """begin + every block against the monolithic accumulate of the same (unforced) epoch, bitwise."""
    e.set_weights(w0)
    e.epoch_accumulate(sigma, ETA, wide)
    mnum, mden, mbmu = e.epoch_fetch_masked()
    e.epoch_accumulate_begin(sigma, ETA, wide)
    total = 0
    for blk in range(e.epoch_block_count()):
        off, n = e.epoch_accumulate_block(blk)
        assert off == total, "%s: block %d starts at %d, not %d" % (what, blk, off, total)
        total += n
    snum, sden, sbmu = e.epoch_fetch_masked()
    assert total == e.accum_device_ptr()[1], what
    assert np.array_equal(mbmu, sbmu), "%s: staged BMUs differ" % what
    assert G.same_bits(mnum, snum) and G.same_bits(mden, sden), "%s: staged != monolithic" % what
    assert np.isfinite(snum).all() and np.isfinite(sden).all(), what


def run_forced(row, weighted=False):
    """One LARGE_FORCED row on the engine (update_ref.run_forced_case for a masked handle); returns (accum, merge) ratios."""
    fam, X, Y, D, N, bpat, mpat, sigma, wide = row
    c = M.large_forced_case(row, weighted=weighted)
    what = M.large_id(row) + ("-weighted" if weighted else "")
    share = M.merge_share(c["ref"], c["mexican"])
    assert share >= M.MIN_MERGE_SHARE, "%s: the merge check covers %.4f of the elements" % (what, share)
    e = G.engine(X, Y, D, **c["kw"])
    try:
        e.set_weights(c["w0"])
        e.set_data(c["data"])
        if weighted:
            e.set_sample_weights(c["weights"])
        e.epoch_accumulate_forced(c["bmu"], sigma, ETA, wide)
        num, den = fetch(e)
        e.epoch_accumulate_forced(c["bmu"], sigma, ETA, wide)
        num2, den2 = fetch(e)
        assert G.same_bits(num, num2) and G.same_bits(den, den2), what + ": a second forced accumulate differs"
        e.epoch_merge()
        w1 = e.get_weights()
        if X > 128:
            assert e.epoch_block_count() >= 2, what
        if e.epoch_block_count() > 1:
            staged_equals_monolithic(e, c["w0"], sigma, wide, what)
    finally:
        e.close()
    assert np.isfinite(num).all() and np.isfinite(den).all() and np.isfinite(w1).all(), what + ": a NaN or an infinity"
    a = M.check_accumulators(num, den, c["ref"], what)
    m = M.check_merge(c["w0"], w1, num, den, c["ref"], c["mexican"], what)
    print("%s: accumulators %.3g, merge %.3g of the bound (merge check on %.4f of the elements)" % (what, a, m, share))
    WORST[what] = (a, m)
    if mpat == "feature":                                  # nobody observes feature D // 2: it stays bit for bit
        d = D // 2
        assert (den[:, d] == 0).all() and G.same_bits(w1[:, d], c["w0"][:, d]) and not G.same_bits(w1[:, 0], c["w0"][:, 0])
    return a, m


# ----------------------------------------------------------------------------- 1: forced update against the model
@pytest.mark.parametrize("row", M.LARGE_FORCED, ids=[M.large_id(r) for r in M.LARGE_FORCED])
def test_forced_update_against_the_model(row):
    run_forced(row)


# ----------------------------------------------------------------------------- 2: weighted twins
WEIGHTED = [row_of(129, 5, 64), row_of(5, 7, 2046), row_of(8, 8, 2)]


@pytest.mark.parametrize("row", WEIGHTED, ids=[M.large_id(r) for r in WEIGHTED])
def test_forced_weighted_update_against_the_model(row):
    c = M.large_forced_case(row, weighted=True)
    zero = np.flatnonzero(c["weights"] == 0)
    assert len(zero) and np.isinf(c["data"][zero[0]]).all()
    run_forced(row, weighted=True)
    plain = M.large_forced_case(row)["ref"]
    assert not np.allclose(plain[0], c["ref"][0], rtol=1e-3, atol=0), "the weights changed nothing: the test is blind"


# ----------------------------------------------------------------------------- 3: streaming
def test_streamed_uneven_chunks_two_row_blocks():
    """129 x 5 x 64 through stream_epoch_accumulate in chunks of 1, 700 and 299 rows.  The BMUs are the engine's own (a
    stream cannot be forced): the resident epoch returns them, the model is built from them, and resident and streamed
    accumulators are both held against it.  One chunk is bitwise the resident epoch."""
    row = row_of(129, 5, 64)
    fam, X, Y, D, N, _, _, sigma, wide = row
    x = M.large_forced_case(row)["data"]
    w0 = Q.make_units("blobs", np.nan_to_num(x), X * Y, D, 31)
    e = G.engine(X, Y, D)
    try:
        e.set_weights(w0)
        e.set_data(x)
        e.epoch_accumulate(sigma, ETA, wide)
        rnum, rden, bmu = e.epoch_fetch_masked()
        e.stream_epoch_accumulate([x], sigma, ETA, wide)
        num1, den1 = fetch(e)
        e.stream_epoch_accumulate([x[:1], x[1:701], x[701:]], sigma, ETA, wide)
        num3, den3 = fetch(e)
        e.epoch_merge()
        w1 = e.get_weights()
    finally:
        e.close()
    assert len(x[701:]) == 299
    Q.check_picks(bmu, *M.masked_scores(x, w0), "stream BMUs")
    assert len(np.unique(bmu // Y)) > 64 and (bmu // Y).max() == X - 1, "the rows do not spread over both row blocks"
    assert G.same_bits(rnum, num1) and G.same_bits(rden, den1)
    ref = M.reference_update_masked(x, bmu, X, Y, ETA, sigma, wide=wide, std_coeff=M.LARGE_STD)
    assert M.merge_share(ref) >= M.MIN_MERGE_SHARE
    a = max(M.check_accumulators(rnum, rden, ref, "resident"), M.check_accumulators(num3, den3, ref, "three chunks"))
    m = M.check_merge(w0, w1, num3, den3, ref, False, "three chunks")
    assert np.isfinite(num3).all() and np.isfinite(den3).all() and np.isfinite(w1).all()
    print("streamed 129x5x64: accumulators %.3g, merge %.3g of the bound" % (a, m))
    WORST["streamed-129x5x64"] = (a, m)


# ----------------------------------------------------------------------------- 4: complete rows
COMPLETE = [row_of(129, 5, 64), row_of(257, 3, 65)]


@pytest.mark.parametrize("row", COMPLETE, ids=[M.large_id(r) for r in COMPLETE])
def test_complete_rows_reproduce_the_unmasked_update(row):
    fam, X, Y, D, N, _, _, sigma, wide = row
    c = M.large_forced_case(row, missing="none")
    assert not np.isnan(c["data"]).any()
    out = {}
    for mode in ("nan", None):
        e = G.engine(X, Y, D, missing=mode, **c["kw"])
        try:
            e.set_weights(c["w0"])
            e.set_data(c["data"])
            e.epoch_accumulate_forced(c["bmu"], sigma, ETA, wide)
            acc = e.epoch_fetch_masked(want_bmu=False) if mode else e.epoch_fetch(want_bmu=False)
            e.epoch_merge()
            out[mode] = (acc[0], acc[1], e.get_weights())
        finally:
            e.close()
    (mnum, mden, mw), (unum, uden, uw) = out["nan"], out[None]
    ref = c["ref"]
    assert G.same_bits(mnum, unum)
    err = np.abs(mden.astype(F64) - uden.astype(F64)[:, None])
    assert (err <= U.accum_bound(ref[3])).all()
    ok, _, bound = M.merge_bound(ref)
    assert ok.mean() >= M.MIN_MERGE_SHARE and (np.abs(mw.astype(F64) - uw.astype(F64))[ok] <= bound[ok]).all()
    a = M.check_accumulators(mnum, mden, ref, "complete rows")
    m = M.check_merge(c["w0"], mw, mnum, mden, ref, False, "complete rows")
    print("%s complete rows: accumulators %.3g, merge %.3g of the bound" % (M.large_id(row), a, m))
    WORST[M.large_id(row) + "-complete"] = (a, m)


# ----------------------------------------------------------------------------- 5: the search at size
BMU_CASES = [   # X, Y, D, N, pattern, precision
    (129, 1, 3, 300, "random30", "f32"),          # K = 129: a tail tile with one live unit
    (7, 23, 33, 129, "payload", "exact"),         # K = 161: tail of 33
    (15, 17, 6, 300, "row", "f32"),               # K = 255: tail of 127
    (129, 40, 33, 300, "random30", "exact"),      # K = 5160: 41 tiles, tail of 40
    (64, 64, 32, 5000, "random30", "exact"),      # K = 4096: whole tiles only, 40 workgroups
    (5, 7, 2046, 129, "halves", "f32"),           # 64 feature chunks
]


def check_picks_in_chunks(ids, x, w, what, step=1000):
    """query_ref.check_picks with missing_ref.masked_scores, a thousand rows at a time (the score matrix is rows x units)."""
    return max(Q.check_picks(ids[s:s + step], *M.masked_scores(x[s:s + step], w), what) for s in range(0, len(x), step))


def bmu_case(X, Y, D, N, pattern):
    """(rows, units) of a BMU_CASES line: tests/test_gpu_missing.py's rows and units; the three units before the last repeat
    the first three (the lowest id must win), and the last unit -- the last live one of the tail tile -- holds row 1's
    observed values, so the model gives row 1 to it by a wide margin."""
    K = X * Y
    x = M.punch(Q.make_rows("blobs", N, D, 11 + D), pattern, 5)
    w = Q.make_units("blobs", np.nan_to_num(Q.make_rows("blobs", 400, D, 11 + D)), K, D, 7)
    w[K - 4:K - 1] = w[:3]
    w[K - 1] = np.nan_to_num(x[1])
    s, E = M.masked_scores(x[1:2], w)
    assert np.argmin(s[0]) == K - 1 and s[0, K - 1] + E[0, K - 1] < np.delete(s[0] - E[0], K - 1).min()
    return x, w


@pytest.mark.parametrize("X, Y, D, N, pattern, precision", BMU_CASES, ids=["%dx%dx%d-n%d-%s-%s" % c for c in BMU_CASES])
def test_bmus_against_the_model(X, Y, D, N, pattern, precision):
    x, w = bmu_case(X, Y, D, N, pattern)
    e = G.engine(X, Y, D, precision=precision)
    try:
        e.set_weights(w)
        host = e.bmu(x)
        dev = G.device_ids(e, x)
        quant = e.bmu(x, quantization=True)
    finally:
        e.close()
    what = "%dx%dx%d n%d %s" % (X, Y, D, N, pattern)
    worst = check_picks_in_chunks(host, x, w, what + " som_bmu")
    print("%s: worst err / bound %.3g" % (what, worst))
    assert np.array_equal(host, dev), what + ": som_bmu_device differs from som_bmu"
    assert np.array_equal(host, quant), what + ": the QUANTIZATION mode differs"
    none = np.flatnonzero(np.isnan(x).all(axis=1))
    assert (host[none] == 0).all()
    if pattern == "row":
        assert len(none) >= 1
    assert host[1] == X * Y - 1, what + ": row 1 belongs to the last unit of the tail tile"


def test_bmus_in_exact_arithmetic_with_ties_between_distant_tiles():
    """5160 units whose last 1290 repeat the first: every score is exact in float32 and a row's best unit in tiles 0 .. 10
    ties with its copy 30 tiles on; the lowest id must win, on host and on device rows."""
    X, Y, D, N = 129, 40, 6, 300
    x, w = M.exact_case(N, X * Y, D, seed=17)
    s, _ = M.masked_scores(x, w)
    want = np.argmin(s, axis=1)
    tied_far = (s[:, X * Y - X * Y // 4:].min(axis=1) == s.min(axis=1))
    assert tied_far.mean() > 0.2, "hardly a tie between distant tiles: the construction lost its point"
    e = G.engine(X, Y, D)
    try:
        e.set_weights(w)
        ids = e.bmu(x)
        dev = G.device_ids(e, x)
    finally:
        e.close()
    Q.check_ties(ids, s, "exact 129x40x6")
    assert np.array_equal(ids, want) and np.array_equal(dev, want)
    assert ids[N // 2] == 0 and np.isnan(x[N // 2]).all()


# ----------------------------------------------------------------------------- 6: one unforced epoch
@pytest.mark.parametrize("precision", ["f32", "exact"])
def test_unforced_epoch_per_precision(precision):
    """epoch_accumulate at 129 x 40 x 33 (41 unit tiles of the search; UD = 66; two row blocks, bands): the accumulators and
    the merge against the model built from the engine's own BMUs, those BMUs against the score model, and the quantization
    error of the merged map against the masked definition."""
    X, Y, D, N, sigma, wide = 129, 40, 33, 2100, 2.0, False
    x = M.punch(Q.make_rows("blobs", N, D, 44), "random30", 18)
    w0 = Q.make_units("blobs", np.nan_to_num(x), X * Y, D, 45)
    e = G.engine(X, Y, D, precision=precision)
    try:
        e.set_weights(w0)
        e.set_data(x)
        e.epoch_accumulate(sigma, ETA, wide)
        num, den, bmu = e.epoch_fetch_masked()
        e.epoch_merge()
        w1 = e.get_weights()
        ids = e.bmu(x)
        qe = e.quantization_error(x)
    finally:
        e.close()
    what = "unforced " + precision
    assert (bmu >= 0).all() and (bmu < X * Y).all()
    p = check_picks_in_chunks(bmu, x, w0, what + " BMUs")
    ref = M.reference_update_masked(x, bmu, X, Y, ETA, sigma, wide=wide, std_coeff=M.LARGE_STD)
    assert np.isfinite(num).all() and np.isfinite(den).all() and np.isfinite(w1).all()
    a = M.check_accumulators(num, den, ref, what)
    m = M.check_merge(w0, w1, num, den, ref, False, what)
    check_picks_in_chunks(ids, x, w1, what + " BMUs on the merged map")
    q = M.check_qe(qe, x, w1, ids, what)
    print("%s 129x40x33: picks %.3g, accumulators %.3g, merge %.3g, QE %.3g of the bound" % (what, p, a, m, q))
    WORST["unforced-%s-129x40x33" % precision] = (a, m)


def test_report_worst_ratio_per_row():
    """(last in the module) the worst err / bound per row, for the record; every case has already passed."""
    for what in WORST:
        print("missing_large worst %-58s accum %.3g  merge %.3g" % (what, WORST[what][0], WORST[what][1]))
    assert all(a <= 1 and m <= 1 for a, m in WORST.values())
