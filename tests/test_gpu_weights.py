"""Per-row sample weights on the device (`train(..., sample_weight=w)`, som_set_sample_weights*, som_stream_rows_weighted).
GPU only (`-m gpu`).

    num[k] = sum_n w_n h(bmu_n -> k) x_n      den[k] = sum_n w_n h(bmu_n -> k)      BMUs: those of the unweighted call

The weights enter at level 0 of the run sum (csrc/update.hpp, runsum_kernel<true, VEC2, true>) and nowhere else, so:
  forced cases   epoch_accumulate_forced with float weights in [0, 2), a tenth of them 0, against the float64 model of
                 tests/weights_ref.py under update_ref's own tolerance (fmaf(w, x, acc) rounds once, as acc + x does) --
                 each shape the smallest that reaches the path it names
  property 2     weights of 1.0 = no weights, bit for bit, on float data (fmaf(1, x, acc) rounds like acc + x)
  property 3, 4  an integer weight m = the row m times and weight 0 = the row absent (a NaN row of weight 0 harms
                 nothing), bit for bit on data whose sums are exact in float32: features in {-3 .. 3}, weights in
                 {0 .. 4}, at most 3 000 rows -- every partial sum is an integer below 3 * 4 * 3 000 < 2^24
  property 5     all weights times 4: every product and sum scales by 4 exactly (no overflow; no underflow either: the
                 test keeps sigma >= 4 on a 16 x 16 map, where the smallest neighbourhood value is exp(-450 / 8) ~ 4e-25,
                 a normal float32 even times eta and the smallest weight), and num / den is unchanged
  property 6     the same weighted epoch twice: bitwise equal accumulators
and the plumbing: streamed = resident, device weights = host weights, set_data clears, the captured graph follows a
change of weights, the faithful cross-check refuses them.
"""
import numpy as np
import pytest

from oracle import som_oracle as O
from tests import update_ref as U
from tests import weights_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32


def engine(*a, **kw):
    from xpysom_dask_amd.engine import HipEngine
    return HipEngine(*a, **kw)


def som(*a, **kw):
    from xpysom_dask_amd import XPySom
    return XPySom(*a, **kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ----------------------------------------------------------------------------- forced BMUs against the float64 model
def _bmu_long_run(K, N, rs):
    """One unit owns rows 100 .. 1 399 (one run, open on both sides of many 32-row chunks and of 512-row workgroups);
    the other rows are scattered."""
    b = rs.randint(0, K, N)
    b[100:1400] = K // 3
    return b


def _bmu_pool(K, N, rs, pool=400):
    """Scattered over `pool` units that include the first and the last one (the float64 model evaluates one
    neighbourhood row per distinct BMU)."""
    units = np.unique(np.r_[0, K - 1, rs.choice(K, size=min(K, pool), replace=False)])
    return units[rs.randint(0, len(units), N)]


FORCED = [   # id, X, Y, D, N, BMUs, sigma, wide
    ("8x8x3-n1500-scalar-lanes-long-run", 8, 8, 3, 1500, _bmu_long_run, 2.0, False),
    ("24x24x16-n4096-vec2-two-levels", 24, 24, 16, 4096, _bmu_pool, 3.0, True),
    ("64x64x784-n4000-8-waves-4-sweeps", 64, 64, 784, 4000, _bmu_pool, 2.0, False),
    ("8x8x2-n300000-three-levels", 8, 8, 2, 300000, _bmu_pool, 1.5, True),
    ("128x64x4-n4096-counting-sort", 128, 64, 4, 4096, _bmu_pool, 2.0, False),      # K = 8 192 = CS_MAX_K
    ("129x64x4-n4096-radix-sort", 129, 64, 4, 4096, _bmu_pool, 2.0, False),         # K = 8 256 > CS_MAX_K
]


def test_forced_cases_reach_the_paths_they_name():
    want = {FORCED[0][0]: {"seg.vec1", "sort.radix", "runsum.upper"}, FORCED[1][0]: {"seg.vec2", "seg.waves16", "runsum.upper"},
            FORCED[2][0]: {"seg.waves8", "seg.vec2"}, FORCED[3][0]: {"seg.vec2", "runsum.upper", "sort.counting"},
            FORCED[4][0]: {"sort.counting"}, FORCED[5][0]: {"sort.radix"}}
    for cid, X, Y, D, N, _, _, _ in FORCED:
        assert want[cid] <= U.update_paths(X, Y, D, "gaussian", "rectangular", False, N), cid


@pytest.mark.parametrize("cid, X, Y, D, N, make_bmu, sigma, wide", FORCED, ids=[c[0] for c in FORCED])
def test_forced_weighted_update_against_the_float64_model(cid, X, Y, D, N, make_bmu, sigma, wide):
    rs = np.random.RandomState(len(cid) + N)
    bmu = make_bmu(X * Y, N, rs).astype(np.int32)
    data = U.make_data(N, D, 1.0, 77 + D)
    w = R.make_weights(N, 5 + D)
    assert 0.05 * N < (w == 0).sum() < 0.15 * N
    w0 = O.default_codebook(X, Y, D, 3).astype(F32).reshape(X * Y, D)
    e = engine(X, Y, D, precision="f32")
    try:
        e.set_weights(w0)
        e.set_data(data)
        e.set_sample_weights(w)
        e.epoch_accumulate_forced(bmu, sigma, 0.5, wide)
        num, den, _ = e.epoch_fetch(want_bmu=False)
        assert e.unit_sort_stats() == ((1, 0) if U.sort_path(X * Y, N) == "counting" else (0, 1)), "%s: not the sort the rule names" % cid
    finally:
        e.close()
    ref = R.reference_update_weighted(data, bmu, w, X, Y, 0.5, sigma, wide=wide)
    worst = U.check_accumulators(num, den, ref, cid)
    print("%s: worst err / bound %.3g" % (cid, worst))


# ----------------------------------------------------------------------------- property 2: weights of 1.0 = no weights
@pytest.mark.parametrize("precision", ["f32", "exact"])
def test_unit_weights_equal_no_weights_bit_for_bit(precision):
    X, Y, D, N = 16, 16, 12, 5000
    x = O.gaussian_blobs(N, D, seed=21)
    ones = np.ones(N, F32)
    plain = som(X, Y, D, random_seed=4, precision=precision).train(x, 3).get_weights()
    weighted = som(X, Y, D, random_seed=4, precision=precision).train(x, 3, sample_weight=ones).get_weights()
    assert same_bits(plain, weighted)
    cuts = [(0, 700), (700, 3333), (3333, N)]                 # three unequal chunks
    s_plain = som(X, Y, D, random_seed=4, precision=precision).train_streaming(lambda: [x[a:b] for a, b in cuts], 3)
    s_weighted = som(X, Y, D, random_seed=4, precision=precision).train_streaming(
        lambda: [(x[a:b], ones[a:b]) for a, b in cuts], 3)
    assert same_bits(s_plain.get_weights(), s_weighted.get_weights())


# ----------------------------------------------------------------------------- properties 3 and 4: integer weights, weight 0
def integer_case(N, D, seed):
    rs = np.random.RandomState(seed)
    x = rs.randint(-3, 4, size=(N, D)).astype(F32)
    w = rs.randint(0, 5, size=N).astype(F32)
    return x, w


@pytest.mark.parametrize("precision", ["f32", "exact"])
@pytest.mark.parametrize("X, Y, N", [(16, 16, 2000), (64, 64, 3000)])
def test_integer_weight_equals_the_row_repeated_and_zero_equals_absent(X, Y, N, precision):
    D = 8
    x, w = integer_case(N, D, seed=X + N)
    zero = np.flatnonzero(w == 0)
    assert len(zero) > 10 and (w == 4).any()
    x[zero[3]] = np.nan                                       # a masked row may hold anything
    x[zero[7], 2] = np.inf
    repeated = np.repeat(x, w.astype(np.int64), axis=0)
    assert np.isfinite(repeated).all() and len(repeated) == int(w.sum())
    a = som(X, Y, D, random_seed=9, precision=precision).train(x, 3, sample_weight=w).get_weights()
    b = som(X, Y, D, random_seed=9, precision=precision).train(repeated, 3).get_weights()
    assert np.isfinite(a).all()
    assert same_bits(a, b)
    assert not same_bits(a, som(X, Y, D, random_seed=9, precision=precision).train(np.nan_to_num(x, posinf=0.0), 3).get_weights()), \
        "the weights changed nothing: the test is blind"


def test_all_weights_zero_leave_the_codebook_unchanged():
    X, Y, D, N = 16, 16, 8, 2000
    x, _ = integer_case(N, D, seed=1)
    s = som(X, Y, D, random_seed=9, precision="f32")
    before = np.asarray(s.get_weights(), dtype=F32).copy()
    s.train(x, 2, sample_weight=np.zeros(N))
    assert same_bits(before, s.get_weights())


# ----------------------------------------------------------------------------- property 5: all weights times a power of two
def test_weights_times_four_leave_the_codebook_bitwise_unchanged():
    X, Y, D, N = 16, 16, 8, 2000
    x = O.gaussian_blobs(N, D, seed=31)
    w = R.make_weights(N, 8)
    w[w != 0] += F32(2.0 ** -10)                              # (no weight so small that anything could underflow)
    kw = dict(sigmaN=4, random_seed=9, precision="f32")       # sigma runs 8 -> 4: see the module docstring
    a = som(X, Y, D, **kw).train(x, 3, sample_weight=w).get_weights()
    b = som(X, Y, D, **kw).train(x, 3, sample_weight=w * F32(4)).get_weights()
    assert same_bits(a, b)
    assert not same_bits(a, som(X, Y, D, **kw).train(x, 3).get_weights())


# ----------------------------------------------------------------------------- property 6: reproducible
def test_a_weighted_epoch_twice_is_bitwise_equal():
    X, Y, D, N = 24, 24, 16, 4096
    x = O.gaussian_blobs(N, D, seed=41)
    w = R.make_weights(N, 9)
    w0 = O.default_codebook(X, Y, D, 3).astype(F32).reshape(X * Y, D)
    e = engine(X, Y, D, precision="f32")
    try:
        e.set_data(x)
        e.set_sample_weights(w)
        out = []
        for _ in range(2):
            e.set_weights(w0)
            e.epoch_accumulate(3.0, 0.5, True)
            out.append(e.epoch_fetch())
    finally:
        e.close()
    assert np.array_equal(out[0][2], out[1][2])
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1])


# ----------------------------------------------------------------------------- streamed = resident
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_streamed_weighted_equals_resident_weighted(pinned):
    """Chunks of 1, 777 and 1 222 rows on the integer data: the sums are exact, so their order does not show."""
    X, Y, D, N = 16, 16, 8, 2000
    x, w = integer_case(N, D, seed=5)
    w0 = O.default_codebook(X, Y, D, 3).astype(F32).reshape(X * Y, D)
    cuts = [(0, 1), (1, 778), (778, N)]
    e = engine(X, Y, D, precision="f32")
    try:
        e.set_weights(w0)
        e.set_data(x)
        e.set_sample_weights(w)
        e.epoch_accumulate(3.0, 0.5, True)
        rnum, rden, _ = e.epoch_fetch(want_bmu=False)
        chunks = []
        for a, b in cuts:
            if pinned:
                cx, cw = e.pinned_empty((b - a, D)), e.pinned_empty((b - a,))
                cx[:], cw[:] = x[a:b], w[a:b]
            else:
                cx, cw = x[a:b].copy(), w[a:b].copy()
            chunks.append((cx, cw))
        e.stream_epoch_accumulate(chunks, 3.0, 0.5, True)
        snum, sden, _ = e.epoch_fetch(want_bmu=False)
    finally:
        e.close()
    assert rden.max() > 0
    assert same_bits(rnum, snum) and same_bits(rden, sden)


# ----------------------------------------------------------------------------- device weights = host weights
def test_device_weights_equal_host_weights():
    import torch
    X, Y, D, N = 16, 16, 8, 2000
    x = O.gaussian_blobs(N, D, seed=51)
    w = R.make_weights(N, 10)
    host = som(X, Y, D, random_seed=9, precision="f32").train(x, 3, sample_weight=w).get_weights()
    xd, wd = torch.as_tensor(x, device="cuda"), torch.as_tensor(w, device="cuda")
    dev = som(X, Y, D, random_seed=9, precision="f32").train(xd, 3, sample_weight=wd).get_weights()
    mixed = som(X, Y, D, random_seed=9, precision="f32").train(xd, 3, sample_weight=w.astype(np.float64)).get_weights()
    assert same_bits(host, dev) and same_bits(host, mixed)


# ----------------------------------------------------------------------------- set_data clears the weights
def test_set_data_clears_the_weights():
    X, Y, D, N = 16, 16, 8, 2000
    x = O.gaussian_blobs(N, D, seed=61)
    w0 = O.default_codebook(X, Y, D, 3).astype(F32).reshape(X * Y, D)
    outs = []
    for with_weights in (True, False):
        e = engine(X, Y, D, precision="f32")
        try:
            e.set_weights(w0)
            e.set_data(x)
            if with_weights:
                e.set_sample_weights(R.make_weights(N, 11))
                e.epoch_accumulate(3.0, 0.5, True)
                outs.append(e.epoch_fetch(want_bmu=False)[:2])
                e.set_data(x)
            e.epoch_accumulate(3.0, 0.5, True)
            outs.append(e.epoch_fetch(want_bmu=False)[:2])
        finally:
            e.close()
    weighted, after, fresh = outs
    assert same_bits(after[0], fresh[0]) and same_bits(after[1], fresh[1])
    assert not same_bits(weighted[1], fresh[1])


# ----------------------------------------------------------------------------- the captured epoch graph follows the weights
def test_epoch_graph_follows_setting_and_clearing_weights(monkeypatch):
    """SOM_GRAPH=1 on a small float32 map: two unweighted epochs (the second captures and replays), weights set (the
    graph is dropped, its warm-up restarts: one eager epoch, one captured with the weighted instance), weights cleared,
    one more epoch.  Every epoch equals the eager handle's, bit for bit (one fixed summation order on both)."""
    X, Y, D, N = 12, 9, 7, 1500
    x = O.gaussian_blobs(N, D, seed=11)
    w = R.make_weights(N, 12)
    w0 = O.default_codebook(X, Y, D, 3).astype(F32)
    steps = [None, None, "set", None, "clear"]                # what happens before epoch t
    outs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SOM_GRAPH", mode)
        e = engine(X, Y, D, precision="f32")
        try:
            e.set_data(x)
            res = []
            for t, step in enumerate(steps):
                if step == "set":
                    e.set_sample_weights(w)
                elif step == "clear":
                    e.set_sample_weights(None)
                e.set_weights(w0 * F32(1.0 + 0.1 * t))
                e.epoch_accumulate(3.0 - 0.4 * t, 0.5 - 0.05 * t, t % 2 == 0)
                res.append(tuple(a.copy() for a in e.epoch_fetch()))
                e.epoch_merge()
        finally:
            e.close()
        outs[mode] = res
    for t, (eager, graph) in enumerate(zip(outs["0"], outs["1"])):
        assert np.array_equal(eager[2], graph[2]), "epoch %d: BMUs" % t
        assert same_bits(eager[0], graph[0]) and same_bits(eager[1], graph[1]), "epoch %d: accumulators" % t
    # the weights were in force in epochs 2 and 3 only: the count column sums to sum(w) there, to N elsewhere
    e0 = outs["0"]
    assert not same_bits(e0[1][1], e0[2][1])


# ----------------------------------------------------------------------------- the faithful cross-check stays unweighted
def test_faithful_form_refuses_weights():
    from xpysom_dask_amd.engine import SomHipError
    X, Y, D, N = 8, 8, 3, 300
    e = engine(X, Y, D, precision="f32")
    try:
        e.set_weights(O.default_codebook(X, Y, D, 3).astype(F32))
        e.set_data(O.gaussian_blobs(N, D, seed=1))
        e.set_sample_weights(np.ones(N, F32))
        with pytest.raises(SomHipError, match="sample weights are set"):
            e.epoch_accumulate_faithful(2.0, 0.5, True)
        e.set_sample_weights(None)
        e.epoch_accumulate_faithful(2.0, 0.5, True)
    finally:
        e.close()


def test_host_weights_are_checked_by_the_library():
    from xpysom_dask_amd.engine import SomHipError
    X, Y, D, N = 8, 8, 3, 300
    e = engine(X, Y, D, precision="f32")
    try:
        e.set_data(O.gaussian_blobs(N, D, seed=1))
        w = np.ones(N, F32)
        w[17] = -1.0
        with pytest.raises(SomHipError, match="weight 17 "):
            e.set_sample_weights(w)
        w[17] = np.nan
        with pytest.raises(SomHipError, match="weight 17 "):
            e.set_sample_weights(w)
        with pytest.raises(SomHipError, match="one weight per resident row"):
            e._check(e._lib.som_set_sample_weights(e._h, e._fp(w), N - 1))
    finally:
        e.close()
