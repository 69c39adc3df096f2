"""The three row sets of a handle -- the resident rows, the query scratch (also the pageable streamed chunks), the two pinned-chunk
slots -- used in turn on ONE handle: what each leaves behind must not reach the others.  GPU only (`-m gpu`).

Nothing here is new behaviour: every case states what the engine did before its row sets had one owner (csrc/row_set.hpp, RowSet in
csrc/somhip.hip), and passes on that engine too.
  interleaving     queries on the resident rows' own device pointer, and on a host copy, between planned exact epochs: the
                   trajectory, and the carried last-BMU positions, are those of a handle that only ran the epochs
  capacity moves   the query set and the slots grow between calls (exact mode: the error half of |x|^2 moves with the capacity);
                   ids are float32's, the streamed accumulator is the resident epoch's bit for bit (integer data: exact sums, the
                   rule of tests/test_gpu_weights.py)
  odd layouts      |x|^2 as scratch only (16-bit + cosine beyond 128 features), the wide kernels, f16, f32 with |x|^2 -- against the
                   references of tests/test_gpu_half_ref.py and tests/test_gpu_parity.py with their tolerances"""
import numpy as np
import pytest

from oracle import som_oracle as O
from tests.half_ref import KEY_ULPS, check_half, family_of, half_paths, make_half_data

pytestmark = pytest.mark.gpu
F32 = np.float32


def engine(*a, **kw):
    from xpysom_dask_amd.engine import HipEngine
    return HipEngine(*a, **kw)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=F32).view(np.uint32), np.ascontiguousarray(b, dtype=F32).view(np.uint32))


def integer_rows(n, D, seed):
    """Features in {-3 .. 3}, weights in {0 .. 4}: every partial sum of up to 12 000 rows is an integer below 2^24."""
    rs = np.random.RandomState(seed)
    return rs.randint(-3, 4, size=(n, D)).astype(F32), rs.randint(0, 5, size=n).astype(F32)


# ----------------------------------------------------------------------------- case 1: interleaving
@pytest.mark.parametrize("X, Y, D", [(16, 16, 8), (12, 11, 5)])
def test_queries_between_epochs_leave_the_resident_rows_alone(X, Y, D, monkeypatch):
    import torch
    monkeypatch.setenv("SOM_EXACT_SKIP", "2")
    n, T = 3000, 4
    x = O.gaussian_blobs(n, D, seed=X + D)
    xd = torch.as_tensor(x, device="cuda")
    torch.cuda.synchronize()
    w0 = O.default_codebook(X, Y, D, 3).astype(F32).reshape(X * Y, D)
    busy, plain, f32 = engine(X, Y, D, precision="exact"), engine(X, Y, D, precision="exact"), engine(X, Y, D, precision="f32")
    try:
        for e in (busy, plain, f32):
            e.set_weights(w0)
            e.set_data_device(xd.data_ptr(), n, keepalive=xd)
        for t in range(T):
            sigma, eta = O.exponential_decay(4.0, 1.0, t, T), O.exponential_decay(0.5, 0.01, t, T)
            for e in (busy, plain, f32):
                e.epoch(sigma, eta, True)
            w = busy.get_weights()
            assert same_bits(w, plain.get_weights()), "epoch %d: the queries moved the trajectory" % t
            assert same_bits(w, f32.get_weights()), "epoch %d: precision 'exact' left the float32 trajectory" % t
            assert busy.exact_chain_stats() == plain.exact_chain_stats(), "epoch %d" % t
            # the same calls on both handles, on the resident rows' own pointer and on a host copy
            got = {}
            for name, e in (("exact", busy), ("f32", f32)):
                got[name] = [e.bmu_device(xd.data_ptr(), n), e.bmu_device(xd.data_ptr(), n, quantization=True),
                             *e.bmu_top2_device(xd.data_ptr(), n), e.bmu(x), *e.bmu_top2(x), e.bmu(x[:700], quantization=True)]
                got[name + "-qe"] = [e.quantization_error_device(xd.data_ptr(), n), e.quantization_error(x)]
            for i, (a, b) in enumerate(zip(got["exact"], got["f32"])):
                assert np.array_equal(a, b), "epoch %d, query %d: %d ids differ from float32's" % (t, i, (a != b).sum())
            # (the same float32 ids; the float64 sum of their distances is taken in no fixed order: n * 2^-53)
            assert np.allclose(got["exact-qe"], got["f32-qe"], rtol=1e-12, atol=0.0)
            assert got["exact-qe"][0] == pytest.approx(got["exact-qe"][1], rel=1e-12)
        assert plain.exact_resident_stats()[0] >= 2, "no epoch ran under a plan: the test is blind"
        assert np.array_equal(busy.epoch_fetch()[2], plain.epoch_fetch()[2])
    finally:
        for e in (busy, plain, f32):
            e.close()


# ----------------------------------------------------------------------------- case 2: capacity moves
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("skip", [None, "2"], ids=["skip-default", "skip-forced"])
def test_query_set_and_slots_grow_between_calls(skip, weighted, monkeypatch):
    if skip is not None:
        monkeypatch.setenv("SOM_EXACT_SKIP", skip)
    X, Y, D = 16, 16, 8
    sizes = (1000, 1000, 4000, 4000, 1000, 1000)              # pinned, pageable, pinned, ... : slot 0, query, slot 1, query, slot 0, query
    x, w = integer_rows(sum(sizes), D, seed=17)
    q = O.gaussian_blobs(5000, D, seed=23)
    w0 = O.default_codebook(X, Y, D, 3).astype(F32).reshape(X * Y, D)
    ex, f32 = engine(X, Y, D, precision="exact"), engine(X, Y, D, precision="f32")
    try:
        resident = {}
        for name, e in (("exact", ex), ("f32", f32)):
            e.set_weights(w0)
            e.set_data(x)
            if weighted:
                e.set_sample_weights(w)
            e.epoch_accumulate(3.0, 0.5, True)
            resident[name] = e.epoch_fetch()
        assert np.array_equal(resident["exact"][2], resident["f32"][2])
        assert same_bits(resident["exact"][0], resident["f32"][0]) and same_bits(resident["exact"][1], resident["f32"][1])
        assert resident["f32"][1].max() > 0

        def queries(what):
            for m in (100, 5000, 100):                        # the query set's error half moves out and stays
                a, b = ex.bmu(q[:m]), f32.bmu(q[:m])
                assert np.array_equal(a, b), "%s, %d rows: %d ids differ from float32's" % (what, m, (a != b).sum())
                a, b = ex.bmu_top2(q[:m]), f32.bmu_top2(q[:m])
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (what, m)

        queries("before the streamed epochs")
        # two streamed epochs: the slots alternate across them, so that the second one grows slot 0 under a 4 000-row chunk
        for epoch in range(2):
            for name, e in (("exact", ex), ("f32", f32)):
                chunks, at = [], 0
                for i, m in enumerate(sizes):
                    if i % 2 == 0:
                        cx, cw = e.pinned_empty((m, D)), e.pinned_empty((m,))
                        cx[:], cw[:] = x[at:at + m], w[at:at + m]
                    else:
                        cx, cw = x[at:at + m].copy(), w[at:at + m].copy()
                    chunks.append((cx, cw) if weighted else cx)
                    at += m
                e.stream_epoch_accumulate(chunks, 3.0, 0.5, True)
                num, den, _ = e.epoch_fetch(want_bmu=False)
                assert same_bits(num, resident[name][0]) and same_bits(den, resident[name][1]), (name, epoch)
            queries("after streamed epoch %d" % epoch)
        # ... and the resident rows were not touched by any of it
        ex.epoch_accumulate(3.0, 0.5, True)
        again = ex.epoch_fetch()
        assert np.array_equal(again[2], resident["exact"][2]) and same_bits(again[0], resident["exact"][0])
    finally:
        ex.close()
        f32.close()


# ----------------------------------------------------------------------------- case 3: the odd layouts
def near_tie_mask(x, w, tol=2e-6):
    """tests/test_gpu_parity.py's: best and second-best squared distance (float64) closer than float32's summation-order noise."""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    d = -2 * x64 @ w64.T + (w64 ** 2).sum(1)[None, :]
    part = np.partition(d, 1, axis=1)
    scale = (x64 ** 2).sum(1) + np.abs(part[:, 0]) + 1e-30
    return (part[:, 1] - part[:, 0]) < tol * scale


def resident_and_query(e, x):
    """BMUs of the same rows as the resident set (one epoch) and as one host query."""
    e.set_data(x)
    e.epoch_accumulate(1.0, 0.1, True)
    return e.epoch_fetch()[2], e.bmu(x)


@pytest.mark.parametrize("X, Y, D, prec, dist", [(8, 8, 130, "bf16", "cosine"), (64, 64, 260, "bf16", "euclidean"), (8, 8, 8, "f16", "euclidean")],
                         ids=["bf16-cosine-8x8x130-xsq-is-scratch", "bf16-64x64x260-wide", "f16-8x8x8"])
def test_half_layouts_against_the_rounded_operand_reference(X, Y, D, prec, dist):
    n = 600
    fam = family_of(half_paths(X, Y, D, n, prec, dist))
    x, w0 = make_half_data("blobs", n, X * Y, D, 7 * X + D, unit_kind=prec if dist == "cosine" else None)
    e = engine(X, Y, D, distance=dist, precision=prec)
    try:
        e.set_weights(w0)
        w = e.get_weights()
        res, ids = resident_and_query(e, x)
    finally:
        e.close()
    check_half(ids, x, w, prec, dist, KEY_ULPS[fam], False, "query")
    check_half(res, x, w, prec, dist, KEY_ULPS[fam], False, "resident")
    assert np.array_equal(ids, res), "the query and the resident path disagree on %d rows" % (ids != res).sum()


@pytest.mark.parametrize("dist", ["euclidean", "cosine"])
def test_exact_wide_layout_returns_float32s_ids(dist):
    X, Y, D, n = 64, 64, 260, 600
    x = np.abs(O.gaussian_blobs(n, D, seed=5))
    w0 = np.abs(O.default_codebook(X, Y, D, 2)).astype(F32).reshape(X * Y, D)
    out = {}
    for prec in ("exact", "f32"):
        e = engine(X, Y, D, distance=dist, precision=prec)
        try:
            e.set_weights(w0)
            out[prec] = resident_and_query(e, x)
            if prec == "exact":
                assert e.exact_stats()[0] >= 2 * n, "the screen did not serve: the test is blind"
        finally:
            e.close()
    for a, b, what in zip(out["exact"], out["f32"], ("resident", "query")):
        assert np.array_equal(a, b), "%s: %d ids differ from float32's" % (what, (a != b).sum())


def test_f32_euclidean_no_opt_reads_its_row_norms():
    X, Y, D, n = 8, 8, 8, 600
    x = O.gaussian_blobs(n, D, seed=9)
    w0 = O.default_codebook(X, Y, D, 3).astype(F32)
    e = engine(X, Y, D, distance="euclidean_no_opt", precision="f32")
    try:
        e.set_weights(w0)
        res, ids = resident_and_query(e, x)
    finally:
        e.close()
    ref = O.winner_ids(x, w0.reshape(X, Y, D), "euclidean_no_opt")
    for got, what in ((res, "resident"), (ids, "query")):
        diff = np.flatnonzero(got != ref)
        assert len(diff) <= max(2, n // 500) and near_tie_mask(x[diff], w0.reshape(-1, D)).all(), (what, len(diff))
    assert np.array_equal(res, ids)
