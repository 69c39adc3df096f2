"""`XPySom.impute` / som_impute* on the device: every NaN of a row replaced by its best matching unit's value.  GPU only (`-m gpu`).

The call does no arithmetic on a value, so every check of the rows is an equality of bits against tests/impute_ref.py; the ids
are som_bmu(ACTIVATION)'s own and are held to missing_ref's float64 scores by query_ref.check_picks.

  1  bits          maps 5 x 7 and 16 x 16 (a second 128-unit tile of the search); input_len 1, 3 (a float a lane), 4, 128 (16
                   bytes a lane), 33, 130 (odd tile fill) -- and 1025 and 4100, rows longer than a tile of the fill: with 4 099
                   of them there are more tiles than workgroups, the only shapes at which a workgroup takes a second tile; 1,
                   63, 257 and 4 099 rows; every pattern of missing_ref.PATTERNS; -0.0, +-inf and a denormal placed by hand
  2  host = device = in place; the input untouched; a view that starts one float past an aligned allocation; refusals of out
  3  n_parallel chunks; impute(impute(x)) = impute(x); no NaN left after training
  4  a handle without the missing mode refuses
  5  usefulness    blobs around 16 centres: the filled values beat column means by more than a factor of two
  6  extent        N * D past 2^31 elements, 16 bytes a lane and -- through a view one float on -- a float a lane
"""
import time

import numpy as np
import pytest

from tests import extent_ref as R
from tests import impute_ref as I
from tests import missing_ref as M
from tests import query_ref as Q

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
NEG_ZERO, DENORMAL = 0x80000000, 0x00000005


def engine(*a, **kw):
    from xpysom_dask_amd.engine import HipEngine
    kw.setdefault("missing", "nan")
    kw.setdefault("precision", "f32")
    return HipEngine(*a, **kw)


def som(X, Y, D, w, **kw):
    from xpysom_dask_amd import XPySom
    kw.setdefault("missing", "nan")
    s = XPySom(X, Y, D, **kw)
    s._weights = np.asarray(w, F32).reshape(X, Y, D).copy()
    return s


def close(s):
    if s._engine_obj is not None:
        s._engine_obj.close()


def dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def host(t):
    return t.detach().cpu().numpy()


def offset_view(n, d, floats=1):
    """An (n, d) float32 view that starts `floats` floats past a fresh (256-byte aligned) allocation."""
    import torch
    buf = torch.zeros(n * d + floats + 3, dtype=torch.float32, device="cuda")
    v = buf[floats:floats + n * d].view(n, d)
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() == buf.data_ptr() + 4 * floats
    return v


def case_rows(X, Y, D, N, pattern, seed=0):
    """(x, w, rows that hold no infinity): blobs with holes of `pattern`, -0.0, +inf, -inf and a denormal placed by hand on
    observed or missing places alike (N >= 5), a codebook near the rows whose unit 0 -- what an empty row becomes -- starts
    with -0.0 and holds a denormal."""
    x = M.punch(Q.make_rows("blobs", N, D, 11 + D + seed), pattern, 5 + seed)
    w = Q.make_units("blobs", np.nan_to_num(Q.make_rows("blobs", 400, D, 11 + D)), X * Y, D, 7, dup=3)
    w.view(np.uint32)[0, 0] = NEG_ZERO
    w.view(np.uint32)[0, D - 1 if D > 1 else 0] = DENORMAL if D > 1 else NEG_ZERO
    v = x.view(np.uint32)
    finite = np.ones(N, bool)
    if N >= 5:
        v[0, 0], v[1, D - 1] = NEG_ZERO, DENORMAL
        x[2, D // 2], x[3, 0] = np.inf, -np.inf
        finite[[2, 3]] = False
    else:
        v[0, 0] = NEG_ZERO
    return x, w, finite


# ----------------------------------------------------------------------------- 1: bits
BITS_CASES = [   # X, Y, D, N, pattern, precision
    (5, 7, 1, 1, "none", "f32"),
    (5, 7, 1, 63, "row", "exact"),
    (16, 16, 1, 4099, "random30", "f32"),
    (5, 7, 3, 257, "payload", "f32"),
    (16, 16, 3, 4099, "halves", "exact"),
    (16, 16, 4, 63, "feature", "f32"),
    (5, 7, 4, 4099, "row", "f32"),
    (5, 7, 33, 257, "random30", "exact"),
    (16, 16, 33, 4099, "payload", "f32"),
    (16, 16, 128, 63, "halves", "f32"),
    (16, 16, 128, 257, "none", "exact"),
    (5, 7, 128, 4099, "random30", "f32"),
    (5, 7, 130, 257, "feature", "f32"),
    (16, 16, 130, 4099, "row", "f32"),
    (5, 7, 1025, 4099, "random30", "f32"),      # a float a lane, 4 099 tiles of one row: more than the grid holds
    (5, 7, 4100, 4099, "payload", "f32"),       # 16 bytes a lane, likewise
]


def test_the_cases_cover_every_axis():
    assert {c[4] for c in BITS_CASES} == set(M.PATTERNS)
    assert {c[3] for c in BITS_CASES} == {1, 63, 257, 4099}
    assert {(c[0], c[1]) for c in BITS_CASES} == {(5, 7), (16, 16)}
    for D in (1, 3, 4, 33, 128, 130):
        ns = {c[3] for c in BITS_CASES if c[2] == D}
        assert ns & {63, 257} and 4099 in ns, D


@pytest.mark.parametrize("X, Y, D, N, pattern, precision", BITS_CASES, ids=["%dx%dx%d-n%d-%s-%s" % c for c in BITS_CASES])
def test_bits(X, Y, D, N, pattern, precision):
    x, w, finite = case_rows(X, Y, D, N, pattern)
    x0 = x.copy()
    e = engine(X, Y, D, precision=precision)
    try:
        e.set_weights(w)
        want_ids = e.bmu(x)
        out, ids = e.impute(x)
        t = dev(x)
        o = dev(np.full_like(x, 7.0))
        ids_dev = e.impute_device(t.data_ptr(), N, o.data_ptr())
        w_after = e.get_weights()
    finally:
        e.close()
    what = "%dx%dx%d n%d %s" % (X, Y, D, N, pattern)
    assert I.same_bits(x, x0), what + ": the input was written"
    assert I.same_bits(w_after, w), what + ": the codebook was written"
    assert ids.dtype == np.int32 and np.array_equal(ids, want_ids), what + ": the ids are not som_bmu's"
    assert np.array_equal(ids_dev, ids), what + ": som_impute_device names other units"
    s, E = M.masked_scores(x[finite], w)
    worst = Q.check_picks(ids[finite], s, E, what)
    print("%s: worst err / bound %.3g, %d holes" % (what, worst, int(np.isnan(x).sum())))
    want = I.impute_reference(x, w, ids)
    assert out.dtype == F32 and out.shape == x.shape
    assert I.same_bits(out, want), "%s: som_impute differs at %r" % (what, I.first_difference(out, want))
    assert I.same_bits(host(o), want), "%s: som_impute_device differs at %r" % (what, I.first_difference(host(o), want))
    assert I.same_bits(host(t), x0), what + ": the device rows were written by an out-of-place call"
    if pattern == "none":
        assert I.same_bits(out, x0)
    empty = np.flatnonzero(np.isnan(x).all(axis=1))
    assert (ids[empty] == 0).all() and all(I.same_bits(out[r], w[0]) for r in empty)
    if pattern == "row":
        assert len(empty) >= 1


# ----------------------------------------------------------------------------- 2: host = device = in place; refusals
def test_host_device_in_place_and_unaligned_views_agree():
    import torch
    from xpysom_dask_amd.engine import SomHipError
    X, Y, D, N = 12, 11, 128, 257
    x, w, _ = case_rows(X, Y, D, N, "payload")
    e = engine(X, Y, D)
    try:
        e.set_weights(w)
        out_h, ids_h = e.impute(x)
        same = x.copy()
        assert e._lib.som_impute(e._h, e._fp(same), N, e._fp(same), None) == 0        # out_host == x_host, ids_out NULL
        t = dev(x)
        o = torch.empty_like(t)
        ids_o = e.impute_device(t.data_ptr(), N, o.data_ptr())
        kept = host(t)
        p = t.clone()
        ids_p = e.impute_device(p.data_ptr(), N, p.data_ptr())                        # in place
        vin, vout = offset_view(N, D), offset_view(N, D)
        vin.copy_(t)
        torch.cuda.synchronize()
        ids_v = e.impute_device(vin.data_ptr(), N, vout.data_ptr())                   # neither 16-byte aligned
        mixed = torch.empty_like(t)
        ids_m = e.impute_device(vin.data_ptr(), N, mixed.data_ptr())                  # only the rows are not
        kept_v = host(vin)
        ids_vp = e.impute_device(vin.data_ptr(), N, vin.data_ptr())                   # in place, a float a lane
        flat = torch.zeros((N + 1) * D, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for shift in (D, 1, -D):
            a, b = (0, shift) if shift > 0 else (-shift, 0)
            with pytest.raises(SomHipError, match="som_impute_device: .*overlap"):
                e.impute_device(flat.data_ptr() + 4 * a, N, flat.data_ptr() + 4 * b)
        with pytest.raises(SomHipError, match="som_impute: .*overlap"):
            e._check(e._lib.som_impute(e._h, e._fp(same), N - 1, e._fp(same[1:]), None))
        with pytest.raises(SomHipError, match="som_impute_device: .*NULL"):
            e.impute_device(t.data_ptr(), N, 0)
        with pytest.raises(SomHipError, match="som_impute_device: .*NULL"):
            e.impute_device(0, N, o.data_ptr())
        with pytest.raises(SomHipError, match="som_impute: .*n_rows < 0"):
            e._check(e._lib.som_impute(e._h, e._fp(same), -1, e._fp(same), None))
        assert e._lib.som_impute_device(e._h, None, 0, None, None) == 0                # no rows: nothing written, no refusal
    finally:
        e.close()
    want = I.impute_reference(x, w, ids_h)
    assert I.same_bits(out_h, want) and I.same_bits(same, want)
    for name, got, ids in (("device", o, ids_o), ("in place", p, ids_p), ("unaligned", vout, ids_v), ("unaligned rows", mixed, ids_m),
                           ("unaligned in place", vin, ids_vp)):
        assert np.array_equal(ids, ids_h), name
        assert I.same_bits(host(got), out_h), "%s differs at %r" % (name, I.first_difference(host(got), out_h))
    assert I.same_bits(kept, x) and I.same_bits(kept_v, x), "an out-of-place call wrote its rows"


class Cai:
    """A torch tensor seen through __cuda_array_interface__ alone."""

    def __init__(self, t, read_only=False):
        self.owner, self.shape = t, tuple(t.shape)
        self.__cuda_array_interface__ = {"shape": tuple(t.shape), "typestr": "<f4", "data": (t.data_ptr(), read_only),
                                         "version": 2, "strides": None}


def test_python_device_rows_and_what_out_may_be():
    import torch
    X, Y, D, N = 5, 7, 4, 63
    x, w, _ = case_rows(X, Y, D, N, "random30")
    s = som(X, Y, D, w)
    try:
        want, ids = s.impute(x, return_ids=True)
        assert ids.dtype == np.int64 and I.same_bits(want, I.impute_reference(x, w, ids))
        t = dev(x)
        new = s.impute(t)
        assert isinstance(new, torch.Tensor) and new.device == t.device and new.data_ptr() != t.data_ptr()
        assert I.same_bits(host(new), want) and I.same_bits(host(t), x)
        o = torch.empty_like(t)
        got, ids_o = s.impute(t, out=o, return_ids=True)
        assert got is o and I.same_bits(host(o), want) and np.array_equal(ids_o, ids) and ids_o.dtype == np.int64
        c = Cai(torch.empty_like(t))
        assert s.impute(Cai(t), out=c) is c and I.same_bits(host(c.owner), want)
        p = t.clone()
        assert s.impute(p, out=p) is p and I.same_bits(host(p), want)
        flat = torch.zeros((N + 1) * D, dtype=torch.float32, device="cuda")
        flat[:N * D] = t.reshape(-1)
        refused = [
            (t, Cai(torch.empty_like(t), read_only=True), "read-only"),
            (Cai(t, read_only=True), None, "out=None"),
            (Cai(t), None, "out=None"),
            (t, torch.empty(N, D + 1, device="cuda"), "shape"),
            (t, torch.empty(N + 1, D, device="cuda"), "shape"),
            (t, Cai(torch.empty(N * D, device="cuda").view(D, N)), "shape"),
            (t, torch.empty(N, D, device="cuda", dtype=torch.float64), "float32"),
            (t, torch.empty(N, 2 * D, device="cuda")[:, :D], "contiguous"),
            (t, np.empty((N, D), F32), "device memory"),
            (flat[:N * D].view(N, D), flat[D:].view(N, D), "overlaps"),
            (flat[:N * D].view(N, D), Cai(flat[1:1 + N * D].view(N, D)), "overlaps"),
        ]
        for data, out, why in refused:
            with pytest.raises(ValueError, match=why):
                s.impute(data, out=out)
        ro = Cai(t.clone(), read_only=True)
        with pytest.raises(ValueError, match="read-only"):
            s.impute(ro, out=ro)
        for converted in (t.double(), torch.empty(N, 2 * D, device="cuda")[:, :D]):
            with pytest.raises(ValueError, match="converted"):
                s.impute(converted, out=converted)
        assert I.same_bits(host(flat[:N * D].view(N, D)), x) and I.same_bits(host(t), x)
        assert I.same_bits(host(s.impute(t.double())), want)          # converted rows, a new result: served
        assert tuple(s.impute(t[:0]).shape) == (0, D)
    finally:
        close(s)


# ----------------------------------------------------------------------------- 3: chunks, round trip, after training
def test_chunks_round_trip_and_no_nan_after_training():
    X, Y, D, N = 5, 7, 6, 257
    x, w, _ = case_rows(X, Y, D, N, "row")
    x = np.nan_to_num(x, posinf=3.0, neginf=-3.0, nan=np.nan)          # (training below: no infinity in the rows)
    e = engine(X, Y, D)
    try:
        e.set_weights(w)
        whole, ids = e.impute(x)
    finally:
        e.close()
    s = som(X, Y, D, w, n_parallel=100)
    try:
        x0 = x.copy()
        got, got_ids = s.impute(x, return_ids=True)
        assert I.same_bits(got, whole) and np.array_equal(got_ids, ids) and I.same_bits(x, x0)
        assert I.same_bits(s.impute(got), got), "impute(impute(x)) != impute(x)"
        one = s.impute(x[5])
        assert one.shape == (D,) and I.same_bits(one, whole[5])
        lists = s.impute(x.astype(F64).tolist())
        assert I.same_bits(lists, whole)
        assert s.impute(np.zeros((0, D), F32)).shape == (0, D)
    finally:
        close(s)
    from xpysom_dask_amd import XPySom
    t = XPySom(X, Y, D, sigma=2.0, learning_rate=0.5, random_seed=4, missing="nan")
    try:
        t.train(x, 3)
        filled = t.impute(x)
        wt = np.asarray(t.get_weights(), F32).reshape(-1, D)
        assert np.isfinite(wt).all() and not np.isnan(filled).any()
        assert I.same_bits(filled, I.impute_reference(x, wt, t.predict(x)))
    finally:
        close(t)


# ----------------------------------------------------------------------------- 4: a handle without the missing mode
def test_a_handle_without_the_missing_mode_refuses():
    from xpysom_dask_amd.engine import SomHipError
    x = Q.make_rows("blobs", 10, 4, 1)
    e = engine(4, 4, 4, missing=None)
    try:
        with pytest.raises(SomHipError, match="som_impute: .*SOM_MISSING_NAN"):
            e.impute(x)
        t = dev(x)
        with pytest.raises(SomHipError, match="som_impute_device: .*SOM_MISSING_NAN"):
            e.impute_device(t.data_ptr(), 10, t.data_ptr())
        assert I.same_bits(host(t), x)
    finally:
        e.close()


# ----------------------------------------------------------------------------- 5: usefulness
def rmse(a, b, where):
    d = a.astype(F64)[where] - b.astype(F64)[where]
    return float(np.sqrt((d * d).mean()))


def test_filled_values_beat_column_means():
    """16 blob centres ~ N(0, 9 I) in 16 dimensions ARE the codebook of a 4 x 4 map; 4 096 rows = centre + N(0, I), 30 % punched.
    A filled value is its row's centre, off by the row's own noise: RMSE about 1.  A column mean misses by the spread of the
    centres and the noise: about sqrt(9 + 1).  The float64 model first, then the device, each below half the column means'."""
    rs = np.random.RandomState(0)
    c = rs.normal(0.0, 3.0, (16, 16)).astype(F32)
    truth = (c[rs.randint(0, 16, 4096)] + rs.normal(0.0, 1.0, (4096, 16))).astype(F32)
    x = M.punch(truth, "random30", 1)
    hole = np.isnan(x)
    means = np.where(hole, np.nanmean(x.astype(F64), axis=0)[None, :], x)
    base = rmse(means, truth, hole)
    model = rmse(I.impute_reference(x, c, M.masked_bmu(x, c)), truth, hole)
    print("RMSE on %d punched entries: column means %.4f, float64 model %.4f" % (hole.sum(), base, model))
    assert model < 0.5 * base
    s = som(4, 4, 16, c)
    try:
        got = s.impute(dev(x))
    finally:
        close(s)
    device = rmse(host(got), truth, hole)
    print("device %.4f" % device)
    assert device < 0.5 * base
    assert I.same_bits(host(got)[~hole], truth[~hole])


# ----------------------------------------------------------------------------- 6: past 2^31 elements
def test_extent_past_2_pow_31_elements():
    """D = 132, N = 2^24 + 4099: N * D = 2^31 + 6.8e7 elements, out of place, 16 bytes a lane; then the same two buffers through
    views that start one float on (N - 1 rows of other content: a float a lane).  Checked on the device, a slab at a time."""
    import torch
    D, N = 132, 2 ** 24 + 4099
    assert N * D > 2 ** 31 and N - (-(-2 ** 31 // D)) - 1 >= R.MIN_BEYOND
    t0 = time.time()
    raw, centres = R.rows_on_device(N, D, 505)
    empty = np.array([0, 2 ** 31 // D, 2 ** 31 // D + 1, N - 2], np.int64)
    x = R.punch_on_device(raw, 506, share=0.3, empty_rows=empty)
    del raw
    w = R.codebook_near(centres, 2, 2, 507)
    w.view(np.uint32)[0, 0] = NEG_ZERO
    out = torch.full_like(x, 7.0)
    tw = dev(w)
    torch.cuda.synchronize()
    t1 = time.time()
    e = engine(2, 2, D)
    try:
        e.set_weights(w)

        def run(xv, ov, what):
            n = len(xv)
            ids = e.impute_device(xv.data_ptr(), n, ov.data_ptr())
            assert np.array_equal(ids, e.bmu_device(xv.data_ptr(), n)), what + ": the ids are not som_bmu_device's"
            ti = dev(ids).long()
            for s, t in R.slabs(n):
                xs = xv[s:t]
                want = torch.where(torch.isnan(xs), tw[ti[s:t]], xs)
                bad = want.view(torch.int32) != ov[s:t].view(torch.int32)
                assert not bool(bad.any()), "%s: row %d differs" % (what, s + int(bad.any(dim=1).nonzero()[0]))
            return ids

        ids = run(x, out, "16 bytes a lane")
        assert (ids[empty] == 0).all() and len(np.unique(ids)) == 4
        assert bool((out[torch.from_numpy(empty).cuda()].view(torch.int32) == tw[0].view(torch.int32)).all())
        t2 = time.time()
        out.fill_(7.0)
        xv = x.view(-1)[1:1 + (N - 1) * D].view(N - 1, D)
        ov = out.view(-1)[1:1 + (N - 1) * D].view(N - 1, D)
        assert xv.data_ptr() % 16 == 4 and ov.data_ptr() % 16 == 4
        run(xv, ov, "a float a lane")
        assert float(out.view(-1)[0]) == 7.0 and bool((out[N - 1, 1:] == 7.0).all()), "the fill left its rows"
    finally:
        e.close()
    print("extent: N * D = %d; data %.2f s, 16-byte path %.2f s, scalar path %.2f s" % (N * D, t1 - t0, t2 - t1, time.time() - t2))
