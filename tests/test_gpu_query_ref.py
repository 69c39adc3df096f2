"""The query kernels -- winner / quantization / quantization_error / topographic_error's top-2 / activate /
distance_from_weights / the float64 rows / the pairwise distances -- against the float64 reference of tests/query_ref.py.
GPU only (`-m gpu`).

Every case is teacher-forced: set a codebook, query rows, compare with the reference computed from the codebook the engine
holds (get_weights).  The checks and their bounds are query_ref's: admissible picks, exact ties on integer data, top-2 in
order, every distance-matrix element within its bound, QE against the float64 mean distance to the handle's own ids.
The grid is built from the tile edges (8 .. 128 features per row image, 64-unit stages, 128-row / 128-unit tiles, the
150 KiB LDS rule at 266 features, qe_kernel's stride above 16 384 rows); tests/test_query_ref_cpu.py checks that it reaches
every label query_ref.query_paths names."""
import numpy as np
import pytest

from tests.query_ref import (F32, F64, check_matrix, check_picks, check_qe, check_ties, check_top2, make_rows, make_units,
                             qe_reference, scores)

pytestmark = pytest.mark.gpu

ALL_CALLS = ("bmu", "quant", "top2", "dist", "dist_q", "f64", "qe", "qe_dev")


def _case(X, Y, D, n, prec="f32", dist="euclidean", data="blobs", calls=ALL_CALLS, env=None, p=2, p_real=0.0, dup=0):
    c = dict(X=X, Y=Y, D=D, n=n, prec=prec, dist=dist, data=data, calls=tuple(calls), env=dict(env or {}), p=p,
             p_real=p_real, dup=dup)
    c["id"] = "%dx%dx%d-n%d-%s-%s%s-%s%s" % (X, Y, D, n, prec, dist, ("-p%g" % (p_real or p)) if dist.startswith("norm_p") else "",
                                          data, "".join("-%s%s" % kv for kv in sorted(c["env"].items())))
    return c


P1 = {"SOM_F32_PARTS": "1"}
P3 = {"SOM_F32_PARTS": "3"}
PAIR = ("bmu",)
CASES = [
    # the float32 resident kernel: every k-group with one part and with merged parts, top-2 on each
    _case(1, 1, 8, 1),
    _case(1, 2, 9, 127, data="int", dup=1),
    _case(3, 5, 16, 128, env=P1),
    _case(4, 4, 17, 129, data="int"),
    _case(1, 17, 32, 255, data="offset30"),
    _case(7, 9, 33, 256),
    _case(8, 8, 64, 257, data="int", dup=8),
    _case(5, 13, 65, 129, data="offset300"),
    _case(1, 127, 128, 255, env=P1),
    _case(3, 43, 1, 257, env=P3),
    _case(3, 43, 8, 129, env=P3, data="int", dup=20),
    _case(8, 16, 16, 1, env=P3),
    _case(3, 43, 32, 255, env=P3, data="offset30"),
    _case(3, 43, 64, 128, env=P3),
    _case(9, 15, 128, 257, env=P3),
    _case(3, 43, 9, 127, env=P1),
    _case(40, 60, 24, 300, env={"SOM_F32_PARTS": "256"}),
    # the tiled kernel beyond 128 features
    _case(3, 43, 129, 129),
    _case(2, 8, 265, 127, data="int"),
    _case(1, 63, 266, 257),
    _case(8, 8, 784, 128, data="offset30"),
    _case(13, 5, 800, 255),
    # the other GEMM-form distances
    _case(3, 43, 33, 257, dist="euclidean_no_opt", calls=("bmu", "dist")),
    _case(2, 8, 17, 129, dist="cosine", calls=("bmu", "dist")),
    _case(3, 43, 129, 255, dist="cosine", calls=("bmu", "dist")),
    # the pairwise kernel: manhattan, norm_p even / odd / real, norm_p_no_opt; rows in LDS and in global memory
    _case(3, 5, 9, 129, dist="manhattan", calls=PAIR, data="int"),
    _case(1, 17, 266, 127, dist="manhattan", calls=PAIR),
    _case(1, 16, 10, 129, dist="norm_p", p=2, calls=PAIR, data="int"),
    _case(1, 17, 33, 128, dist="norm_p", p=3, calls=PAIR),
    _case(3, 5, 16, 129, dist="norm_p", p=4, calls=PAIR, data="int"),
    _case(1, 15, 8, 127, dist="norm_p", p=16, calls=PAIR),
    _case(1, 2, 265, 129, dist="norm_p", p=4, calls=PAIR),
    _case(1, 2, 266, 129, dist="norm_p", p=16, calls=PAIR),
    _case(1, 16, 266, 128, dist="norm_p", p=3, calls=PAIR),
    _case(1, 17, 17, 129, dist="norm_p", p_real=2.5, calls=PAIR),
    _case(1, 2, 266, 127, dist="norm_p", p_real=2.5, calls=PAIR),
    _case(1, 15, 65, 129, dist="norm_p_no_opt", p=2, calls=PAIR, data="int"),
    # qe_kernel striding, host and device rows
    _case(2, 8, 16, 20011, calls=("qe", "qe_dev", "quant")),
    # 'exact' handles: the value-only search under the screen (and a plan on a map of a few thousand units)
    _case(4, 16, 32, 1000, prec="exact", calls=("bmu", "quant", "top2", "dist", "dist_q", "f64", "qe", "qe_dev")),
    _case(4, 16, 32, 1000, prec="exact", data="offset30", calls=("bmu", "quant", "qe", "qe_dev")),
    _case(64, 64, 24, 3000, prec="exact", data="offset300", calls=("bmu", "quant", "qe", "qe_dev"),
          env={"SOM_EXACT_SKIP": "2"}),
    _case(4, 16, 20, 20011, prec="exact", data="blobs", calls=("qe", "qe_dev")),
]

def engine(X, Y, D, **kw):
    from xpysom_dask_amd.engine import HipEngine
    return HipEngine(X, Y, D, **kw)


def _activation_scores(c, x, w):
    d = c["dist"]
    if d == "euclidean":
        return scores(x, w, "part")
    if d == "euclidean_no_opt":
        return scores(x, w, "sq")
    if d == "cosine":
        return scores(x, w, "cosine")
    if d == "manhattan":
        return scores(x, w, "generic", p=1)
    if d == "norm_p" and not c["p_real"] and c["p"] % 2 == 0:
        return scores(x, w, "even", p=c["p"])
    return scores(x, w, "generic", p=c["p"], p_real=c["p_real"])


def _device_rows(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, F32)).cuda()


def run_query_case(c, worst=None):
    """Every call of the case against the reference; returns {call: worst err/bound}."""
    worst = {} if worst is None else worst
    X, Y, D, n = c["X"], c["Y"], c["D"], c["n"]
    K = X * Y
    seed = (X * 7919 + Y * 131 + D * 17 + n) % 100003
    x = make_rows(c["data"], n, D, seed)
    w0 = make_units(c["data"], x, K, D, seed, c["dup"])
    if c["dist"] == "cosine":
        x[0] = 0                                         # a zero row and a zero unit: nan_to_num's 1
        w0[-1] = 0
    exact_data = c["data"] == "int"
    kw = dict(distance=c["dist"], precision=c["prec"])
    if c["dist"].startswith("norm_p"):
        kw.update(norm_p=c["p"], norm_p_real=c["p_real"])
    e = engine(X, Y, D, **kw)
    try:
        e.set_weights(w0)
        w = e.get_weights()

        def note(call, r):
            worst[call] = max(worst.get(call, 0.0), r)

        for call in c["calls"]:
            what = "%s %s" % (c["id"], call)
            if call == "bmu":
                ids = e.bmu(x)
                s, E = _activation_scores(c, x, w)
                note(call, check_picks(ids, s, E, what))
                # (integer rows: exact scores while every power and partial sum stays below 2^24 -- |x|, |w| <= 3)
                pw = 1 if c["dist"] in ("euclidean", "euclidean_no_opt", "manhattan") else c["p"]
                if exact_data and c["dist"] != "cosine" and not c["p_real"] and 6.0 ** max(pw, 2) * 4 * D < 2.0 ** 24:
                    check_ties(ids, s, what)
            elif call == "quant":
                ids = e.bmu(x, quantization=True)
                s, E = scores(x, w, "sqrt")
                note(call, check_picks(ids, s, E, what))
                if exact_data:
                    check_ties(ids, s, what)
            elif call == "top2":
                a, b = e.bmu_top2(x)
                s, E = scores(x, w, "sqrt")
                note(call, check_top2(a, b, s, E, what, exact=exact_data))
            elif call in ("dist", "dist_q"):
                got = e.distance_matrix(x, quantization=call == "dist_q")
                mode = "sqrt" if call == "dist_q" else {"euclidean": "part", "euclidean_no_opt": "sq",
                                                        "cosine": "cosine"}[c["dist"]]
                s, E = scores(x, w, mode)
                note(call, check_matrix(got, s, E, what))
            elif call == "f64":
                x64 = x.astype(F64) * (1 + 2.0 ** -40)   # (not float32 values: the float64 arithmetic matters)
                ids = e.bmu_f64(x64)
                s, E = scores(x64, w, "f64")
                note(call, check_picks(ids, s, E, what))
            elif call in ("qe", "qe_dev"):
                if call == "qe":
                    qe = e.quantization_error(x)
                else:
                    t = _device_rows(x)
                    qe = e.quantization_error_device(t.data_ptr(), n)
                ids = e.bmu(x, quantization=True)
                note(call, check_qe(qe, x, w, ids, what))
            else:
                raise ValueError(call)
    finally:
        e.close()
    return worst


@pytest.fixture
def env_of(monkeypatch):
    def set_env(c):
        for k in ("SOM_F32_PARTS", "SOM_EXACT_SKIP"):
            monkeypatch.delenv(k, raising=False)
        for k, v in c["env"].items():
            monkeypatch.setenv(k, v)
    return set_env


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_query_case(c, env_of):
    env_of(c)
    run_query_case(c)


# ------------------------------------------------------------------------------------------ every precision's handle
@pytest.mark.parametrize("D", [24, 129])
def test_float32_calls_are_the_same_on_every_precision(D):
    """top-2, the distance matrix and the float64 rows always run the float32 kernels: bit-identical on every handle."""
    X, Y, n = 65, 65, 300                                 # (>= 4096 units: the wide exact screen beyond 128 features)
    x = make_rows("blobs", n, D, 3)
    w = make_units("blobs", x, X * Y, D, 3, dup=5)
    outs = {}
    for prec in ("f32", "exact", "bf16", "f16"):
        e = engine(X, Y, D, precision=prec)
        try:
            e.set_weights(w)
            outs[prec] = (e.bmu_top2(x), e.distance_matrix(x), e.distance_matrix(x, quantization=True), e.bmu_f64(x.astype(F64)))
        finally:
            e.close()
    ref = outs["f32"]
    for prec, o in outs.items():
        assert np.array_equal(o[0][0], ref[0][0]) and np.array_equal(o[0][1], ref[0][1]), prec
        assert np.array_equal(o[1].view(np.uint32), ref[1].view(np.uint32)), prec
        assert np.array_equal(o[2].view(np.uint32), ref[2].view(np.uint32)), prec
        assert np.array_equal(o[3], ref[3]), prec
    s, E = scores(x, w, "sqrt")
    check_top2(ref[0][0], ref[0][1], s, E, "top2")


# ------------------------------------------------------------------------------------------ stale operand images
def _check_all_queries(e, x, what, float32_picks=True):
    """float32_picks: the handle's own winner / quantization are float32's (f32, exact); a bf16 handle's are not"""
    w = e.get_weights()
    s, E = scores(x, w, "sqrt")
    a, b = e.bmu_top2(x)
    check_top2(a, b, s, E, what + " top2")
    check_matrix(e.distance_matrix(x, quantization=True), s, E, what + " dist_q")
    sp, Ep = scores(x, w, "part")
    check_matrix(e.distance_matrix(x), sp, Ep, what + " dist")
    ids = e.bmu(x, quantization=True)
    if float32_picks:
        check_picks(e.bmu(x), sp, Ep, what + " bmu")
        check_picks(ids, s, E, what + " quant")
    check_qe(e.quantization_error(x), x, w, ids, what + " qe")
    sf, Ef = scores(x.astype(F64), w, "f64")
    check_picks(e.bmu_f64(x.astype(F64)), sf, Ef, what + " f64")


@pytest.mark.parametrize("prec", ["exact", "bf16"])
def test_queries_after_an_epoch_see_the_merged_codebook(prec, monkeypatch):
    """after an epoch (exact with the plan on: patch-ordered images; bf16: the fused merge + operand preparation), after
    set_weights and after an exact winner: every query answers for the codebook get_weights returns"""
    monkeypatch.setenv("SOM_EXACT_SKIP", "2")
    X, Y, D, n = 64, 64, 32, 3000
    data = make_rows("blobs", 20000, D, 21)
    q = make_rows("blobs", n, D, 22)
    w0 = make_units("blobs", data, X * Y, D, 21)
    e = engine(X, Y, D, precision=prec)
    try:
        e.set_weights(w0)
        e.set_data(data)
        e.epoch(2.0, 0.5, False)
        e.epoch(1.5, 0.5, False)
        _check_all_queries(e, q, prec + " after epochs", prec != "bf16")
        e.set_weights(w0[::-1].copy())
        _check_all_queries(e, q, prec + " after set_weights", prec != "bf16")
        e.epoch(1.5, 0.5, False)
        e.bmu(q)                                          # (an exact winner: the images in the screen's order)
        _check_all_queries(e, q, prec + " after a winner", prec != "bf16")
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ edges
def test_duplicate_units_and_rows_equal_to_units():
    X, Y, D = 5, 13, 20
    rs = np.random.RandomState(4)
    w = rs.normal(0, 1, (X * Y, D)).astype(F32)
    w[40:] = w[:25]                                      # every unit of 40.. repeats a lower one
    x = np.concatenate([w[rs.randint(0, X * Y, 200)], w]).astype(F32)
    e = engine(X, Y, D, precision="f32")
    try:
        e.set_weights(w)
        s, E = scores(x, w, "sqrt")
        ids = e.bmu(x, quantization=True)
        a, b = e.bmu_top2(x)
        base = np.where(np.arange(X * Y) >= 40, np.arange(X * Y) - 40, np.arange(X * Y))
        assert (ids < 40).all() and (a < 40).all()
        assert np.array_equal(ids[200:], base) and np.array_equal(a[200:], base)
        dupped = np.flatnonzero(np.arange(X * Y) < 25)
        assert np.array_equal(b[200:][dupped], dupped + 40)   # the equal twin is the second, named after its lower id
        check_top2(a, b, s, E, "dup")
        assert e.quantization_error(w) == 0.0
    finally:
        e.close()


def test_one_unit_map():
    """som_bmu_top2 names the one unit twice; topographic_error is the reference's NaN (rectangular) / 0.0 (hexagonal)"""
    from xpysom_dask_amd import XPySom
    x = make_rows("blobs", 50, 6, 1)
    for D in (6, 200):
        xx = make_rows("blobs", 50, D, 1)
        e = engine(1, 1, D, precision="f32")
        try:
            e.set_weights(np.ones((1, D), F32))
            a, b = e.bmu_top2(xx)
            assert (a == 0).all() and (b == 0).all()
        finally:
            e.close()
    for prec in ("f32", "exact"):
        rect = XPySom(1, 1, 6, precision=prec)
        assert np.isnan(rect.topographic_error(x))
        hexa = XPySom(1, 1, 6, precision=prec, topology="hexagonal")
        assert hexa.topographic_error(x) == 0.0


def test_class_level_chunking():
    """quantization_error / topographic_error in chunks of n_parallel rows, n not a multiple of it"""
    from xpysom_dask_amd import XPySom
    X, Y, D, n = 6, 7, 9, 1001
    x = make_rows("blobs", n, D, 8)
    w = make_units("blobs", x, X * Y, D, 8)
    for prec in ("f32", "exact"):
        a = XPySom(X, Y, D, precision=prec, n_parallel=64)
        a._weights = w.reshape(X, Y, D)
        e = engine(X, Y, D, precision="f32")
        try:
            e.set_weights(w)
            ids = e.bmu(x, quantization=True)
            p1, p2 = e.bmu_top2(x)
        finally:
            e.close()
        want = qe_reference(x, w, ids)
        assert abs(a.quantization_error(x) - want) <= 1e-6 * want
        i1, j1, i2, j2 = p1 // Y, p1 % Y, p2 // Y, p2 % Y
        te = float(((np.abs(i1 - i2) > 1) | (np.abs(j1 - j2) > 1)).mean())
        assert a.topographic_error(x) == pytest.approx(te, abs=1e-12)


# ------------------------------------------------------------------------------------------ exact == f32 on the value path
def _qe_data(kind, X, Y, D):
    if kind == "weights":                                # data == weights, offset 50
        rs = np.random.RandomState(9)
        w = (50.0 + rs.normal(0.0, 1e-2, (X * Y, D))).astype(F32)
        return w.copy(), w
    n = 20000
    x = make_rows(kind, n, D, 31)
    return x, make_units(kind, x, X * Y, D, 31)


@pytest.mark.parametrize("skip", ["2", None])
@pytest.mark.parametrize("kind", ["blobs", "offset30", "offset300", "weights"])
def test_exact_quantization_error_is_the_float32_one(kind, skip, monkeypatch):
    """'exact' promises float32's results: the QE of an exact handle equals the f32 handle's to 1e-12 relative (room for
    the order of qe_kernel's float64 atomics only -- i.e. the same ids), with the plan forced on and with the defaults."""
    if skip is None:
        monkeypatch.delenv("SOM_EXACT_SKIP", raising=False)
    else:
        monkeypatch.setenv("SOM_EXACT_SKIP", skip)
    X, Y, D = 64, 64, 32
    x, w = _qe_data(kind, X, Y, D)
    f = engine(X, Y, D, precision="f32")
    g = engine(X, Y, D, precision="exact")
    try:
        f.set_weights(w)
        g.set_weights(w)
        qf, qg = f.quantization_error(x), g.quantization_error(x)
        ids = f.bmu(x, quantization=True)
        check_qe(qf, x, w, ids, kind + " f32")
        assert abs(qg - qf) <= 1e-12 * qf, "%s: exact QE %r, f32 QE %r" % (kind, qg, qf)
        t = _device_rows(x)
        qd = g.quantization_error_device(t.data_ptr(), len(x))
        assert abs(qd - qf) <= 1e-12 * qf, "%s: exact device QE %r, f32 QE %r" % (kind, qd, qf)
        rows, sent = g.qe_stats()
        assert rows == 2 * len(x) and 0 <= sent <= rows
    finally:
        f.close()
        g.close()
