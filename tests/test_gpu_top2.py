"""The exact mode's top-2 path on the device (csrc/bmu_exact.hpp "TOP-2", csrc/exact_top2_host.hpp): the screen's
second-smallest window, one select, two float32 re-score rounds, the tie test of the sqrt'd distance on both units, the
float32 top-2 kernel for the rest.  GPU only (`-m gpu`).

The ids must be the float32 top-2 kernel's BIT FOR BIT: every case compares som_bmu_top2 and som_bmu_top2_device of an
'exact' handle with som_bmu_top2 of an 'f32' handle and of the same handle created under SOM_EXACT_TOP2=0 (the float32
kernel for every row: the path before this one existed), and checks the pair against the float64 scores of
tests/query_ref.py.  The CPU side of the same rules is tests/test_top2_ref_cpu.py."""
import warnings

import numpy as np
import pytest

from tests.conftest import load_golden
from tests.top2_ref import F32, check_top2, make_rows, make_units, scores, top2_fast_path, unsettled_share

pytestmark = pytest.mark.gpu

ENV_KEYS = ("SOM_EXACT_TOP2", "SOM_EXACT_PASS_ROWS", "SOM_EXACT_SKIP", "SOM_BF16_PARTS")


def engine(X, Y, D, **kw):
    from xpysom_dask_amd.engine import HipEngine
    return HipEngine(X, Y, D, **kw)


def _device_rows(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, F32)).cuda()


@pytest.fixture
def env(monkeypatch):
    def set_env(**kv):
        for k in ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in kv.items():
            monkeypatch.setenv(k, str(v))
    set_env()
    return set_env


def _top2_of(env, X, Y, D, w, x, precision="exact", distance="euclidean", device=False, **envkw):
    """(ids1, ids2, (rows, rows_f32)) of one handle created under the given environment."""
    env(**envkw)
    e = engine(X, Y, D, precision=precision, distance=distance)
    try:
        e.set_weights(w)
        if device:
            t = _device_rows(x)
            a, b = e.bmu_top2_device(t.data_ptr(), len(x))
        else:
            a, b = e.bmu_top2(x)
        return a, b, e.exact_top2_stats()
    finally:
        e.close()
        env()


def _codebook(kind, X, Y, D, x, seed):
    K = X * Y
    if kind == "default":                                  # the seeded default codebook of the class
        from xpysom_dask_amd import XPySom
        return np.asarray(XPySom(X, Y, D, random_seed=seed)._weights, F32).reshape(K, D)
    if kind == "smooth":                                   # a few epochs on the rows
        from xpysom_dask_amd import XPySom
        som = XPySom(X, Y, D, sigma=max(X, Y) / 4.0, random_seed=seed, precision="exact")
        som.train(x, 3)
        return np.asarray(som._weights, F32).reshape(K, D)
    if kind == "int":
        return make_units("int", x, K, D, seed, dup=min(K // 3, 40))
    return make_units(kind, x, K, D, seed)


def _case(X, Y, D, n, rows="blobs", book=None, special=None, **envkw):
    return dict(X=X, Y=Y, D=D, n=n, rows=rows, book=book or rows, special=special, env=envkw,
                id="%dx%dx%d-n%d-%s-%s%s%s" % (X, Y, D, n, rows, book or rows, "-" + special if special else "",
                                              "".join("-%s%s" % kv for kv in sorted(envkw.items()))))


CASES = [
    # one group (K <= 64), a short last group, whole patches, a side that is no multiple of 8; 3 .. 128 features
    _case(4, 16, 3, 1000, book="default"),
    _case(9, 7, 32, 777, book="default"),
    _case(4, 16, 32, 300, rows="int"),
    _case(9, 7, 100, 513, rows="offset30"),
    _case(64, 64, 3, 1000, book="default"),
    _case(64, 64, 32, 1000, book="smooth"),
    _case(64, 64, 32, 1000, rows="int"),
    _case(64, 64, 100, 777, rows="blobs", special="rows_are_units"),
    _case(64, 64, 128, 700, rows="offset30"),
    _case(64, 64, 32, 900, rows="offset300"),
    _case(64, 64, 32, 1000, rows="blobs", special="nan_inf"),
    _case(13, 21, 32, 1000, book="smooth"),
    _case(13, 21, 100, 600, rows="int"),
    _case(13, 21, 128, 700, rows="offset300"),
    _case(128, 128, 32, 700, book="default"),
    _case(128, 128, 128, 700, rows="blobs"),
    _case(128, 128, 100, 500, rows="int"),
    _case(128, 128, 3, 600, rows="offset30"),
    # more rows than one pass holds; forced codebook parts
    _case(64, 64, 32, 2500, rows="blobs", SOM_EXACT_PASS_ROWS=1024),
    _case(13, 21, 32, 2500, rows="int", SOM_EXACT_PASS_ROWS=1024),
    _case(64, 64, 32, 1000, rows="blobs", SOM_BF16_PARTS=3),
    _case(64, 64, 128, 1000, book="smooth", SOM_BF16_PARTS=1),
]


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_ids_are_the_float32_kernels_bit_for_bit(c, env):
    X, Y, D, n = c["X"], c["Y"], c["D"], c["n"]
    K = X * Y
    seed = (X * 7919 + Y * 131 + D * 17 + n) % 100003
    x = make_rows(c["rows"], n, D, seed)
    w = _codebook(c["book"], X, Y, D, x, seed)
    finite = np.ones(n, bool)
    if c["special"] == "rows_are_units":
        x = w[np.random.RandomState(seed).randint(0, K, n)].copy()
    if c["special"] == "nan_inf":
        x[3, 0] = np.nan
        x[17, D - 1] = np.inf
        x[40] = -np.inf
        x[41, 1] = 3.0e38
        x[99] = np.nan
        finite = np.isfinite(x).all(axis=1) & (np.abs(x).max(axis=1) < 1e30)
    assert top2_fast_path(X, Y, D, "exact", "euclidean")
    ref1, ref2, st_ref = _top2_of(env, X, Y, D, w, x, precision="f32")
    off1, off2, st_off = _top2_of(env, X, Y, D, w, x, SOM_EXACT_TOP2=0, **c["env"])
    a1, a2, st = _top2_of(env, X, Y, D, w, x, **c["env"])
    d1, d2, st_d = _top2_of(env, X, Y, D, w, x, device=True, **c["env"])
    print("%s: rows %d, to the float32 kernel %d (host rows), %d (device rows)" % (c["id"], st[0], st[1], st_d[1]))
    for what, (p1, p2) in (("SOM_EXACT_TOP2=0", (off1, off2)), ("host rows", (a1, a2)), ("device rows", (d1, d2))):
        bad = np.flatnonzero((p1 != ref1) | (p2 != ref2))
        assert len(bad) == 0, "%s: %d rows differ from the f32 handle, first row %d: (%d, %d) vs (%d, %d)" % (
            what, len(bad), bad[0], p1[bad[0]], p2[bad[0]], ref1[bad[0]], ref2[bad[0]])
    assert st_ref == (n, n) and st_off == (n, n) and st[0] == n and st_d[0] == n
    # admissibility against the float64 scores (rows the reference arithmetic covers)
    s, E = scores(x[finite], w, "sqrt")
    check_top2(a1[finite], a2[finite], s, E, c["id"], exact=c["rows"] == "int")


@pytest.mark.parametrize("X,Y,D", [(64, 64, 32), (128, 128, 128)])
def test_the_fast_path_is_really_taken(X, Y, D, env):
    """Centred blobs: nearly every row is answered by the screen + re-score.  The cap of 5 % keeps the test from passing on
    the float32 kernel alone; tests/top2_ref.py's CPU estimate for these very inputs is 0 (64 x 64 x 32) and 0.02 %."""
    n = 4096
    x = make_rows("blobs", n, D, 11)
    w = make_units("blobs", x, X * Y, D, 11)
    assert unsettled_share(x[:512], w) <= 0.01
    a1, a2, st = _top2_of(env, X, Y, D, w, x, device=True)
    r1, r2, _ = _top2_of(env, X, Y, D, w, x, precision="f32")
    print("%dx%dx%d: %d of %d rows to the float32 kernel" % (X, Y, D, st[1], st[0]))
    assert np.array_equal(a1, r1) and np.array_equal(a2, r2)
    assert st[0] == n
    assert st[1] / st[0] <= 0.05


@pytest.mark.parametrize("prec,dist,D,envkw", [("exact", "euclidean", 32, {"SOM_EXACT_TOP2": 0}), ("f32", "euclidean", 32, {}),
                                               ("exact", "cosine", 32, {}), ("exact", "euclidean", 130, {}),
                                               ("bf16", "euclidean", 32, {}), ("f16", "euclidean", 32, {})])
def test_off_switches_keep_the_float32_kernel(prec, dist, D, envkw, env):
    X, Y, n = 64, 64, 700
    x = make_rows("blobs", n, D, 5)
    w = make_units("blobs", x, X * Y, D, 5)
    a1, a2, st = _top2_of(env, X, Y, D, w, x, precision=prec, distance=dist, **envkw)
    d1, d2, st_d = _top2_of(env, X, Y, D, w, x, precision=prec, distance=dist, device=True, **envkw)
    r1, r2, _ = _top2_of(env, X, Y, D, w, x, precision="f32")
    assert st == (n, n) and st_d == (n, n)
    assert np.array_equal(a1, r1) and np.array_equal(a2, r2) and np.array_equal(d1, r1) and np.array_equal(d2, r2)


def test_one_unit_map_names_unit_zero_twice(env):
    x = make_rows("blobs", 100, 8, 1)
    a, b, st = _top2_of(env, 1, 1, 8, x[:1], x, device=True)
    assert (a == 0).all() and (b == 0).all() and st == (100, 100)


def test_device_call_checks_its_arguments(env):
    from xpysom_dask_amd.engine import SomHipError
    e = engine(4, 4, 8)
    try:
        with pytest.raises(SomHipError, match="som_bmu_top2_device: bad argument"):
            e.bmu_top2_device(0, 5)
        a, b = e.bmu_top2_device(0, 0)
        assert len(a) == 0 and len(b) == 0
    finally:
        e.close()


@pytest.mark.parametrize("topology", ["rectangular", "hexagonal"])
def test_topographic_error_of_device_rows(topology, env):
    from xpysom_dask_amd import XPySom
    X, Y, D, n = 24, 24, 32, 3000
    x = make_rows("blobs", n, D, 9)
    vals = {}
    trained = None
    for prec in ("exact", "f32"):
        som = XPySom(X, Y, D, sigma=4.0, random_seed=3, precision=prec, topology=topology, n_parallel=1024)
        if trained is None:
            som.train(x, 2)
            trained = som._weights
        else:
            som._weights = trained                         # (the same codebook under both precisions)
        host = som.topographic_error(x)                    # (n_parallel < n: three chunks)
        dev = som.topographic_error(_device_rows(x))
        assert dev == host, (prec, dev, host)
        assert type(dev) is type(host)
        vals[prec] = host
        rows, rows_f32 = som._engine().exact_top2_stats()
        assert rows == 2 * n
        assert rows_f32 <= 0.05 * rows if prec == "exact" else rows_f32 == rows
    assert vals["exact"] == vals["f32"]
    # the 1-by-1 and the empty cases keep their values for device rows too
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.isnan(XPySom(1, 1, 1).topographic_error(_device_rows(x[:, :1])))
    r = XPySom(1, 1, D, topology=topology).topographic_error(_device_rows(x[:10]))
    assert (np.isnan(r) if topology == "rectangular" else r == 0.0)


def test_later_epochs_and_queries_are_undisturbed(env):
    """A top-2 call between two epochs: the plan's counters do not move, and the next epoch and winner call give the ids and
    accumulators of a handle that made no top-2 call."""
    X, Y, D, n = 64, 64, 32, 8192
    x = make_rows("blobs", n, D, 21)
    w = make_units("blobs", x, X * Y, D, 21)
    probe = make_rows("blobs", 20000, D, 22)
    out = {}
    for name in ("with_top2", "without"):
        env(SOM_EXACT_SKIP=2)
        e = engine(X, Y, D, precision="exact")
        try:
            e.set_weights(w)
            e.set_data(x)
            for t in range(3):
                e.epoch(6.0 - t, 0.5, 0)
            if name == "with_top2":
                before = (e.exact_skip_stats(), e.exact_resident_stats(), e.exact_scout_stats(), e.exact_stats())
                t_small, t_big = _device_rows(probe[:2000]), _device_rows(probe)
                p_small = e.bmu_top2_device(t_small.data_ptr(), 2000)
                p_big = e.bmu_top2_device(t_big.data_ptr(), len(probe))          # (more rows than the pass scratch holds)
                after = (e.exact_skip_stats(), e.exact_resident_stats(), e.exact_scout_stats(), e.exact_stats())
                assert before == after
                assert e.exact_top2_stats()[0] == 2000 + len(probe)
                out["pairs"] = (p_small, p_big)
            e.epoch_accumulate(3.0, 0.4, 0)
            num, den, bmu = e.epoch_fetch()
            e.epoch_merge()
            out[name] = (num, den, bmu, e.bmu(probe[:3000]), e.get_weights(), e.exact_resident_stats())
        finally:
            e.close()
            env()
    a, b = out["with_top2"], out["without"]
    for i in range(5):
        assert np.array_equal(a[i], b[i]), i
    assert a[5] == b[5]
    r1, r2, _ = _top2_of(env, X, Y, D, _weights_after_three_epochs(env, X, Y, D, w, x), probe, precision="f32")
    assert np.array_equal(out["pairs"][1][0], r1) and np.array_equal(out["pairs"][1][1], r2)
    assert np.array_equal(out["pairs"][0][0], r1[:2000]) and np.array_equal(out["pairs"][0][1], r2[:2000])


def _weights_after_three_epochs(env, X, Y, D, w, x):
    """The codebook after the three epochs of test_later_epochs_and_queries_are_undisturbed (what its top-2 calls saw)."""
    env(SOM_EXACT_SKIP=2)
    e = engine(X, Y, D, precision="exact")
    try:
        e.set_weights(w)
        e.set_data(x)
        for t in range(3):
            e.epoch(6.0 - t, 0.5, 0)
        return e.get_weights()
    finally:
        e.close()
        env()


def test_full_size_map(env):
    """256 x 256 x 128 on 65 536 device rows: the ids of a 4 096-row sample are the f32 handle's."""
    X, Y, D, n = 256, 256, 128, 65536
    x = make_rows("blobs", n, D, 31)
    w = make_units("blobs", x, X * Y, D, 31)
    a1, a2, st = _top2_of(env, X, Y, D, w, x, device=True)
    sample = np.arange(0, n, n // 4096)
    r1, r2, _ = _top2_of(env, X, Y, D, w, x[sample], precision="f32")
    print("256x256x128: %d of %d rows to the float32 kernel" % (st[1], st[0]))
    assert np.array_equal(a1[sample], r1) and np.array_equal(a2[sample], r2)
    assert st[0] == n and st[1] / st[0] <= 0.05


def test_golden_topographic_error(env):
    """tests/golden/g21 (tools/make_golden_topographic.py): a codebook the reference trained, its topographic_error on 4 096
    probe rows and their two smallest distances.  Values are pinned on every row (the reference takes its pair from an
    unstable argsort), ids where the two smallest float32 distances differ from each other and from the third.  The probe
    rows are other rows of the training mixture; the generator recomputed the tie test's unsettled share for them on the CPU
    (tests/top2_ref.py: 0.0, stored in the fixture) before they were fixed, so the fast path's 5 % cap holds here too.
    What pins the pair: the ids on the `distinct` rows (all but two) and the exact `te`.  The value check is a sanity bound
    only -- the float32 sqrt'd distance is off by up to sqrt(gamma) (|x| + |w|) ~ 1e-2 on distances of order 1-10, wide enough
    for a third-best unit to pass it."""
    from xpysom_dask_amd import XPySom
    from xpysom_dask_amd.synthetic import gaussian_blobs
    g = load_golden("g21_topographic_64x64x32")
    w = g["w"]
    X, Y, D = w.shape
    probe = gaussian_blobs(int(g["n_probe"]), D, seed=int(g["probe_seed"])).astype(F32)
    som = XPySom(X, Y, D, precision="exact")
    som._weights = w
    te_host = som.topographic_error(probe)
    te_dev = som.topographic_error(_device_rows(probe))
    assert te_host == te_dev == float(g["te"])
    a1, a2 = som._engine().bmu_top2(probe)
    rows, rows_f32 = som._engine().exact_top2_stats()
    print("g21: %d of %d rows to the float32 kernel" % (rows_f32, rows))
    assert float(g["unsettled_share_cpu"]) <= 0.01
    assert rows == 3 * len(probe) and rows_f32 <= 0.05 * rows
    wf = w.reshape(-1, D).astype(np.float64)
    p64 = probe.astype(np.float64)
    d1 = np.linalg.norm(p64 - wf[a1], axis=1)
    d2 = np.linalg.norm(p64 - wf[a2], axis=1)
    # the reference's float32 distances: |sqrt(a) - sqrt(b)| <= sqrt|a - b|, radicands off by gamma(D + 3)(2|x||w| + |w|^2 + |x|^2)
    u = 2.0 ** -24
    rad = (D + 3) * u / (1 - (D + 3) * u) * (np.linalg.norm(p64, axis=1) + np.linalg.norm(wf, axis=1).max()) ** 2
    tol = np.sqrt(rad) + 4 * u * g["d12"].max()
    assert (np.abs(d1 - g["d12"][:, 0]) <= tol).all() and (np.abs(d2 - g["d12"][:, 1]) <= tol).all()
    keep = g["distinct"]
    assert keep.sum() > 0.9 * len(keep)
    assert np.array_equal(a1[keep], g["ids12"][keep, 0]) and np.array_equal(a2[keep], g["ids12"][keep, 1])
