"""Sparse rows (csrc/sparse.hpp) against the float64 references of tests/query_ref.py and tests/update_ref.py on data.toarray().

Every case is the smallest that reaches a tail of the kernels: K below one wave (5 x 7) and one past a workgroup's 1 024-unit slab
(33 x 33: the parts merge), D = 3 and D one past a 2 048-column slab of the segment sum, n = 1 and n no multiple of the 32-row tile,
rows without entries first, in the middle and last, one fully dense row (at D = 2 049 longer than a 1 024-entry staging chunk),
densities of about 1 % and 30 %."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests import query_ref as Q, torus_ref as T, update_ref as U
from xpysom_dask_amd import XPySom
from xpysom_dask_amd.engine import HipEngine, SomHipError
from xpysom_dask_amd.xpysom import _csr_rows

pytestmark = pytest.mark.gpu

#        id        X   Y   D     n    density kind     dup
CASES = {"k35":   (5,  7,  3,    1,   0.5,  "blobs", 0),
         "k1089": (33, 33, 40,   70,  0.3,  "blobs", 0),
         "slab":  (6,  6,  2049, 45,  0.01, "blobs", 0),
         "int35": (5,  7,  3,    33,  0.5,  "int",   3),
         "int":   (33, 33, 24,   100, 0.3,  "int",   40)}
MODES = {"euclidean": "part", "euclidean_no_opt": "sq", "cosine": "cosine"}
FAMILIES = {"gaussian-rect": ("gaussian", "rectangular"), "mexican-torus": ("mexican_hat", "toroidal"), "gaussian-hex": ("gaussian", "hexagonal")}
SIGMA, ETA, STD = np.float64(1.5), 0.5, 0.5
_made = {}


def inputs(name):
    """(dense rows, csr arrays, units) of a case, made once: rows of query_ref.make_rows under a seeded support mask"""
    if name not in _made:
        X, Y, D, n, density, kind, dup = CASES[name]
        rs = np.random.RandomState(len(name) + D)
        x = Q.make_rows(kind, n, D, 7) * (rs.rand(n, D) < density)
        if n >= 4:
            x[[0, n // 2, n - 1]] = 0                                  # rows without entries: first, in the middle, last
            x[1] = Q.make_rows(kind, 1, D, 8)[0] + (0.5 if kind == "int" else 0.0)   # one fully dense row (int: no zero in it)
        x = x.astype(np.float32)
        w = Q.make_units(kind, x, X * Y, D, 9, dup=dup)
        _made[name] = (x, _csr_rows(sp.csr_matrix(x), D), w)
    return _made[name]


def engine(name, distance="euclidean", precision="exact", **kw):
    X, Y, D = CASES[name][:3]
    e = HipEngine(X, Y, D, distance=distance, precision=precision, std_coeff=STD, **kw)
    e.set_weights(inputs(name)[2])
    return e


@pytest.mark.parametrize("distance", MODES)
@pytest.mark.parametrize("name", CASES)
def test_search(name, distance):
    x, csr, w = inputs(name)
    e = engine(name, distance, "f32" if distance == "cosine" else "exact")
    try:
        ids = e.bmu_csr(csr)
        s, E = Q.scores(x, w, MODES[distance])
        if CASES[name][5] == "int" and distance != "cosine":
            Q.check_ties(ids, s, name)                                  # exact data: the lowest-index float64 argmin, bit for bit
        else:
            print("%s %s: err/bound %.3g" % (name, distance, Q.check_picks(ids, s, E, name)))
        for parts in ("1", "3", "64", None):                           # every geometry, and a second call: the same ids
            os.environ.pop("SOM_SPARSE_PARTS", None)
            if parts:
                os.environ["SOM_SPARSE_PARTS"] = parts
            assert np.array_equal(e.bmu_csr(csr), ids), parts
    finally:
        os.environ.pop("SOM_SPARSE_PARTS", None)
        e.close()


@pytest.mark.parametrize("name", CASES)
def test_quantization_error(name):
    x, csr, w = inputs(name)
    e = engine(name)
    try:
        qe, ids = e.quantization_error_csr(csr), e.bmu_csr(csr, quantization=True)
        Q.check_picks(ids, *Q.scores(x, w, "sqrt"), name)
        print("%s: QE err/bound %.3g" % (name, Q.check_qe(qe, x, w, ids, name)))
        assert e.quantization_error_csr(csr) == qe
    finally:
        e.close()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", CASES)
def test_epoch(name, family):
    x, csr, w = inputs(name)
    X, Y, D = CASES[name][:3]
    neigh, topo = FAMILIES[family]
    exact = CASES[name][5] == "int"
    e = engine(name, neighborhood=neigh, topology=topo)
    try:
        runs = []
        for _ in range(2):                                             # twice from the same state: the same bits
            e.set_weights(w)
            e.set_data_csr(csr)
            e.epoch_accumulate(SIGMA, ETA, True)
            num, den, bmu = e.epoch_fetch()
            S, c = e.debug_segment_sums()
            e.epoch_merge()
            runs.append((num, den, bmu, S, c, e.get_weights()))
        for a, b in zip(*runs):
            assert np.array_equal(a, b)
        num, den, bmu, S, c, w1 = runs[0]
        Q.check_picks(bmu, *Q.scores(x, w, "part"), name)
        ref_fn = T.reference_update if topo == "toroidal" else U.reference_update
        kw = {} if topo == "toroidal" else {"topology": topo}
        ref = ref_fn(x, bmu, X, Y, ETA, SIGMA, wide=True, neighbourhood=neigh, std_coeff=STD, **kw)
        a = U.check_accumulators(num, den, ref, name)
        m = U.check_merge(w, w1, num, den, ref, neigh == "mexican_hat", name)
        print("%s %s: accumulators err/bound %.3g, merge err/bound %.3g" % (name, family, a, m))
        units, S_ref, _, c_ref = U.segment_sums(x, bmu)
        full = np.zeros((X * Y, D)); full[units] = S_ref
        cnt = np.zeros(X * Y); cnt[units] = c_ref
        assert np.array_equal(c, cnt)
        if exact:                                                      # small integers (and halves): every sum is exact
            assert np.array_equal(S, full)
            d = engine(name, precision="f32")
            try:
                assert np.array_equal(d.bmu(x), bmu)
            finally:
                d.close()
        else:
            assert np.abs(S - full).max() <= 1e-5 * np.abs(full).max()
        # dense rows drop the sparse ones, and the dense epoch runs as ever
        e.set_weights(w)
        e.set_data(x)
        e.epoch_accumulate(SIGMA, ETA, True)
        assert len(e.epoch_fetch()[2]) == len(x)
    finally:
        e.close()


def test_bad_arguments_are_messages():
    x, (indptr, indices, values), w = inputs("k1089")
    e = engine("k1089")
    try:
        good = e.bmu_csr((indptr, indices, values))
        for bad, what in (((indptr[::-1].copy(), indices, values), "indptr"),
                          ((np.r_[indptr[:5], indptr[3], indptr[6:]], indices, values), "indptr decreases"),
                          ((indptr, np.where(np.arange(len(indices)) == 5, 40, indices).astype(np.int32), values), "outside"),
                          ((indptr, np.where(np.arange(len(indices)) == 41, indices[40], indices).astype(np.int32), values), "ascend")):
            with pytest.raises(SomHipError, match=what):
                e.bmu_csr(bad)
            with pytest.raises(SomHipError, match=what):
                e.set_data_csr(bad)
        assert np.array_equal(e.bmu_csr((indptr, indices, values)), good)   # a refused call leaves the handle usable
    finally:
        e.close()
    h = engine("k1089", precision="bf16")
    try:
        with pytest.raises(SomHipError, match="bf16"):
            h.bmu_csr((indptr, indices, values))
    finally:
        h.close()


def test_class_surface():
    x, csr, _ = inputs("k1089")
    m = sp.coo_matrix(x)                                               # not CSR: goes through tocsr()
    soms = [XPySom(9, 8, 40, sigma=2.0, random_seed=3).train(m, 3) for _ in range(2)]
    assert np.array_equal(soms[0]._weights, soms[1]._weights) and np.isfinite(soms[0]._weights).all()
    som = soms[0]
    e = HipEngine(9, 8, 40)
    try:
        e.set_weights(som._weights)
        ids = e.bmu_csr(csr)
        assert np.array_equal(som.predict(m), ids)
        assert som.winner(m) == [tuple(divmod(int(i), 8)) for i in ids]
        assert som.quantization_error(m) == e.quantization_error_csr(csr)
    finally:
        e.close()
    for call, err in ((lambda: som.train(m, 1, sample_weight=np.ones(len(x))), NotImplementedError),
                      (lambda: som.train(m, 1, monitor=True), NotImplementedError),
                      (lambda: som.train_streaming(lambda: [m], 1), NotImplementedError),
                      (lambda: som.topographic_error(m), NotImplementedError),
                      (lambda: som.nearest_units(m, 2), NotImplementedError),
                      (lambda: som.density_map(m, 1.0), NotImplementedError),
                      (lambda: som.random_weights_init(m), NotImplementedError),
                      (lambda: som.pca_weights_init(m), NotImplementedError),
                      (lambda: XPySom(9, 8, 40, missing="nan").impute(m), NotImplementedError),
                      (lambda: XPySom(9, 8, 40, missing="nan").train(m, 1), NotImplementedError),
                      (lambda: XPySom(9, 8, 40, activation_distance="manhattan").train(m, 1), NotImplementedError),
                      (lambda: XPySom(9, 8, 40, precision="bf16").train(m, 1), ValueError),
                      (lambda: XPySom(9, 8, 40, precision="f16").winner(m), ValueError),
                      (lambda: som.train(sp.csr_matrix(x[:, :7]), 1), ValueError)):
        with pytest.raises(err):
            call()
    dense = XPySom(9, 8, 40, sigma=2.0, random_seed=3).train(x, 3)
    mixed = XPySom(9, 8, 40, sigma=2.0, random_seed=3)
    w0 = mixed._weights.copy()
    mixed.train(m, 1)
    mixed._weights = w0
    assert np.array_equal(mixed.train(x, 3)._weights, dense._weights)   # a dense train after a sparse one: the dense result
