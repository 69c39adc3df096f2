"""precision='exact' on 801 .. 4096 features (maps of >= 4096 units): the group-minimum instance of the two-sided tiling
(csrc/bmu_bf16_tiled.hpp, GM) + the float32 re-score return the float32 kernel's BMUs bit for bit.  The checker is a
precision='f32' handle.  GPU only (`-m gpu`)."""
import numpy as np
import pytest

from oracle import som_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32
_DATA = {}


def engine(X, Y, D, **kw):
    from xpysom_dask_amd.engine import HipEngine
    return HipEngine(X, Y, D, **kw)


def planted(w, D, inf, n=600):
    """600 blob rows (two 256-row tiles and one of 88); w[2, 3] = w[2, 2]: a tie inside one group (an 8 x 8 patch), w[40, 41] =
    w[2, 2]: the same unit in another unit block; rows on / next to that unit, a zero, a NaN and (inf) a +-inf row."""
    if D not in _DATA:
        _DATA[D] = O.gaussian_blobs(n, D, seed=D + n)
    x, w = _DATA[D].copy(), np.array(w, F32)
    w[2, 3] = w[2, 2]; w[40, 41] = w[2, 2]
    x[0] = w[2, 2]; x[1] = w[2, 2] * F32(1.0000001); x[300] = w[5, 60]; x[2] = 0.0
    x[3] = np.nan
    if inf:
        x[4, 7] = np.inf; x[4, 9] = -np.inf
    return x, w, 2 if inf else 1                         # (rows, codebook, non-finite rows)


def searched(e, f, x, bad):
    # both query paths of e against f's; e's rows counted, its fallback rows within (non-finite rows + 2 % of the rows)
    import torch
    r0, f0, _ = e.exact_stats()
    want = f.bmu(x)
    dev = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    got = e.bmu(x)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(e.bmu_device(dev.data_ptr(), len(x)), want)
    r1, f1, _ = e.exact_stats()
    print("rows", r1 - r0, "fallback", f1 - f0)
    assert r1 - r0 == 2 * len(x)                         # (on the parent the handle is silently 'f32': the counter stays 0)
    assert f1 - f0 <= 2 * (bad + len(x) // 50)           # (two searches of the rows)
    return f1 - f0


@pytest.mark.parametrize("dist", ["euclidean", "cosine"])
@pytest.mark.parametrize("D", [801, 1024, 1100])
@pytest.mark.parametrize("X,Y", [(64, 64), (64, 72), (72, 63)])
def test_ids_are_the_float32_ids(X, Y, D, dist):
    """Seeded codebook, then the smooth map two float32 epochs leave; 600 rows and 1 row.
    The fallback cap and the +-inf row: a row of infinite norm makes the launch's max |x|^2 infinite, and under the euclidean
    distance no bound covers any row of that launch -- measured on the unchanged wide screen at 800 features, these rows and
    seed: 600 of 600 rows fall back (cosine, unit-length operands: 3 of 600 -- the zero, the NaN and the inf row).  So the capped
    searches carry the inf row under cosine only; under euclidean it is searched in a launch of its own, ids only.  Measured
    here at 1024 features, 64 x 64, seeded codebook: euclidean 2 of 600 (zero and NaN row), cosine 3 of 600; 1 row: 0."""
    e, f = engine(X, Y, D, precision="exact", distance=dist), engine(X, Y, D, precision="f32", distance=dist)
    try:
        x, w, bad = planted(O.default_codebook(X, Y, D, 11), D, dist == "cosine")
        for state in range(2):
            e.set_weights(w); f.set_weights(w)
            searched(e, f, x, bad)
            assert searched(e, f, x[10:11], 0) == 0
            xi = x.copy(); xi[4, 7] = np.inf; xi[4, 9] = -np.inf
            assert np.array_equal(e.bmu(xi), f.bmu(xi))
            if state == 0:
                f.set_data(x[5:])
                for sigma in (8.0, 4.0):
                    f.epoch(sigma, 0.5, True)
                x, w, bad = planted(f.get_weights().reshape(X, Y, D), D, dist == "cosine")
    finally:
        e.close(); f.close()


def test_training_and_quantization_error():
    import torch
    X, Y, D, n = 64, 64, 1024, 3000
    x, w = O.gaussian_blobs(n, D, seed=5), O.default_codebook(X, Y, D, 3).astype(F32)
    x[17] = w[9, 9]                                       # a copy of a unit: distance 0 under the sqrt window
    eng = [engine(X, Y, D, precision=p) for p in ("exact", "f32")]
    try:
        for e in eng:
            e.set_weights(w); e.set_data(x)
        for sigma in (6.0, 3.0, 1.5):
            bmus = []
            for e in eng:
                e.epoch_accumulate(sigma, 0.4, True); bmus.append(e.epoch_fetch()[2]); e.epoch_merge()
            assert np.array_equal(bmus[0], bmus[1]) and np.array_equal(eng[0].get_weights(), eng[1].get_weights()), sigma
        for e in eng:
            a, b = e.pinned_empty((1500, D)), e.pinned_empty((1500, D))
            a[:] = x[:1500]; b[:] = x[1500:]
            e.stream_epoch_accumulate([a, b], 1.0, 0.3, True)
            e.epoch_merge()
        assert np.array_equal(eng[0].get_weights(), eng[1].get_weights())
        assert eng[0].exact_stats()[0] == 4 * n
        x[17] = eng[1].get_weights().reshape(X, Y, D)[9, 9]
        dev = torch.from_numpy(x).cuda()
        # (measured at input_len = 784 on the wide path, same rows' generator and seed: exact == f32 to the last bit, 88.18098264567057)
        assert eng[0].quantization_error(x) == eng[1].quantization_error(x)
        assert eng[0].quantization_error_device(dev.data_ptr(), n) == eng[1].quantization_error_device(dev.data_ptr(), n)
        assert eng[0].qe_stats()[0] == 2 * n
    finally:
        for e in eng:
            e.close()


def test_the_class_and_the_switch(monkeypatch):
    from xpysom_dask_amd import XPySom
    data = O.gaussian_blobs(2000, 1024, seed=8)
    soms = [XPySom(64, 64, 1024, random_seed=1, **kw).train(data, 2) for kw in ({}, {"precision": "f32"})]
    assert np.array_equal(soms[0].get_weights(), soms[1].get_weights())
    assert soms[0].winner(data) == soms[1].winner(data)
    assert soms[0]._engine().exact_stats()[0] >= 2 * len(data)
    monkeypatch.setenv("SOM_EXACT_LONG", "0")
    e = engine(64, 64, 1024, precision="exact")
    e.set_weights(soms[1].get_weights()); e.bmu(data[:300])
    assert e.exact_stats()[0] == 0
    e.close()


@pytest.mark.parametrize("X,Y,D,dist,screened", [(64, 64, 800, "euclidean", True), (64, 64, 1024, "euclidean", True),
                                                 (64, 64, 4096, "cosine", True), (64, 64, 4097, "euclidean", False),
                                                 (32, 32, 1024, "euclidean", False), (64, 64, 1024, "manhattan", False)])
def test_boundaries(X, Y, D, dist, screened, monkeypatch):
    """800 features: the wide kernel, whatever SOM_EXACT_LONG says; beyond 4096 features, below 4096 units and on the other
    distances: the float32 kernels.  The device memory of every handle returns with close()."""
    if D == 800:
        monkeypatch.setenv("SOM_EXACT_LONG", "0")
    from tests.test_gpu_exact_scratch import device_bytes
    x, w = O.gaussian_blobs(300, D, seed=D), O.default_codebook(X, Y, D, 4).astype(F32)
    before = device_bytes()
    e, f = engine(X, Y, D, precision="exact", distance=dist), engine(X, Y, D, precision="f32", distance=dist)
    e.set_weights(w); f.set_weights(w)
    assert np.array_equal(e.bmu(x), f.bmu(x))
    assert e.exact_stats()[0] == (len(x) if screened else 0)
    e.close(); f.close()
    assert device_bytes() == before
