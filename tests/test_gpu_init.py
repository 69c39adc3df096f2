"""The codebook initialisers on rows that live in HBM -- XPySom.random_weights_init / pca_weights_init / linear_weights_init -- against
their host paths and the float64 moments.  GPU only (`-m gpu`).  The tolerance of the linear initialisation is derived from the
moments bound (tests/moments_ref.py, linear_tolerance), never from the result."""
import numpy as np
import pytest

from tests import moments_ref as M
from xpysom_dask_amd import XPySom
from xpysom_dask_amd.xpysom import _linear_codebook, _pca_codebook

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
N = 5000


def _dev(a, dtype=F32):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()      # (a copy: the shared rows are read-only)


_ROWS = {}


def spectrum(D):
    """n = 5000 rows, top eigenvalues 16, 9, 4 on a rotated basis, the rest <= 1: computed once per D, never written to."""
    if D not in _ROWS:
        x = M.spectrum_rows(N, D, 20 + D)
        x.setflags(write=False)
        _ROWS[D] = x
    return _ROWS[D]


def device_pivot(som, xd, wd=None):
    """float32(s1 / wsum) of the first pass, as _row_moments forms it (deterministic: the same bits)."""
    eng = som._engine()
    wsum, s1, _ = eng.row_moments_device(xd.data_ptr(), xd.shape[0], wd.data_ptr() if wd is not None else None, None, False)
    return (s1 / wsum).astype(F32)


def unit_errors(got, want):
    return np.linalg.norm(got.astype(F64) - want, axis=-1).max()


@pytest.mark.parametrize("X, Y, D", [(5, 7, 3), (64, 64, 32)])
def test_random_weights_init_on_device_rows_is_the_host_codebook(X, Y, D):
    x = M.spectrum_rows(700, D, 5)
    a, b = XPySom(X, Y, D, random_seed=11), XPySom(X, Y, D, random_seed=11)
    a.random_weights_init(x)
    b.random_weights_init(_dev(x))
    assert a._weights.dtype == b._weights.dtype and np.array_equal(a._weights, b._weights)
    assert a._random_generator.randint(1 << 30) == b._random_generator.randint(1 << 30)     # the generators moved alike


def test_pca_weights_init_on_device_rows():
    D, X, Y = 33, 6, 5
    x = spectrum(D)
    xd = _dev(x)
    som = XPySom(X, Y, D, random_seed=1)
    wsum, mean, Mc = som._row_moments(xd, None, 'pca_weights_init')
    cov = Mc / (wsum - 1.0)
    # the covariance handed to eig: within the moments bound over n - 1 of the float64 np.cov
    bound = M.central_bound(x, None, device_pivot(som, xd)) / (N - 1)
    err = np.abs(cov - np.cov(x.astype(F64).T))
    assert wsum == N and (err <= bound).all(), (err / bound).max()
    som.pca_weights_init(xd)
    want = _pca_codebook(cov, X, Y).astype(som._weights.dtype)
    assert np.array_equal(som._weights, want)


@pytest.mark.parametrize("D", [4, 33, 128])
def test_linear_weights_init(D):
    X, Y = 9, 6
    x = spectrum(D)
    xd = _dev(x)
    want = _linear_codebook(*M.moments64(x), X, Y)
    dev = XPySom(X, Y, D, random_seed=1)
    tol = M.linear_tolerance(x, None, device_pivot(dev, xd))
    dev.linear_weights_init(xd)
    assert dev._weights.shape == (X, Y, D) and dev._weights.dtype == F32
    err = unit_errors(dev._weights, want)
    print("D = %d: largest unit error %.3g, tolerance %.3g" % (D, err, tol))
    assert err <= tol
    # host rows in one chunk: the same kernels on the same rows, the same bits
    host = XPySom(X, Y, D, random_seed=1)
    host.linear_weights_init(x)
    assert np.array_equal(host._weights.view(np.uint32), dev._weights.view(np.uint32))
    # host rows in three chunks: another order of addition, inside the same tolerance
    chunked = XPySom(X, Y, D, random_seed=1, n_parallel=2000)
    chunked.linear_weights_init(x)
    assert unit_errors(chunked._weights, want) <= tol
    # the map lies in the data: along the longer side it spans 2 sqrt(16)
    assert abs(np.linalg.norm(dev._weights[-1, 0].astype(F64) - dev._weights[0, 0]) - 8.0) < 0.5


def test_linear_weights_init_with_device_weights():
    D, X, Y = 33, 7, 7
    x = spectrum(D)
    w = np.random.RandomState(3).uniform(0, 2, N).astype(F32)
    w[::7] = 0
    xd, wd = _dev(x), _dev(w)
    som = XPySom(X, Y, D, random_seed=1)
    tol = M.linear_tolerance(x, w, device_pivot(som, xd, wd))
    som.linear_weights_init(xd, sample_weight=wd)
    assert unit_errors(som._weights, _linear_codebook(*M.moments64(x, w), X, Y)) <= tol
    host = XPySom(X, Y, D, random_seed=1)
    host.linear_weights_init(x, sample_weight=w)
    assert np.array_equal(host._weights.view(np.uint32), som._weights.view(np.uint32))
    with pytest.raises(ValueError, match="sum to 0"):
        som.linear_weights_init(xd, sample_weight=_dev(np.zeros(N, F32)))


def test_nan_rows_are_refused():
    x = spectrum(4).copy()
    x[123, 2] = np.nan
    for rows in (x, _dev(x)):
        with pytest.raises(ValueError, match="the data holds NaN"):
            XPySom(5, 5, 4, random_seed=1).linear_weights_init(rows)
    with pytest.raises(ValueError, match="the data holds NaN"):     # (host rows keep the reference's np.cov, NaN and all)
        XPySom(5, 5, 4, random_seed=1).pca_weights_init(_dev(x))
    x[123, 2] = np.inf
    with pytest.raises(ValueError, match="the data holds NaN"):
        XPySom(5, 5, 4, random_seed=1).linear_weights_init(_dev(x))


def test_train_after_linear_weights_init():
    D = 33
    xd = _dev(spectrum(D))
    som = XPySom(12, 10, D, random_seed=1)
    som.linear_weights_init(xd)
    before = som.quantization_error(xd)
    som.train(xd, 5)
    after = som.quantization_error(xd)
    assert np.isfinite(after) and after < before, (before, after)


# ---- device tensors that are not contiguous float32: _device_rows converts them, and the copy must outlive the kernels ----
def _variants(x):
    """The rows of x as CUDA tensors the initialisers have to convert: float64, and a column slice of a wider block."""
    import torch
    wide = torch.from_numpy(np.concatenate([x, np.full((len(x), 5), 7.0, F32)], axis=1)).cuda()
    return {"float64": _dev(x).double(), "column slice": wide[:, :x.shape[1]]}


def _held_bytes(som, method, n_bytes):
    """Wraps the engine's `method` so that every call asserts torch still holds n_bytes more than when the wrapper was made:
    the converted copy of the rows is alive while the kernel reads it.  Returns the list the calls are counted in."""
    import torch
    eng = som._engine()
    inner, base, calls = getattr(eng, method), torch.cuda.memory_allocated(), []

    def checked(*a, **kw):
        calls.append(torch.cuda.memory_allocated() - base)
        assert calls[-1] >= n_bytes, "%s ran with %d bytes of torch memory held, the rows' copy alone is %d" % (method, calls[-1], n_bytes)
        return inner(*a, **kw)
    setattr(eng, method, checked)
    return calls


@pytest.mark.parametrize("kind", ["float64", "column slice"])
def test_converted_device_tensors_give_the_float32_bits_and_stay_alive(kind):
    D, X, Y = 33, 7, 6
    x = spectrum(D)
    w = np.random.RandomState(4).uniform(0, 2, N).astype(F32)          # HOST weights beside device rows: an allocation between
    ref = XPySom(X, Y, D, random_seed=5)
    ref.linear_weights_init(_dev(x), sample_weight=w)
    som = XPySom(X, Y, D, random_seed=5)
    xv = _variants(x)[kind]
    calls = _held_bytes(som, "row_moments_device", N * D * 4)
    som.linear_weights_init(xv, sample_weight=w)
    assert len(calls) == 2                                              # both passes saw the copy
    assert np.array_equal(som._weights.view(np.uint32), ref._weights.view(np.uint32))
    som.pca_weights_init(xv)
    ref.pca_weights_init(_dev(x))
    assert len(calls) == 4 and np.array_equal(som._weights, ref._weights)
    calls = _held_bytes(som, "gather_rows_device", N * D * 4)
    som.random_weights_init(xv)
    ref.random_weights_init(x)
    assert len(calls) == 1 and np.array_equal(som._weights, ref._weights)


def test_pca_weights_init_refuses_one_device_row():
    with pytest.raises(ValueError, match="at least 2 rows"):
        XPySom(4, 4, 3, random_seed=1).pca_weights_init(_dev(np.ones((1, 3), F32)))


def test_random_weights_init_with_missing_values_refuses_before_it_draws():
    """missing='nan': any NaN in device rows is refused as on the host path -- before an index is drawn, sampled or not."""
    x = M.spectrum_rows(50, 3, 2)
    x[49, 1] = np.nan
    for rows in (x, _dev(x)):
        som = XPySom(1, 1, 3, random_seed=9, missing='nan')             # one unit: it would sample one row of fifty
        with pytest.raises(ValueError, match="the data holds NaN"):
            som.random_weights_init(rows)
        untouched = XPySom(1, 1, 3, random_seed=9, missing='nan')      # (the constructor draws the default codebook)
        assert som._random_generator.randint(1 << 30) == untouched._random_generator.randint(1 << 30)
