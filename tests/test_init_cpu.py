"""The initialisers' host side without a GPU: the pure codebook functions (_linear_codebook, _pca_codebook), the index stream of
random_weights_init on device rows, and every refusal that needs no engine."""
import numpy as np
import pytest

from tests.moments_ref import moments64, spectrum_rows
from xpysom_dask_amd import XPySom
from xpysom_dask_amd.xpysom import _linear_codebook, _pca_codebook

F32, F64 = np.float32, np.float64


def brute_force(x, X, Y):
    """lininit by the SVD of the centred rows, written without eigh: (mean, first axis, second axis) with the sign rule applied."""
    x = np.asarray(x, F64)
    mean = x.mean(axis=0)
    _, s, vt = np.linalg.svd(x - mean, full_matrices=False)
    axes = []
    for k in (0, 1):
        v = vt[k]
        if v[np.argmax(np.abs(v))] < 0:
            v = -v
        axes.append(s[k] / np.sqrt(len(x)) * v)
    return mean, axes[0], axes[1]


@pytest.mark.parametrize("X, Y", [(7, 5), (5, 7), (6, 6), (1, 9), (9, 1), (1, 1)])
def test_linear_codebook_against_svd(X, Y):
    x = spectrum_rows(4000, 6, 3)
    mean, a1, a2 = brute_force(x, X, Y)
    cb = _linear_codebook(*moments64(x), X, Y)
    assert cb.shape == (X, Y, 6) and cb.dtype == F64
    cx = np.linspace(-1, 1, X) if X > 1 else np.zeros(1)
    cy = np.linspace(-1, 1, Y) if Y > 1 else np.zeros(1)
    ax, ay = (a1, a2) if X >= Y else (a2, a1)              # the first axis along the longer side; a tie: along x
    want = mean + cx[:, None, None] * ax + cy[None, :, None] * ay
    assert np.abs(cb - want).max() < 1e-9
    # the plane: the centre of the map is the mean, the corners span +- both axes
    assert np.abs(cb.reshape(-1, 6).mean(axis=0) - mean).max() < 1e-9
    if X > 1 and Y > 1:
        assert np.abs((cb[-1, 0] - cb[0, 0]) - 2 * ax).max() < 1e-9 and np.abs((cb[0, -1] - cb[0, 0]) - 2 * ay).max() < 1e-9
        long_side = cb[-1, 0] - cb[0, 0] if X >= Y else cb[0, -1] - cb[0, 0]
        assert abs(np.linalg.norm(long_side) - 2 * 4.0) < 0.5        # sqrt(16) per unit of coordinate


def test_linear_codebook_sign_rule_and_clipping():
    cov = np.diag([4.0, 1.0, -1e-18])                      # a slightly negative eigenvalue is clipped at 0
    cb = _linear_codebook(10.0, np.zeros(3), cov, 3, 1)
    assert np.array_equal(cb[:, 0, 0], [-2.0, 0.0, 2.0]) and not cb[:, :, 1:].any()
    for v in (np.array([1.0, -3.0, 2.0]), np.array([-1.0, 3.0, -2.0])):    # either way round, the largest component ends up positive
        v = v / np.linalg.norm(v)
        cb = _linear_codebook(1.0, np.zeros(3), 9.0 * np.outer(v, v), 2, 1)
        assert np.abs(cb[1, 0] - 3.0 * np.sign(v[1]) * v).max() < 1e-12 and cb[1, 0, 1] > 0


def test_integer_weights_are_repeated_rows():
    x = spectrum_rows(500, 5, 8)
    w = np.random.RandomState(1).randint(0, 4, 500)
    a = _linear_codebook(*moments64(x, w), 6, 4)
    b = _linear_codebook(*moments64(np.repeat(x, w, axis=0)), 6, 4)
    assert np.abs(a - b).max() < 1e-9


def test_linear_codebook_refusals():
    with pytest.raises(ValueError, match="sum to 0"):
        _linear_codebook(0.0, np.zeros(3), np.eye(3), 2, 2)
    with pytest.raises(ValueError, match="the data holds NaN"):
        _linear_codebook(5.0, np.array([0.0, np.nan, 0.0]), np.eye(3), 2, 2)
    with pytest.raises(ValueError, match="the data holds NaN"):
        _linear_codebook(5.0, np.zeros(3), np.full((3, 3), np.inf), 2, 2)


@pytest.mark.parametrize("X, Y, D", [(5, 7, 3), (1, 4, 2), (8, 8, 9)])
def test_pca_codebook_is_the_loop_it_replaces(X, Y, D):
    x = spectrum_rows(300, D, 4, lam=(5.0, 2.0))
    cov = np.cov(np.transpose(x))
    pc_length, pc = np.linalg.eig(cov)
    order = np.argsort(-pc_length)
    want = np.zeros((X, Y, D))
    for i, c1 in enumerate(np.linspace(-1, 1, X)):
        for j, c2 in enumerate(np.linspace(-1, 1, Y)):
            want[i, j] = c1 * pc[order[0]] + c2 * pc[order[1]]
    got = _pca_codebook(cov, X, Y)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_pca_weights_init_on_host_rows_is_unchanged():
    x = spectrum_rows(300, 4, 6)
    som = XPySom(5, 6, 4, random_seed=1)
    som.pca_weights_init(x)
    want = _pca_codebook(np.cov(np.transpose(x)), 5, 6).astype(som._weights.dtype)
    assert np.array_equal(som._weights, want)


@pytest.mark.parametrize("n", [7, 150, 2 ** 20, 2 ** 32 + 5])
def test_randint_draws_the_stream_of_scalar_calls(n):
    """random_weights_init on device rows draws x * y indices in one call: the same stream as the host path's scalar calls."""
    a = np.random.RandomState(42)
    b = np.random.RandomState(42)
    one = a.randint(n, size=300)
    many = np.array([b.randint(n) for _ in range(300)])
    assert np.array_equal(one, many)
    assert a.randint(n) == b.randint(n)                    # ... and the generators are left in the same state


def test_refusals_without_an_engine():
    som = XPySom(4, 4, 1, random_seed=1)
    with pytest.raises(ValueError, match="at least 2 features"):
        som.linear_weights_init(np.zeros((10, 1), F32))
    with pytest.raises(ValueError, match="at least 2 features"):
        som.pca_weights_init(np.zeros((10, 1), F32))
    som = XPySom(4, 4, 3, random_seed=1)
    with pytest.raises(ValueError, match="Received 5 features, expected 3"):
        som.linear_weights_init(np.zeros((10, 5), F32))
    with pytest.raises(ValueError, match="2-dimensional"):
        som.linear_weights_init(np.zeros(10, F32))
    x = np.zeros((10, 3), F32)
    with pytest.raises(ValueError, match="sample_weight has 9 values for 10 rows"):
        som.linear_weights_init(x, sample_weight=np.ones(9))
    with pytest.raises(ValueError, match="finite and >= 0"):
        som.linear_weights_init(x, sample_weight=np.r_[np.ones(9), -1.0])
    with pytest.raises(ValueError, match="finite and >= 0"):
        som.linear_weights_init(x, sample_weight=np.r_[np.ones(9), np.nan])
    with pytest.raises(TypeError):
        som.linear_weights_init(x, np.ones(10))             # sample_weight is keyword-only
    assert som._engine_obj is None                          # none of these needed an engine
