"""The toroidal topology's host side: construction and refusals, the wrapped U-matrix, the adjacency rule of
topographic_error as a pure function, and the sanity of the float64 reference the GPU tests use (tests/torus_ref.py).
No device needed: nothing here creates an engine."""
import pickle
import warnings

import numpy as np
import pytest

from tests import torus_ref as T
from xpysom_dask_amd import XPySom
from xpysom_dask_amd.xpysom import units_adjacent


def test_constructs_and_keeps_the_topology_through_pickle():
    som = XPySom(5, 4, 3, topology='toroidal', random_seed=1)
    assert som.topology == 'toroidal'
    back = pickle.loads(pickle.dumps(som))
    assert back.topology == 'toroidal' and np.array_equal(back._weights, som._weights)
    for neigh in ('gaussian', 'mexican_hat', 'bubble', 'triangle'):
        XPySom(5, 4, 3, topology='toroidal', neighborhood_function=neigh)
    XPySom(5, 4, 3, topology='toroidal', compact_support=True)
    XPySom(5, 4, 3, topology='toroidal', neighborhood_function='triangle', compact_support=True)
    from xpysom_dask_amd import _lib
    assert _lib.SOM_TOPO['toroidal'] == 2 and _lib.SOM_TOPO['rectangular'] == 0 and _lib.SOM_TOPO['hexagonal'] == 1


def test_mexican_hat_with_compact_support_is_refused():
    with pytest.raises(ValueError, match='toroidal'):
        XPySom(5, 5, 3, topology='toroidal', neighborhood_function='mexican_hat', compact_support=True)


def test_unknown_topology_keeps_its_message():
    with pytest.raises(ValueError, match='triangular not supported only hexagonal and rectangular available'):
        XPySom(5, 4, 3, topology='triangular')


def test_sigma_warning_stays():
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        XPySom(5, 4, 3, sigma=4, topology='toroidal')
    assert any('sigma is too high' in str(x.message) for x in w)


def test_coordinates_are_the_grid():
    a = XPySom(5, 4, 3, topology='toroidal')
    b = XPySom(5, 4, 3, topology='rectangular')
    for u, v in zip(a.get_euclidean_coordinates(), b.get_euclidean_coordinates()):
        assert np.array_equal(u, v)
    assert a.convert_map_to_euclidean((4, 3)) == b.convert_map_to_euclidean((4, 3))


@pytest.mark.parametrize("X,Y,D", [(5, 4, 3), (3, 3, 2)])
def test_distance_map_wraps(X, Y, D):
    som = XPySom(X, Y, D, topology='toroidal', random_seed=X)
    w = np.random.RandomState(X * 7 + Y).standard_normal((X, Y, D))
    som._weights = w
    want = np.zeros((X, Y))
    for i in range(X):
        for j in range(Y):
            for di in (-1, 0, 1):
                for dj in (-1, 0, 1):
                    if (di, dj) != (0, 0):
                        want[i, j] += np.linalg.norm(w[i, j] - w[(i + di) % X, (j + dj) % Y])
    want /= want.max()
    got = som.distance_map()
    assert got.shape == (X, Y) and got.max() == 1.0
    assert np.allclose(got, want, rtol=1e-13, atol=0)
    # the rectangular map's border units have fewer neighbours: the two differ
    rect = XPySom(X, Y, D, random_seed=X)
    rect._weights = w
    assert not np.allclose(rect.distance_map(), got)


def wrapped_abs(a, b, L):
    return min((a - b) % L, (b - a) % L)


@pytest.mark.parametrize("X,Y", [(6, 5), (2, 7), (1, 4)])
def test_adjacency_on_the_torus_against_brute_force(X, Y):
    K = X * Y
    b1, b2 = (a.ravel() for a in np.meshgrid(np.arange(K), np.arange(K), indexing='ij'))
    got = units_adjacent(b1, b2, X, Y, 'toroidal')
    want = np.array([wrapped_abs(p // Y, q // Y, X) <= 1 and wrapped_abs(p % Y, q % Y, Y) <= 1 for p, q in zip(b1, b2)])
    assert got.dtype == bool and np.array_equal(got, want)
    if X == 6:
        assert units_adjacent(np.array([0 * Y + 2]), np.array([5 * Y + 2]), X, Y, 'toroidal')[0]
        assert not units_adjacent(np.array([0 * Y + 2]), np.array([5 * Y + 2]), X, Y, 'rectangular')[0]


@pytest.mark.parametrize("X,Y", [(6, 5), (5, 5), (2, 7), (1, 4)])
def test_adjacency_unchanged_on_the_other_topologies(X, Y):
    """Against the rule as topographic_error stated it inline before it became a function."""
    K = X * Y
    b1, b2 = (a.ravel() for a in np.meshgrid(np.arange(K), np.arange(K), indexing='ij'))
    i1, j1, i2, j2 = b1 // Y, b1 % Y, b2 // Y, b2 % Y
    rect_bad = (np.abs(i1 - i2) > 1) | (np.abs(j1 - j2) > 1)
    assert np.array_equal(units_adjacent(b1, b2, X, Y, 'rectangular'), ~rect_bad)
    if X == Y:
        x1, y1 = j1 - 0.5 * ((Y - 1 - i1) % 2 == 0), i1
        x2, y2 = j2 - 0.5 * ((Y - 1 - i2) % 2 == 0), i2
    else:
        x1, y1 = i1 - 0.5 * ((Y - 1 - j1) % 2 == 0), j1
        x2, y2 = i2 - 0.5 * ((Y - 1 - j2) % 2 == 0), j2
    hex_bad = np.hypot(x1 - x2, (y1 - y2).astype(float)) > 1.5
    assert np.array_equal(units_adjacent(b1, b2, X, Y, 'hexagonal'), ~hex_bad)


@pytest.mark.parametrize("neigh,compact", [("gaussian", False), ("gaussian", True), ("mexican_hat", False), ("bubble", False),
                                           ("triangle", False), ("triangle", True)])
@pytest.mark.parametrize("wide", [False, True])
def test_reference_rows_are_cyclic_shifts_of_one_another(neigh, compact, wide):
    """h(b -> k) depends on the wrapped offset alone: the row of BMU (ci, cj), rolled back by (ci, cj), is the row of BMU
    (0, 0) -- on odd sides, where no offset sits on the tie |delta| = L / 2, bit for bit."""
    X, Y = 7, 5
    h_of, habs_of = T.make_h(X, Y, neigh, compact, 0.5, 1.7, 0.3, wide)
    units = np.arange(X * Y)
    for f in (h_of, habs_of):
        H = f(units).reshape(X * Y, X, Y)
        for u in units:
            assert np.array_equal(np.roll(H[u], (-(u // Y), -(u % Y)), axis=(0, 1)), H[0])
    H = h_of(units).reshape(X * Y, X, Y)
    assert H[0, 0, 0] != 0 and H[0, 1, 0] == H[0, X - 1, 0] and H[0, 0, 1] == H[0, 0, Y - 1]      # even in the offset
    if neigh == "bubble":
        assert H[0].sum() == pytest.approx(0.3 * 9)          # |delta| < 1.7: three units per axis, across the seam


def test_reference_offsets():
    assert np.array_equal(T.wrapped_offset(np.arange(6), 0, 6)[[0, 1, 2, 4, 5]], [0, 1, 2, -2, -1])
    assert abs(T.wrapped_offset(3, 0, 6)) == 3
    assert np.array_equal(T.wrapped_offset(np.arange(5), 4, 5), [1, 2, -2, -1, 0])
    with pytest.raises(ValueError):
        T.make_h(4, 4, "mexican_hat", True, 0.5, 1.0, 0.5, False)
