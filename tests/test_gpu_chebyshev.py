"""activation_distance='chebyshev' (csrc/bmu_chebyshev.hpp) against the NumPy model of tests/chebyshev_ref.py.  fl32(x - w) is
correctly rounded and max is exact, so the kernel's ids equal the model's with no tolerance, whatever the tiling."""
import numpy as np
import pytest

from tests import chebyshev_ref as R
from xpysom_dask_amd.engine import HipEngine
from xpysom_dask_amd.xpysom import XPySom

pytestmark = pytest.mark.gpu

# (X, Y, input_len, rows): one partial tile on every axis | two chunks, two unit blocks, three row tiles | past the resident
# rows, streamed | few rows: the parts merge runs, many chunks | the last input_len with resident rows and the first without
CASES = [(5, 7, 3, 130), (12, 11, 33, 300), (20, 13, 129, 257), (33, 31, 300, 70), (13, 11, 64, 131), (13, 11, 65, 131)]
_REF = {}


def case(c):
    if c not in _REF:
        x, w = R.planted_case(*c)
        _REF[c] = (x, w, R.bmu(x, w))
        _REF[c][2].setflags(write=False)
    return _REF[c]


def ids_of(c, rows, parts, monkeypatch):
    import torch
    X, Y, D, N = c
    x, w, _ = case(c)
    if parts is not None:
        monkeypatch.setenv("SOM_CHEBYSHEV_PARTS", str(parts))
    e = HipEngine(X, Y, D, distance="chebyshev", precision="f32")
    try:
        e.set_weights(w)
        if rows == "host":
            return e.bmu(x)
        t = torch.from_numpy(x).cuda()
        return e.bmu_device(t.data_ptr(), N)
    finally:
        e.close()


@pytest.mark.parametrize("parts", [None, 1, 1 << 20], ids=["parts_auto", "parts_1", "parts_max"])
@pytest.mark.parametrize("rows", ["host", "device"])
@pytest.mark.parametrize("c", CASES, ids=lambda c: "%dx%dx%d_n%d" % c)
def test_ids_equal_the_model(c, rows, parts, monkeypatch):
    x, w, ref = case(c)
    got = ids_of(c, rows, parts, monkeypatch)
    bad = np.flatnonzero(got != ref)
    print("%s %s parts=%s: %d of %d rows differ" % (c, rows, parts, len(bad), len(ref)))
    assert len(bad) == 0, (bad[:10], got[bad[:10]], ref[bad[:10]])
    assert got[0] == 2 and (got[[2, 3, c[3] - 1]] == 0).all()   # the lowest of three equal units; NaN, +inf, -inf rows


@pytest.mark.parametrize("c", CASES, ids=lambda c: "%dx%dx%d_n%d" % c)
def test_chosen_unit_against_float64(c, monkeypatch):
    """Two float32 roundings of relative size 2^-24 each (the winner's distance up, the true minimum's down): the float64
    distance of the chosen unit is within a factor 1 + 2^-22 of the float64 minimum."""
    x, w, _ = case(c)
    got = ids_of(c, "host", None, monkeypatch)
    fin = np.isfinite(x).all(axis=1)
    d64 = R.distances(x[fin], w, R.F64)
    chosen, least = d64[np.arange(fin.sum()), got[fin]], d64.min(axis=1)
    print("%s: worst chosen / least - 1 = %.3g" % (c, (chosen / np.where(least > 0, least, 1) - 1).max()))
    assert (chosen <= least * (1 + 2.0 ** -22)).all()


def test_training_follows_the_model():
    """Two epochs of the class against an engine that is fed the model's ids (the teacher-forced path): the same BMUs in
    each epoch."""
    X, Y, D, N = 12, 11, 33, 300
    x = np.random.RandomState(5).rand(N, D).astype(R.F32)
    som = XPySom(X, Y, D, sigma=3.0, activation_distance='chebyshev', random_seed=3)
    t = HipEngine(X, Y, D, precision="f32")
    try:
        t.set_weights(som.get_weights().reshape(-1, D))
        t.set_data(x)
        for it in range(2):
            ids = R.bmu(x, t.get_weights().reshape(-1, D))
            sig = som._decay_function(som._sigma, som._sigmaN, it, 2)
            eta = som._decay_function(som._learning_rate, som._learning_rateN, it, 2)
            t.epoch_accumulate_forced(ids, sig, eta, isinstance(sig, np.generic))
            t.epoch_merge()
            som.train(x, 2, iter_beg=it, iter_end=it + 1)
            assert np.array_equal(som._engine().epoch_fetch()[2], ids), "epoch %d" % it
        assert len(np.unique(ids)) > 20
    finally:
        t.close()
