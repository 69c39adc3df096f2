"""activation_distance='manhattan' on the register-tiled kernel (csrc/bmu_manhattan.hpp) against NumPy itself in float32:
np.abs(x[:, None, :] - w[None]).sum(-1).argmin(1).  The kernel reproduces NumPy's pairwise summation order bit for bit, so
the ids are equal with no tolerance.  The inputs are planted: for i < min(N, K // 2) row i is w[2i] plus noise of width 0.05
and unit 2i + 1 is x_i - (x_i - w[2i])[perm] -- the same L1 distance in real arithmetic, so the float32 summation order (and,
on an exact tie, the first-minimum rule) decides between units 2i and 2i + 1.  The last three rows hold a NaN, +inf, -inf."""
import numpy as np
import pytest

from xpysom_dask_amd.engine import HipEngine, SomHipError
from xpysom_dask_amd.xpysom import XPySom

pytestmark = pytest.mark.gpu
F32 = np.float32

# (X, Y, input_len, rows): n < 8, a partial tile on every axis | four chain steps and a tail of 1, two unit blocks, three row
# tiles | a tail of 7 | a full leaf | the first split, 64 + 65 (the streamed instance) | an uneven two-level tree | the first
# length the one-thread-a-row kernel refuses, few rows: the part merge runs | the longest rows
CASES = [(5, 7, 3, 130), (12, 11, 33, 300), (13, 11, 127, 131), (13, 11, 128, 131), (13, 11, 129, 131), (20, 13, 300, 257),
         (13, 11, 2401, 70), (6, 5, 4096, 40)]
IDS = lambda c: "%dx%dx%d_n%d" % c
_REF = {}


def numpy_bmu(x, w):
    with np.errstate(invalid="ignore"):
        return np.concatenate([np.abs(x[s:s + 8, None, :] - w[None]).sum(-1).argmin(1) for s in range(0, len(x), 8)]).astype(np.int32)


def case(c):
    if c not in _REF:
        X, Y, D, N = c
        rs = np.random.RandomState(0)
        x, w = rs.rand(N, D).astype(F32), rs.rand(X * Y, D).astype(F32)
        for i in range(min(N, X * Y // 2)):
            x[i] = w[2 * i] + ((rs.rand(D) - 0.5) * 0.05).astype(F32)
            w[2 * i + 1] = x[i] - (x[i] - w[2 * i])[rs.permutation(D)]
        x[N - 3, D // 2], x[N - 2, 0], x[N - 1, D - 1] = np.nan, np.inf, -np.inf
        ref = numpy_bmu(x, w)
        ref.setflags(write=False)
        _REF[c] = (x, w, ref)
    return _REF[c]


def ids_of(c, rows, monkeypatch, parts=None, tiled=None):
    import torch
    X, Y, D, N = c
    x, w, _ = case(c)
    if parts is not None:
        monkeypatch.setenv("SOM_MANHATTAN_PARTS", str(parts))
    if tiled is not None:
        monkeypatch.setenv("SOM_MANHATTAN_TILED", str(tiled))
    e = HipEngine(X, Y, D, distance="manhattan", precision="f32")
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
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_ids_equal_numpy(c, rows, parts, monkeypatch):
    x, w, ref = case(c)
    got = ids_of(c, rows, monkeypatch, parts=parts)
    bad = np.flatnonzero(got != ref)
    print("%s %s parts=%s: %d of %d rows differ" % (c, rows, parts, len(bad), len(ref)))
    assert len(bad) == 0, (bad[:10], got[bad[:10]], ref[bad[:10]])
    assert (got[-3:] == 0).all()                                  # the NaN, +inf and -inf rows


@pytest.mark.parametrize("c", [c for c in CASES if c[2] <= 2400], ids=IDS)
def test_one_thread_a_row_kernel_agrees(c, monkeypatch):
    """SOM_MANHATTAN_TILED=0 sends the distance to bmu_pairwise_kernel: the same ids from both kernels of one build."""
    assert np.array_equal(ids_of(c, "host", monkeypatch, tiled=0), ids_of(c, "host", monkeypatch, tiled=1))


def test_switch_reaches_the_one_thread_a_row_kernel(monkeypatch):
    """The switch is obeyed: under SOM_MANHATTAN_TILED=0 the first length beyond bmu_pairwise_kernel's LDS tile is refused by
    its launcher, by name, as before the tiled kernel."""
    with pytest.raises(SomHipError, match="input_len too large for the LDS unit tile"):
        ids_of((13, 11, 2401, 70), "host", monkeypatch, tiled=0)


def test_training_follows_numpy():
    """Two epochs of the class against an engine that is fed NumPy's ids (the teacher-forced path): the same BMUs in each
    epoch."""
    X, Y, D, N = 12, 11, 33, 300
    x = np.random.RandomState(5).rand(N, D).astype(F32)
    som = XPySom(X, Y, D, sigma=3.0, activation_distance='manhattan', random_seed=3)
    t = HipEngine(X, Y, D, precision="f32")
    try:
        t.set_weights(som.get_weights().reshape(-1, D))
        t.set_data(x)
        for it in range(2):
            ids = numpy_bmu(x, t.get_weights().reshape(-1, D))
            sig = som._decay_function(som._sigma, som._sigmaN, it, 2)
            eta = som._decay_function(som._learning_rate, som._learning_rateN, it, 2)
            t.epoch_accumulate_forced(ids, sig, eta, isinstance(sig, np.generic))
            t.epoch_merge()
            som.train(x, 2, iter_beg=it, iter_end=it + 1)
            assert np.array_equal(som._engine().epoch_fetch()[2], ids), "epoch %d" % it
        assert len(np.unique(ids)) > 20
    finally:
        t.close()
