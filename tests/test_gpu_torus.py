"""The toroidal topology on the device: the neighbourhood tables of wrapped offsets (csrc/update.hpp, neigh_offset), the band
ranges that follow the neighbourhood across the seam (band_wrap_mid, leftmul_wrap_f32_kernel) and the Python surface.

There is no reference implementation of a toroidal map to compare with: tests/torus_ref.py evaluates the semantics the
project states (include/somhip.h) per pair of units in float64, and tests/update_ref.py's checks apply with
their own tolerance (TOL = 1e-5 of the magnitude sums).  BMUs are teacher-forced (som_epoch_accumulate_forced) with
update_ref.make_bmu's patterns: `edges` -- corners, both sides of both seams, the 128-row block boundaries -- and `spread`.

  1  accumulators and merged codebook against the float64 reference: maps without bands (8 x 8) and with them, sides with a
     partial last 32-row tile / 128-row block / a one-row last block, sigma narrower than a lattice step (0.3), straddling a
     chunk (1.2, 4.0), wider than a side (12, 80); 5 features (whole rows, the VALU kernel), 128 (stage 2 batched per map
     column) and 131 (a narrow last tile); every neighbourhood; sigma as a Python float and as numpy.float64
  2  the same cases under SOM_NO_BANDS=1: bit for bit
  3  the recorded ranges are the first and last nonzero of each piece of the tables read back with them, and seam tiles walk
     less than their table's width (else 2 proves nothing)
  4  a torus whose BMUs keep away from the seam is the rectangle, bit for bit
  5  the faithful K x N x D form reads the same tables
  6  a schedule whose bands shrink and grow, with and without the captured epoch
  7  the BMU search does not see the lattice: precision 'exact' = 'f32' bit for bit
  8  topographic_error across the seam"""
import numpy as np
import pytest

from oracle import som_oracle as O
from tests import torus_ref as T
from tests import update_ref as U

pytestmark = pytest.mark.gpu
F32 = np.float32
N, ETA, STD = 2000, 0.4, 0.5


def engine(X, Y, D, **kw):
    from xpysom_dask_amd.engine import HipEngine
    return HipEngine(X, Y, D, **kw)


def rel_err(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def mid_of(side):
    return ((side // 2 + 4) // 8) * 8


#        X    Y    D    neighbourhood  compact sigma  wide   BMUs
CASES = [
    (8,   8,   5,   "gaussian",    False, 1.2,  False, "spread"),
    (8,   8,   128, "bubble",      False, 4.0,  True,  "edges"),
    (33,  40,  5,   "gaussian",    False, 0.3,  False, "edges"),
    (33,  40,  131, "mexican_hat", False, 1.2,  True,  "spread"),
    (33,  40,  5,   "triangle",    True,  4.0,  False, "edges"),
    (33,  40,  128, "gaussian",    False, 80.0, True,  "spread"),
    (64,  33,  128, "gaussian",    True,  1.2,  False, "spread"),
    (64,  33,  5,   "bubble",      False, 12.0, False, "edges"),
    (64,  33,  131, "triangle",    False, 80.0, True,  "spread"),
    (64,  33,  5,   "mexican_hat", False, 0.3,  False, "edges"),
    (97,  65,  5,   "gaussian",    False, 1.2,  False, "edges"),
    (97,  65,  128, "gaussian",    False, 4.0,  True,  "spread"),
    (97,  65,  131, "gaussian",    True,  12.0, False, "edges"),
    (97,  65,  5,   "mexican_hat", False, 4.0,  False, "spread"),
    (97,  65,  5,   "bubble",      False, 0.3,  True,  "edges"),
    (97,  65,  128, "triangle",    True,  12.0, False, "edges"),
    (97,  65,  5,   "gaussian",    False, 80.0, True,  "edges"),
    (160, 96,  5,   "gaussian",    False, 1.2,  True,  "edges"),
    (160, 96,  128, "gaussian",    False, 1.2,  False, "spread"),
    (160, 96,  131, "mexican_hat", False, 12.0, False, "edges"),
    (160, 96,  5,   "bubble",      False, 4.0,  False, "edges"),
    (160, 96,  128, "triangle",    False, 4.0,  True,  "edges"),
    (160, 96,  5,   "gaussian",    True,  0.3,  False, "edges"),
    (160, 96,  5,   "gaussian",    False, 80.0, False, "edges"),
    (129, 200, 5,   "gaussian",    False, 4.0,  False, "edges"),
    (129, 200, 128, "gaussian",    True,  1.2,  True,  "edges"),
    (129, 200, 131, "bubble",      False, 12.0, False, "edges"),
    (129, 200, 5,   "mexican_hat", False, 1.2,  True,  "edges"),
    (129, 200, 5,   "triangle",    True,  80.0, False, "edges"),
    (129, 200, 128, "gaussian",    False, 12.0, False, "edges"),
]
LM128 = (160, 96, 5, "mexican_hat", False, 4.0, False, "edges")       # run under SOM_LM_ROWS=128


def case_id(c):
    return "%dx%dx%d-%s%s-s%g%s-%s" % (c[0], c[1], c[2], c[3], "-compact" if c[4] else "", c[5], "-wide" if c[6] else "", c[7])


_inputs, _runs, _refs = {}, {}, {}


def inputs(case):
    """(data, forced BMUs, codebook) of a case: made once, shared, never written."""
    if case not in _inputs:
        X, Y, D = case[:3]
        seed = X * 1000 + Y + D
        rs = np.random.RandomState(seed)
        bmu = U.make_bmu(case[7], X, Y, N, rs)
        data = U.make_data(N, D, 1.0, seed)
        w0 = O.default_codebook(X, Y, D, seed).astype(F32).reshape(X * Y, D)
        for a in (bmu, data, w0):
            a.setflags(write=False)
        _inputs[case] = (data, bmu, w0)
    return _inputs[case]


def sigma_of(case):
    return np.float64(case[5]) if case[6] else float(case[5])


def run(monkeypatch, case, no_bands=False, lm_rows=None, topology="toroidal", bmu=None):
    """(num, den, merged codebook) of one forced accumulate + merge on a fresh handle."""
    key = (case, no_bands, lm_rows, topology, None if bmu is None else bmu.tobytes())
    if key not in _runs:
        X, Y, D, neigh, compact = case[:5]
        for name, v in (("SOM_NO_BANDS", "1" if no_bands else None), ("SOM_LM_ROWS", lm_rows)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, v)
        data, forced, w0 = inputs(case)
        e = engine(X, Y, D, neighborhood=neigh, topology=topology, compact_support=compact, std_coeff=STD, precision="f32")
        try:
            e.set_weights(w0)
            e.set_data(data)
            e.epoch_accumulate_forced(forced if bmu is None else bmu, sigma_of(case), ETA, case[6])
            num, den, _ = e.epoch_fetch(want_bmu=False)
            num, den = num.copy(), den.copy()
            e.epoch_merge()
            w1 = e.get_weights()
        finally:
            e.close()
        _runs[key] = (num, den, w1)
    return _runs[key]


def reference(case):
    if case not in _refs:
        X, Y, D, neigh, compact = case[:5]
        data, bmu, _ = inputs(case)
        _refs[case] = T.reference_update(data, bmu, X, Y, ETA, sigma_of(case), wide=case[6], neighbourhood=neigh,
                                         compact=compact, std_coeff=STD)
    return _refs[case]


def check_against_reference(case, got):
    num, den, w1 = got
    ref = reference(case)
    a = U.check_accumulators(num, den, ref, case_id(case))
    m = U.check_merge(inputs(case)[2], w1, num, den, ref, case[3] == "mexican_hat", case_id(case))
    print("%s: accumulators err/bound %.3g, merge err/bound %.3g" % (case_id(case), a, m))


# ---------------------------------------------------------------------------------------------------------------- 1, 2
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_accumulators_and_merge_against_the_float64_reference(monkeypatch, case):
    check_against_reference(case, run(monkeypatch, case))


def test_the_128_row_workgroup_against_the_reference_and_the_full_walk(monkeypatch):
    got = run(monkeypatch, LM128, lm_rows="128")
    check_against_reference(LM128, got)
    full = run(monkeypatch, LM128, no_bands=True, lm_rows="128")
    for a, b in zip(got, full):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bands_change_nothing(monkeypatch, case):
    got, full = run(monkeypatch, case), run(monkeypatch, case, no_bands=True)
    for what, a, b in zip(("numerator", "denominator", "merged codebook"), got, full):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


# ------------------------------------------------------------------------------------------------------------------- 3
def model_entries(p1, p2, X, Y, nt):
    """[entry][piece] = {side - first nonzero column, last nonzero column + 1} over the piece's columns, from the tables
    themselves, in the buffer's layout (csrc/update.hpp); a piece of a tile without a nonzero: {0, 0}."""
    ty, tx = -(-Y // 32), -(-X // 32)
    out = np.zeros((nt * (ty + tx), 2, 2), dtype=np.int32)

    def entry(block, side):
        mid = mid_of(side)
        r = []
        for a, b in ((0, mid), (mid, side)):
            cols = a + np.flatnonzero((block[:, a:b] != 0).any(axis=0))
            r.append((side - cols[0], cols[-1] + 1) if cols.size else (0, 0))
        return r
    for t in range(nt):
        for tile in range(ty):
            out[t * ty + tile] = entry(p1[t, tile * 32:(tile + 1) * 32, :], Y)
        for tile in range(tx):
            out[nt * ty + tile * nt + t] = entry(p2[tile * 32:(tile + 1) * 32, t * X:(t + 1) * X], X)
    return out


def walked(ent, side):
    """columns a tile walks in one segment: its two ranges, each rounded outwards to the skipping group of 8"""
    n = 0
    for x, y in ent:
        if y > 0:
            n += -(-min(int(y), side) // 8) * 8 - ((side - int(x)) // 8) * 8
    return n


@pytest.mark.parametrize("X,Y,neigh,sigma", [(160, 96, "gaussian", 1.2), (129, 200, "gaussian", 4.0), (129, 200, "mexican_hat", 4.0),
                                             (97, 65, "bubble", 0.3), (64, 33, "triangle", 12.0), (160, 96, "gaussian", 80.0)])
def test_recorded_ranges_are_the_nonzeros_of_each_piece(monkeypatch, X, Y, neigh, sigma):
    """Read back after two epochs of different sigma, so both buffers have been filled and zeroed."""
    D = 5
    data = O.gaussian_blobs(500, D, seed=X)
    w = O.default_codebook(X, Y, D, 8).astype(F32)
    for mode in (None, "1"):
        if mode is None:
            monkeypatch.delenv("SOM_NO_BANDS", raising=False)
        else:
            monkeypatch.setenv("SOM_NO_BANDS", mode)
        e = engine(X, Y, D, neighborhood=neigh, topology="toroidal", precision="f32")
        try:
            e.set_weights(w)
            e.set_data(data)
            for sig in (7.0, sigma):
                e.epoch_accumulate(sig, ETA, True)
                on, ent, p1, p2 = e.band_tables_wrap()
                nt = p1.shape[0]
                if mode == "1":
                    assert not on and not ent.any()
                    continue
                assert on
                assert np.array_equal(ent, model_entries(p1, p2, X, Y, nt)), "sigma %g" % sig
            from xpysom_dask_amd.engine import SomHipError
            with pytest.raises(SomHipError, match="toroidal"):
                e.band_tables()                                       # the one-range read-back is not for this handle
        finally:
            e.close()
        if mode is None and (X, Y, neigh, sigma) in ((160, 96, "gaussian", 1.2), (129, 200, "gaussian", 4.0)):
            # the seam tiles -- the first and the last of each table -- hold nonzeros in both pieces and walk less than a row
            ty, tx = -(-Y // 32), -(-X // 32)
            for tile, side in [(0, Y), (ty - 1, Y), (nt * ty, X), (nt * ty + (tx - 1) * nt, X)]:
                assert ent[tile, 0, 1] > 0 and ent[tile, 1, 1] > 0
                assert walked(ent[tile], side) < side, (tile, ent[tile].tolist())
            # and the rows of the tables are cyclic: the table of a torus
            assert (p1[0, 0, 1:] == p1[0, 0, :0:-1]).all() and p1[0, 0, Y - 1] != 0


# ------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("sigma", [2.5, 3.0])
@pytest.mark.parametrize("neigh,compact", [("bubble", False), ("gaussian", True)])
@pytest.mark.parametrize("X,Y", [(97, 65), (96, 33)])
def test_bmus_away_from_the_seam_give_the_rectangle(monkeypatch, X, Y, neigh, compact, sigma):
    """With every BMU coordinate in [ceil(sigma), L - 1 - ceil(sigma)] no unit inside the support is reached across the seam:
    the compact tables agree entry for entry on the BMUs' columns, and the other columns multiply sums that are zero."""
    case = (X, Y, 5, neigh, compact, sigma, False, "spread")
    m = int(np.ceil(sigma))
    rs = np.random.RandomState(X + Y)
    bmu = (rs.randint(m, X - m, N) * Y + rs.randint(m, Y - m, N)).astype(np.int32)
    bmu[:4] = [m * Y + m, m * Y + (Y - 1 - m), (X - 1 - m) * Y + m, (X - 1 - m) * Y + (Y - 1 - m)]
    tor = run(monkeypatch, case, bmu=bmu)
    rect = run(monkeypatch, case, topology="rectangular", bmu=bmu)
    for what, a, b in zip(("numerator", "denominator", "merged codebook"), tor, rect):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what
    assert np.abs(tor[1]).max() > 0


# ------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("X,Y,D,neigh,sigma,wide", [(40, 33, 5, "bubble", 4.0, True), (64, 33, 7, "gaussian", 12.0, False)])
def test_faithful_form_reads_the_same_tables(X, Y, D, neigh, sigma, wide):
    data = O.gaussian_blobs(N, D, seed=X + D)
    w = O.default_codebook(X, Y, D, 2).astype(F32)
    e = engine(X, Y, D, neighborhood=neigh, topology="toroidal", precision="f32")
    try:
        e.set_weights(w)
        e.set_data(data)
        sig = np.float64(sigma) if wide else float(sigma)
        e.epoch_accumulate(sig, ETA, wide)
        num0, den0, bmu0 = (a.copy() for a in e.epoch_fetch())
        e.epoch_accumulate_faithful(sig, ETA, wide)
        num1, den1, bmu1 = (a.copy() for a in e.epoch_fetch())
    finally:
        e.close()
    assert np.array_equal(bmu0, bmu1)
    ref = T.reference_update(data, bmu1, X, Y, ETA, sig, wide=wide, neighbourhood=neigh, std_coeff=STD)
    U.check_accumulators(num0, den0, ref, "bucketed")
    U.check_accumulators(num1, den1, ref, "faithful")
    assert rel_err(num1, num0) < 1e-5 and rel_err(den1, den0) < 1e-5


# ------------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("graph", ["0", "1"])
def test_a_schedule_whose_bands_shrink_and_grow(monkeypatch, graph):
    """Each build of the tables fills the range buffer the build before zeroed; with SOM_GRAPH=1 the handle replays a captured
    epoch from the third one on and the torus flag, like the buffer's role, travels through device memory."""
    X, Y, D = 97, 65, 5
    monkeypatch.setenv("SOM_GRAPH", graph)
    monkeypatch.delenv("SOM_NO_BANDS", raising=False)
    data = O.gaussian_blobs(N, D, seed=5)
    e = engine(X, Y, D, topology="toroidal", precision="f32")
    try:
        e.set_weights(O.default_codebook(X, Y, D, 3).astype(F32))
        e.set_data(data)
        for sigma in (0.6, 9.0, 1.2, 30.0):
            w0 = e.get_weights()
            e.epoch_accumulate(sigma, ETA, True)
            num, den, bmu = (a.copy() for a in e.epoch_fetch())
            e.epoch_merge()
            w1 = e.get_weights()
            ref = T.reference_update(data, bmu, X, Y, ETA, np.float64(sigma), wide=True, std_coeff=STD)
            U.check_accumulators(num, den, ref, "sigma %g" % sigma)
            U.check_merge(w0, w1, num, den, ref, False, "sigma %g" % sigma)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 7, 8
def test_the_search_does_not_see_the_lattice():
    from xpysom_dask_amd import XPySom
    data = O.gaussian_blobs(4096, 16, seed=9)
    a = XPySom(64, 64, 16, topology="toroidal", random_seed=4, precision="exact").train(data, 3)
    b = XPySom(64, 64, 16, topology="toroidal", random_seed=4, precision="f32").train(data, 3)
    assert np.array_equal(a._weights, b._weights)
    r = XPySom(64, 64, 16, topology="rectangular", random_seed=4, precision="f32").train(data, 3)
    assert not np.array_equal(r._weights, b._weights)               # (and the lattice does reach the update)


def test_topographic_error_across_the_seam():
    from xpysom_dask_amd import XPySom
    w = 100.0 + np.arange(6 * 5 * 2, dtype=np.float64).reshape(6, 5, 2)
    w[0, 2] = [0.0, 0.0]
    w[5, 2] = [1.0, 0.0]
    row = np.array([[0.1, 0.0]], dtype=F32)
    got = {}
    for topo in ("toroidal", "rectangular"):
        som = XPySom(6, 5, 2, topology=topo, random_seed=1)
        som._weights = w.copy()
        assert tuple(som.winner(row)[0]) == (0, 2)
        got[topo] = som.topographic_error(row)
    assert got == {"toroidal": 0.0, "rectangular": 1.0}


def test_refused_combination_at_the_c_abi():
    from xpysom_dask_amd.engine import SomHipError
    with pytest.raises(SomHipError, match="toroidal"):
        engine(6, 6, 3, neighborhood="mexican_hat", compact_support=True, topology="toroidal")
