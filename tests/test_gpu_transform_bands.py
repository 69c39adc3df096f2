"""The transform's nonzero bands at the MFMA tile's granularity (csrc/update.hpp, "ranges" and leftmul_f32_kernel).

neigh_tables_kernel records, per 32-row tile of a neighbourhood table and per column segment, the column range
that holds every nonzero float32 it stored; the two GEMMs of the transform stage only the chunks inside the union
of a workgroup's tiles and issue an a-tile's MFMA steps only inside that tile's own range.  A skipped step would
have added 0 * m = +0, so numerator, denominator and BMUs must equal the full walk (SOM_NO_BANDS=1) BIT FOR BIT;
for the rectangular gaussian they must also agree with the float64 oracle (BMUs forced) within the suite's
rel_err < 1e-5.

The shapes are the ones at which the range arithmetic can go wrong: map sides with a partial last 32-row tile, a
partial last 128-row block and a one-row last block (160 x 96, 129 x 200, 97 x 65), sides of at most 64 (the 64-row
workgroup), and sigma such that the band is narrower than one MFMA step (0.3), straddles a chunk boundary (1.2,
4.0), is clipped at both map edges (12) and is dense (80); every neighbourhood (mexican_hat: negative entries and
two terms; bubble, triangle: compact, whole tiles of a table all zero) on both topologies (hexagonal: three
segments); 128 features (stage 2 batched per map column), 5 (whole rows, the VALU kernel) and 131 (a narrow last
tile); the headline's map, whose default this granularity turns on.  The ranges live in two buffers that change
roles from one build of the tables to the next: the schedule tests run epochs whose bands shrink and grow.  The ranges the
device recorded are read back and compared with the nonzeros of the tables it wrote, and narrow ones must be there: the
comparisons with the full walk mean nothing if the default quietly walked everything.  The 128-row workgroup tile, which
no launch with ranges takes by default, runs its banded walk under SOM_LM_ROWS=128."""
import numpy as np
import pytest

from oracle import som_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32

MAPS = [(160, 96), (129, 200), (97, 65)]
SMALL = [(48, 40), (64, 33)]
SIGMAS = [0.3, 1.2, 4.0, 12.0, 80.0]
OTHERS = [("mexican_hat", "rectangular"), ("bubble", "rectangular"), ("triangle", "rectangular"),
          ("gaussian", "hexagonal"), ("mexican_hat", "hexagonal"), ("bubble", "hexagonal")]


def engine(X, Y, D, **kw):
    from xpysom_dask_amd.engine import HipEngine
    return HipEngine(X, Y, D, **kw)


def rel_err(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def oracle_update(data, w, eta, sigma, bmu, rows=512):
    """oracle.som_oracle.update with the BMUs forced, summed over row chunks in float64 (its g is rows x units)."""
    num = den = None
    for s in range(0, len(data), rows):
        _, n, d = O.update(data[s:s + rows], w, eta, sigma, wide=True, forced_bmu=bmu[s:s + rows])
        num = n if num is None else num + n
        den = d if den is None else den + d
    return num, den


def model_entries(p1, p2, X, Y, nt):
    """{segw - first nonzero column, last nonzero column + 1} per 32-row tile and segment from the tables themselves, in the
    buffer's layout (csrc/update.hpp); a tile without a nonzero: {0, 0}."""
    ty, tx = -(-Y // 32), -(-X // 32)
    out = np.zeros((nt * (ty + tx), 2), dtype=np.int32)

    def entry(block, segw):
        cols = np.flatnonzero((block != 0).any(axis=0))
        return (segw - cols[0], cols[-1] + 1) if cols.size else (0, 0)
    for t in range(nt):
        for tile in range(ty):
            out[t * ty + tile] = entry(p1[t, tile * 32:(tile + 1) * 32, :], Y)
        for tile in range(tx):
            out[nt * ty + tile * nt + t] = entry(p2[tile * 32:(tile + 1) * 32, t * X:(t + 1) * X], X)
    return out


@pytest.mark.parametrize("X,Y,neigh,topo,sigma", [(160, 96, "gaussian", "rectangular", 1.2), (129, 200, "mexican_hat", "hexagonal", 4.0),
                                                  (97, 65, "bubble", "rectangular", 0.3), (97, 65, "triangle", "rectangular", 12.0),
                                                  (64, 33, "gaussian", "hexagonal", 0.3), (160, 96, "gaussian", "rectangular", 80.0),
                                                  (256, 256, "gaussian", "rectangular", 2.6)])
def test_device_ranges_are_the_tables_nonzeros_and_the_default_is_banded(monkeypatch, X, Y, neigh, topo, sigma):
    """The entries neigh_tables_kernel recorded (ballots, the LDS combine, the atomicMax pair), read back after two epochs of
    different sigma -- so both buffers have been filled and zeroed -- against the nonzeros of the tables read back with them:
    exactly the first and last nonzero column of every 32-row tile.  Bands on by default on all these maps; except at sigma 80
    some tile must be narrower than its table (the banded walk is taken), and under SOM_NO_BANDS=1 nothing is recorded."""
    D, n = 5, 500
    data = O.gaussian_blobs(n, D, seed=X)
    w = O.default_codebook(X, Y, D, 8).astype(F32)
    for mode in (None, "1"):
        if mode is None:
            monkeypatch.delenv("SOM_NO_BANDS", raising=False)
        else:
            monkeypatch.setenv("SOM_NO_BANDS", mode)
        e = engine(X, Y, D, neighborhood=neigh, topology=topo)
        e.set_weights(w)
        e.set_data(data)
        for sig in (7.0, sigma, 0.5, sigma):
            e.epoch_accumulate(sig, 0.4, True)
            on, ent, p1, p2 = e.band_tables()
            nt = p1.shape[0]
            if mode == "1":
                assert not on and not ent.any()
                continue
            assert on
            assert np.array_equal(ent, model_entries(p1, p2, X, Y, nt)), "sigma %g" % sig
        if mode is None and sigma < 80.0:
            widths = ent[:, 1] - (np.where(np.arange(len(ent)) < nt * -(-Y // 32), Y, X) - ent[:, 0])
            assert (widths[ent[:, 1] > 0] <= 32 + 2 * 8 * sigma + 2).all() and (ent[:, 1] > 0).any()
        e.close()


def both_walks(monkeypatch, X, Y, D, n, neigh, topo, sigma):
    data = O.gaussian_blobs(n, D, seed=X)
    w = O.default_codebook(X, Y, D, 8).astype(F32)
    outs = {}
    for mode in (None, "1"):                               # the default, then the full walk
        if mode is None:
            monkeypatch.delenv("SOM_NO_BANDS", raising=False)
        else:
            monkeypatch.setenv("SOM_NO_BANDS", mode)
        e = engine(X, Y, D, neighborhood=neigh, topology=topo)
        e.set_weights(w)
        e.set_data(data)
        e.epoch_accumulate(sigma, 0.4, True)
        num, den, bmu = e.epoch_fetch()
        outs[mode] = (num.copy(), den.copy(), bmu.copy())
        e.close()
    return data, w, outs[None], outs["1"]


def check(monkeypatch, X, Y, D, n, neigh, topo, sigma):
    data, w, got, full = both_walks(monkeypatch, X, Y, D, n, neigh, topo, sigma)
    assert np.array_equal(got[2], full[2])
    assert np.array_equal(got[0], full[0])
    assert np.array_equal(got[1], full[1])
    if neigh == "gaussian" and topo == "rectangular":
        onum, oden = oracle_update(data, w, 0.4, sigma, got[2])
        assert rel_err(got[0], onum.reshape(-1, D)) < 1e-5 and rel_err(got[1], oden.reshape(-1)) < 1e-5


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("X,Y", MAPS + SMALL)
def test_gaussian_bands_equal_the_full_walk_and_the_oracle(monkeypatch, X, Y, sigma):
    check(monkeypatch, X, Y, 5, 4000, "gaussian", "rectangular", sigma)


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("neigh,topo", OTHERS)
@pytest.mark.parametrize("X,Y", MAPS)
def test_every_neighbourhood_and_topology_equals_the_full_walk(monkeypatch, X, Y, neigh, topo, sigma):
    check(monkeypatch, X, Y, 5, 4000, neigh, topo, sigma)


@pytest.mark.parametrize("sigma", [1.2, 12.0])
@pytest.mark.parametrize("neigh,topo", [("gaussian", "rectangular"), ("mexican_hat", "hexagonal")])
@pytest.mark.parametrize("D", [128, 131])
@pytest.mark.parametrize("X,Y", [(160, 96), (97, 65)])
def test_batched_and_narrow_column_tiles_equal_the_full_walk(monkeypatch, X, Y, D, neigh, topo, sigma):
    check(monkeypatch, X, Y, D, 4000, neigh, topo, sigma)


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("X,Y,D,neigh,topo", [(160, 96, 5, "gaussian", "rectangular"), (129, 200, 128, "mexican_hat", "hexagonal"),
                                              (97, 65, 131, "gaussian", "rectangular"), (129, 200, 5, "bubble", "rectangular")])
def test_the_128_row_workgroup_tile_walks_its_bands_too(monkeypatch, X, Y, D, neigh, topo, sigma):
    """SOM_LM_ROWS=128: four tiles a workgroup (waves with rows 64..127 own tiles 2 and 3; a last block of fewer than four tiles)."""
    monkeypatch.setenv("SOM_LM_ROWS", "128")
    check(monkeypatch, X, Y, D, 4000, neigh, topo, sigma)


@pytest.mark.parametrize("sigma", [2.6, 48.0])
def test_headline_map_default_equals_the_full_walk_and_the_oracle(monkeypatch, sigma):
    """256 x 256 x 128: the shape whose default turns from off to on."""
    check(monkeypatch, 256, 256, 128, 4096, "gaussian", "rectangular", sigma)


@pytest.mark.parametrize("graph", ["0", "1"])
@pytest.mark.parametrize("precision", ["f32", "exact"])
def test_bands_follow_a_schedule_that_shrinks_and_grows(monkeypatch, graph, precision):
    """Epoch after epoch on one handle: each build of the tables fills the range buffer the build before zeroed.  A
    range left over from a wider or a narrower epoch would show as a difference from the full walk.  With SOM_GRAPH=1
    the float32 handle replays a captured epoch from the third one on and the buffer's role travels through device
    memory; the exact mode builds its tables early, under the BMU pass's read-back."""
    X, Y, D, n = 70, 97, 6, 3000
    data = O.gaussian_blobs(n, D, seed=5)
    w0 = O.default_codebook(X, Y, D, 3).astype(F32)
    sched = [12.0, 1.2, 0.3, 80.0, 4.0, 0.3, 12.0]
    monkeypatch.setenv("SOM_GRAPH", graph)
    outs = {}
    for mode in (None, "1"):
        if mode is None:
            monkeypatch.delenv("SOM_NO_BANDS", raising=False)
        else:
            monkeypatch.setenv("SOM_NO_BANDS", mode)
        e = engine(X, Y, D, precision=precision)
        e.set_data(data)
        res = []
        for t, sigma in enumerate(sched):
            e.set_weights(w0 * F32(1.0 + 0.1 * t))
            e.epoch_accumulate(sigma, 0.4, True)
            res.append(tuple(a.copy() for a in e.epoch_fetch()))
        e.close()
        outs[mode] = res
    for t, (got, full) in enumerate(zip(outs[None], outs["1"])):
        for a, b in zip(got, full):
            assert np.array_equal(a, b), "epoch %d (sigma %g)" % (t, sched[t])
    onum, oden = oracle_update(data, w0 * F32(1.0 + 0.1 * 2), 0.4, sched[2], outs[None][2][2])
    assert rel_err(outs[None][2][0], onum.reshape(-1, D)) < 1e-5 and rel_err(outs[None][2][1], oden.reshape(-1)) < 1e-5
