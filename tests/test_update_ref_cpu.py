"""The float64 update reference (tests/update_ref.py) itself: it agrees with the oracle's update, the elementwise check
the GPU module applies rejects plausible wrong accumulators, and the GPU module's case list reaches every branch of the
host's update dispatch.  No GPU needed."""
import numpy as np
import pytest

from oracle import som_oracle as O
from tests import test_gpu_update_ref as G
from tests.update_ref import (ALL_LABELS, FAMILIES, OFF_LATTICE, F32, F64, make_bmu, make_data, reference_update,
                              segment_sums, update_paths)

COMBOS = [(n, t, c) for t in ("rectangular", "hexagonal") for n in ("gaussian", "mexican_hat", "bubble", "triangle")
          for c in (False, True) if not (t == "hexagonal" and n == "triangle")]


def _oracle64(data, bmu, X, Y, eta, sigma, wide, neigh, topo, compact, std):
    """O.update with forced BMUs on float64 rows plus a column of ones: the reference's own h, every product and sum
    in float64 (den = the ones column, since O.update sums a float32 g in float32)."""
    x = np.c_[np.asarray(data, F64), np.ones(len(data))]
    w3 = np.zeros((X, Y, x.shape[1]), F32)
    _, num, _ = O.update(x, w3, eta, sigma, wide=wide, neighbourhood=neigh + ("_hex" if topo == "hexagonal" else ""),
                         compact=compact, std_coeff=std, forced_bmu=bmu)
    num = np.asarray(num, F64).reshape(X * Y, -1)
    return num[:, :-1], num[:, -1]


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("sigma", [3.0, OFF_LATTICE, 1.5])
@pytest.mark.parametrize("neigh,topo,compact", COMBOS)
def test_reference_equals_the_oracle_update(neigh, topo, compact, sigma, wide):
    X, Y = (6, 6) if neigh == "mexican_hat" and compact and topo == "rectangular" else (7, 6)
    D, N = 5, 300
    rs = np.random.RandomState(3)
    bmu = rs.randint(0, X * Y, N).astype(np.int32)
    data = make_data(N, D, 1.0, 4)
    for std in (0.5, 0.25):
        num, den, mnum, mden = reference_update(data, bmu, X, Y, 0.4, sigma, wide=wide, neighbourhood=neigh,
                                                topology=topo, compact=compact, std_coeff=std)
        onum, oden = _oracle64(data, bmu, X, Y, 0.4, sigma, wide, neigh, topo, compact, std)
        assert (np.abs(num - onum) <= 1e-12 * mnum).all()
        assert (np.abs(den - oden) <= 1e-12 * mden).all()
        assert (np.abs(num) <= mnum * (1 + 1e-12)).all() and (mden >= 0).all()


def test_segment_sums_against_a_loop():
    rs = np.random.RandomState(1)
    data = rs.standard_normal((500, 3)).astype(F32)
    bmu = rs.randint(0, 20, 500) * 3
    units, S, A, c = segment_sums(data, bmu)
    assert list(units) == sorted(set(bmu.tolist()))
    for k, u in enumerate(units):
        rows = data[bmu == u].astype(F64)
        np.testing.assert_allclose(S[k], rows.sum(0), rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(A[k], np.abs(rows).sum(0), rtol=1e-13)
        assert c[k] == len(rows)


# ------------------------------------------------------------------------------------------------ the checker has teeth
def _separable_gaussian(data, bmu, X, Y, eta, sigma, std, round_tables=None, shift_row=None):
    """The rectangular gaussian the way the library forms it: [num|den](i, j) = sum_a Px[i, a] sum_b Py[j, b] [S|c](a, b)
    from float32 factor tables Px[i, a] = eta * exp(-(i - a)^2 / d), Py[j, b] = exp(-(j - b)^2 / d); optionally the
    tables rounded through `round_tables`, or Py's row `shift_row` holding the row before it."""
    d = 2 * std ** 2 * sigma ** 2
    ii = np.arange(X)
    jj = np.arange(Y)
    Px = (np.exp(-np.power(ii[:, None] - ii[None, :], 2, dtype=F32) / d) * eta).astype(F32)
    Py = np.exp(-np.power(jj[:, None] - jj[None, :], 2, dtype=F32) / d).astype(F32)
    if round_tables is not None:
        Px, Py = round_tables(Px), round_tables(Py)
    if shift_row is not None:
        Py[shift_row] = Py[shift_row - 1]
    units, S, _, c = segment_sums(data, bmu)
    D = S.shape[1]
    SC = np.zeros((X, Y, D + 1))
    SC[units // Y, units % Y, :D] = S
    SC[units // Y, units % Y, D] = c
    acc = np.einsum("ia,jb,abd->ijd", Px.astype(F64), Py.astype(F64), SC).reshape(X * Y, D + 1).astype(F32)
    return acc[:, :D], acc[:, D]


def _bf16(a):
    u = np.asarray(a, F32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16                 # round to nearest even on the 16 dropped bits
    return u.astype(np.uint32).view(F32)


@pytest.fixture(scope="module")
def rect():
    X, Y, D, N = 5, 140, 4, 3000
    rs = np.random.RandomState(8)
    bmu = make_bmu("spread", X, Y, N, rs)
    data = make_data(N, D, 1.0, 9)
    ref = reference_update(data, bmu, X, Y, 0.5, 40.0, wide=False)
    return X, Y, D, data, bmu, ref


def test_unmutated_separable_form_passes(rect):
    """the control: the float32 separable form and the float32 reference itself are within the bound"""
    X, Y, D, data, bmu, ref = rect
    G.check_accumulators(ref[0].astype(F32), ref[1].astype(F32), ref)
    num, den = _separable_gaussian(data, bmu, X, Y, 0.5, 40.0, 0.5)
    assert G.check_accumulators(num, den, ref) < 0.1


def test_checker_rejects_a_table_row_shifted_across_the_block_edge(rect):
    X, Y, D, data, bmu, ref = rect
    num, den = _separable_gaussian(data, bmu, X, Y, 0.5, 40.0, 0.5, shift_row=128)
    with pytest.raises(AssertionError):
        G.check_accumulators(num, den, ref)


def test_checker_rejects_bf16_tables(rect):
    X, Y, D, data, bmu, ref = rect
    num, den = _separable_gaussian(data, bmu, X, Y, 0.5, 40.0, 0.5, round_tables=_bf16)
    with pytest.raises(AssertionError):
        G.check_accumulators(num, den, ref)


def test_checker_rejects_a_segment_sum_missing_a_row(rect):
    X, Y, D, data, bmu, ref = rect
    u, cnt = np.unique(bmu, return_counts=True)
    drop = np.flatnonzero(bmu == u[np.argmax(cnt)])[0]               # a row of the unit with most rows
    keep = np.arange(len(bmu)) != drop
    bad = reference_update(data[keep], bmu[keep], X, Y, 0.5, 40.0, wide=False)
    with pytest.raises(AssertionError):
        G.check_accumulators(bad[0].astype(F32), bad[1].astype(F32), ref)


def test_checker_rejects_the_hex_class_offset_with_its_sign_flipped(monkeypatch):
    """every second map row shifted by +0.5 instead of -0.5: the separable hexagonal terms with the class offset's sign
    flipped, which is what a sign error in the library's class table would compute"""
    X, Y, D, N = 9, 8, 3, 2000
    rs = np.random.RandomState(2)
    bmu = make_bmu("spread", X, Y, N, rs)
    data = make_data(N, D, 1.0, 5)
    kw = dict(wide=False, neighbourhood="gaussian", topology="hexagonal", std_coeff=0.5)
    ref = reference_update(data, bmu, X, Y, 0.5, 2.0, **kw)
    G.check_accumulators(ref[0].astype(F32), ref[1].astype(F32), ref)
    real = O.hex_coords

    def flipped(X, Y):
        xx, yy = real(X, Y)
        xx[::-2] += 1.0
        return xx, yy
    monkeypatch.setattr(O, "hex_coords", flipped)
    bad = reference_update(data, bmu, X, Y, 0.5, 2.0, **kw)
    monkeypatch.undo()
    with pytest.raises(AssertionError):
        G.check_accumulators(bad[0].astype(F32), bad[1].astype(F32), ref)


def test_merge_checker_rejects_an_approximate_division(rect):
    X, Y, D, data, bmu, ref = rect
    num, den = ref[0].astype(F32), ref[1].astype(F32)
    w0 = np.zeros((X * Y, D), F32)
    good = (num / den[:, None]).astype(F32)
    G.check_merge(w0, good, num, den, ref, False)
    bad = (num * (F32(1) / den)[:, None]).astype(F32)                # reciprocal, then multiply: off by an ulp here and there
    assert not np.array_equal(bad, good)
    with pytest.raises(AssertionError):
        G.check_merge(w0, bad, num, den, ref, False)


# ------------------------------------------------------------------------------------------------ the grid's coverage
def test_grid_reaches_every_update_branch():
    reached = set()
    for c in G.CASES:
        n, t, cp = FAMILIES[c["family"]]
        reached |= update_paths(c["X"], c["Y"], c["D"], n, t, cp, c["N"])
    assert ALL_LABELS - reached == set()
    assert reached <= ALL_LABELS


def test_grid_covers_every_family_on_large_maps():
    for fam in FAMILIES:
        big = [c for c in G.CASES if c["family"] == fam and max(c["X"], c["Y"]) > 128]
        assert len({(c["X"], c["Y"]) for c in big}) >= 2, fam
        assert any(max(c["X"], c["Y"]) > 256 for c in big), fam
    assert {c["D"] for c in G.CASES} >= {3, 6, 24, 100, 128, 136, 256, 507, 508, 784, 1020, 2044}
    assert {c["pattern"] for c in G.CASES} == {"spread", "edges", "skewed", "sparse"}
    assert {c["std"] for c in G.CASES} == {0.25, 0.5, 1.0} and {c["wide"] for c in G.CASES} == {False, True}
    assert {1, 2047, 2048, 100003, 400000} <= {c["N"] for c in G.CASES}


def test_update_paths_follows_the_dispatch_rules():
    def paths(X, Y, D, N, neigh="gaussian", topo="rectangular", compact=False, **kw):
        return update_paths(X, Y, D, neigh, topo, compact, N, **kw)

    def waves(D, **kw):
        return [x for x in paths(4, 4, D, 1, **kw) if x.startswith("seg.waves")]

    p = paths(300, 260, 3, 2047)
    assert {"s1.narrow2", "s1.rows3+", "s2.rows3+", "bands.on", "s2.whole_rows", "sort.radix", "seg.waves16",
            "seg.vec1", "runsum.upper"} <= p
    # ranges on (a side > 32): the 64-row tile whatever the stage's height
    p = paths(40, 200, 128, 1)
    assert {"s2.per_column", "s2.tile64", "s1.tile64", "runsum.single", "bands.on", "seg.vec2"} <= p
    assert not {"s1.tile128", "s2.tile128", "s1.wrap", "s2.wrap"} & p
    # bands: on iff a side exceeds the 32-row range tile, and never for the swapped order
    assert "bands.off" in paths(32, 32, 24, 10) and "bands.on" in paths(33, 32, 24, 10) and "bands.on" in paths(32, 33, 24, 10)
    assert "bands.on" in paths(1, 33, 24, 10) and "bands.off" in paths(1, 32, 24, 10)
    p = paths(130, 130, 24, 10, "mexican_hat", compact=True)
    assert {"swapped.on", "bands.off", "s1.tile128", "s2.tile128"} <= p and not {"s1.tile64", "s2.tile64"} & p
    assert {"s1.tile64", "s2.tile64"} <= paths(64, 64, 24, 10, "mexican_hat", compact=True)       # no ranges, Ro <= 64
    assert "s2.tile128" not in paths(66, 66, 3, 10, "mexican_hat", compact=True)                  # D1p = 4: a narrow tile alone
    # a toroidal handle with ranges launches the wrap kernels (its narrow tile is the ordinary one)
    p = paths(129, 40, 24, 10, topo="toroidal")
    assert {"s1.wrap", "s2.wrap", "s1.tile64", "s2.tile64", "bands.on", "hex.classes0"} <= p
    assert not {"s1.wrap", "s2.wrap"} & paths(32, 32, 24, 10, topo="toroidal")
    assert "s1.wrap" not in paths(129, 40, 3, 10, topo="toroidal") and "s1.narrow2" in paths(129, 40, 3, 10, topo="toroidal")
    assert "swapped.on" in update_paths(130, 130, 6, "mexican_hat", "rectangular", True, 10)
    assert "hex.classes4" in update_paths(130, 130, 6, "mexican_hat", "hexagonal", True, 10)
    assert "hex.classes0" in update_paths(130, 130, 6, "bubble", "hexagonal", True, 10)
    assert [waves(D) for D in (507, 508, 1020, 2044, 4091, 4092)] == [
        ["seg.waves16"], ["seg.waves8"], ["seg.waves4"], ["seg.waves2"], ["seg.waves2"], ["seg.waves1"]]
    # a masked handle: rows of 2 D features, D1p = round_up(2 D + 1, 4); level 0 keeps D's parity
    assert [waves(D, masked=True) for D in (253, 254, 510, 1022, 2046)] == [
        ["seg.waves16"], ["seg.waves8"], ["seg.waves4"], ["seg.waves2"], ["seg.waves1"]]
    assert [waves(D, masked=True) for D in (509, 1021, 2045)] == [["seg.waves8"], ["seg.waves4"], ["seg.waves2"]]
    assert "seg.vec1" in paths(4, 4, 3, 1, masked=True) and "seg.vec2" in paths(4, 4, 2, 1, masked=True)
    p = paths(129, 5, 64, 1000, masked=True)                                    # UD = 128: per column, no narrow tile
    assert {"s2.per_column", "s1.narrow_none", "s2.narrow_none", "s2.last1", "s2.rows2"} <= p
    assert "s2.whole_rows" in paths(129, 5, 64, 1000)
    p = paths(257, 3, 65, 2100, masked=True)                                    # UD = 130: a narrow tile of 2 columns
    assert {"s1.narrow2", "s1.tile64", "s2.whole_rows", "s2.rows3+", "s2.last1"} <= p
    assert {"s1.narrow4", "s2.narrow_none"} <= paths(1, 300, 3, 10, masked=True) and \
        "s1.tile64" not in paths(1, 300, 3, 10, masked=True)                    # UD = 6: stage 1 is a narrow tile alone
    assert "sort.counting" in update_paths(64, 64, 3, "gaussian", "rectangular", False, 2048)
    assert "sort.radix" in update_paths(64, 128, 3, "gaussian", "rectangular", False, 1 << 20)     # 1024 blocks x 8192
