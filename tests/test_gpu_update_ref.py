"""The neighbourhood update (segment sum, separable transform, merge) against a direct-form float64 reference on large
maps (tests/update_ref.py).  GPU only (`-m gpu`).

Every forced case goes through epoch_accumulate_forced, so the BMUs are the test's and no search noise enters:
  accumulators  |num - ref| <= 1e-5 * mag_num elementwise, the same for den (below 2^-120 of an array's largest
                magnitude: that absolute level instead -- float32 tables underflow there)
  merge         float32(num / den) bit for bit where the engine's den != 0, the old row where it is 0; and within the
                first-order quotient bound of the reference (update_ref.check_merge)
  repeatability a second forced accumulate is bitwise equal; with more than one map-row block, begin + every block is
                bitwise the monolithic accumulate
The grid's axes: map shapes past the 64-row tile, several 128-row blocks with a one-row last block, bands on, square
maps for the swapped stage order, one stage on each tile size, degenerate axes; D on every narrow tile, per-column
stage 2 and segment-sum workgroup width (16, 8, 4, 2 waves and 1, odd and even); all twelve neighbourhood families at two
shapes with a side > 128, one of them with bands; rows 1 .. 400 000; BMU patterns spread / edges / skewed / sparse.
tests/test_update_ref_cpu.py checks that the grid reaches every branch update_ref.update_paths names."""
import numpy as np
import pytest

from oracle import som_oracle as O
from tests.update_ref import (FAMILIES, OFF_LATTICE, F32, accum_ratio, case_id, check_accumulators, check_merge,  # noqa: F401
                              reference_update, run_forced_case)

pytestmark = pytest.mark.gpu

_ROWS = [  # family, X, Y, D, N, pattern, sigma, std, wide, scale
    ("gaussian", 65, 66, 3, 2047, "spread", 1.5, 0.5, False, 1.0),
    ("gaussian", 300, 260, 24, 100003, "edges", 150.0, 0.5, True, 1e3),
    ("gaussian", 256, 257, 3, 400000, "skewed", 3.0, 0.5, False, 1.0),
    ("gaussian", 200, 40, 136, 2048, "sparse", 1.0, 0.25, False, 1e-3),
    ("gaussian", 40, 200, 128, 100003, "edges", OFF_LATTICE, 1.0, True, 1.0),
    ("gaussian", 1, 300, 24, 2048, "spread", 150.0, 0.5, False, 1.0),
    ("gaussian", 129, 130, 24, 1, "edges", 2.0, 0.5, True, 1.0),
    ("gaussian", 20, 30, 2044, 2047, "spread", 3.0, 0.5, False, 1.0),
    ("gaussian_compact", 129, 130, 256, 2048, "edges", 3.0, 1.0, False, 1.0),
    ("gaussian_compact", 300, 260, 507, 30011, "skewed", np.nextafter(3.0, 0.0), 0.5, False, 1.0),
    ("gaussian_compact", 300, 1, 6, 2047, "spread", 1.5, 0.25, True, 1e-3),
    ("mexican_hat", 129, 130, 100, 2047, "edges", 65.0, 0.5, True, 1.0),
    ("mexican_hat", 300, 260, 508, 30011, "sparse", 2.5, 0.5, False, 1e3),
    ("mexican_hat", 65, 66, 24, 100003, "spread", 1.0, 1.0, False, 1.0),
    ("mexican_hat_compact", 130, 130, 6, 2048, "edges", OFF_LATTICE, 0.5, False, 1.0),
    ("mexican_hat_compact", 257, 257, 24, 100003, "skewed", 3.0, 1.0, True, 1.0),
    ("mexican_hat_compact", 65, 65, 3, 2047, "spread", 1.5, 0.25, False, 1e-3),
    ("bubble", 256, 257, 784, 2048, "sparse", 3.0, 0.5, False, 1.0),
    ("bubble", 130, 130, 1020, 30011, "edges", 1.5, 0.5, True, 1e-3),
    ("triangle", 129, 130, 24, 100003, "skewed", 65.0, 0.5, False, 1.0),
    ("triangle", 1, 300, 3, 2047, "spread", OFF_LATTICE, 0.5, True, 1.0),
    ("triangle", 257, 257, 136, 2048, "edges", 2.0, 0.5, False, 1e3),
    ("triangle_compact", 300, 260, 136, 2048, "edges", 1.0, 0.5, False, 1.0),
    ("triangle_compact", 200, 40, 6, 100003, "skewed", 3.5, 0.5, True, 1.0),
    ("hex_gaussian", 129, 130, 24, 100003, "edges", 1.5, 0.5, False, 1.0),
    ("hex_gaussian", 300, 260, 100, 2048, "skewed", 130.0, 0.5, True, 1.0),
    ("hex_gaussian_compact", 256, 257, 6, 100003, "edges", OFF_LATTICE, 1.0, False, 1.0),
    ("hex_gaussian_compact", 130, 130, 508, 2047, "sparse", 3.0, 0.5, True, 1e3),
    ("hex_mexican_hat", 256, 257, 128, 2048, "edges", 2.0, 0.5, False, 1e3),
    ("hex_mexican_hat", 200, 40, 3, 100003, "skewed", 20.0, 0.5, True, 1.0),
    ("hex_mexican_hat_compact", 257, 257, 6, 2047, "edges", 3.0, 1.0, False, 1.0),
    ("hex_mexican_hat_compact", 129, 130, 24, 100003, "skewed", 1.5, 0.5, True, 1.0),
    ("hex_bubble", 300, 260, 3, 2047, "edges", 1.5, 0.5, False, 1.0),
    ("hex_bubble", 40, 200, 24, 100003, "spread", 3.0, 0.5, True, 1.0),
    ("hex_bubble", 257, 257, 136, 2048, "sparse", np.nextafter(3.0, 4.0), 0.5, False, 1.0),
    # regressions (fuzz_update.py 4242 400, cases 29, 207, 329): compact support at std_coeff 0.25, where exp(px / d) reaches
    # e^8 inside the box -- the old terms [-mx][my (ey - Q)] + [1][ey - Q] cancelled there, err/bound 1.7 .. 11.8
    ("mexican_hat_compact", 252, 252, 136, 2048, "edges", np.nextafter(126.0, 200.0), 0.25, False, 1e3),
    ("mexican_hat_compact", 139, 139, 256, 5000, "edges", np.nextafter(69.5, 0.0), 0.25, True, 1e3),
    ("hex_mexican_hat_compact", 271, 198, 136, 2048, "edges", np.nextafter(1.5, 2.0), 0.25, False, 1.0),
    # (rows are appended, never inserted: a row's eta and seed come from its position)
    # D1p = 4096: the run sum's one-wave workgroup, its slots written straight into the next list
    ("gaussian", 5, 7, 4092, 300, "skewed", 2.0, 0.5, True, 1.0),
]
CASES = []
for _i, (_f, _X, _Y, _D, _N, _p, _s, _std, _w, _sc) in enumerate(_ROWS):
    _c = dict(family=_f, X=_X, Y=_Y, D=_D, N=_N, pattern=_p, sigma=float(_s), std=_std, wide=_w, scale=_sc,
              eta=(0.5, 0.1, 1.0)[_i % 3], seed=1000 + _i)
    _c["id"] = case_id(_c)
    CASES.append(_c)

WORST = {}      # family -> worst err / bound over the forced cases (printed at the end of the module)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_forced_update_against_the_float64_reference(case):
    r = run_forced_case(case)
    w = WORST.setdefault(case["family"], {"accum": 0.0, "merge": 0.0})
    w["accum"], w["merge"] = max(w["accum"], r["accum"]), max(w["merge"], r["merge"])


@pytest.mark.parametrize("precision", ["f32", "exact", "bf16", "f16"])
def test_unforced_epoch_per_precision(precision):
    """epoch_accumulate on a 4096-unit map in every precision (the exact mode's early tables and zeroing; the 16-bit modes'
    fused merge + operand preparation), the accumulators checked against the reference from the engine's own BMUs."""
    from xpysom_dask_amd.engine import HipEngine
    X, Y, D, N = 64, 64, 24, 20000
    data = O.gaussian_blobs(N, D, seed=77)
    w0 = O.default_codebook(X, Y, D, 5).astype(F32).reshape(X * Y, D)
    e = HipEngine(X, Y, D, precision=precision)
    try:
        e.set_weights(w0)
        e.set_data(data)
        e.epoch_accumulate(3.0, 0.5, False)
        num, den, bmu = e.epoch_fetch()
        e.epoch_merge()
        w1 = e.get_weights()
    finally:
        e.close()
    assert (bmu >= 0).all() and (bmu < X * Y).all()
    ref = reference_update(data, bmu, X, Y, 0.5, 3.0, wide=False)
    check_accumulators(num, den, ref, precision)
    check_merge(w0, w1, num, den, ref, False, precision)


def test_streamed_uneven_chunks_large_map():
    """stream_epoch_accumulate over uneven chunks (the run sum's accumulate mode) at K > 8192 and D >= 508: every row a
    codebook row plus tiny noise, so its BMU is that unit by a wide margin."""
    from xpysom_dask_amd.engine import HipEngine
    X, Y, D = 100, 90, 508
    K = X * Y
    rs = np.random.RandomState(9)
    w0 = rs.standard_normal((K, D)).astype(F32)
    sizes = [1000, 3333, 1, 7000, 2047, 513]
    units = np.concatenate([rs.randint(0, 50, 6000), rs.randint(0, K, sum(sizes) - 6000)])   # 50 units own 6000 rows
    units = rs.permutation(units).astype(np.int32)
    data = (w0[units] + 1e-3 * rs.standard_normal((len(units), D))).astype(F32)
    e = HipEngine(X, Y, D, precision="f32", neighborhood="gaussian", std_coeff=0.5)
    try:
        e.set_weights(w0)
        assert np.array_equal(e.bmu(data), units)
        chunks, s = [], 0
        for n in sizes:
            chunks.append(data[s:s + n])
            s += n
        e.stream_epoch_accumulate(chunks, 4.0, 0.3, True)
        num, den, _ = e.epoch_fetch(want_bmu=False)
        e.epoch_merge()
        w1 = e.get_weights()
    finally:
        e.close()
    ref = reference_update(data, units, X, Y, 0.3, 4.0, wide=True)
    check_accumulators(num, den, ref, "stream")
    check_merge(w0, w1, num, den, ref, False, "stream")


def test_report_worst_ratio_per_family():
    """(last in the module) the worst err / bound per family, for the record; every forced case has already passed."""
    for fam in sorted(WORST):
        print("update_ref worst %-26s accum %.3g  merge %.3g" % (fam, WORST[fam]["accum"], WORST[fam]["merge"]))
    assert all(w["accum"] <= 1 and w["merge"] <= 1 for w in WORST.values())
