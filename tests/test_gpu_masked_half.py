"""The 16-bit MFMA masked BMU search on the device (`missing='nan', missing_search='bf16' | 'f16'`; som_set_masked_search,
csrc/bmu_masked_half.hpp).  GPU only (`-m gpu`).

The float64 reference on the kernel's own images, its derived bound and the grid of shapes are tests/masked_half_ref.py's
(tests/test_masked_half_cpu.py shows that the reference alone decides every point of it).

  1, 3, 4  admissible picks, the operand bound and one id per row whatever the route, on every (shape, data, hole pattern)
  2        exact ties on small-integer data: NumPy's first argmin, duplicated units many tiles apart
  -        1, 3 and the maximum number of codebook parts: identical ids
  5        a forced-BMU epoch under missing_search='f16' against the update's model; two identical epochs bitwise equal
  6        XPySom end to end: the final masked QE against the float32 search's
  7        refusals of the C ABI
"""
import numpy as np
import pytest

from tests import masked_half_ref as H
from tests import missing_ref as M
from tests.test_gpu_missing import FORCED, bits, device_ids, engine, forced_case, som

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPE_IDS = ["n%d-%dx%dx%d" % s for s in H.SHAPES]


# ----------------------------------------------------------------------------- 1, 3, 4
@pytest.mark.parametrize("shape", H.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("kind", H.KINDS)
def test_picks_operand_bound_and_routes(kind, shape):
    N, X, Y, D = shape
    e = engine(X, Y, D, missing_search=kind)
    try:
        for data, pattern in H.DATA:
            if data == "tiny" and kind != "f16":
                continue
            x, w = H.case(shape, data, pattern)
            e.set_weights(w)
            ids = e.bmu(x)
            what = "%s %r %s %s" % (kind, shape, data, pattern)
            pick, operand = H.check(ids, x, w, kind, what)
            print("%s: pick %.3g, operand %.3g of the bound" % (what, pick, operand))
            assert np.array_equal(ids, device_ids(e, x)), what + ": som_bmu_device differs"
            assert np.array_equal(ids, e.bmu(x, quantization=True)), what + ": the quantization rule differs"
            assert np.array_equal(ids, e.impute(x)[1]), what + ": impute's ids differ"
    finally:
        e.close()


# ----------------------------------------------------------------------------- 2
@pytest.mark.parametrize("shape", H.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("kind", H.KINDS)
def test_exact_ties(kind, shape):
    N, X, Y, D = shape
    x, w = M.exact_case(N, X * Y, D, seed=D + N)
    e = engine(X, Y, D, missing_search=kind)
    try:
        e.set_weights(w)
        ids = e.bmu(x)
    finally:
        e.close()
    H.check_ties(ids, M.masked_sq_dist(x, w) if N * X * Y * D < 1 << 24 else M.masked_scores(x, w)[0], "%s %r" % (kind, shape))


# ----------------------------------------------------------------------------- codebook parts
@pytest.mark.parametrize("kind, shape", [("bf16", H.SHAPES[3]), ("f16", (129, 9, 29, 160))], ids=["resident", "streamed"])
def test_ids_do_not_depend_on_the_part_count(monkeypatch, kind, shape):
    N, X, Y, D = shape
    x, w = H.case(shape, "blobs", "random30")
    got = []
    for parts in (1, 3, 1 << 20):                      # (clamped to the stages: the maximum)
        monkeypatch.setenv("SOM_MASKED_PARTS", str(parts))
        e = engine(X, Y, D, missing_search=kind)
        try:
            e.set_weights(w)
            got.append(e.bmu(x))
        finally:
            e.close()
    H.check(got[0], x, w, kind, "%s %r one part" % (kind, shape))
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


# ----------------------------------------------------------------------------- 5
def test_forced_epoch_and_determinism():
    case = FORCED[1]
    fam, X, Y, D, N, bpat, mpat, sigma, wide = case
    data, bmu, w0, ref, kw = forced_case(case)
    e = engine(X, Y, D, missing_search="f16", **kw)
    try:
        e.set_weights(w0)
        e.set_data(data)
        e.epoch_accumulate_forced(bmu, sigma, 0.5, wide)
        num, den, _ = e.epoch_fetch_masked(want_bmu=False)
        e.epoch_merge()
        w1 = e.get_weights()
        M.check_accumulators(num, den, ref, "forced f16")
        M.check_merge(w0, w1, num, den, ref, False, "forced f16")
        runs = []
        for _ in range(2):
            e.set_weights(w0)
            e.epoch_accumulate(sigma, 0.5, wide)
            runs.append(e.epoch_fetch_masked())
    finally:
        e.close()
    (n0, d0, b0), (n1, d1, b1) = runs
    H.check(b0, data, w0, "f16", "epoch ids")
    assert np.array_equal(b0, b1) and np.array_equal(bits(n0), bits(n1)) and np.array_equal(bits(d0), bits(d1))


# ----------------------------------------------------------------------------- 6
def test_trained_quantization_error_against_the_float32_search():
    X, Y, D, N = 16, 16, 33, 5000
    x = M.punch(H.case((N, X, Y, D), "blobs", "none")[0], "random30", 4)
    qe = {}
    for ms in ("f32", "f16"):
        qe[ms] = som(X, Y, D, sigma=3.0, random_seed=2, precision="f32", missing_search=ms).train(x, 10).quantization_error(x)
    gap = abs(qe["f16"] - qe["f32"]) / qe["f32"]
    print("masked QE after 10 epochs: f32 search %.6f, f16 search %.6f, gap %.4f %%" % (qe["f32"], qe["f16"], 100 * gap))
    assert gap <= 0.0014                                # README: the unmasked 16-bit modes' gap


# ----------------------------------------------------------------------------- 7
def test_refusals():
    from xpysom_dask_amd import _lib
    from xpysom_dask_amd.engine import SomHipError
    u, m = engine(5, 7, 3, missing=None), engine(5, 7, 3)
    try:
        assert u._lib.som_set_masked_search(u._h, _lib.SOM_PREC["bf16"]) != 0
        assert b"SOM_MISSING_NAN" in u._lib.som_last_error(u._h)
        for bad in (_lib.SOM_PREC["exact"], 2, -1, 99):
            assert m._lib.som_set_masked_search(m._h, bad) != 0
        assert m._lib.som_get_masked_search(m._h) == _lib.SOM_PREC["f32"]
        m.set_missing_search("bf16")
        assert m._lib.som_get_masked_search(m._h) == _lib.SOM_PREC["bf16"]
    finally:
        u.close()
        m.close()
    with pytest.raises(SomHipError, match="float32 masked kernel"):
        engine(5, 7, 3, precision="bf16")
