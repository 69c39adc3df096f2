"""The reference of the 16-bit masked search (tests/masked_half_ref.py) and the `missing_search` keyword, without a GPU."""
import pickle

import numpy as np
import pytest

from tests import masked_half_ref as H
from tests import missing_ref as M


@pytest.mark.parametrize("kind", H.KINDS)
@pytest.mark.parametrize("N, K, D", [(40, 37, 1), (130, 70, 33), (64, 300, 160)])
def test_reference_names_the_masked_bmu_on_exact_data(kind, N, K, D):
    x, w = M.exact_case(N, K, D, seed=N + D)
    s, E = H.scores(x, w, kind)
    assert np.array_equal(np.argmin(s, axis=1), M.masked_bmu(x, w))
    # every score is exact: the reference equals the float32 model's, half of c2 - 2 c1
    assert np.array_equal(2 * s, M.masked_scores(x, w)[0])


@pytest.mark.parametrize("kind, rel", [("bf16", 0.0), ("f16", 2.0 ** -17)])
def test_image_split(kind, rel):
    rs = np.random.RandomState(3)
    w = (rs.normal(0, 1, (200, 40)) * 10.0 ** rs.uniform(-3, 4, (200, 40))).astype(np.float32)
    w[0, :4] = [65504.0, -7.0e4, 0.0, 2.0 ** -20]
    wr, hi, lo = H.images(w, kind)
    q = wr * wr
    assert (np.abs(2 * (hi + lo) - q) <= rel * q).all()
    assert (lo != 0).any() and np.isfinite(hi).all()


@pytest.mark.parametrize("kind", H.KINDS)
def test_the_gpu_grid_is_decided_by_the_reference_alone(kind):
    """Every (shape, data) point of the GPU module: the bound is finite, and the reference's own first minimum passes both
    checks with nothing to spare for -- check() asks nothing of a pick that float64 on the images cannot answer."""
    for shape in H.SHAPES[:3] + H.SHAPES[4:5]:
        for data, pattern in H.DATA:
            if data == "tiny" and kind != "f16":
                continue
            x, w = H.case(shape, data, pattern)
            s, _ = H.scores(x, w, kind)
            ids = np.argmin(s, axis=1)
            ids[np.isnan(x).all(axis=1)] = 0
            assert H.check(ids, x, w, kind, "%r %s %s" % (shape, data, pattern))[0] == 0.0


def test_constructor_accepts_and_refuses():
    from xpysom_dask_amd import XPySom
    for ms in ("f32", "bf16", "f16"):
        s = XPySom(5, 5, 4, missing="nan", missing_search=ms)
        assert s._missing_search == ms and pickle.loads(pickle.dumps(s))._missing_search == ms
    assert XPySom(5, 5, 4)._missing_search == "f32"
    with pytest.raises(ValueError, match="missing_search must be"):
        XPySom(5, 5, 4, missing="nan", missing_search="f64")
    with pytest.raises(ValueError, match="needs missing='nan'"):
        XPySom(5, 5, 4, missing_search="bf16")
    with pytest.raises(ValueError, match="float32 masked kernel"):          # the existing refusal stays
        XPySom(5, 5, 4, missing="nan", precision="bf16", missing_search="bf16")
    with pytest.raises(TypeError):
        XPySom(5, 5, 4, 1.0, 1.0, 0, 0.5, 1.0, "exponential_decay", "gaussian", "rectangular", "euclidean", {}, None, 0, False,
               None, False, "auto", "bf16")


def test_keyword_reaches_the_engine(monkeypatch):
    from xpysom_dask_amd import XPySom, engine
    seen = {}

    class Stub:
        def __init__(self, *a, **kw):
            seen.update(kw)

    monkeypatch.setattr(engine, "HipEngine", Stub)
    XPySom(5, 5, 4, missing="nan", missing_search="f16")._engine()
    assert seen["missing"] == "nan" and seen["missing_search"] == "f16"
    monkeypatch.undo()
    with pytest.raises(ValueError, match="needs missing='nan'"):            # (refused before the library is loaded)
        engine.HipEngine(5, 5, 4, missing_search="f16")
