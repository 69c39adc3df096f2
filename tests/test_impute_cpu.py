"""`XPySom.impute` (missing values: the completed rows), the part that needs no GPU: what the call refuses before any engine
exists, the bit-exact model of tests/impute_ref.py on a case written out by hand, and the two entry points in the header and in
the ctypes binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import impute_ref as I
from xpysom_dask_amd import _lib
from xpysom_dask_amd.xpysom import XPySom

F32 = np.float32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "somhip.h")


class NoEngine:
    def __call__(self):
        raise AssertionError("the engine was asked for before the call was refused")


def holes(n=30, d=4, seed=0):
    x = np.random.RandomState(seed).rand(n, d).astype(F32)
    x[3, 1] = np.nan
    return x


def f32_of(words):
    return np.array(words, dtype=np.uint32).view(F32)


# ------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kw", [dict(), dict(precision='f32'), dict(precision='bf16')])
def test_impute_needs_the_missing_mode(monkeypatch, kw):
    s = XPySom(4, 4, 4, random_seed=1, **kw)
    monkeypatch.setattr(s, "_engine", NoEngine())
    with pytest.raises(ValueError, match=r"impute\(\) needs missing='nan'"):
        s.impute(holes())
    with pytest.raises(ValueError, match=r"impute\(\) needs missing='nan'"):
        s.impute(holes(), out=holes(), return_ids=True)


def test_wrong_feature_count_raises_before_an_engine_exists(monkeypatch):
    s = XPySom(4, 4, 5, missing='nan', random_seed=1)
    monkeypatch.setattr(s, "_engine", NoEngine())
    with pytest.raises(ValueError, match="Received 4 features, expected 5"):
        s.impute(holes())
    with pytest.raises(ValueError, match="Received 4 features, expected 5"):
        s.impute(holes()[0])                                # one sample


@pytest.mark.parametrize("out", ["same", "other", "list"])
def test_out_with_host_rows_raises(monkeypatch, out):
    s = XPySom(4, 4, 4, missing='nan', random_seed=1)
    monkeypatch.setattr(s, "_engine", NoEngine())
    x = holes()
    before = x.copy()
    target = {"same": x, "other": np.empty_like(x), "list": [[0.0] * 4] * 30}[out]
    with pytest.raises(ValueError, match="out is for rows in device memory"):
        s.impute(x, out=target)
    assert I.same_bits(x, before)


def test_out_and_return_ids_are_keyword_only():
    s = XPySom(4, 4, 4, missing='nan', random_seed=1)
    with pytest.raises(TypeError):
        s.impute(holes(), None)


def test_constructor_docstring_lists_impute():
    doc = XPySom.__init__.__doc__
    assert "impute" in doc[doc.index("missing        None"):]


# ------------------------------------------------------------------------------------------------------ the model
NAN_PAYLOAD, NAN_NEG, NAN_SIGNALLING = 0x7FC12345, 0xFFC00000, 0xFF800001
NEG_ZERO, INF, NEG_INF, DENORMAL = 0x80000000, 0x7F800000, 0xFF800000, 0x00000001


def test_model_on_a_case_written_out_by_hand():
    one, two = 0x3F800000, 0x40000000
    x = f32_of([[one, NAN_PAYLOAD, NEG_ZERO, INF],
                [NAN_NEG, NAN_SIGNALLING, 0x7FC00000, NAN_PAYLOAD],           # nothing observed
                [DENORMAL, two, NAN_SIGNALLING, NEG_INF]])
    w = f32_of([[0x41200000, 0x41300000, NEG_ZERO, 0x41500000],               # 10, 11, -0.0, 13
                [0x41A00000, 0x00000003, 0x41B00000, 0x41B80000]])            # 20, a denormal, 22, 23
    ids = np.array([1, 0, 1])
    want = f32_of([[one, 0x00000003, NEG_ZERO, INF],
                   [0x41200000, 0x41300000, NEG_ZERO, 0x41500000],
                   [DENORMAL, two, 0x41B00000, NEG_INF]])
    assert np.isnan(x).sum() == 6 and np.isnan(x[1]).all()
    x0 = x.copy()
    got = I.impute_reference(x, w, ids)
    assert got.dtype == F32 and got.shape == (3, 4)
    assert I.same_bits(got, want), I.first_difference(got, want)
    assert I.same_bits(x, x0), "the model wrote its input"
    assert not np.isnan(got).any()
    # a complete row comes back as it is; the codebook as a (X, Y, D) array serves too; a NaN in the codebook is handed on
    assert I.same_bits(I.impute_reference(want, w, ids), want)
    assert I.same_bits(I.impute_reference(x, w.reshape(1, 2, 4), ids), want)
    wn = w.copy()
    wn.view(np.uint32)[1, 1] = NAN_PAYLOAD
    assert I.bits(I.impute_reference(x, wn, ids))[0, 1] == NAN_PAYLOAD


def test_same_bits_tells_what_equality_of_values_does_not():
    a = f32_of([0x00000000, 0x7FC00000, 0x3F800000])
    b = f32_of([NEG_ZERO, 0x7FC00000, 0x3F800000])
    c = f32_of([0x00000000, NAN_PAYLOAD, 0x3F800000])
    assert I.same_bits(a, a.copy())
    assert a[0] == b[0] and not I.same_bits(a, b)
    assert not I.same_bits(a, c)
    assert I.first_difference(a, c)[0] == 1 and I.first_difference(a, a) is None
    assert not I.same_bits(a, a[:2])


# ------------------------------------------------------------------------------------------------------ header and binding
def test_header_declares_both_entry_points():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    assert "int som_impute(som_handle* h, const float* x_host, int64_t n_rows, float* out_host, int32_t* ids_out);" in flat
    assert "int som_impute_device(som_handle* h, const void* x_dev, int64_t n_rows, void* out_dev, int32_t* ids_out);" in flat
    assert flat.index("int som_bmu_distances_device(") < flat.index("int som_impute(") < flat.index("int som_unit_label_counts(")


def test_binding_gives_them_argtypes():
    F, Iptr = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    assert _lib.SIGNATURES["som_impute"] == (C.c_int, [C.c_void_p, F, C.c_int64, F, Iptr])
    assert _lib.SIGNATURES["som_impute_device"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, Iptr])
    from xpysom_dask_amd.engine import HipEngine
    assert callable(HipEngine.impute) and callable(HipEngine.impute_device)
