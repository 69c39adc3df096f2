"""The nearest-rows scan without a GPU: exemplar_plan through its hook (include/somhip_test.h) and XPySom.nearest_samples' refusals."""
import ctypes as C

import numpy as np
import pytest


@pytest.mark.parametrize("n,K,slots,forced", [(1, 1, 512, 0), (127, 130, 512, 0), (300, 130, 512, 2), (300, 130, 512, 3), (300, 1, 512, 64),
                                              (1 << 20, 65536, 512, 0), (1 << 20, 4096, 512, 0), (2**31 - 1, 1, 10**6, 0), (4096, 16, 512, 7)])
def test_exemplar_plan(n, K, slots, forced):
    from xpysom_dask_amd import _lib
    out = (C.c_int64 * 4)()
    assert _lib.load().som_debug_exemplar_plan(n, K, slots, forced, out) == 0
    unit_tiles, stages, parts, per = list(out)
    assert unit_tiles == -(-K // 128) and stages == -(-n // 128)
    asked = min(forced or -(-slots // unit_tiles), stages, 65535)
    assert 1 <= parts <= asked                               # never more parts than row stages: a forced count is clamped
    assert (parts - 1) * per < stages <= parts * per         # every part has a stage, and every stage a part
    assert per == -(-stages // asked)


def test_exemplar_plan_refuses_bad_arguments():
    from xpysom_dask_amd import _lib
    lib, out = _lib.load(), (C.c_int64 * 4)()
    for bad in ((0, 8, 512, 0), (2**31, 8, 512, 0), (10, 0, 512, 0), (10, 8, 0, 0), (10, 8, 512, -1)):
        assert lib.som_debug_exemplar_plan(*bad, out) != 0
    assert lib.som_debug_exemplar_plan(10, 8, 512, 0, None) != 0


def test_nearest_samples_refuses_by_name_without_an_engine():
    sparse = pytest.importorskip("scipy.sparse")
    from xpysom_dask_amd import XPySom
    x = np.zeros((4, 3), np.float32)
    som = XPySom(2, 3, 3, random_seed=1)
    for k in (0, 9):
        with pytest.raises(ValueError, match="k must be between 1 and 8"):
            som.nearest_samples(x, k)
    with pytest.raises(NotImplementedError, match="nearest_samples.*missing='nan'"):
        XPySom(2, 3, 3, random_seed=1, missing="nan").nearest_samples(x, 2)
    with pytest.raises(NotImplementedError, match="nearest_samples.*GEMM-form.*manhattan"):
        XPySom(2, 3, 3, random_seed=1, activation_distance="manhattan").nearest_samples(x, 2)
    with pytest.raises(NotImplementedError, match="nearest_samples.*sparse rows"):
        som.nearest_samples(sparse.csr_matrix(x), 2)
