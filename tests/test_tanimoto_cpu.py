"""activation_distance='tanimoto' without a GPU: what the class accepts and what it refuses by name before any engine exists."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.conftest import _gpu_present
from xpysom_dask_amd.xpysom import XPySom


def test_accepted_and_refused_by_name(monkeypatch):
    for precision in ("exact", "f32"):
        assert XPySom(4, 4, 4096, activation_distance='tanimoto', precision=precision)._activation_distance_name == 'tanimoto'
    with pytest.raises(ValueError, match="'tanimoto' serves input_len <= 4096, got 4097"):
        XPySom(20, 20, 4097, activation_distance='tanimoto')
    for precision in ("bf16", "f16"):
        with pytest.raises(ValueError, match="'tanimoto' needs precision='f32'"):
            XPySom(4, 4, 3, activation_distance='tanimoto', precision=precision)
    with pytest.raises(ValueError, match="missing='nan' .*'euclidean' only, got 'tanimoto'"):
        XPySom(4, 4, 3, activation_distance='tanimoto', missing='nan')
    s = XPySom(4, 4, 3, activation_distance='tanimoto')
    monkeypatch.setattr(s, "_engine", lambda: pytest.fail("the engine was asked for before the call was refused"))
    rows, x = sp.csr_matrix(np.eye(3, dtype=np.float32)), np.zeros((2, 3), np.float32)
    for call in (lambda: s.train(rows, 1), lambda: s.winner(rows)):
        with pytest.raises(NotImplementedError, match="sparse rows are served under .* not 'tanimoto'"):
            call()
    with pytest.raises(NotImplementedError, match="'tanimoto'.* fused distance\\+argmin kernel"):
        s.activate(x)
    for what, call in (("nearest_units", lambda: s.nearest_units(x, 2)), ("rank_hits", lambda: s.rank_hits(x, 2)),
                       ("smoothed_hits", lambda: s.smoothed_hits(x, 2)), ("nearest_samples", lambda: s.nearest_samples(x, 1))):
        with pytest.raises(NotImplementedError, match="%s\\(\\).*'tanimoto' is a fused distance\\+argmin kernel" % what):
            call()


@pytest.mark.skipif(_gpu_present(), reason="checks the no-GPU failure mode")
def test_train_fails_loudly_without_a_gpu():
    from xpysom_dask_amd.engine import SomHipError
    with pytest.raises(SomHipError, match="no HIP device"):
        XPySom(4, 4, 2, activation_distance='tanimoto', random_seed=0).train(np.ones((8, 2)), 1)
