"""activation_distance='chebyshev', the part that needs no GPU: what the class accepts and what it refuses -- in the words
it uses for 'manhattan' -- before any engine exists."""
import numpy as np
import pytest
import scipy.sparse as sp

from xpysom_dask_amd import _lib
from xpysom_dask_amd.xpysom import XPySom


def test_the_class_accepts_it():
    for precision in ("exact", "f32"):
        assert XPySom(4, 4, 3, activation_distance='chebyshev', precision=precision)._activation_distance_name == 'chebyshev'
    assert _lib.SOM_DIST["chebyshev"] == 6


def test_unknown_distance_message_lists_it():
    with pytest.raises(ValueError, match="Distances available: .*chebyshev"):
        XPySom(4, 4, 3, activation_distance='minkowski')


@pytest.mark.parametrize("distance", ["manhattan", "chebyshev"])
def test_refusals_are_manhattans(distance, monkeypatch):
    with pytest.raises(ValueError, match="'%s' needs precision='f32'" % distance):
        XPySom(4, 4, 3, activation_distance=distance, precision='bf16')
    with pytest.raises(ValueError, match="'euclidean' only, got '%s'" % distance):
        XPySom(4, 4, 3, activation_distance=distance, missing='nan')
    s = XPySom(4, 4, 3, activation_distance=distance)
    monkeypatch.setattr(s, "_engine", lambda: pytest.fail("the engine was asked for before the call was refused"))
    rows = sp.csr_matrix(np.eye(3, dtype=np.float32))
    for call in (lambda: s.train(rows, 1), lambda: s.winner(rows)):
        with pytest.raises(NotImplementedError, match="sparse rows are served under .* not '%s'" % distance):
            call()
    with pytest.raises(NotImplementedError, match="'%s'.* fused distance\\+argmin kernel" % distance):
        s.activate(np.zeros((2, 3), np.float32))
