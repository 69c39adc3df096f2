"""_csr_rows (xpysom_dask_amd/xpysom.py): what a scipy.sparse input becomes on its way to the engine.  No device."""
import numpy as np
import pytest
import scipy.sparse as sp

from xpysom_dask_amd.xpysom import _csr_rows, _is_sparse

ROWS = np.array([0, 0, 2, 2, 2, 0, 3])
COLS = np.array([4, 1, 3, 0, 3, 4, 2])
VALS = np.array([1.5, 2.0, 1.0, -1.0, 2.5, 0.25, 0.0])          # (0, 4) and (2, 3) twice, an explicit zero at (3, 2), row 1 empty


def coo():
    return sp.coo_matrix((VALS, (ROWS, COLS)), shape=(4, 5))


def test_coo_with_duplicates_becomes_canonical_csr_and_is_left_alone():
    m = coo()
    dense = m.toarray()
    indptr, indices, values = _csr_rows(m, 5)
    assert (indptr.dtype, indices.dtype, values.dtype) == (np.int64, np.int32, np.float32)
    assert indptr.shape == (5,) and indices.shape == values.shape == (5,)
    np.testing.assert_array_equal(indptr, [0, 2, 2, 4, 5])
    np.testing.assert_array_equal(indices, [1, 4, 0, 3, 2])          # ascending inside a row, duplicates joined
    np.testing.assert_array_equal(values, np.float32([2.0, 1.75, -1.0, 3.5, 0.0]))   # ... and summed; the stored zero is an entry
    np.testing.assert_array_equal(sp.csr_matrix((values, indices, indptr), shape=(4, 5)).toarray(), dense)
    np.testing.assert_array_equal(m.row, ROWS)
    np.testing.assert_array_equal(m.data, VALS)


@pytest.mark.parametrize("make", [lambda: coo().tocsc(), lambda: sp.csr_array(coo()), lambda: coo().tolil()], ids=["csc", "csr_array", "lil"])
def test_other_formats_and_arrays_are_accepted(make):
    m = make()
    assert _is_sparse(m) and not _is_sparse(m.toarray())
    indptr, indices, values = _csr_rows(m, 5)
    np.testing.assert_array_equal(sp.csr_matrix((values, indices, indptr), shape=(4, 5)).toarray(), coo().toarray())


def test_unsorted_csr_is_copied_not_modified():
    m = sp.csr_matrix((np.float64([1, 2, 3]), np.array([3, 0, 1]), np.array([0, 2, 3])), shape=(2, 4))
    assert not m.has_sorted_indices
    indptr, indices, values = _csr_rows(m, 4)
    np.testing.assert_array_equal(indices, [0, 3, 1])
    np.testing.assert_array_equal(values, np.float32([2, 1, 3]))
    np.testing.assert_array_equal(m.indices, [3, 0, 1])               # the caller's matrix: as it was
    np.testing.assert_array_equal(m.data, [1, 2, 3])


def test_wrong_column_count_gives_the_references_message():
    with pytest.raises(ValueError, match=r"^Received 5 features, expected 7\.$"):
        _csr_rows(coo(), 7)
