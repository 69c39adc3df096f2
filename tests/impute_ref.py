"""The bit-exact model of `XPySom.impute` / som_impute* (include/somhip.h): out = x where observed, W[ids] where NaN.

Shared by tests/test_impute_cpu.py and tests/test_gpu_impute.py (not a conftest).  The call does no arithmetic on a value,
so the model is one np.where and every comparison is an equality of bits.  None of this shares code with csrc/.
"""
import numpy as np

F32 = np.float32


def bits(a):
    """The uint32 image of float32 values: NaN payloads and the sign of a zero count."""
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def impute_reference(x, w, ids):
    """float32 (N, D): x where it is not a NaN (bit for bit), else the value of row ids[n] of the (K, D) codebook w."""
    x32 = np.ascontiguousarray(x, dtype=F32)
    w32 = np.ascontiguousarray(w, dtype=F32).reshape(-1, x32.shape[-1])
    fill = w32[np.asarray(ids, np.int64)]
    return np.where(np.isnan(x32), fill.reshape(x32.shape), x32)


def first_difference(a, b):
    """(row, feature, bits of a, bits of b) of the first element whose bits differ, or None."""
    ua, ub = bits(a), bits(b)
    bad = np.argwhere(ua != ub)
    if not len(bad):
        return None
    i = tuple(bad[0])
    return i + (hex(int(ua[i])), hex(int(ub[i])))
