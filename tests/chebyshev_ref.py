"""The NumPy model of activation_distance='chebyshev': ids = argmin_k max_d |float32(x_nd - w_kd)|, first minimum wins; a
row holding a NaN or an infinity gets unit 0."""
import numpy as np

F32, F64 = np.float32, np.float64


def distances(x, w, dtype=F32, block=64):
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    out = np.empty((x.shape[0], w.shape[0]), dtype)
    with np.errstate(invalid="ignore"):
        for i in range(0, x.shape[0], block):
            out[i:i + block] = np.abs(x[i:i + block, None, :] - w[None, :, :]).max(axis=2)
    return out


def bmu(x, w):
    ids = np.argmin(distances(x, w), axis=1).astype(np.int32)
    ids[~np.isfinite(np.asarray(x, F32)).all(axis=1)] = 0
    return ids


def planted_case(X, Y, D, N, seed=0):
    """(rows, codebook) with a unit duplicated at a higher id in the same and in another 128-unit block, a row equal to that
    unit, a zero row, a NaN row and rows holding +inf and -inf.  The codebook and the even rows lie on a grid of 1/8 (plenty
    of exact ties); the odd rows are continuous (their differences round)."""
    rs = np.random.RandomState(seed)
    K = X * Y
    w = (rs.randint(-16, 17, (K, D)) / 8).astype(F32)
    x = (rs.randint(-16, 17, (N, D)) / 8).astype(F32)
    x[1::2] = rs.randn(len(x[1::2]), D).astype(F32)
    w[min(5, K - 1)] = w[2]
    w[K - 1] = w[2]
    x[0] = w[2]
    x[1] = 0
    x[2, D // 2] = np.nan
    x[3, 0] = np.inf
    x[N - 1, D - 1] = -np.inf
    return x, w
