"""A direct-form float64 reference of the neighbourhood on the TOROIDAL topology (no reference implementation has one: the
semantics are the project's own, include/somhip.h and DESIGN.md 3.2).

Shared by tests/test_torus_cpu.py and tests/test_gpu_torus.py (not a conftest).  `make_h` returns h_of(units) -> (n, K)
rows of h(b -> k) times eta, and the magnitude rows that go with them, for tests/update_ref.py's accumulate /
check_accumulators / check_merge.  h is evaluated per pair of units from the wrapped offsets; it shares no table, term or
range with csrc/update.hpp.

  offset        delta = (n - c) - L * round((n - c) / L) per axis: the nearest image, |delta| <= L / 2, ONE image
  gaussian      exp(-dx^2 / d) * exp(-dy^2 / d)                                  d = 2 std_coeff^2 sigma^2
  mexican_hat   ex (1 - 2 dx^2 / d) * ey  -  ex * (2 dy^2 / d) ey
  bubble        [-sigma < dx < sigma] * [-sigma < dy < sigma]
  triangle      max(sigma - |dx|, 0) * max(sigma - |dy|, 0)
  compact       gaussian and triangle times the bubble's mask
  wide          float64 throughout (a NumPy-scalar sigma; triangle always); otherwise the exponent's argument is rounded to
                float32 before a float64 exp, as the rectangular topology evaluates it
"""
import numpy as np

F32, F64 = np.float32, np.float64


def wrapped_offset(n, c, L):
    """Nearest-image offset of coordinates n from c on a ring of L (float64; the tie |delta| = L / 2 takes round's sign)."""
    d = np.asarray(n, F64) - np.asarray(c, F64)
    return d - L * np.round(d / L)


def _exp(d2, d, wide):
    if wide:
        return np.exp(-d2 / d)
    return np.exp((-(d2.astype(F32)) / F32(d)).astype(F64))


def _axis(L, c, sigma, d, wide, neighbourhood, compact):
    """(factor, |factor| terms) of one axis for BMU coordinates c (n,): arrays (n, L); mexican_hat returns (e, q)."""
    dl = wrapped_offset(np.arange(L)[None, :], np.asarray(c)[:, None], L)
    box = ((dl > -sigma) & (dl < sigma)).astype(F64)
    if neighbourhood == "bubble":
        return box
    if neighbourhood == "triangle":
        v = np.maximum(sigma - np.abs(dl), 0.0)
        return v * box if compact else v
    e = _exp(dl * dl, d, wide)
    if neighbourhood == "gaussian":
        return e * box if compact else e
    return e, (2.0 / d) * (dl * dl)                    # mexican_hat


def make_h(X, Y, neighbourhood, compact, std_coeff, sigma, eta, wide):
    """(h_of, habs_of) for update_ref.accumulate: units -> (n, K) float64.  habs_of: the magnitudes a float32 evaluation
    rounds in proportion to -- |h|, and for the mexican hat the sum of the two terms it is the difference of."""
    if neighbourhood == "mexican_hat" and compact:
        raise ValueError("mexican_hat with compact_support is not defined on the toroidal topology")
    wide = wide or neighbourhood == "triangle"
    sigma = float(sigma)
    d = 2.0 * std_coeff ** 2 * sigma ** 2
    eta = float(eta)

    def both(units):
        units = np.asarray(units, np.int64)
        fx = _axis(X, units // Y, sigma, d, wide, neighbourhood, compact)
        fy = _axis(Y, units % Y, sigma, d, wide, neighbourhood, compact)
        if neighbourhood == "mexican_hat":
            (ex, qx), (ey, qy) = fx, fy
            e = ex[:, :, None] * ey[:, None, :]
            q = qx[:, :, None] + qy[:, None, :]
            # ex (1 - qx) ey - ex qy ey = e (1 - q); the two terms' magnitudes: e + e q
            return (eta * e * (1.0 - q)).reshape(len(units), X * Y), (abs(eta) * (e + e * q)).reshape(len(units), X * Y)
        h = eta * fx[:, :, None] * fy[:, None, :]
        return h.reshape(len(units), X * Y), np.abs(h).reshape(len(units), X * Y)

    return (lambda u: both(u)[0]), (lambda u: both(u)[1])


def reference_update(data, bmu, X, Y, eta, sigma, *, wide, neighbourhood="gaussian", compact=False, std_coeff=0.5):
    """update_ref.reference_update's (num, den, mag_num, mag_den) for the toroidal topology."""
    from tests import update_ref as U
    units, S, A, c = U.segment_sums(data, bmu)
    h_of, habs_of = make_h(X, Y, neighbourhood, compact, std_coeff, sigma, eta, wide)
    return U.accumulate(S, A, c, units, X * Y, h_of, habs_of)
