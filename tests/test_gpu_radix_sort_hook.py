"""The stable radix sort of csrc/update.hpp (rs_hist, rs_scan, rs_scatter) through som_debug_radix_sort, against
np.argsort(kind='stable'): sorted keys AND the items' indices, exactly.  GPU only (`-m gpu`).

The scatter kernel ranks an item inside its wave by ballots, leaves every (256-step, wave)'s count of each digit in an LDS cell and
lets the digit's thread turn the 32 cells of a 2 048-item block into first destinations.  The sizes sit around one wave, one step,
one block and several blocks with a ragged tail; the key patterns put all items on one digit (one digit owns every cell), change
the digit per lane, per wave and per step (the three levels the destinations are composed over), and separate the passes (equal low
byte with distinct high byte, and the reverse: a pass that is not stable, or that reads the other pass's digit, shows there)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 255, 256, 257, 2047, 2048, 2049, 5 * 2048 + 3, 70001)
BITS = (1, 8, 9, 16, 20)


def _equal(n, mask, rng):
    return np.full(n, 0xA5A5A5 & mask)


def _descending(n, mask, rng):
    return (n - 1 - np.arange(n)) & mask


def _alternating(period):
    def make(n, mask, rng):
        return np.where((np.arange(n) // period) % 2 == 0, mask, mask >> 1)     # (the larger key first)
    return make


def _random(n, mask, rng):
    return rng.randint(0, mask + 1, n)


def _equal_low_byte(n, mask, rng):
    return (((np.arange(n) * 7919) << 8) | 0x5A) & mask


def _equal_high_bytes(n, mask, rng):
    return (mask & ~0xFF) | (rng.randint(0, 256, n) & mask)


PATTERNS = {
    "all_equal": _equal,
    "descending": _descending,
    "two_digits_per_lane": _alternating(1),
    "two_digits_per_wave": _alternating(64),
    "two_digits_per_step": _alternating(256),
    "random": _random,
    "equal_low_byte": _equal_low_byte,
    "equal_high_bytes": _equal_high_bytes,
}


@pytest.fixture(scope="module")
def eng():
    from xpysom_dask_amd.engine import HipEngine
    e = HipEngine(4, 4, 3, precision="f32")
    yield e
    e.close()


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_radix_sort_matches_stable_argsort(eng, pattern):
    rng = np.random.RandomState(1234)
    for bits in BITS:
        mask = (1 << bits) - 1
        for n in SIZES:
            keys = np.asarray(PATTERNS[pattern](n, mask, rng)).astype(np.int32)
            assert keys.shape == (n,) and keys.min() >= 0 and keys.max() <= mask
            order = np.argsort(keys, kind="stable").astype(np.int32)
            ko, vo = eng.debug_radix_sort(keys, bits)
            what = "%s, n=%d, bits=%d" % (pattern, n, bits)
            bad = np.flatnonzero(vo != order)
            assert bad.size == 0, "%s: %d indices differ, first at %d: %d, want %d" % (what, bad.size, bad[0], vo[bad[0]], order[bad[0]])
            assert np.array_equal(ko, keys[order]), "%s: the keys differ from the sorted keys" % what
