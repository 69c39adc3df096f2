"""exact_select2_kernel and exact_tiles_kernel (csrc/bmu_exact.hpp) through som_debug_exact_select2 and som_debug_exact_tiles,
against NumPy models.  GPU only (`-m gpu`).

select2 compacts every group's list in place, 1 024 entries a turn (four a thread), the next turn's entries loaded before the
turn's barrier: the list lengths sit around one wave's, one 256-step's, one turn's and several turns' ends, with empty groups
between full ones, and the keep patterns move the survivors to where a turn's writes come closest to what is still to be
read (all kept), leave a turn without any, or with only its first or its last entry.  Checked: the survivors and their
order, gcount, kept_total, and that nothing at or behind a list's old end was written.

The tile table is written a thread per entry, which finds its group by binary search over the threads' tile prefixes:
compared entry by entry with a Python loop over the groups, on maps of one group per thread and of three (2 500 groups), with
and without gstart, on grids of 1 and 16 workgroups, and with the capacity exceeded (overflow raised, no tile written)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 255, 256, 257, 1023, 1024, 1025, 2049, 4100)
TURN = 1024
TILE = 128          # EX_TR, csrc/exact_scratch.hpp
PATTERNS = ("none", "all", "alternating", "first_of_turn", "last_of_turn", "thr2_all_ones")


@pytest.fixture(scope="module")
def eng():
    from xpysom_dask_amd.engine import HipEngine
    e = HipEngine(4, 4, 3, precision="f32")
    yield e
    e.close()


def keep_mask(pattern, n):
    i = np.arange(n)
    if pattern == "none":
        return np.zeros(n, bool)
    if pattern in ("all", "thr2_all_ones"):
        return np.ones(n, bool)
    if pattern == "alternating":
        return i % 2 == 0
    if pattern == "first_of_turn":
        return i % TURN == 0
    if pattern == "last_of_turn":
        return (i % TURN == TURN - 1) | (i == n - 1)
    raise ValueError(pattern)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_select2_compacts_in_place_and_in_order(eng, pattern):
    rng = np.random.RandomState(77)
    counts = np.zeros(2 * len(LENGTHS) + 1, np.int32)       # an empty group before, between and behind the full ones
    counts[1::2] = LENGTHS
    n_groups, stride, n_rows = counts.size, max(LENGTHS) + 5, 6000
    plist = np.full((n_groups, stride), -7, np.int32)        # (behind a list's end: never read, never written)
    rmin = rng.randint(0, 1 << 32, size=(n_groups, stride), dtype=np.uint64).astype(np.uint32)
    if pattern == "thr2_all_ones":
        thr2 = np.full(n_rows, 0xFFFFFFFF, np.uint32)        # (nothing bounds the row: every pair stays, whatever its minimum)
    else:
        thr2 = (0x3F000000 + 16 * rng.permutation(n_rows)).astype(np.uint32)
    want = []
    for g, c in enumerate(counts):
        rows = rng.randint(0, n_rows, c).astype(np.int32)
        plist[g, :c] = rows
        keep = keep_mask(pattern, c)
        if pattern == "thr2_all_ones":
            rmin[g, :c:3] = 0xFFFFFFFF                          # (equal to the threshold: kept)
        else:
            below = thr2[rows] - rng.randint(0, 3, c).astype(np.uint32)      # (<=: equality keeps)
            above = thr2[rows] + rng.randint(1, 4, c).astype(np.uint32)
            rmin[g, :c] = np.where(keep, below, above)
        want.append(rows[keep])
    got, gcount, kept = eng.debug_exact_select2(plist, rmin, counts, thr2)
    for g, c in enumerate(counts):
        w = want[g]
        what = "%s, group %d of %d entries" % (pattern, g, c)
        assert gcount[g] == w.size, "%s: gcount %d, want %d" % (what, gcount[g], w.size)
        bad = np.flatnonzero(got[g, :w.size] != w)
        assert bad.size == 0, "%s: %d survivors differ, first at %d" % (what, bad.size, bad[0])
        assert (got[g, c:] == -7).all(), "%s: written at or behind the list's end" % what
    assert kept == sum(w.size for w in want), "%s: kept_total %d" % (pattern, kept)


def tiles_model(gcount, gstart, stride):
    tab, pairs = [], 0
    for g in range(len(gcount)):
        first = 0 if gstart is None else int(gstart[g])
        c = int(gcount[g]) - first
        pairs += c
        for i in range((c + TILE - 1) // TILE):
            tab.append((g, g * stride + first + i * TILE, min(TILE, c - i * TILE), 0))
    return np.array(tab, np.int32).reshape(-1, 4), pairs


def tile_lengths():
    s = set()
    for n in LENGTHS:
        s.update(m for m in (n - 1, n, n + 1) if m >= 0)
    return sorted(s)


def tile_counts(n_groups):
    """The lengths and their neighbours in turn, an empty group after every third."""
    lens = tile_lengths()
    out = np.zeros(n_groups, np.int32)
    k = 0
    for g in range(n_groups):
        if g % 4 != 3:
            out[g] = lens[k % len(lens)]
            k += 1
    return out


@pytest.mark.parametrize("with_gstart", (False, True))
@pytest.mark.parametrize("blocks", (1, 16))
@pytest.mark.parametrize("n_groups", (40, 2500))
def test_tile_table_entry_by_entry(eng, n_groups, blocks, with_gstart):
    rng = np.random.RandomState(5)
    gcount = tile_counts(n_groups)
    stride = int(gcount.max()) + 3
    gstart = None
    if with_gstart:
        gstart = np.array([rng.choice((0, c, rng.randint(0, c + 1), max(c - TILE, 0))) for c in gcount], np.int32)
    want, pairs = tiles_model(gcount, gstart, stride)
    entries = len(want) + 37
    tab, out3, gso = eng.debug_exact_tiles(gcount, stride, pairs, blocks, entries, gstart=gstart, want_gstart_out=True)   # capacity = the pairs exactly
    assert out3.tolist() == [len(want), 0, pairs], "n_tiles, overflow, pairs = %r, want %r" % (out3.tolist(), [len(want), 0, pairs])
    bad = np.flatnonzero((tab[:len(want)] != want).any(axis=1))
    assert bad.size == 0, "%d entries differ, first %d: %r, want %r" % (bad.size, bad[0], tab[bad[0]].tolist(), want[bad[0]].tolist())
    assert (tab[len(want):] == -1).all(), "written behind the table's last entry"
    assert np.array_equal(gso, gcount), "gstart_out is not the lists' lengths"


@pytest.mark.parametrize("blocks", (1, 16))
def test_tile_table_overflow_writes_no_tile(eng, blocks):
    gcount = tile_counts(40)
    stride = int(gcount.max()) + 3
    want, pairs = tiles_model(gcount, None, stride)
    tab, out3, gso = eng.debug_exact_tiles(gcount, stride, pairs - 1, blocks, len(want), want_gstart_out=True)
    assert out3.tolist() == [0, 1, pairs]
    assert (tab == -1).all(), "tiles written although the pass overflowed"
    assert (gso == -1).all(), "gstart_out written although the pass overflowed"
