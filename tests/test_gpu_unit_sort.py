"""The sort by unit on the device: WHICH of the two sorts ran (som_debug_unit_sort_stats, the handle's counters) against the rule
(csrc/unit_sort.hpp, restated once in update_ref.sort_path and pinned to the library by tests/test_unit_sort_cpu.py), and what
the per-unit kernels make of its output against the float64 models of tests/diag_ref.py and tests/project_ref.py.  GPU only
(`-m gpu`).  Both sorts are stable and give the same order, so only the counters can tell a drifted threshold."""
import numpy as np
import pytest

from tests import diag_ref as R
from tests import project_ref as P
from tests import query_ref as Q
from tests import update_ref as U

pytestmark = pytest.mark.gpu

F32 = np.float32


def engine(X, Y, D, **kw):
    from xpysom_dask_amd.engine import HipEngine
    return HipEngine(X, Y, D, precision="f32", **kw)


def rows_and_units(X, Y, D, n, seed):
    x = Q.make_rows("blobs", n, D, seed)
    return x, Q.make_units("blobs", x, X * Y, D, seed, 0)


def check_stats_call(e, x, w, K, what):
    """One som_unit_stats call, checked as tests/test_gpu_diag.py checks it: the distances against the float64 distances to the
    returned units, the four per-unit arrays against the model on the returned ids and distances."""
    ids, d = e.bmu_distances(x)
    R.check_distances(d, x, w, ids, what=what)
    R.check_unit_stats(e.unit_stats(x), ids, d, K, what=what)


def ran(e, before):
    """The sort that ran since `before` (one sort): 'counting' or 'radix'."""
    c, r = e.unit_sort_stats()
    assert (c - before[0], r - before[1]) in ((1, 0), (0, 1)), "not one sort: %r after %r" % ((c, r), before)
    return "counting" if c > before[0] else "radix"


def test_query_scratch_across_capacities():
    """One handle, 8 x 8 units, som_unit_stats on 1500, 2048, 5000, 2047, 3000 rows: a capacity of 2 048 holds a table but 1 500
    rows are under two blocks (radix); counting at exactly two blocks; a regrow to 5 120; one row under the floor (radix);
    three blocks inside the five-block table (counting, the totals row at B * K, not at cs_blocks * K).  Then
    som_unit_label_counts at 3 000 rows: the same buffers, no regrow, counting."""
    X, Y, D = 8, 8, 3
    K = X * Y
    x, w0 = rows_and_units(X, Y, D, 5000, 11)
    e = engine(X, Y, D)
    try:
        e.set_weights(w0)
        w = e.get_weights()
        paths = []
        for n in (1500, 2048, 5000, 2047, 3000):
            before = e.unit_sort_stats()
            check_stats_call(e, x[:n], w, K, "8x8x3 n=%d" % n)
            paths.append(ran(e, before))
            assert paths[-1] == U.sort_path(K, n), "n=%d: the %s sort ran" % (n, paths[-1])
        assert paths == ["radix", "counting", "counting", "radix", "counting"]
        n, C = 3000, 3
        labels = np.random.RandomState(5).randint(0, C, n).astype(np.int32)
        before = e.unit_sort_stats()
        counts = e.label_counts(x[:n], labels, C)
        assert ran(e, before) == "counting"
        want = P.label_counts_model(e.bmu(x[:n]), labels, K, C)
        assert np.array_equal(counts, want), "label counts differ from the model at %r" % np.argwhere(counts != want)[:5].tolist()
    finally:
        e.close()


@pytest.mark.parametrize("n, path", [(262144, "counting"), (262145, "radix")])
def test_the_tables_ceiling_on_the_query_side(n, path):
    """128 x 64 = 8 192 units: 256 blocks of rows x 8 192 units is the table's ceiling of 2^21 counts exactly; one row more is a
    257th block and the radix sort."""
    X, Y, D = 128, 64, 4
    K = X * Y
    assert U.sort_path(K, n) == path
    x, w0 = rows_and_units(X, Y, D, n, 13)
    e = engine(X, Y, D)
    try:
        e.set_weights(w0)
        ids, d = e.bmu_distances(x)
        before = e.unit_sort_stats()
        assert before == (0, 0)
        R.check_unit_stats(e.unit_stats(x), ids, d, K, what="128x64x4 n=%d" % n)
        assert ran(e, before) == path
    finally:
        e.close()


def test_streamed_chunks(monkeypatch):
    """One streamed epoch on 12 x 11 x 5, pageable chunks of 3000, 1000, 5000, 2048 rows: the chunk scratch starts at 3 072 rows
    (a three-block table), takes the radix sort for the 1 000 rows under two blocks and grows to 5 120 in mid-epoch.  Under
    SOM_COUNTING_SORT=0 every chunk takes the radix sort; numerator and denominator are bitwise the same, as are the ids the
    two handles' searches give the rows."""
    X, Y, D = 12, 11, 5
    K = X * Y
    sizes = (3000, 1000, 5000, 2048)
    x, w0 = rows_and_units(X, Y, D, sum(sizes), 17)
    cuts = np.cumsum((0,) + sizes)
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("SOM_COUNTING_SORT", mode)
        e = engine(X, Y, D)
        try:
            e.set_weights(w0)
            e.stream_epoch_accumulate([x[a:b] for a, b in zip(cuts[:-1], cuts[1:])], 2.0, 0.5, False)
            num, den, _ = e.epoch_fetch(want_bmu=False)
            outs[mode] = (num, den, e.bmu(x), e.unit_sort_stats())
        finally:
            e.close()
    want = [U.sort_path(K, n) for n in sizes]
    assert want == ["counting", "radix", "counting", "counting"]
    assert outs["1"][3] == (3, 1) and outs["0"][3] == (0, 4)
    for name, a, b in zip(("numerator", "denominator", "ids"), outs["1"], outs["0"]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s differs between the two sorts" % name
