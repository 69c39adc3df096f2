"""The row kernels past 2^31 elements (2^32 bytes) of one row set, and past 2^24 rows on one unit.  GPU only (`-m gpu`).

include/somhip.h promises up to 2^31 - 1 rows per row set and per call; every kernel that walks rows forms row * pitch.  The
rows are generated in HBM (tests/extent_ref.py), go in through set_data_device and the *_device calls only, and everything
row-sized is checked there: on all N rows by the float64 torch references of extent_ref (the inequalities of query_ref,
diag_ref and update_ref restated on tensors; tests/test_extent_cpu.py holds the two forms equal), and by the NumPy checks
themselves on the boundary windows -- the first and last 4096 rows, the rows around element 2^31 and byte 2^32 of the float32
and of the 16-bit image, and every 4099th row.  No shape below the boundary can stand in for these: test_extent_cpu.py shows
on a model engine that a wrapped offset, a truncated row id and a float32 count pass every check until N crosses it.

  A   16 x 8 map, D = 128, N = 2^24 + 2^17 + 3 rows (2^31 + 1.7e7 elements, 8.65 GB): the vector-load paths, the resident
      float32 kernel, the k16 screen; SOM_EXACT_SKIP=2, so sort, gather, scout, plan, lists, select, refine and re-score run
      -- and a copy with 3 % of the features NaN and one all-NaN row inside each boundary window for a handle with missing
      values (masked search, [x~ | m] accumulators and merge, masked QE)
  B   16 x 8 map, D = 136, N = ceil(2^31 / 136) + 2^17 + 1: the tiled float32 kernel and its top-2 form; a 64 x 64 map on
      the same rows for the wide screen, wide_gather_sorted_kernel and the K-looped re-score
  C   8 x 8 map, D = 2, N = 2^24 + 4097: every row forced onto one unit -- one run open across every chunk, workgroup and
      level of the run sum, a count beyond float32's integers
  R   129 x 64 map, D = 4, N = 2^24 + 3: the radix sort with row ids beyond 24 bits

One data set lives at a time (the `sets` fixture frees the previous one), one engine at a time, closed in `finally`.  Every
test prints its wall time, torch's peak allocation and the engine's own footprint (from the free-memory difference).

Not here, on purpose: a streamed epoch (its chunks are bounded by the staging buffers and cannot cross the boundary) and
som_epoch_accumulate_faithful (K * N * D work).
"""
import contextlib
import time

import numpy as np
import pytest

from oracle import som_oracle as O
from tests import diag_ref
from tests import extent_ref as R
from tests import project_ref
from tests import query_ref as Q
from tests import update_ref as U
from tests import weights_ref

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SETS = {
    "A": dict(X=16, Y=8, D=128, N=2 ** 24 + 2 ** 17 + 3, seed=101),
    "B": dict(X=16, Y=8, D=136, N=-(-2 ** 31 // 136) + 2 ** 17 + 1, seed=202),
    "C": dict(X=8, Y=8, D=2, N=2 ** 24 + 4097, seed=303),
    "R": dict(X=129, Y=64, D=4, N=2 ** 24 + 3, seed=404),
}
SIGMA, ETA = 2.0, 0.5
EPOCHS = 3


def engine(*a, **kw):
    from xpysom_dask_amd.engine import HipEngine
    return HipEngine(*a, **kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


class RowSet:
    def __init__(self, name):
        import torch
        c = SETS[name]
        self.name, self.X, self.Y, self.D, self.N = name, c["X"], c["Y"], c["D"], c["N"]
        self.K = self.X * self.Y
        self.x, self.centres = R.rows_on_device(self.N, self.D, c["seed"])
        self.w0 = R.codebook_near(self.centres, self.X, self.Y, c["seed"] + 1)
        self.cache = {}
        if self.N * self.D > 2 ** 31:
            self.win = R.boundary_windows(self.N, self.D)
            self.rows = R.window_rows(self.win, self.N)
            self.x_win = self.x[torch.from_numpy(self.rows).cuda()].cpu().numpy()
            self.beyond = "N*D = %d > 2^31; window rows %d, beyond 2^30 elements (2^32 bytes) %d, beyond 2^31 elements %d" % (
                self.N * self.D, len(self.rows), R.rows_beyond(self.rows, self.D, 2 ** 30), R.rows_beyond(self.rows, self.D, 2 ** 31))

    def dev(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def windows(self):
        return [v for k, v in self.win.items() if k != "stride"]

    def masked(self):
        """(rows with 3 % of the features NaN and one row of each boundary window NaN throughout, those rows, the window rows
        of the copy on the host), built on first use and held with the set."""
        import torch
        if "masked" not in self.cache:
            empty = np.array(sorted((lo + hi) // 2 + 1 for lo, hi in self.windows()), np.int64)
            xm = R.punch_on_device(self.x, SETS[self.name]["seed"] + 3, empty_rows=empty)
            self.cache["masked"] = (xm, empty, xm[torch.from_numpy(self.rows).cuda()].cpu().numpy())
        return self.cache["masked"]

    def codebook(self, X, Y):
        return self.w0 if (X, Y) == (self.X, self.Y) else R.codebook_near(self.centres, X, Y, SETS[self.name]["seed"] + 2)


@pytest.fixture(scope="module")
def sets():
    """sets(name): the row set `name`, built on first use; the one held before it is freed first."""
    import torch
    held = {}

    def get(name):
        if name not in held:
            held.clear()
            torch.cuda.empty_cache()
            held[name] = RowSet(name)
        return held[name]
    yield get
    held.clear()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def running(ds, what, precision="f32", X=None, Y=None, resident=True, rows=None, **kw):
    """An engine on the row set (codebook set, rows resident -- `rows`: a copy of the set's rows to hold instead), closed in
    `finally`; prints time, peak and footprint."""
    import torch
    X, Y = X or ds.X, Y or ds.Y
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    free0, reserved0 = torch.cuda.mem_get_info()[0], torch.cuda.memory_reserved()
    t0 = time.time()
    e = engine(X, Y, ds.D, precision=precision, **kw)
    foot = [0]

    def footprint():
        foot[0] = max(foot[0], (free0 - torch.cuda.mem_get_info()[0]) - (torch.cuda.memory_reserved() - reserved0))
    e.footprint = footprint
    try:
        e.set_weights(ds.codebook(X, Y))
        if resident:
            held = ds.x if rows is None else rows
            e.set_data_device(held.data_ptr(), ds.N, keepalive=held)
        yield e
        e.sync()
        footprint()
    finally:
        e.close()
        print("%s [%s, %s]: %.2f s, torch peak %.2f GB, engine footprint %.2f GB" % (
            what, ds.name, getattr(ds, "beyond", "N = %d" % ds.N), time.time() - t0,
            torch.cuda.max_memory_allocated() / 1e9, foot[0] / 1e9))


def check_search(ds, ids, mode, what, w=None, every=1):
    """Picks admissible on all N rows (torch) and by query_ref.check_picks on the boundary windows; on the set's own
    codebook the BMUs must also spread over the whole map and the bound must decide 99 rows in a hundred (a trained codebook
    has closer units; there the share is printed)."""
    spread = w is None
    w = ds.w0 if w is None else w
    assert ids.shape == (ds.N,) and ids.dtype == np.int32
    worst, share, seen = R.check_picks_all_rows(ds.dev(ids), ds.x, ds.dev(w), mode, what, every=every, max_undecided=0.01 if spread else 1.0)
    if mode == "quant":
        Q.check_picks(ids[ds.rows], *Q.scores(ds.x_win, w, "sqrt"), what + " (windows, sqrt bound)")
        s, E = R.widen_for_sqrt(*Q.scores(ds.x_win, w, "sq"))
    else:
        s, E = Q.scores(ds.x_win, w, mode)
    ww = Q.check_picks(ids[ds.rows], s, E, what + " (windows)")
    print("%s: %d rows, worst err / bound %.3g (windows: %.3g), undecided share %.3g, distinct BMUs %d" % (
        what, seen, worst, ww, share, len(np.unique(ids))))
    assert not spread or len(np.unique(ids)) >= 0.9 * len(w)


# ------------------------------------------------------------------------------------------------------ float32 search
def run_f32_search(ds):
    with running(ds, "float32 resident epoch + query") as e:
        e.epoch_accumulate(SIGMA, ETA, False)
        ids_epoch = e.epoch_fetch()[2]
        e.footprint()
        ids_query = e.bmu_device(ds.x.data_ptr(), ds.N)
    check_search(ds, ids_epoch, "part", "resident epoch ids")
    check_search(ds, ids_query, "part", "bmu_device ids")


def run_f32_qe(ds):
    with running(ds, "quantization_error_device", resident=False) as e:
        qe = e.quantization_error_device(ds.x.data_ptr(), ds.N)
        ids = e.bmu_device(ds.x.data_ptr(), ds.N, quantization=True)
    check_search(ds, ids, "quant", "quantization ids")
    ratio = R.check_qe_t(qe, ds.x, ds.dev(ds.w0), ds.dev(ids), "QE")
    print("QE %r: err / bound %.3g" % (qe, ratio))


def run_top2(ds):
    with running(ds, "bmu_top2_device", resident=False) as e:
        a, b = e.bmu_top2_device(ds.x.data_ptr(), ds.N)
    worst = R.check_top2_all_rows(ds.dev(a), ds.dev(b), ds.x, ds.dev(ds.w0), "top-2")
    s, E = Q.scores(ds.x_win, ds.w0, "sqrt")
    ww = Q.check_top2(a[ds.rows], b[ds.rows], s, E, "top-2 (windows)")
    print("top-2: %d rows, worst err / bound %.3g (windows: %.3g)" % (ds.N, worst, ww))


def f32_trajectory(ds, X, Y):
    """EPOCHS resident epochs of a float32 engine: ids of every epoch, the merged codebook, and a query on it (cached)."""
    if ("traj", X, Y) not in ds.cache:
        with running(ds, "float32 trajectory, %d epochs" % EPOCHS, X=X, Y=Y) as e:
            ids = []
            for t in range(EPOCHS):
                e.epoch(O.exponential_decay(SIGMA, 1.0, t, EPOCHS), O.exponential_decay(ETA, 0.01, t, EPOCHS), True)
                ids.append(e.epoch_fetch()[2])
            w = e.get_weights()
            q = e.bmu_device(ds.x.data_ptr(), ds.N)
        ds.cache["traj", X, Y] = (ids, w, q)
    return ds.cache["traj", X, Y]


def run_exact(ds, monkeypatch, planned, X=None, Y=None, every=1):
    X, Y = X or ds.X, Y or ds.Y
    ids32, w32, q32 = f32_trajectory(ds, X, Y)
    check_search(ds, q32, "part", "float32 query on the trained codebook", w=w32, every=every)
    monkeypatch.setenv("SOM_EXACT_SKIP", "2")
    with running(ds, "exact, %d resident epochs + query" % EPOCHS, precision="exact", X=X, Y=Y) as e:
        for t in range(EPOCHS):
            e.epoch(O.exponential_decay(SIGMA, 1.0, t, EPOCHS), O.exponential_decay(ETA, 0.01, t, EPOCHS), True)
            ids = e.epoch_fetch()[2]
            bad = np.flatnonzero(ids != ids32[t])
            assert len(bad) == 0, "epoch %d: %d rows leave the float32 BMUs, first row %d: %d against %d" % (
                t, len(bad), bad[0], ids[bad[0]], ids32[t][bad[0]])
            e.footprint()
        w = e.get_weights()
        q = e.bmu_device(ds.x.data_ptr(), ds.N)
        stats = dict(resident=e.exact_resident_stats(), skip=e.exact_skip_stats(), exact=e.exact_stats(), scout=e.exact_scout_stats())
    print("exact: %r" % (stats,))
    assert np.array_equal(bits(w), bits(w32)), "the merged codebook leaves the float32 engine's"
    bad = np.flatnonzero(q != q32)
    assert len(bad) == 0, "query: %d rows leave the float32 BMUs, first row %d" % (len(bad), bad[0] if len(bad) else -1)
    if planned:
        assert stats["resident"][0] >= 2, "the second and third epoch must run under a plan: %r" % (stats,)
        assert stats["skip"][0] < stats["skip"][1], "no block was skipped: %r" % (stats,)
        assert stats["exact"][0] >= EPOCHS * ds.N, "the screen did not serve every epoch: %r" % (stats,)
        assert stats["exact"][1] == 0, "rows went to the float32 fallback: %r" % (stats,)
        assert stats["scout"][0] >= 1, "the query did not run the scout: %r" % (stats,)


# ------------------------------------------------------------------------------------------------------ update chain
def run_forced_update(ds, what, X=None, Y=None, bmu=None, weights=None, merge=True):
    import torch
    X, Y = X or ds.X, Y or ds.Y
    K = X * Y
    bmu = R.forced_bmus(ds.N, K) if bmu is None else bmu
    w0 = ds.codebook(X, Y)
    with running(ds, what, X=X, Y=Y) as e:
        if weights is not None:
            e.set_sample_weights(weights)
        e.epoch_accumulate_forced(bmu.numpy(), SIGMA, ETA, True)
        num, den, _ = e.epoch_fetch(want_bmu=False)
        e.footprint()
        e.epoch_accumulate_forced(bmu.numpy(), SIGMA, ETA, True)
        num2, den2, _ = e.epoch_fetch(want_bmu=False)
        w1 = None
        if merge:
            e.epoch_merge()
            w1 = e.get_weights()
    assert np.array_equal(bits(num), bits(num2)) and np.array_equal(bits(den), bits(den2)), "%s: a second accumulate differs" % what
    S, A, c = R.segment_sums_t(ds.x, bmu.cuda(), K, None if weights is None else torch.from_numpy(weights).cuda())
    ref = R.reference_from_sums(S, A, c, X, Y, ETA, SIGMA, True)
    a = U.check_accumulators(num, den, ref, what)
    m = U.check_merge(w0, w1, num, den, ref, False, what) if merge else 0.0
    print("%s: rows per unit %d .. %d; worst err / bound: accumulators %.3g, merge %.3g" % (what, c.min(), c.max(), a, m))
    return num, den, c


# ====================================================================================================== set A
def test_a_float32_resident_epoch_and_query(sets):
    run_f32_search(sets("A"))


def test_a_quantization_error(sets):
    run_f32_qe(sets("A"))


def test_a_top2(sets):
    run_top2(sets("A"))


def test_a_exact_three_epochs_under_a_plan(sets, monkeypatch):
    run_exact(sets("A"), monkeypatch, planned=True)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_a_half_precision_resident_epoch(sets, kind):
    """One resident epoch of the 16-bit search: picks within half_ref's E on the boundary windows and the stride sample.  E
    takes the largest rounded row norm of the LAUNCH: the row that attains it over all N rows is found on the device and
    joins the sample, so the sample's maximum is the launch's."""
    import torch
    from tests import half_ref as H
    ds = sets("A")
    with running(ds, "%s resident epoch" % kind, precision=kind) as e:
        e.epoch_accumulate(SIGMA, ETA, False)
        ids = e.epoch_fetch()[2]
    top, arg = -1.0, 0
    for s, t in R.slabs(ds.N):
        xs = ds.x[s:t]
        xr = (xs.bfloat16() if kind == "bf16" else xs.clamp(-H.HALF_MAX, H.HALF_MAX).half()).double()
        q = (xr * xr).sum(1)
        i = int(q.argmax())
        if float(q[i]) > top:
            top, arg = float(q[i]), s + i
    rows = np.r_[ds.rows, arg]
    x = np.concatenate([ds.x_win, ds.x[arg:arg + 1].cpu().numpy()])
    out = H.check_half(ids[rows], x, ds.w0, kind, "euclidean", what="%s resident epoch" % kind)
    assert abs(float(np.sqrt(top)) - np.sqrt((H.round_operand(x, kind)[0] ** 2).sum(1).max())) <= 1e-9 * np.sqrt(top)
    print("%s: %d rows (%s), worst err / bound %r, distinct BMUs %d" % (kind, len(rows), ds.beyond, out, len(np.unique(ids))))
    assert len(np.unique(ids)) >= 0.9 * ds.K


def test_a_forced_update_and_merge(sets):
    ds = sets("A")
    # (16 516 sort blocks x 128 units is just past the counting sort's table: the radix sort; set C takes the counting sort)
    assert {"sort.radix", "runsum.upper"} <= U.update_paths(ds.X, ds.Y, ds.D, "gaussian", "rectangular", False, ds.N)
    run_forced_update(ds, "forced update")


def test_a_staged_blocks_equal_the_monolithic_call(sets):
    """A 129 x 2 map (two map-row blocks) on the same rows: begin + every block, bit for bit the one call."""
    ds = sets("A")
    with running(ds, "staged accumulate", X=129, Y=2) as e:
        assert e.epoch_block_count() >= 2
        e.epoch_accumulate(SIGMA, ETA, True)
        mnum, mden, mbmu = e.epoch_fetch()
        e.epoch_accumulate_begin(SIGMA, ETA, True)
        for blk in range(e.epoch_block_count()):
            e.epoch_accumulate_block(blk)
        snum, sden, sbmu = e.epoch_fetch()
    assert np.array_equal(mbmu, sbmu), "staged BMUs differ"
    assert np.array_equal(bits(mnum), bits(snum)) and np.array_equal(bits(mden), bits(sden)), "staged != monolithic"
    check_search(ds, mbmu, "part", "129 x 2 epoch ids", w=ds.codebook(129, 2))


def test_a_sample_weights(sets):
    ds = sets("A")
    w = weights_ref.make_weights(ds.N, 9)
    assert 0.05 * ds.N < (w == 0).sum() < 0.15 * ds.N
    run_forced_update(ds, "weighted forced update", weights=w, merge=False)


def test_a_distances_and_unit_stats(sets):
    ds = sets("A")
    with running(ds, "bmu_distances_device + unit_stats_device", resident=False) as e:
        ids, d = e.bmu_distances_device(ds.x.data_ptr(), ds.N)
        st = e.unit_stats_device(ds.x.data_ptr(), ds.N)
        qe = e.quantization_error_device(ds.x.data_ptr(), ds.N)
    check_search(ds, ids, "quant", "bmu_distances ids")
    assert d.dtype == F32 and d.shape == (ds.N,)
    tw, ti, td = ds.dev(ds.w0), ds.dev(ids), ds.dev(d)
    worst = 0.0
    for s, t in R.slabs(ds.N):
        ref = R.row_distances_t(ds.x[s:t], tw, ti[s:t])
        r = (td[s:t].double() - ref).abs() / (diag_ref.dist_bound(ds.D) * ref)
        assert bool((r <= 1.0).all()), "row %d: distance %r, float64 %r" % (s + int(r.argmax()), float(td[s + int(r.argmax())]), float(ref[int(r.argmax())]))
        worst = max(worst, float(r.max()))
    ww = diag_ref.check_distances(d[ds.rows], ds.x_win, ds.w0, ids[ds.rows], what="distances (windows)")
    us = diag_ref.check_unit_stats(st, ids, d, ds.K, what="unit stats")
    # sum_k sum_k / N, quantization_error and the float64 sum of the returned distances agree to diag_ref.QE_RTOL = 1e-12 at
    # this size too: a float32 distance in [8, 16) is a multiple of 2^-20 and N of them stay below 2^28, so every double sum of
    # them is exact whatever its order
    diag_ref.check_qe_agreement(st[1], ds.N, qe, "unit sums against QE")
    total = float(td.double().sum()) / ds.N
    assert abs(total - qe) <= diag_ref.QE_RTOL * abs(qe), "the float64 mean of the distances %r, quantization_error %r" % (total, qe)
    assert int(st[0].sum()) == ds.N
    print("distances: %d rows, worst err / bound %.3g (windows: %.3g); unit sums %.3g" % (ds.N, worst, ww, us))


def distances_under(ds, x, w, ids, q_ids, q_d, masked=False, what=""):
    """bmu_dist_kernel's float32 distance of every row to the unit the EPOCH gave it, as tests/test_gpu_monitor.py takes it:
    bmu_distances names the quantization search's unit, the epoch the training search's, and on a tie at float32's resolution
    the two differ.  Such rows are held to be ties (monitor_ref.check_near_ties) and their distance is taken again from the
    same kernel on a 5 x 4 handle whose every unit is the epoch's unit.  Returns (distances, rows re-scored)."""
    import torch
    from tests import monitor_ref
    diff = np.flatnonzero(q_ids != ids)
    if len(diff) == 0:
        return q_d, 0
    xd = x[torch.from_numpy(diff).cuda()].cpu().numpy()
    monitor_ref.check_near_ties(xd, w, ids[diff], q_ids[diff], np.arange(len(diff)), masked, what)
    d32 = q_d.copy()
    f = engine(5, 4, ds.D, precision="f32", **({"missing": "nan"} if masked else {}))
    try:
        for k in np.unique(ids[diff]):
            sel = np.flatnonzero(ids[diff] == k)
            f.set_weights(np.repeat(w[k][None, :], 20, axis=0))
            d32[diff[sel]] = f.bmu_distances(xd[sel])[1]
    finally:
        f.close()
    return d32, len(diff)


def test_a_two_monitored_epochs(sets):
    """tests/test_gpu_monitor.py's replay on the device rows, two epochs: rows, changed and the weight exactly and QE within
    gamma(D + 10) (monitor_ref.check_rows through extent_ref.row_metrics_t over all N rows), the shift by
    monitor_ref.check_shift, and monitor_ref.check_rows_tight -- sum_wd against math.fsum of the float32 distances
    bmu_distances_device returns under the epoch's codebook, within 2 rows 2^-53: one misread row fails it."""
    from tests import monitor_ref
    ds = sets("A")
    prev = None
    with running(ds, "two monitored epochs") as e:
        e.monitor(True)
        for t in range(2):
            tag = "monitored epoch %d" % t
            w_old = e.get_weights()
            q_ids, q_d = e.bmu_distances_device(ds.x.data_ptr(), ds.N)       # (the query's own row set: the resident rows are untouched)
            e.epoch_accumulate(O.exponential_decay(SIGMA, 1.0, t, 2), O.exponential_decay(ETA, 0.01, t, 2), True)
            ids = e.epoch_fetch()[2]
            e.epoch_measure_rows()
            e.epoch_measure_shift()
            e.epoch_merge()
            w_new = e.get_weights()
            m = e.epoch_metrics()
            ref = R.row_metrics_t(ds.x, ds.dev(w_old), ds.dev(ids), None if prev is None else ds.dev(prev))
            assert m["rows"] == ref["rows"] == ds.N and m["sum_w"] == ref["sum_w"], "%s: %r" % (tag, m)
            assert m["changed"] == ref["changed"], "%s: changed %r, the ids say %r" % (tag, m["changed"], ref["changed"])
            qref = monitor_ref.qe_of(ref)
            qr = abs(monitor_ref.qe_of(m) - qref) / (Q.gamma(ds.D + 10) * qref)
            assert qr <= 1.0, "%s: QE %r, float64 model %r" % (tag, monitor_ref.qe_of(m), qref)
            sr = monitor_ref.check_shift(m, w_old, w_new, tag)
            d32, ties = distances_under(ds, ds.x, w_old, ids, q_ids, q_d, what=tag)
            tr = monitor_ref.check_rows_tight(m, d32, None, tag)
            print("%s: rows %d changed %d QE %.9g (err/bound %.3g) shift max %.9g (err/bound %.3g); sum_wd against the float32 "
                  "distances: err/bound %.3g (%d rows re-scored at the epoch's unit)" % (
                      tag, m["rows"], m["changed"], monitor_ref.qe_of(m), qr, m["shift_max"], sr, tr, ties))
            prev = ids
    assert prev is not None and m["changed"] > 0


# ------------------------------------------------------------------------------------------------------ missing values on A
def masked_engine(ds, what, **kw):
    return running(ds, what, rows=ds.masked()[0], missing="nan", **kw)


def check_masked_search(ds, ids, what):
    """Masked picks admissible on all N rows (extent_ref.masked_scores_t) and by query_ref.check_picks on missing_ref's scores
    of the boundary windows; a row with nothing observed goes to unit 0."""
    from tests import missing_ref as M
    xm, empty, xm_win = ds.masked()
    worst, share, seen = R.check_picks_all_rows(ds.dev(ids), xm, ds.dev(ds.w0), "masked", what)
    ww = Q.check_picks(ids[ds.rows], *M.masked_scores(xm_win, ds.w0), what + " (windows)")
    assert (ids[empty] == 0).all(), "%s: rows with nothing observed must name unit 0: %r" % (what, ids[empty])
    print("%s: %d rows, worst err / bound %.3g (windows: %.3g), undecided share %.3g, distinct BMUs %d" % (
        what, seen, worst, ww, share, len(np.unique(ids))))
    assert len(np.unique(ids)) >= 0.9 * ds.K


def test_a_missing_values_masked_search(sets):
    """A handle with missing values on A's rows with 3 % of the features NaN and one all-NaN row inside each boundary window:
    the ids of a resident epoch and of bmu_device against the masked score reference."""
    ds = sets("A")
    xm, empty, _ = ds.masked()
    assert len(empty) == 5 and all(lo < r < hi - 1 for r, (lo, hi) in zip(empty, sorted(ds.windows())))
    with masked_engine(ds, "masked resident epoch + query") as e:
        e.epoch_accumulate(SIGMA, ETA, False)
        ids_epoch = e.epoch_fetch_masked()[2]
        e.footprint()
        ids_query = e.bmu_device(xm.data_ptr(), ds.N)
    check_masked_search(ds, ids_epoch, "masked resident epoch ids")
    check_masked_search(ds, ids_query, "masked bmu_device ids")


def test_a_missing_values_forced_update(sets):
    """som_epoch_fetch_masked's accumulators of a forced epoch against the segment sums of the augmented rows [x~ | m]."""
    from tests import missing_ref as M
    ds = sets("A")
    xm = ds.masked()[0]
    D = ds.D
    bmu = R.forced_bmus(ds.N, ds.K)
    with masked_engine(ds, "masked forced update") as e:
        e.epoch_accumulate_forced(bmu.numpy(), SIGMA, ETA, True)
        num, den, _ = e.epoch_fetch_masked(want_bmu=False)
        e.footprint()
        e.epoch_accumulate_forced(bmu.numpy(), SIGMA, ETA, True)
        num2, den2, _ = e.epoch_fetch_masked(want_bmu=False)
        e.epoch_merge()
        w1 = e.get_weights()
    assert np.array_equal(bits(num), bits(num2)) and np.array_equal(bits(den), bits(den2)), "a second masked accumulate differs"
    S, A, c = R.segment_sums_t(xm, bmu.cuda(), ds.K, masked=True)
    rnum, _, mag, _ = R.reference_from_sums(S, A, c, ds.X, ds.Y, ETA, SIGMA, True)
    ref = (rnum[:, :D], rnum[:, D:], mag[:, :D], mag[:, D:])
    a = M.check_accumulators(num, den, ref, "masked forced update")
    mr = M.check_merge(ds.w0, w1, num, den, ref, False, "masked forced update")
    print("masked forced update: observed share %.4f; worst err / bound: accumulators %.3g, merge %.3g" % (
        S[:, D:].sum() / (ds.N * D), a, mr))


def test_a_missing_values_quantization_error(sets):
    """qe_masked_kernel: quantization_error_device of the rows with NaNs against missing_ref.check_qe's form on all N rows."""
    ds = sets("A")
    xm = ds.masked()[0]
    with masked_engine(ds, "masked quantization error", resident=False) as e:
        qe = e.quantization_error_device(xm.data_ptr(), ds.N)
        ids = e.bmu_device(xm.data_ptr(), ds.N, quantization=True)
    check_masked_search(ds, ids, "masked quantization ids")
    ratio = R.check_qe_t(qe, xm, ds.dev(ds.w0), ds.dev(ids), "masked QE", masked=True)
    print("masked QE %r: err / bound %.3g" % (qe, ratio))


def test_a_label_counts_and_value_sums(sets):
    import torch
    ds = sets("A")
    C = 5
    r = torch.arange(ds.N, dtype=torch.int64, device="cuda")
    labels = (((r * 40503) >> 3) % C).to(torch.int32)
    lo, hi = ds.win["last"]
    labels[lo + 5], labels[lo + 77], labels[hi - 1] = -1, C, 2 ** 31 - 1            # unlabelled: counted nowhere
    g = torch.Generator(device="cuda")
    g.manual_seed(77)
    values = torch.randn(ds.N, 2, generator=g, device="cuda", dtype=torch.float32)
    values[:, 1][torch.rand(ds.N, generator=g, device="cuda") < 0.1] = float("nan")
    with running(ds, "label counts + value sums", resident=False) as e:
        ids = e.bmu_device(ds.x.data_ptr(), ds.N)
        counts = e.label_counts_device(ds.x.data_ptr(), labels.data_ptr(), ds.N, C)
        got = e.value_sums_device(ds.x.data_ptr(), values.data_ptr(), ds.N, 2)
    check_search(ds, ids, "part", "bmu_device ids of the maps")
    want = project_ref.label_counts_model(ids, labels.cpu().numpy(), ds.K, C)
    assert np.array_equal(counts, want), "label counts differ at %r" % (np.argwhere(counts != want)[:5].tolist(),)
    assert int(counts.sum()) == ds.N - 3
    assert np.array_equal(counts, R.label_counts_t(ds.dev(ids), labels, ds.K, C)), "label counts differ from the device bincount"
    tc, tt, tq, ta = R.value_sums_t(ds.dev(ids), values, ds.K)
    assert np.array_equal(got[0], tc), "value counts differ from the device model"
    worst = project_ref.check_value_sums(got, ids, values.cpu().numpy(), ds.K, "value sums")
    print("label counts exact over %d rows; value sums worst err / bound %.3g" % (ds.N, worst))


# ====================================================================================================== set B
def test_b_float32_tiled_search(sets):
    run_f32_search(sets("B"))


def test_b_top2(sets):
    run_top2(sets("B"))


def test_b_exact_handle_three_epochs(sets, monkeypatch):
    """(A 16 x 8 map with more than 128 features is below the wide screen's 4096 units: the exact handle serves these epochs
    with the float32 kernels, query_ref.is_exact -- the trajectories must still be one.)"""
    ds = sets("B")
    assert not Q.is_exact(ds.X, ds.Y, ds.D, "exact", "euclidean")
    run_exact(ds, monkeypatch, planned=False)


def test_b_wide_screen_on_a_64x64_map(sets, monkeypatch):
    """The wide screen, wide_gather_sorted_kernel and the K-looped re-score need >= 4096 units beyond 128 features: a 64 x 64
    map on B's rows, three resident epochs and a query against the float32 engine's (the tiled float32 kernel over 32 unit
    tiles).  No row may go to the float32 fallback, as on A."""
    ds = sets("B")
    assert Q.is_exact(64, 64, ds.D, "exact", "euclidean")
    # (the float32 ids' own float64 check: K is 32 times A's, so every eighth slab and the boundary windows; the exact ids are
    # compared with them on every row)
    run_exact(ds, monkeypatch, planned=True, X=64, Y=64, every=8)


def test_b_forced_update(sets):
    run_forced_update(sets("B"), "forced update, D = 136")


# ====================================================================================================== set C
def test_c_one_unit_owns_every_row(sets):
    """2^24 + 4097 rows on one unit: a float32 count stops at 2^24 (4097 / 2^24 = 2.4e-4 of den, 24 times update_ref.TOL)."""
    import torch
    ds = sets("C")
    assert {"sort.counting", "runsum.upper"} <= U.update_paths(ds.X, ds.Y, ds.D, "gaussian", "rectangular", False, ds.N)
    bmu = torch.full((ds.N,), 27, dtype=torch.int32)
    num, den, c = run_forced_update(ds, "one unit", bmu=bmu)
    assert c[27] == ds.N and c.sum() == ds.N


def test_c_three_units_own_2_pow_24_plus_1_4096_and_0_rows(sets):
    import torch
    ds = sets("C")
    bmu = torch.full((ds.N,), 5, dtype=torch.int32)
    bmu[2 ** 24 + 1:] = 40
    num, den, c = run_forced_update(ds, "three units", bmu=bmu)
    assert c[5] == 2 ** 24 + 1 and c[40] == 4096 and c[63] == 0


def test_c_unit_stats_hits_are_exact_integers(sets):
    """A codebook whose unit 27 is nearest to every row: its hits are N exactly, every other unit's 0."""
    ds = sets("C")
    w = np.stack([1000.0 + np.arange(ds.K), np.full(ds.K, 1000.0)], axis=1).astype(F32)
    w[27] = 0
    with running(ds, "unit_stats_device, one unit", resident=False) as e:
        e.set_weights(w)
        count, tot, sq, mx = e.unit_stats_device(ds.x.data_ptr(), ds.N)
        ids, d = e.bmu_distances_device(ds.x.data_ptr(), ds.N)
    assert count[27] == ds.N and count.sum() == ds.N and (ids == 27).all()
    ref = float(ds.x.double().pow(2).sum(1).sqrt().sum())
    assert abs(tot[27] - ref) <= (diag_ref.dist_bound(ds.D) + ds.N * diag_ref.U64) * ref
    assert mx[27] == d.max()
    print("unit 27: %d hits, sum of distances %r (float64 %r)" % (count[27], tot[27], ref))


# ====================================================================================================== set R
def test_r_radix_sort_with_row_ids_beyond_24_bits(sets):
    """129 x 64 x 4 (test_gpu_weights.FORCED's radix shape) at N = 2^24 + 3: forced BMUs on a pool of 400 units."""
    import torch
    ds = sets("R")
    assert "sort.radix" in U.update_paths(ds.X, ds.Y, ds.D, "gaussian", "rectangular", False, ds.N)
    rs = np.random.RandomState(5)
    pool = np.unique(np.r_[0, ds.K - 1, rs.choice(ds.K, size=400, replace=False)])
    bmu = torch.from_numpy(pool)[R.forced_bmus(ds.N, len(pool)).long()].to(torch.int32)
    run_forced_update(ds, "radix sort", bmu=bmu)
