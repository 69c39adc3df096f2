"""tests/extent_ref.py on the CPU: the boundary windows against brute force, the torch slab references against the NumPy
references they restate (query_ref, update_ref, weights_ref, diag_ref, missing_ref, monitor_ref, project_ref), the named mutants
of the model engine against the checks meant to catch them -- far from, and one row either side of, their boundaries -- and the share of rows
the pick bound leaves undecided on the data sets of tests/test_gpu_extent.py.  No GPU."""
import numpy as np
import pytest

from tests import diag_ref
from tests import extent_ref as R
from tests import query_ref as Q
from tests import update_ref as U
from tests import weights_ref

torch = pytest.importorskip("torch")

F32, F64 = np.float32, np.float64
ELEMS, BYTES = 2 ** 12, 2 ** 13            # the emulated boundaries: 4096 elements, 8192 bytes (2048 float32 elements)


# ------------------------------------------------------------------------------------------------------ the windows
@pytest.mark.parametrize("D", [8, 12, 33])               # 8 divides 2^12; 12 and 33 leave a row astride it
def test_boundary_windows_against_brute_force(D):
    N = ELEMS // D + R.MIN_BEYOND + 77
    win = R.boundary_windows(N, D, elems=ELEMS, bytes_=BYTES, width=64)
    assert win["stride"] == R.STRIDE and win["first"] == (0, 64) and win["last"] == (N - 64, N)
    rows = np.arange(N, dtype=np.int64)
    dp = R.half_pitch(D)
    # the rows that hold (or begin at) the boundary, from every row's own first and last element / byte
    holds_elem = rows[(rows * D <= ELEMS) & (ELEMS < (rows + 1) * D)]
    holds_byte = rows[(rows * D * 4 <= BYTES) & (BYTES < (rows + 1) * D * 4)]
    holds_half = rows[(rows * dp * 2 <= BYTES) & (BYTES < (rows + 1) * dp * 2)]
    for name, holds in (("elems", holds_elem), ("bytes_f32", holds_byte), ("bytes_half", holds_half)):
        lo, hi = win[name]
        assert len(holds) == 1 and hi - lo == 64 and 0 <= lo and hi <= N
        assert lo + 8 <= holds[0] < hi - 8, "%s: row %d not well inside [%d, %d)" % (name, holds[0], lo, hi)   # both sides seen
    if ELEMS % D:
        r = int(holds_elem[0])
        assert r * D < ELEMS < (r + 1) * D                # it straddles
    picked = R.window_rows(win, N)
    assert picked[0] == 0 and picked[-1] == N - 1 and len(np.unique(picked)) == len(picked)
    assert R.rows_beyond(picked, D, ELEMS) >= 64 + (N - ELEMS // D) // R.STRIDE - 1
    assert set(range(0, N, R.STRIDE)) <= set(picked.tolist())


def test_boundary_windows_refuse_a_row_set_that_proves_nothing():
    D = 8
    with pytest.raises(AssertionError, match="wholly beyond"):
        R.boundary_windows(ELEMS // D + R.MIN_BEYOND - 1, D, elems=ELEMS, bytes_=BYTES, width=64)
    with pytest.raises(AssertionError, match="wholly beyond"):
        R.boundary_windows(ELEMS // D - 5, D, elems=ELEMS, bytes_=BYTES, width=64)             # never reaches the boundary
    with pytest.raises(AssertionError):
        R.boundary_windows(100, D, elems=16, bytes_=64, width=64)                               # windows do not fit
    with pytest.raises(AssertionError, match="leaves"):
        R.boundary_windows(2 ** 17, D, elems=ELEMS, bytes_=2 ** 40, width=64)                   # the byte boundary beyond N
    R.boundary_windows(ELEMS // D + R.MIN_BEYOND, D, elems=ELEMS, bytes_=BYTES, width=64)     # exactly enough


def test_the_gpu_shapes_cross_their_boundaries():
    from tests import test_gpu_extent as G
    for name in ("A", "B"):
        c = G.SETS[name]
        N, D = c["N"], c["D"]
        assert N * D > 2 ** 31 and N * D * 4 > 2 ** 32 and N * R.half_pitch(D) * 2 > 2 ** 32
        win = R.boundary_windows(N, D)
        rows = R.window_rows(win, N)
        assert R.rows_beyond(rows, D, 2 ** 31) >= 4096 + 16 and R.rows_beyond(rows, D, 2 ** 30) >= 3 * 4096
        assert N % 256 and N % 1024 and N % 64            # partial last tiles, chunks and passes
    assert G.SETS["A"]["D"] == 128 and G.SETS["B"]["D"] == 136
    assert G.SETS["C"]["N"] > 2 ** 24 + 4096
    a = G.SETS["A"]
    paths = U.update_paths(a["X"], a["Y"], a["D"], "gaussian", "rectangular", False, a["N"])
    # 16 516 sort blocks x 128 units is just past the counting sort's table of 2^21 entries: A takes the radix sort, C (64
    # units) the counting sort, R the radix sort with 14 key bits
    assert {"sort.radix", "runsum.upper", "seg.vec2"} <= paths
    c = G.SETS["C"]
    assert {"sort.counting", "runsum.upper"} <= U.update_paths(c["X"], c["Y"], c["D"], "gaussian", "rectangular", False, c["N"])
    r = G.SETS["R"]
    assert "sort.radix" in U.update_paths(r["X"], r["Y"], r["D"], "gaussian", "rectangular", False, r["N"]) and r["N"] > 2 ** 24


def test_forced_bmus_move_a_wrapped_row_to_another_unit():
    N, K = 70000, 128
    b = R.forced_bmus(N, K).numpy()
    assert b.dtype == np.int32 and b.min() == 0 and b.max() == K - 1
    want = [0] * 300                                     # the hash in Python integers, row by row
    for r in range(300):
        h = (r * R.HASH) % 2 ** 32
        h ^= h >> 16
        h = (h * R.HASH2) % 2 ** 32
        h ^= h >> 13
        h = (h * R.HASH3) % 2 ** 32
        want[r] = (h ^ (h >> 16)) % K
    assert b[:300].tolist() == want
    counts = np.bincount(b, minlength=K)
    assert counts.min() > 0.8 * N / K and counts.max() < 1.2 * N / K
    for back in (2 ** 12, 2 ** 15, 2 ** 16):            # the distances at which an index wraps (emulated)
        assert (b[back:] != b[:-back]).mean() > 0.97
    # at the real distances too: rows r and r - 2^24 (a 24-bit id), r - 2^31/128, r - 2^30/128, r - 2^32/136
    r = np.arange(2 ** 25, 2 ** 25 + 50000, dtype=np.int64)
    f = lambda q: R.hash_mix(q) % K
    for back in (2 ** 24, 2 ** 23, 2 ** 22, 2 ** 32 // 136, 2 ** 31 // 136):
        assert (f(r) != f(r - back)).mean() > 0.97, back


# ------------------------------------------------------------------------------------------------------ torch against NumPy
def _small(n=700, D=24, K=35, seed=3):
    x = Q.make_rows("blobs", n, D, seed)
    w = Q.make_units("blobs", x, K, D, seed)
    return x, w


@pytest.mark.parametrize("mode", ["part", "sq", "sqrt"])
def test_scores_and_pick_ratio_equal_query_ref(mode):
    x, w = _small()
    s, E = Q.scores(x, w, mode)
    st, Et = R.scores_t(torch.from_numpy(x), torch.from_numpy(w), mode)
    assert np.allclose(st.numpy(), s, rtol=1e-12, atol=1e-12 * np.abs(s).max()) and np.allclose(Et.numpy(), E, rtol=1e-11)
    rs = np.random.RandomState(0)
    ids = np.argmin(s, axis=1)
    ids[::3] = rs.randint(0, len(w), len(ids[::3]))      # a third of the picks wrong
    ids[5], ids[6] = -1, len(w)                          # and two out of range
    got = R.pick_ratio_t(torch.from_numpy(ids), st, Et).numpy()
    want = Q.pick_ratio(np.clip(ids, 0, len(w) - 1), s, E)
    want[[5, 6]] = np.inf
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and np.allclose(got[fin], want[fin], rtol=1e-6, atol=1e-9)
    assert (got > 1).sum() > 100 and (got == 0).sum() > 400
    und = R.undecided_t(st, Et).numpy()
    cap = (s + E).min(axis=1)[:, None]
    assert np.array_equal(und, ((s <= cap + E).sum(axis=1) > 1))


def test_check_picks_all_rows_and_top2_agree_with_query_ref():
    x, w = _small(n=900)
    tx, tw = torch.from_numpy(x), torch.from_numpy(w)
    s, E = Q.scores(x, w, "sqrt")
    order = np.argsort(s, axis=1)
    i1, i2 = order[:, 0].copy(), order[:, 1].copy()
    worst, share, seen = R.check_picks_all_rows(torch.from_numpy(i1), tx, tw, "sqrt", max_undecided=1.0)
    assert worst == 0.0 and seen == len(x) and 0 <= share <= 1
    assert R.check_top2_all_rows(torch.from_numpy(i1), torch.from_numpy(i2), tx, tw) == 0.0
    Q.check_top2(i1, i2, s, E)
    for name, (a, b) in {"third for second": (i1, order[:, 2].copy()), "swapped": (i2, i1), "twice": (i1, i1),
                         "out of range": (i1, np.full_like(i2, len(w)))}.items():
        if name == "out of range":
            b = i2.copy()
            b[17] = len(w)
        with pytest.raises(AssertionError):
            R.check_top2_all_rows(torch.from_numpy(a), torch.from_numpy(b), tx, tw, what=name)
        with pytest.raises(AssertionError):
            Q.check_top2(a, b, s, E, name)
    # the quantization mode's check: picks made on float32 roots of float32 squares pass it, a runner-up does not
    sq32 = ((x[:, None, :] - w[None, :, :]) ** 2).sum(axis=2, dtype=F32)
    q32 = torch.from_numpy(np.argmin(np.sqrt(sq32), axis=1))
    worst, share, _ = R.check_picks_all_rows(q32, tx, tw, "quant", max_undecided=1.0)
    assert worst <= 1.0 and share < R.check_picks_all_rows(q32, tx, tw, "sqrt", max_undecided=1.0)[1]
    s2, E2 = R.widen_for_sqrt(*Q.scores(x, w, "sq"))
    assert np.allclose(R.widen_for_sqrt(*R.scores_t(tx, tw, "sq"))[1].numpy(), E2, rtol=1e-11) and (E2 > Q.scores(x, w, "sq")[1]).all()
    Q.check_picks(q32.numpy(), s2, E2)
    with pytest.raises(AssertionError):
        R.check_picks_all_rows(torch.from_numpy(i2), tx, tw, "quant", max_undecided=1.0)
    bad = i1.copy()
    bad[401] = order[401, -1]
    with pytest.raises(AssertionError, match="row 401"):
        R.check_picks_all_rows(torch.from_numpy(bad), tx, tw, "sqrt")
    with pytest.raises(AssertionError):
        Q.check_picks(bad, s, E)


def test_distances_and_qe_equal_their_numpy_forms():
    x, w = _small()
    tx, tw = torch.from_numpy(x), torch.from_numpy(w)
    ids = np.argmin(Q.scores(x, w, "sqrt")[0], axis=1)
    d = R.row_distances_t(tx, tw, torch.from_numpy(ids)).numpy()
    assert np.allclose(d, diag_ref.row_distances(x, w, ids), rtol=1e-13)
    ref = Q.qe_reference(x, w, ids)
    assert abs(R.qe_sum_t(tx, tw, torch.from_numpy(ids), slab=97) / len(x) - ref) <= 1e-13 * ref
    good = float(np.float32(ref))
    assert abs(R.check_qe_t(good, tx, tw, torch.from_numpy(ids)) - Q.check_qe(good, x, w, ids)) < 1e-6
    for fn in (lambda q: R.check_qe_t(q, tx, tw, torch.from_numpy(ids)), lambda q: Q.check_qe(q, x, w, ids)):
        with pytest.raises(AssertionError):
            fn(ref * (1 + 1e-4))


def test_segment_sums_equal_update_ref_and_weights_ref():
    X, Y, D, N = 9, 7, 6, 5000
    K = X * Y
    x = U.make_data(N, D, 1.0, 5)
    bmu = R.forced_bmus(N, K)
    bmu[bmu == 11] = 12                                   # a unit without rows
    tx = torch.from_numpy(x)
    S, A, c = R.segment_sums_t(tx, bmu, K, slab=777)
    for a, b in zip((S, A, c), R.segment_sums_t(tx, bmu, K, slab=5000, lanes=1)):          # one copy of the table: the plain form
        assert np.allclose(a, b, rtol=1e-12, atol=1e-12)
    units, S0, A0, c0 = U.segment_sums(x, bmu.numpy())
    assert c[11] == 0 and np.array_equal(np.flatnonzero(c), units)
    assert np.allclose(S[units], S0, rtol=1e-12, atol=1e-12) and np.allclose(A[units], A0, rtol=1e-12) and np.array_equal(c[units], c0)
    ref0 = U.reference_update(x, bmu.numpy(), X, Y, 0.5, 2.0, wide=True)
    ref = R.reference_from_sums(S, A, c, X, Y, 0.5, 2.0, True)
    for a, b in zip(ref, ref0):
        assert np.allclose(a, b, rtol=1e-11, atol=1e-300)
    wts = weights_ref.make_weights(N, 3)
    S, A, c = R.segment_sums_t(tx, bmu, K, weights=torch.from_numpy(wts), slab=1001)
    units, S0, A0, c0 = weights_ref.weighted_segment_sums(x, bmu.numpy(), wts)
    assert np.allclose(S[units], S0, rtol=1e-12, atol=1e-12) and np.allclose(A[units], A0, rtol=1e-12) and np.allclose(c[units], c0, rtol=1e-13)
    ref0 = weights_ref.reference_update_weighted(x, bmu.numpy(), wts, X, Y, 0.5, 2.0, wide=False)
    ref = R.reference_from_sums(S, A, c, X, Y, 0.5, 2.0, False)
    for a, b in zip(ref, ref0):
        assert np.allclose(a, b, rtol=1e-11, atol=1e-300)


# ------------------------------------------------------------------------------ torch against missing_ref, monitor_ref, project_ref
def _punched(n=600, D=9, seed=4):
    from tests import missing_ref as M
    x = M.punch(Q.make_rows("blobs", n, D, seed), "random30", 5)
    x[7] = np.nan                                                       # a row with nothing observed
    w = Q.make_units("blobs", np.nan_to_num(x), 35, D, seed)
    return x, w


def test_masked_references_equal_missing_ref():
    from tests import missing_ref as M
    x, w = _punched()
    tx, tw = torch.from_numpy(x), torch.from_numpy(w)
    xt, m = R.split_t(tx)
    assert np.array_equal(xt.numpy(), M.split(x)[0]) and np.array_equal(m.numpy(), M.split(x)[1])
    s, E = M.masked_scores(x, w)
    st, Et = R.masked_scores_t(tx, tw)
    assert np.allclose(st.numpy(), s, rtol=1e-12, atol=1e-12 * np.abs(s).max()) and np.allclose(Et.numpy(), E, rtol=1e-11)
    ids = M.masked_bmu(x, w)
    assert ids[7] == 0
    worst, _, seen = R.check_picks_all_rows(torch.from_numpy(ids), tx, tw, "masked", max_undecided=1.0)
    assert worst == 0.0 and seen == len(x)
    Q.check_picks(ids, s, E)
    bad = ids.copy()
    bad[100] = np.argmax(s[100])
    with pytest.raises(AssertionError, match="row 100"):
        R.check_picks_all_rows(torch.from_numpy(bad), tx, tw, "masked", max_undecided=1.0)
    # the masked distances and QE
    d = R.row_distances_t(tx, tw, torch.from_numpy(ids), masked=True).numpy()
    assert d[7] == 0 and np.allclose(d, diag_ref.row_distances(x, w, ids, masked=True), rtol=1e-13)
    ref = M.qe_reference(x, w, ids)
    good = float(np.float32(ref))
    assert abs(R.check_qe_t(good, tx, tw, torch.from_numpy(ids), masked=True) - M.check_qe(good, x, w, ids)) < 1e-6
    with pytest.raises(AssertionError):
        R.check_qe_t(ref * (1 + 1e-4), tx, tw, torch.from_numpy(ids), masked=True)
    # the augmented segment sums [x~ | m], plain and weighted, through to the reference update
    X, Y, D = 7, 5, x.shape[1]
    bmu = R.forced_bmus(len(x), X * Y)
    for wts in (None, weights_ref.make_weights(len(x), 3)):
        S, A, c = R.segment_sums_t(tx, bmu, X * Y, None if wts is None else torch.from_numpy(wts), slab=211, lanes=4, masked=True)
        num, _, mag, _ = R.reference_from_sums(S, A, c, X, Y, 0.5, 1.5, True)
        want = M.reference_update_masked(x, bmu.numpy(), X, Y, 0.5, 1.5, wide=True, weights=wts)
        for a, b in zip((num[:, :D], num[:, D:], mag[:, :D], mag[:, D:]), want):
            assert np.allclose(a, b, rtol=1e-11, atol=1e-300)


def test_punch_on_device_leaves_the_other_features_alone():
    x, _ = R.rows_on_device(30000, 16, seed=1, device="cpu", slab=7000)
    y = R.punch_on_device(x, 9, empty_rows=[0, 12345, 29999], slab=7000)
    hole = torch.isnan(y)
    assert not torch.isnan(x).any() and torch.equal(y[~hole], x[~hole])
    assert hole[[0, 12345, 29999]].all() and 0.025 < float(hole.double().mean()) < 0.035
    assert int(hole.all(dim=1).sum()) == 3 and torch.equal(torch.isnan(R.punch_on_device(x, 9, slab=7000)) | hole, hole)


def test_row_metrics_equal_monitor_ref():
    from tests import monitor_ref
    for masked in (False, True):
        x, w = _punched() if masked else _small()
        s = (R.masked_scores_t if masked else lambda a, b: R.scores_t(a, b, "part"))(torch.from_numpy(x), torch.from_numpy(w))[0]
        ids = s.argmin(dim=1)
        prev = ids.clone()
        prev[::7] = (prev[::7] + 1) % len(w)
        for p in (None, prev):
            got = R.row_metrics_t(torch.from_numpy(x), torch.from_numpy(w), ids, p, masked, slab=97)
            want = monitor_ref.row_metrics(x, w, ids.numpy(), None, None if p is None else p.numpy(), masked)
            assert got["rows"] == want["rows"] and got["changed"] == want["changed"] and got["sum_w"] == want["sum_w"]
            assert abs(got["sum_wd"] - want["sum_wd"]) <= 1e-13 * want["sum_wd"]


def test_label_counts_and_value_sums_equal_project_ref():
    from tests import project_ref as P
    rs = np.random.RandomState(8)
    n, K, C = 5000, 35, 5
    ids = rs.randint(0, K, n)
    ids[ids == 9] = 10                                                  # a unit without rows
    labels = rs.randint(-1, C + 1, n).astype(np.int32)                  # -1 and C: unlabelled
    labels[3] = 2 ** 31 - 1
    got = R.label_counts_t(torch.from_numpy(ids), torch.from_numpy(labels), K, C)
    assert got.dtype == np.int64 and np.array_equal(got, P.label_counts_model(ids, labels, K, C)) and got[9].sum() == 0
    values = rs.normal(0, 3, (n, 3)).astype(F32)
    values[rs.rand(n) < 0.2, 1] = np.nan
    values[:, 2] = np.nan                                               # a column nobody observes
    count, tot, sq, sa = R.value_sums_t(torch.from_numpy(ids), torch.from_numpy(values), K, slab=777, lanes=3)
    rc, rt, rq = P.value_sums_model(ids, values, K)
    ra, rqa = P.abs_sums(ids, values, K)
    assert count.dtype == np.int64 and np.array_equal(count, rc) and (count[:, 2] == 0).all()
    g = P.gamma(rc)
    assert (np.abs(tot - rt) <= g * ra).all() and (np.abs(sq - rq) <= g * rqa).all() and np.allclose(sa, ra, rtol=1e-12)
    P.check_value_sums((count, tot, sq), ids, values, K, "the torch form as a device")


# ------------------------------------------------------------------------------------------------------ the mutants
X_, Y_, D_ = 4, 2, 8                                      # 8 units: above the boundary every unit owns > 2^11 rows
K_ = X_ * Y_
N_ABOVE = ELEMS // D_ + R.MIN_BEYOND + 77                 # 66 125 rows: past 2^12 elements, 2^13 bytes, 2^10 row ids, 2^11 per unit
N_BELOW = 100                                             # 800 elements: below every emulated boundary
MUTANTS = R.mutants(ELEMS, BYTES, id_bits=10, count_dtype=np.float16)


def _model_case(N):
    x, c = R.rows_on_device(N, D_, seed=11, device="cpu", grid=(2, 2), slab=5000)
    x = x.numpy()
    w = R.codebook_near(c, X_, Y_, seed=12, grid=(2, 2))
    return x, w


def _check_search(e, x, w, N):
    """The pick check of the GPU module: query_ref.check_picks on the boundary windows (every row when N is small)."""
    rows = R.window_rows(R.boundary_windows(N, D_, elems=ELEMS, bytes_=BYTES, width=64), N) if N >= N_ABOVE else np.arange(N)
    s, E = Q.scores(x[rows], w, "part")
    Q.check_picks(e.bmu(w, rows), s, E, "model engine")


def _check_update(e, x, N, bmu=None):
    """The accumulator check of the GPU module: forced BMUs, update_ref.check_accumulators against the slab segment sums."""
    bmu = R.forced_bmus(N, K_) if bmu is None else bmu
    ref = R.reference_from_sums(*R.segment_sums_t(torch.from_numpy(x), bmu, K_), X_, Y_, 0.5, 1.5, True)
    S, c = e.segment_sums(bmu.numpy(), K_)
    num, den, _, _ = R.reference_from_sums(S, np.abs(S), c, X_, Y_, 0.5, 1.5, True)
    U.check_accumulators(num.astype(F32), den.astype(F32), ref, "model engine")


CAUGHT_BY = {"offset_mod_elems": ("search", "update"), "offset_mod_bytes": ("search", "update"),
             "sort_id_truncated": ("update",), "count_sequential_low_precision": ("update",)}


def test_the_correct_model_engine_passes_every_check():
    for N in (N_BELOW, N_ABOVE):
        x, w = _model_case(N)
        e = R.ModelEngine(x)
        _check_search(e, x, w, N)
        _check_update(e, x, N)


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_each_mutant_fails_its_check_above_the_boundary_and_passes_below(name):
    assert sorted(MUTANTS) == sorted(CAUGHT_BY)
    x, w = _model_case(N_BELOW)
    e = R.ModelEngine(x, **MUTANTS[name])
    _check_search(e, x, w, N_BELOW)                       # below: indistinguishable from the correct engine
    _check_update(e, x, N_BELOW)
    x, w = _model_case(N_ABOVE)
    e = R.ModelEngine(x, **MUTANTS[name])
    for check in ("search", "update"):
        run = (lambda: _check_search(e, x, w, N_ABOVE)) if check == "search" else (lambda: _check_update(e, x, N_ABOVE))
        if check in CAUGHT_BY[name]:
            with pytest.raises(AssertionError):
                run()
        else:
            run()                                         # (the search neither sorts nor counts)


# the largest N still below each mutant's own boundary, and the first one past it: (N, every row on unit 3)
TIGHT = {"offset_mod_elems": (ELEMS // D_, False),                  # 512 rows: the last offset is 4088 < 2^12
         "offset_mod_bytes": (BYTES // 4 // D_, False),             # 256 rows: the last byte offset is 8160 < 2^13
         "sort_id_truncated": (2 ** 10, False),                     # row ids 0 .. 1023 fit 10 bits
         "count_sequential_low_precision": (2 ** 11, True)}         # float16 counts 2048 exactly, and 2048 + 1 == 2048


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_each_mutant_passes_at_the_last_n_below_its_boundary_and_fails_one_row_later(name):
    """'Passes every check until N crosses it', tightly: at the last N below the mutant's own boundary both checks pass; with
    one row more -- the single row that wraps, or the single count that is lost -- the accumulator check fails."""
    n, one_unit = TIGHT[name]
    for N, passes in ((n, True), (n + 1, False)):
        x, w = _model_case(N)
        e = R.ModelEngine(x, **MUTANTS[name])
        bmu = torch.full((N,), 3, dtype=torch.int32) if one_unit else None
        if passes:
            _check_search(e, x, w, N)
            _check_update(e, x, N, bmu)
        else:
            with pytest.raises(AssertionError):
                _check_update(e, x, N, bmu)
        _check_search(R.ModelEngine(x), x, w, N)                      # the correct engine passes on both sides
        _check_update(R.ModelEngine(x), x, N, bmu)


def test_float32_sequential_count_stops_at_2_pow_24():
    """The real boundary of the fourth mutant, without 2^24 additions: float32(2^24) + 1 == float32(2^24)."""
    assert F32(2 ** 24) + F32(1) == F32(2 ** 24) and F32(2 ** 24 - 1) + F32(1) == F32(2 ** 24)
    assert np.float16(2 ** 11) + np.float16(1) == np.float16(2 ** 11)      # and of its float16 stand-in
    # a count stuck at 2^24 misses update_ref.TOL on set C (2^24 + 4097 rows on one unit) by a factor of 24
    assert 4097 / (2 ** 24 + 4097) > 24 * U.TOL


# ------------------------------------------------------------------------------------------------------ near-ties
@pytest.mark.parametrize("name", ["A", "B"])
def test_the_pick_bound_leaves_at_most_one_row_in_a_hundred_undecided(name):
    """From the reference alone, at a reduced N with the generator and the codebook of the GPU module's sets: the share of rows
    whose admissible set holds more than one unit.  The GPU test asserts the same on all N rows."""
    from tests import test_gpu_extent as G
    c = G.SETS[name]
    K = c["X"] * c["Y"]
    x, cen = R.rows_on_device(20000, c["D"], seed=c["seed"], device="cpu", slab=4096)
    w = torch.from_numpy(R.codebook_near(cen, c["X"], c["Y"], seed=c["seed"] + 1))
    s, E = R.scores_t(x, w, "part")
    share = float(R.undecided_t(s, E).double().mean())
    print("%s: undecided share %.3g" % (name, share))
    assert share <= 0.01
    # query_ref's bound of the quantization mode carries sqrt(E_sq) (|sqrt a - sqrt b| <= sqrt |a - b|), a hundred times the
    # gap it would take to decide these rows: it is the existing bound and is applied as it stands, but what decides the
    # quantization-mode ids in the GPU module is the 'sq' form of the same scores, whose bound is as tight as 'part's
    s, E = R.scores_t(x, w, "sq")
    share = float(R.undecided_t(s, E).double().mean())
    print("%s sq: undecided share %.3g" % (name, share))
    assert share <= 0.01
    picks = s.argmin(dim=1)
    assert len(torch.unique(picks)) >= 0.9 * K, "the BMUs must spread over the whole map"
