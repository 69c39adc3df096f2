"""Block skipping's bound (csrc/exact_skip.hpp, csrc/exact_skip_wide.hpp: group_centroids, exact_centroids_kernel,
exact_merge_prep_kernel, exact_centroid_image_*, exact_plan_kernel at both levels, wide_centroids_kernel) on codebooks built to
defeat it, against the float32 engine, the float64 BMUs and a float64 computation of the plan's geometry.  GPU only (`-m gpu`).

The cases are tests/skip_ref.py's: tests/test_skip_ref_cpu.py shows on a float64 model of the test that each of them turns a
radius that forgot a unit, centroids of the codebook before set_weights, a seed under that codebook, a sub-block filed
under the wrong slot or the ignored tail of a partial group into a dropped BMU block -- a wrong id here.

Every exact engine is paired with a precision='f32' engine.  Teacher-forced resident epoch: set_weights(A), set_data,
epoch_accumulate (the last BMUs are the sheet units), set_weights(B) (ids_valid survives it), epoch_accumulate -- ids equal
the float32 engine's on every row and the float64 BMU on every adversarial row, the launch ran under a plan and skipped
(blocks_run < blocks_total); then a real merge (sigma 0.05: most units are reached by no row, den == 0) and a second epoch
on the fused merge's centroids.  After both epochs the device's centroids, radii and |c|^2 are read back
(som_debug_exact_centroids) and compared with float64 values from get_weights().  The same rows then go through bmu (the
scout's plan), a streamed chunk, bmu_top2 and quantization_error.  Arbitrary last units (random, K - 1, the farthest unit; the
BMU, the second- and the fifth-best unit) are planted with epoch_accumulate_forced with the scout off, so that the planted unit
alone bounds the row.

WHAT IT FOUND: nothing.  All cases pass on an MI355X with the kernels as they were; every planned case ran fewer blocks than a
full scan.  Over all cases the device's radius sat between 1.0019529 and 1.0019533 times max |w - c_dev| (the kernel's 1 + 2^-9),
the centroids within 0.053 of their allowance, |c|^2 within 0.28 of its.

MEASURED on an MI355X, teacher-forced epoch under B: executed (256-row tile, 16-unit block) pairs | the model's kept share of
(row, group) and of (row, 16-unit block) pairs (rows, not tiles: a tile runs what any of its 256 rows needs)
  64x64x32 SKIP=2                  803 / 3072 = 0.261 | 0.062, 0.017      (default switches: the same plan, 0.261)
  64x64x3                          718 / 3072 = 0.234 | 0.050, 0.013
  16x16x7                           65 /   96 = 0.677 | 0.448, 0.235
  33x17x128                        140 /  288 = 0.486 | 0.405, 0.146
  70x3x100                          55 /   96 = 0.573 | 0.484, 0.286
  35x15x16                         116 /  216 = 0.537 | 0.480, 0.185
  72x64x128                        824 / 3456 = 0.238 | 0.045, 0.011
  64x64x32 SUBBLOCKS=0            1116 / 3072 = 0.363 | 0.062, 0.062
  64x64x32 SUB44=0                 945 / 3072 = 0.308 | 0.061, 0.023
  33x17x128 PASS_ROWS=1024 n=2537  213 /  360 = 0.592 | 0.475, 0.160
  64x64x200 (wide)                 916 / 2048 = 0.447 | 0.059, 0.059
  64x72x129 (wide)                 968 / 2304 = 0.420 | 0.054, 0.054
  64x64x800 (wide)                 728 / 1536 = 0.474 | 0.061, 0.061
  collinear 32x32x8, every eps     182 /  384 (scout off), 169 / 384 (scout on)
Queries and streamed chunks ran under a plan that skipped in every SKIP=2 case (64x64x32: 656 / 3072 and 922 / 3328 blocks);
with the default switches neither planned (3 072 rows are too few for the scout) and only the ids are checked there.
Planted last units: random units, unit K - 1 and the farthest unit keep every block on the 64 x 64 maps (198 / 216 on
35x15x16) -- a valid, useless bound; the BMU itself, the second-best and the fifth-best unit as the last unit run 669, 694 and
695 of 3072 (33x17x128: 159, 169, 168 of 288; 35x15x16: 130, 129, 144 of 216; 64x64x200: 860, 848, 840 of 2048).
Collinear rows: the float64 margin exceeds the float32 window on 15, 14, 4 and 0 of the 15 collinear rows at eps = 2^-2, 2^-5,
2^-8, 2^-12 (and on every filler row).  The cap of 10 % left out is taken over the collinear rows and holds at 2^-2 and 2^-5
(skip_ref.COLLINEAR_F64_EPS, checked on the CPU); at 2^-8 and 2^-12 the float64 check covers the decided rows only and the
collinear rows' check is the float32 engine's ids.
"""
import contextlib
import os

import numpy as np
import pytest

from tests import skip_ref as R
from tests.query_ref import check_qe

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
ENV_KEYS = ("SOM_EXACT_SKIP", "SOM_EXACT_SUBBLOCKS", "SOM_EXACT_SUB44", "SOM_EXACT_PASS_ROWS", "SOM_EXACT_RESORT",
            "SOM_EXACT_SCOUT", "SOM_EXACT_REFINE", "SOM_EXACT_QUEUE", "SOM_EXACT_CHAIN", "SOM_EXACT_FUSE_SELECT", "SOM_FUSE_MERGE",
            "SOM_VERIFY")
CASES = R.CASES
MOVED = [c for c in CASES if c["kind"] == "moved_units"]
COLLINEAR = [c for c in CASES if c["kind"] == "collinear"]
SIGMA_MERGE = 0.05                           # exp(-1 / (2 sigma^2)) = exp(-200) = 0 in float32: a unit no row picks keeps den == 0


def ids_of(cases):
    return [c["id"] for c in cases]


@contextlib.contextmanager
def case_env(env):
    """The library reads its switches in som_create: set them around the handles' creation, restore afterwards."""
    old = {k: os.environ.get(k) for k in ENV_KEYS}
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@contextlib.contextmanager
def engines(c, env=None):
    from xpysom_dask_amd.engine import HipEngine
    with case_env(c["env"] if env is None else env):
        f = HipEngine(c["X"], c["Y"], c["D"], precision="f32")
        x = HipEngine(c["X"], c["Y"], c["D"], precision="exact")
    try:
        yield f, x
    finally:
        f.close()
        x.close()


def both(f, x, name, *args):
    getattr(f, name)(*args)
    getattr(x, name)(*args)


def same_ids(f, x, what):
    a, b = f.epoch_fetch()[2], x.epoch_fetch()[2]
    bad = np.flatnonzero(a != b)
    assert len(bad) == 0, "%s: %d rows leave the float32 ids, first %s: exact %s, float32 %s" % (what, len(bad), bad[:6], b[bad[:6]], a[bad[:6]])
    return b


def f64_ids(ids, b, rows, what):
    bad = rows[ids[rows] != b["bmu"][rows]]
    assert len(bad) == 0, "%s: %d rows leave the float64 BMU, first %s: got %s, float64 %s (margin %s)" % (
        what, len(bad), bad[:6], ids[bad[:6]], b["bmu"][bad[:6]], b["margin"][bad[:6]])


class Launch:
    """The exact engine's counters around one launch."""

    def __init__(self, x):
        self.x = x

    def __enter__(self):
        self.s0, self.r0, self.t0 = self.x.exact_skip_stats(), self.x.exact_resident_stats()[0], self.x.exact_scout_stats()[1]
        return self

    def __exit__(self, *exc):
        s1 = self.x.exact_skip_stats()
        self.run, self.total = s1[0] - self.s0[0], s1[1] - self.s0[1]
        self.planned = self.x.exact_resident_stats()[0] - self.r0
        self.transient = self.x.exact_scout_stats()[1] - self.t0
        return False

    def assert_skipped(self, what, resident=True):
        """A resident epoch must have advanced exact_resident_stats; a query or a streamed chunk the transient plans' counter."""
        assert (self.planned if resident else self.transient) >= 1, "%s: the launch did not run under a plan" % what
        assert 0 < self.run < self.total, "%s: the plan ran %d of %d blocks: a full scan proves nothing" % (what, self.run, self.total)


# ------------------------------------------------------------------------------------------------ centroid readback
def check_centroids(x, perm, levels, what):
    """The device's centroids, radii and |c|^2 of every slot against float64 values from the codebook the engine holds."""
    w = x.get_weights().astype(F64)
    K, D = w.shape
    worst = dict(r_lo=np.inf, r_hi=0.0, c=0.0, csq=0.0)
    for level in range(levels):
        Cd, rd, qd = x.debug_exact_centroids(level)
        assert len(rd) == R.n_slots(K, level), (what, level, len(rd))
        Cd, rd, qd = Cd.astype(F64), rd.astype(F64), qd.astype(F64)
        for s in range(len(rd)):
            units = perm[R.block_positions(K, level, s)]
            tag = "%s level %d slot %d" % (what, level + 1, s)
            if not len(units):
                assert rd[s] == -1.0, "%s: an empty slot has radius %r" % (tag, rd[s])
                continue
            wk = w[units]
            if np.isnan(wk).any():
                assert np.isnan(rd[s]), "%s: a NaN unit, radius %r" % (tag, rd[s])
                continue
            far = np.sqrt(((wk - Cd[s]) ** 2).sum(1)).max()
            assert rd[s] >= far, "%s: radius %r below max |w - c_dev| = %r (%d units)" % (tag, rd[s], far, len(units))
            assert rd[s] <= far * (1 + 2.0 ** -9) * (1 + 2.0 ** -10) + 1e-29, "%s: radius %r, max |w - c_dev| = %r" % (tag, rd[s], far)
            cerr = np.abs(Cd[s] - wk.mean(0))
            cbound = 64 * 2.0 ** -23 * np.abs(wk).max(0)
            assert (cerr <= cbound).all(), "%s: centroid off by %r in feature %d (bound %r)" % (
                tag, cerr.max(), int(np.argmax(cerr - cbound)), cbound[int(np.argmax(cerr - cbound))])
            q = (Cd[s] * Cd[s]).sum()
            assert abs(qd[s] - q) <= D * 2.0 ** -23 * q, "%s: |c|^2 %r, sum of c_dev^2 %r" % (tag, qd[s], q)
            worst["r_lo"] = min(worst["r_lo"], rd[s] / far if far > 0 else np.inf)
            worst["r_hi"] = max(worst["r_hi"], rd[s] / far if far > 0 else 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                worst["c"] = max(worst["c"], float(np.nanmax(np.where(cbound > 0, cerr / cbound, 0.0))))
            worst["csq"] = max(worst["csq"], abs(qd[s] - q) / (D * 2.0 ** -23 * q) if q > 0 else 0.0)
    return {k: round(float(v), 7) for k, v in worst.items()}


# ------------------------------------------------------------------------------------------------ the teacher-forced epoch
@pytest.mark.parametrize("c", MOVED, ids=ids_of(MOVED))
def test_teacher_forced_epoch_after_a_moved_codebook(c):
    b = R.build(c)
    levels = R.levels_of(c)
    adv, full = b["adv"], c["check"] == "full"
    with engines(c) as (f, x):
        both(f, x, "set_weights", b["wA"])
        both(f, x, "set_data", b["x"])
        both(f, x, "epoch_accumulate", 1.0, 0.5, True)
        last = same_ids(f, x, c["id"] + " under A")
        assert np.array_equal(last[adv], b["last"][adv]), "the adversarial rows' last units are not the model's"
        both(f, x, "set_weights", b["wB"])
        with Launch(x) as l1:
            both(f, x, "epoch_accumulate", SIGMA_MERGE, 0.5, True)
        ids = same_ids(f, x, c["id"] + " under B")
        f64_ids(ids, b, adv, c["id"] + " under B")
        k1, k2 = R.plan(b, None, levels)
        print("%s executed %d / %d = %.3f | model %.3f groups, %.3f blocks" % ((c["id"], l1.run, l1.total, l1.run / max(1, l1.total)) + R.shares(b, k1, k2)))
        if full:
            l1.assert_skipped(c["id"] + " under B")
            print("   centroids after set_weights:", check_centroids(x, b["perm"], levels, c["id"] + " after set_weights"))
        # a real merge (most units: den == 0, the old weights stay), then the epoch on the merged codebook: the fused merge's centroids
        both(f, x, "epoch_merge")
        wm = x.get_weights()
        assert np.array_equal(wm, f.get_weights()) and not np.array_equal(wm, b["wB"])
        assert (wm == b["wB"]).all(axis=1).sum() >= len(wm) // 8, "the merge reached nearly every unit: no den == 0 rows"
        with Launch(x) as l2:
            both(f, x, "epoch_accumulate", 1.0, 0.5, True)
        same_ids(f, x, c["id"] + " after the merge")
        if full:
            l2.assert_skipped(c["id"] + " after the merge")
            print("   centroids after the merge:  ", check_centroids(x, b["perm"], levels, c["id"] + " after the merge"))


@pytest.mark.parametrize("c", [MOVED[3], MOVED[4], MOVED[11]], ids=ids_of([MOVED[3], MOVED[4], MOVED[11]]))
def test_a_nan_unit_gives_its_blocks_a_nan_radius(c):
    """A group (and sub-block) holding a NaN unit has a NaN radius: it is never skipped; every other slot keeps its bounds."""
    b = R.build(c)
    K = c["X"] * c["Y"]
    w = b["wB"].copy()
    w[b["perm"][K // 2]] = np.nan
    with engines(c) as (f, x):
        both(f, x, "set_weights", w)
        both(f, x, "set_data", b["x"])
        both(f, x, "epoch_accumulate", 1.0, 0.5, True)
        same_ids(f, x, c["id"] + " first epoch")
        with Launch(x) as l:
            both(f, x, "epoch_accumulate", 1.0, 0.5, True)
        same_ids(f, x, c["id"] + " second epoch")
        assert l.planned >= 1
        check_centroids(x, b["perm"], R.levels_of(c), c["id"] + " with a NaN unit")
        rad = x.debug_exact_centroids(0)[1]
        assert np.isnan(rad[(K // 2) >> 6]) and np.isnan(rad).sum() == 1


def test_readback_refuses_a_handle_without_centroids():
    from xpysom_dask_amd.engine import HipEngine, SomHipError
    with case_env({}):
        x = HipEngine(16, 16, 7, precision="exact")
    try:
        x.set_weights(R.build(MOVED[3])["wA"])
        with pytest.raises(SomHipError):
            x.debug_exact_centroids(0)
    finally:
        x.close()


# ------------------------------------------------------------------------------------------------ the same rows on the other paths
@pytest.mark.parametrize("c", MOVED, ids=ids_of(MOVED))
def test_the_same_rows_as_query_stream_top2_and_quantization_error(c):
    """bmu takes the scout's path (a plan over transient rows), a streamed chunk another transient plan; bmu_top2 and
    quantization_error search in their own way.  Where the counters show a plan, it must have skipped; where they show none
    (printed), the ids are all the test has."""
    b = R.build(c)
    adv = b["adv"]
    with engines(c) as (f, x):
        both(f, x, "set_weights", b["wB"])
        with Launch(x) as lq:
            iq_f, iq_x = f.bmu(b["x"]), x.bmu(b["x"])
        assert np.array_equal(iq_f, iq_x), (c["id"], np.flatnonzero(iq_f != iq_x)[:6])
        f64_ids(iq_x, b, adv, c["id"] + " query")
        if lq.transient:
            lq.assert_skipped(c["id"] + " query", resident=False)
        with Launch(x) as ls:
            outs = []
            for e in (f, x):
                e.stream_epoch_accumulate([b["x"][:1000], b["x"][1000:]], 1.0, 0.5, True)
                outs.append(e.epoch_fetch(want_bmu=False)[:2])
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), c["id"] + ": streamed accumulators differ"
        if ls.transient:
            ls.assert_skipped(c["id"] + " stream", resident=False)
        (a_f, s_f), (a_x, s_x) = f.bmu_top2(b["x"]), x.bmu_top2(b["x"])
        assert np.array_equal(a_f, a_x) and np.array_equal(s_f, s_x), c["id"] + ": top-2 ids differ"
        f64_ids(a_x, b, adv, c["id"] + " top-2")
        q_f, q_x = f.quantization_error(b["x"]), x.quantization_error(b["x"])
        assert abs(q_f - q_x) <= 1e-6 * q_f, (q_f, q_x)
        check_qe(q_x, b["x"], b["wB"], iq_x, c["id"] + " quantization_error")
        print("%s: query planned %d (%d / %d blocks), stream planned %d (%d / %d blocks)" % (
            c["id"], lq.transient, lq.run, lq.total, ls.transient, ls.run, ls.total))


# ------------------------------------------------------------------------------------------------ arbitrary last units
PLANTED = [MOVED[0], MOVED[4], MOVED[6], MOVED[11]]


@pytest.mark.parametrize("c", PLANTED, ids=ids_of(PLANTED))
def test_any_planted_last_unit_gives_a_valid_bound(c):
    """Random units, unit K - 1 and the unit farthest from each row (valid bounds that keep nearly everything), then the BMU
    itself, the second-best and the fifth-best unit (bounds under which most blocks are skipped), planted with
    epoch_accumulate_forced after one real epoch; the scout is off, so the planted unit alone bounds its row."""
    b = R.build(c)
    K = c["X"] * c["Y"]
    rng = np.random.RandomState(R.case_seed(c))
    xs, ws = b["x"].astype(F64), b["wB"].astype(F64)
    d2 = (xs * xs).sum(1)[:, None] - 2.0 * xs @ ws.T + (ws * ws).sum(1)[None, :]
    near = np.argsort(d2, axis=1, kind="stable")[:, :5]
    plants = (("random", rng.randint(K, size=len(xs))), ("last", np.full(len(xs), K - 1)), ("farthest", np.argmax(d2, axis=1)),
              ("the BMU", b["bmu"]), ("second", near[:, 1]), ("fifth", near[:, 4]))
    with engines(c, dict(c["env"], SOM_EXACT_SCOUT="0")) as (f, x):
        both(f, x, "set_weights", b["wB"])
        both(f, x, "set_data", b["x"])
        both(f, x, "epoch_accumulate", 1.0, 0.5, True)
        ref = same_ids(f, x, c["id"] + " first epoch")
        for name, last in plants:
            x.epoch_accumulate_forced(last.astype(np.int32), 1.0, 0.5, True)
            with Launch(x) as l:
                x.epoch_accumulate(1.0, 0.5, True)
            ids = x.epoch_fetch()[2]
            assert l.planned == 1, "%s, %s: the launch did not plan" % (c["id"], name)
            bad = np.flatnonzero(ids != ref)
            assert len(bad) == 0, "%s, last units %s: %d rows leave the float32 ids, first %s" % (c["id"], name, len(bad), bad[:6])
            print("%s, last units %-8s: ran %d / %d blocks" % (c["id"], name, l.run, l.total))
            if name in ("the BMU", "second", "fifth"):              # (near units: a bound that bites -- the plan must skip AND keep the ids)
                l.assert_skipped(c["id"] + " " + name)


# ------------------------------------------------------------------------------------------------ collinear rows
@pytest.mark.parametrize("scout", ["0", "1"], ids=["scout-off", "scout-on"])
@pytest.mark.parametrize("c", COLLINEAR, ids=ids_of(COLLINEAR))
def test_collinear_rows_keep_their_group(c, scout):
    """The row lies beyond its group's farthest unit k on the ray from the centroid; its planted last unit is (1 + eps) times
    as far as k: the bound has a relative slack of eps / 20 (scout off), or none at all once the scout offers k itself."""
    b = R.build(c)
    with engines(c, dict(c["env"], SOM_EXACT_SCOUT=scout)) as (f, x):
        both(f, x, "set_weights", b["wB"])
        both(f, x, "set_data", b["x"])
        both(f, x, "epoch_accumulate", 1.0, 0.5, True)
        same_ids(f, x, c["id"] + " first epoch")
        both(f, x, "epoch_accumulate_forced", b["last"], 1.0, 0.5, True)
        with Launch(x) as l:
            both(f, x, "epoch_accumulate", 1.0, 0.5, True)
        ids = same_ids(f, x, c["id"])
        l.assert_skipped(c["id"])
        left_out = R.undecided(b)
        if c["eps"] in R.COLLINEAR_F64_EPS:
            assert left_out[b["adv"]].mean() <= R.COLLINEAR_F64_CAP            # (of the collinear rows: the filler is always decided)
        f64_ids(ids, b, np.flatnonzero(~left_out), c["id"])
        print("%s scout %s: ran %d / %d blocks; float64 decides %d of %d rows, %d of the %d collinear ones" % (
            c["id"], scout, l.run, l.total, int((~left_out).sum()), len(ids), int((~left_out[b["adv"]]).sum()), len(b["adv"])))

