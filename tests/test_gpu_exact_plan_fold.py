"""Exact mode, euclidean, up to 128 features, under a plan: the row threshold P folded into the plan kernels' extra MFMA step
(plan_split_threshold / plan_extra_step / plan_run_tile of csrc/exact_skip.hpp, the default) against the compare with P that it
replaces (SOM_EXACT_PLAN_FOLD=0), and against the float32 engine.  GPU only (`-m gpu`).

The folded test subtracts P~ = c (p1 + p2 + p3) >= P from every accumulator and reads a sign; tests/test_plan_fold_cpu.py checks the
split itself.  Here the kernels run: the teacher-forced resident epoch of tests/test_gpu_skip_bound.py (tests/skip_ref.py's moved
units: codebook A, then B, whose moved units punish a plan that drops a block) on 64 x 64 maps, the smallest with a plan -- a single
stage of 64 groups, so the fused launch (one workgroup per tile) serves them --, rows 3 072 and 2 537 (a last tile that is not
full), features 7, 33, 64, 100, 128 (every KS32 with a padded tail), fused and split plans, with and without level 2.  Under B the
epoch is repeated without a merge: the first planned launch is one the policy times (always the split kernels), the next ones are
not, and take the fused launch where it is switched on.

No case runs bfloat16 operands: every exact handle's screen and plan run IEEE half (ExactEl, csrc/bmu_exact.hpp), and the plan
kernels have no Bf16 instance (tests/test_kernel_instances_cpu.py); the bfloat16 split (8-bit parts) is checked on the CPU.

MEASURED on an MI355X, blocks run by the four launches under B, folded against compared: identical ids in all forty cases; the
folded plan never ran fewer blocks and in 18 of the 40 cases ran a few more -- per launch 0 to 4 of 600 to 1 200 (0.6 % at most);
summed over a case's four launches 1, 3, 4, 8 or 16 blocks, the 16 at 7 features with 2 537 rows (675 / 624 / 624 / 624 against
671 / 620 / 620 / 620 of 2 560) and at 100 features without level 2 (1 168 / 1 076 x 3 against 1 164 / 1 072 x 3 of 3 072).  The two
tests differ only through P~: one float32 step, 2^-19 relative from the split, and 28 more ulps of S'Bm' in the folded threshold's
MFMA charge (at 7 features 76 ulps where the compare charges 48).  Codebooks scaled by 2^-20 and 2^20 against the rows run every
block under either test (3 072 of 3 072)."""
import contextlib
import os

import numpy as np
import pytest

from tests import skip_ref as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
X = Y = 64
K = X * Y
TILE = 256
SIGMA = 0.05
ROWS = (3072, 2537)
FEATURES = (7, 33, 64, 100, 128)
ENV_KEYS = ("SOM_EXACT_SKIP", "SOM_EXACT_SUBBLOCKS", "SOM_EXACT_FUSE_PLAN", "SOM_EXACT_PLAN_FOLD", "SOM_EXACT_RESORT", "SOM_EXACT_SCOUT")
EPOCHS_B = 4                                 # launches under B: one timed (split), three not (fused where switched on)
# |blocks run folded - blocks run compared| summed over a case's four launches under B, the largest over the forty cases as measured
# on an MI355X (the module's docstring).  Asserted: this plus one block per tile and launch.
FOLD_DIFF_MEASURED = 16


@contextlib.contextmanager
def _env(env):
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


def _switches(fuse, sub, fold):
    return {"SOM_EXACT_SKIP": "2", "SOM_EXACT_FUSE_PLAN": str(int(fuse)), "SOM_EXACT_SUBBLOCKS": str(int(sub)),
            "SOM_EXACT_PLAN_FOLD": str(int(fold)), "SOM_EXACT_RESORT": "1000"}


_DATA, _REF, _RUNS = {}, {}, {}


def _data(d, n):
    if (d, n) not in _DATA:
        b = R.moved_units(X, Y, d, n, (d * 17 + n) % 100003)
        _DATA[(d, n)] = dict(x=b["x"], wA=b["wA"], wB=b["wB"])
    return _DATA[(d, n)]


def _reference(key, dat):
    """The float32 engine's ids under A and under B, once per data set."""
    if key not in _REF:
        from xpysom_dask_amd.engine import HipEngine
        with _env({}):
            f = HipEngine(X, Y, dat["x"].shape[1], precision="f32")
        try:
            f.set_weights(dat["wA"])
            f.set_data(dat["x"])
            f.epoch_accumulate(1.0, 0.5, True)
            a = f.epoch_fetch()[2].copy()
            f.set_weights(dat["wB"])
            f.epoch_accumulate(SIGMA, 0.5, True)
            _REF[key] = (a, f.epoch_fetch()[2].copy())
        finally:
            f.close()
    return _REF[key]


def _run(key, dat, fuse, sub, fold, epochs=EPOCHS_B):
    """One exact engine through the teacher-forced epoch: ids under A, then per launch under B the ids and (blocks run, blocks in
    all); the plans by form (folded, compared) and by launch (fused, split).  Cached: several tests read the same run."""
    rk = (key, fuse, sub, fold, epochs)
    if rk in _RUNS:
        return _RUNS[rk]
    from xpysom_dask_amd.engine import HipEngine
    with _env(_switches(fuse, sub, fold)):
        e = HipEngine(X, Y, dat["x"].shape[1], precision="exact")
    try:
        e.set_weights(dat["wA"])
        e.set_data(dat["x"])
        e.epoch_accumulate(1.0, 0.5, True)
        rec = dict(ids_a=e.epoch_fetch()[2].copy(), ids_b=[], blocks=[])
        e.set_weights(dat["wB"])
        fold0, plan0, res0 = e.exact_plan_fold_stats(), e.exact_plan_stats(), e.exact_resident_stats()[0]
        for _ in range(epochs):
            s0 = e.exact_skip_stats()
            e.epoch_accumulate(SIGMA, 0.5, True)
            s1 = e.exact_skip_stats()
            rec["ids_b"].append(e.epoch_fetch()[2].copy())
            rec["blocks"].append((s1[0] - s0[0], s1[1] - s0[1]))
        rec["fold"] = tuple(np.subtract(e.exact_plan_fold_stats(), fold0))
        rec["plan"] = tuple(np.subtract(e.exact_plan_stats(), plan0))
        rec["planned"] = e.exact_resident_stats()[0] - res0
    finally:
        e.close()
    _RUNS[rk] = rec
    return rec


def _assert_ids(rec, ref, what):
    assert np.array_equal(rec["ids_a"], ref[0]), "%s under A: %d rows leave the float32 ids" % (what, int((rec["ids_a"] != ref[0]).sum()))
    for i, ids in enumerate(rec["ids_b"]):
        bad = np.flatnonzero(ids != ref[1])
        assert len(bad) == 0, "%s under B, launch %d: %d rows leave the float32 ids, first %s: exact %s, float32 %s" % (
            what, i, len(bad), bad[:6], ids[bad[:6]], ref[1][bad[:6]])


CASES = [(d, n, fuse, sub) for d in FEATURES for n in ROWS for fuse in (1, 0) for sub in (1, 0)]
CASE_IDS = ["d%d-n%d-%s-%s" % (d, n, "fused" if fuse else "split", "l2" if sub else "l1") for d, n, fuse, sub in CASES]


@pytest.mark.parametrize("d,n,fuse,sub", CASES, ids=CASE_IDS)
def test_folded_plan_keeps_the_float32_ids(d, n, fuse, sub):
    """1. FOLD=1: the float32 engine's ids on every row, every launch planned, folded, and skipping."""
    dat = _data(d, n)
    rec = _run((d, n), dat, fuse, sub, 1)
    _assert_ids(rec, _reference((d, n), dat), CASE_IDS[CASES.index((d, n, fuse, sub))])
    print("folded %s: blocks %s, plans (folded, compared) %s, (fused, split) %s" % ((d, n, fuse, sub), rec["blocks"], rec["fold"], rec["plan"]))
    assert rec["planned"] == EPOCHS_B, "launches under a plan: %d of %d" % (rec["planned"], EPOCHS_B)
    assert rec["fold"][0] == EPOCHS_B and rec["fold"][1] == 0, "the plans did not run folded: %r" % (rec["fold"],)
    for run, total in rec["blocks"]:
        assert 0 < run < total, "the plan ran %d of %d blocks: a full scan proves nothing" % (run, total)
    if fuse and sub:
        assert rec["plan"][0] >= 1, "no launch took the fused plan: (fused, split) = %r" % (rec["plan"],)
    else:
        assert rec["plan"][0] == 0, "the fused plan ran where it is switched off or has no level 2: %r" % (rec["plan"],)


@pytest.mark.parametrize("d,n,fuse,sub", CASES, ids=CASE_IDS)
def test_folded_and_compared_plans_agree(d, n, fuse, sub):
    """2. FOLD=1 against FOLD=0 on identical inputs: identical ids; blocks run within the measured difference (FOLD_DIFF_MEASURED,
    over the launches under B) plus one block per tile and launch."""
    dat = _data(d, n)
    a, b = _run((d, n), dat, fuse, sub, 1), _run((d, n), dat, fuse, sub, 0)
    assert b["fold"][1] == EPOCHS_B and b["fold"][0] == 0, "SOM_EXACT_PLAN_FOLD=0 did not run the compare: %r" % (b["fold"],)
    assert np.array_equal(a["ids_a"], b["ids_a"])
    for i, (u, v) in enumerate(zip(a["ids_b"], b["ids_b"])):
        assert np.array_equal(u, v), "launch %d: %d ids differ between the folded and the compared plan" % (i, int((u != v).sum()))
    diff = sum(abs(p[0] - q[0]) for p, q in zip(a["blocks"], b["blocks"]))
    print("fold-vs-compare %s: folded %s, compared %s, |difference| %d" % ((d, n, fuse, sub), a["blocks"], b["blocks"], diff))
    assert [p[1] for p in a["blocks"]] == [q[1] for q in b["blocks"]]
    tiles = -(-n // TILE)
    assert diff <= FOLD_DIFF_MEASURED + tiles * EPOCHS_B, "blocks run differ by %d (measured %d + %d tiles x %d launches)" % (
        diff, FOLD_DIFF_MEASURED, tiles, EPOCHS_B)


# ------------------------------------------------------------------------------------------------ rows that keep everything
def _one_tile(d=32, seed=5):
    """255 ordinary rows near the units of the first four patches of a sheet, and one slot (row 100) for a planted row: ONE tile, so
    'the tile runs every block' reads blocks run == blocks in all."""
    rng = np.random.RandomState(seed)
    w = R.sheet(X, Y, d, rng)
    perm = R.patch_order(X, Y)
    units = perm[rng.randint(256, size=TILE)]
    x = (w[units].astype(F64) + 0.02 * rng.standard_normal((TILE, d))).astype(F32)
    return w, x


def _planted(kind, w, x):
    w2, x2 = w.copy(), x.copy()
    if kind == "nan":
        x2[100, 3] = np.nan
    elif kind == "inf":
        x2[100, 1] = np.inf
    elif kind == "zero":
        x2[100] = 0.0
    elif kind == "far":
        # the row's last BMU (under A) is carried far away in B: sqrt(U) -- the row's distance to that unit -- is then more than four
        # times the longest row, and sx sqrt(U) leaves the half range (the longest row's scaled norm is in [2^13, 2^14))
        xs, ws = x.astype(F64), w.astype(F64)
        u = int(np.argmin(((xs[100][None, :] - ws) ** 2).sum(1)))
        w2[u, 2] += F32(12.0 * np.sqrt((xs * xs).sum(1).max()))
    return w2, x2


@pytest.mark.parametrize("kind", ["nan", "inf", "far", "zero"])
@pytest.mark.parametrize("fuse", [1, 0], ids=["fused", "split"])
def test_rows_that_must_keep_everything(kind, fuse):
    """3. One row with a NaN feature, one with +inf, one whose sx sqrt(U) leaves the half range, one all-zero row, each in a tile of
    ordinary rows: the float32 engine's ids, and for the first three the tile runs every block (without the row it does not).
    MEASURED: the plain tile runs 27 of 256 blocks in every launch; with the NaN, the +inf and the zero row 256 of 256 in every
    launch; with the far row 256 in the teacher-forced launch and 32 after it."""
    w, x = _one_tile()
    base = dict(x=x, wA=w, wB=w)
    wB, xp = _planted(kind, w, x)
    dat = dict(x=xp, wA=w, wB=wB)
    r0 = _run(("tile", "plain"), base, fuse, 1, 1)
    r1 = _run(("tile", kind), dat, fuse, 1, 1)
    _assert_ids(r0, _reference(("tile", "plain"), base), "plain tile")
    _assert_ids(r1, _reference(("tile", kind), dat), "tile with a %s row" % kind)
    print("tile %s: plain %s, planted %s, plans %s %s" % (kind, r0["blocks"], r1["blocks"], r1["fold"], r1["plan"]))
    assert r1["fold"] == (EPOCHS_B, 0) and r0["fold"] == (EPOCHS_B, 0)
    if fuse:
        assert r1["plan"][0] >= 1
    for run, total in r0["blocks"]:
        assert 0 < run < total, "the plain tile ran %d of %d blocks" % (run, total)
    if kind != "zero":
        # (the far row's bound is its LAST unit's: the first launch under B is the teacher-forced one -- a launch the policy times, so
        #  the split kernels' --, after it the row's last unit is its BMU under B and the row is an ordinary one)
        for run, total in r1["blocks"][:1 if kind == "far" else EPOCHS_B]:
            assert run == total == K // 16, "a tile with a %s row ran %d of %d blocks" % (kind, run, total)


# ------------------------------------------------------------------------------------------------ the scale at its extremes
@pytest.mark.parametrize("log2", [-20, 20])
@pytest.mark.parametrize("fuse", [1, 0], ids=["fused", "split"])
def test_codebooks_far_from_the_rows_scale(log2, fuse):
    """4. The codebook scaled by 2^-20 and by 2^20 against the rows, 32 features: S'Bm', the scale c and the small parts of the split
    at their extremes.  The float32 engine's ids (what such a plan can skip is not asserted)."""
    b = _data(32, 3072)
    s = F32(2.0 ** log2)
    dat = dict(x=b["x"], wA=b["wA"] * s, wB=b["wB"] * s)
    rec = _run((32, 3072, log2), dat, fuse, 1, 1)
    _assert_ids(rec, _reference((32, 3072, log2), dat), "codebook x 2^%d" % log2)
    old = _run((32, 3072, log2), dat, fuse, 1, 0)
    _assert_ids(old, _reference((32, 3072, log2), dat), "codebook x 2^%d, compared" % log2)
    print("codebook x 2^%d: blocks folded %s, compared %s, plans %s %s" % (log2, rec["blocks"], old["blocks"], rec["fold"], rec["plan"]))
    assert rec["fold"][1] == 0 and old["fold"][0] == 0
