"""The 16-bit BMU search (precision 'bf16' / 'f16': bmu_bf16_k16_kernel, bmu_bf16_tiled_kernel, bmu_bf16_wide_kernel and the
preparation kernels that feed them) against the float64 reference ON THE ROUNDED OPERANDS of tests/half_ref.py.
GPU only (`-m gpu`).

Every case is teacher-forced through HipEngine: set a codebook, query the rows AND run them as the resident set
(epoch_accumulate), compare both with the reference built from the codebook the engine holds (get_weights).  The checks and
their bounds are half_ref's: admissible picks within the float32 arithmetic's bound, the lowest-index argmin on pinned
integer data, and the rigorous operand bound against the unrounded float64 distances.  tests/test_half_ref_cpu.py shows
that CASES reaches every label half_ref.half_paths names.

What it found: every kernel resolved EXACT ties between units of different stages (unit blocks) held by one lane towards
the lower (tile << 2 | register) code instead of the lower unit -- the stage fold compared whole keys, index bits included.
On the kernels before the fix case 17x241x200-n257-bf16-euclidean-int-SOM_BF16_PARTS3 picked unit 3628 for 2911 (row 11),
and test_equal_units_in_two_stages_of_one_lane_go_to_the_lower_unit failed in all three families; the folds now compare
the value bits only and both pass.

Measured on an MI355X with the fix in: all cases pass; worst excess / allowance of the operand bound k16 0.22, tiled
0.012, wide 0.014; no pick anywhere sat above min_j (s_j + E_j) (pick ratio 0: the float32 bound has room -- KAPPA = 6
charges 2.5 times the measured MFMA error, and the key floor is charged to both sides).  The f16 MFMA KEEPS subnormal
inputs (no flush)."""
import contextlib
import os

import numpy as np
import pytest

from tests.half_ref import KEY_ULPS, check_half, family_of, half_paths, half_scores, make_half_data

pytestmark = pytest.mark.gpu
F32 = np.float32
ENV_KEYS = ("SOM_BF16_PARTS", "SOM_BF16_WIDE", "SOM_FUSE_MERGE", "SOM_VERIFY")


def _case(X, Y, D, n, prec, dist="euclidean", data="blobs", env=None, epochs=0, dup=0, seed=None):
    c = dict(X=X, Y=Y, D=D, n=n, prec=prec, dist=dist, data=data, env=dict(env or {}), epochs=epochs, dup=dup, seed=seed)
    c["id"] = "%dx%dx%d-n%d-%s-%s-%s%s%s" % (X, Y, D, n, prec, dist, data, "-ep%d" % epochs if epochs else "",
                                             "".join("-%s%s" % kv for kv in sorted(c["env"].items())))
    return c


def P(n):
    return {"SOM_BF16_PARTS": str(n)}


NOWIDE = {"SOM_BF16_WIDE": "0"}
_WIDE_DATA = ("blobs", "int", "offset30", "offset300", "tiny")
_WIDE_ROWS = (1, 127, 255, 256, 257, 600)
_WIDE_MAPS = ((64, 64), (17, 241), (64, 65))


def _wide_cases():
    """KS32 = 5 .. 25, the operand types alternating (half_ref.required_type), feature counts at and off multiples of 32
    and 8, maps on both sides of a 32-unit stage; cosine on bf16 at every fourth (half's ambiguous share grows with D)."""
    out = []
    for ks in range(5, 26):
        D = 800 if ks == 25 else (32 * ks, 32 * ks - 31, 32 * ks - 7, 32 * ks - 8)[ks % 4]
        X, Y = _WIDE_MAPS[ks % 3]
        prec = "bf16" if ks % 2 else "f16"
        dist = "cosine" if ks % 4 == 1 else "euclidean"
        data = _WIDE_DATA[ks % 5] if dist == "euclidean" else "blobs"
        out.append(_case(X, Y, D, _WIDE_ROWS[ks % 6], prec, dist, data, dup=5 if data == "int" else 0))
    return out


CASES = [
    # bmu_bf16_k16_kernel: KS32 = 1 .. 4, both types; maps off the 64-unit stage; rows 1 .. a few thousand
    _case(1, 1, 1, 1, "bf16"),
    _case(3, 5, 8, 127, "f16", data="int", dup=3),
    _case(3, 43, 8, 129, "bf16", data="int", dup=20),
    _case(7, 9, 31, 255, "bf16", data="offset30"),
    _case(5, 13, 33, 256, "f16"),
    _case(9, 15, 64, 257, "f16", data="offset300"),
    _case(8, 8, 96, 129, "bf16", data="int", dup=8),
    _case(3, 43, 97, 255, "f16", data="tiny"),
    _case(1, 127, 128, 3001, "bf16"),
    _case(64, 64, 128, 256, "f16"),
    _case(63, 65, 128, 257, "bf16", data="offset30"),
    _case(9, 15, 64, 200, "f16", data="huge"),
    _case(20, 24, 100, 300, "f16", data="int", dup=30),
    # ... forced part counts, and the few-row regime that splits into many parts
    _case(9, 15, 64, 257, "bf16", env=P(1)),
    _case(20, 24, 96, 300, "f16", data="int", env=P(3), dup=40),
    _case(20, 24, 128, 255, "bf16", data="offset300", env=P(7)),
    _case(40, 60, 24, 1, "bf16"),
    _case(40, 60, 24, 2, "f16", data="int", dup=50),
    # ... cosine
    _case(7, 9, 31, 255, "bf16", "cosine"),
    _case(9, 15, 64, 257, "f16", "cosine"),
    _case(20, 24, 128, 300, "bf16", "cosine", env=P(3)),
    # bmu_bf16_tiled_kernel 4x2x2 (more than 128 features, fewer than 4096 units)
    _case(3, 43, 129, 129, "bf16"),
    _case(9, 9, 160, 255, "f16", data="int", dup=9),
    _case(1, 127, 801, 127, "bf16", data="offset30"),
    _case(13, 5, 900, 256, "f16"),
    _case(1, 100, 200, 300, "f16", data="offset300"),
    _case(3, 43, 129, 1, "f16", data="tiny"),
    _case(3, 43, 160, 257, "f16", data="int", env=P(3), dup=10),
    _case(2, 8, 265, 257, "bf16", "cosine"),
    _case(13, 5, 140, 127, "f16", "cosine"),
    # bmu_bf16_tiled_kernel 8x2x4 (from 4096 units on: beyond 800 features, or SOM_BF16_WIDE=0)
    _case(64, 64, 801, 255, "bf16"),
    _case(64, 65, 900, 257, "f16", data="offset300"),
    _case(64, 64, 160, 256, "bf16", data="int", env=NOWIDE, dup=64),
    _case(64, 64, 200, 129, "f16", "cosine", env=NOWIDE),
    _case(17, 241, 129, 300, "bf16", env=dict(NOWIDE, **P(7))),
    _case(64, 64, 129, 1, "f16", env=dict(NOWIDE, **P(1))),
    # bmu_bf16_wide_kernel: every KS32, then forced parts and the A/B against the tiled kernel's shape above
    *_wide_cases(),
    _case(64, 64, 160, 256, "bf16", data="int", dup=64),
    _case(64, 64, 200, 129, "f16", "cosine"),
    _case(64, 64, 129, 300, "f16", env=P(1)),
    _case(17, 241, 200, 257, "bf16", data="int", env=P(3), dup=17),
    _case(64, 65, 784, 255, "f16", data="offset300", env=P(7)),
    _case(64, 64, 200, 129, "f16", data="huge"),
    # after two real epochs: the images of the fused merge + preparation kernels, and of the separate launches
    _case(20, 24, 96, 1000, "bf16", epochs=2),
    _case(20, 24, 96, 1000, "bf16", epochs=2, env={"SOM_FUSE_MERGE": "0"}),
    _case(20, 24, 33, 500, "f16", data="offset30", epochs=2),
    _case(64, 64, 200, 700, "f16", epochs=2),
    _case(64, 64, 200, 700, "f16", epochs=2, env={"SOM_FUSE_MERGE": "0"}),
    _case(64, 66, 133, 600, "bf16", "cosine", epochs=2),
    _case(9, 9, 300, 500, "f16", epochs=2),
]

WORST = {}                                   # family -> {check: worst err/bound}, printed by the last test


def engine(X, Y, D, **kw):
    from xpysom_dask_amd.engine import HipEngine
    return HipEngine(X, Y, D, **kw)


@contextlib.contextmanager
def case_env(env):
    """The library reads its switches in som_create: set them around the handle's creation, restore afterwards."""
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


def unit_kind(c):
    """Cosine cases: the data is kept clear of the unit-length rounding boundaries (half_ref.clear_of_boundaries)."""
    return c["prec"] if c["dist"] == "cosine" else None


def case_seed(c):
    if c.get("seed") is not None:
        return c["seed"]
    return (c["X"] * 7919 + c["Y"] * 131 + c["D"] * 17 + c["n"]) % 100003


def _note(worst, fam, res):
    d = worst.setdefault(fam, {})
    for k, v in res.items():
        d[k] = max(d.get(k, 0.0), v)


def _both_paths(e, c, x, w, fam, worst, what, x_res=None):
    """Query path and resident-row path of the same rows: each admissible, and equal to each other."""
    ties = c["data"] == "int" and c["dist"] == "euclidean"
    ku = KEY_ULPS[fam]
    ids = e.bmu(x)
    _note(worst, fam, check_half(ids, x, w, c["prec"], c["dist"], ku, ties, what + " query"))
    xr = x if x_res is None else x_res
    e.set_data(xr)
    e.epoch_accumulate(1.0, 0.1, True)
    res = e.epoch_fetch()[2]
    _note(worst, fam, check_half(res, xr, w, c["prec"], c["dist"], ku, ties, what + " resident"))
    if x_res is None:
        assert np.array_equal(ids, res), "%s: the query and the resident path disagree on %d rows" % (what, (ids != res).sum())


def run_half_case(c, worst=None):
    """One case against the reference; fills worst[family] = {check: err/bound}."""
    worst = WORST if worst is None else worst
    X, Y, D, n = c["X"], c["Y"], c["D"], c["n"]
    K = X * Y
    fam = family_of(half_paths(X, Y, D, n, c["prec"], c["dist"], c["env"], c["epochs"]))
    x, w0 = make_half_data(c["data"], n, K, D, case_seed(c), c["dup"], unit_kind=unit_kind(c))
    x_res = make_half_data(c["data"], n, K, D, case_seed(c), c["dup"], query=False)[0] if c["data"] == "huge" else None
    if c["dist"] == "cosine" and n > 2:
        x[0] = 0                                             # a zero row stays zero: every unit scores 0
    with case_env(c["env"]):
        e = engine(X, Y, D, distance=c["dist"], precision=c["prec"])
    try:
        e.set_weights(w0)
        w = e.get_weights()
        assert np.array_equal(w, w0)
        if not c["epochs"]:
            _both_paths(e, c, x, w, fam, worst, c["id"], x_res)
            return worst
        # two real epochs, then the codebook the engine holds: the picks of the NEXT resident launch (the fused kernels'
        # images and norms) and of a query; then set_weights again (stale images and tails would show)
        e.set_data(x)
        for sigma, eta in ((3.0, 0.5), (1.0, 0.2)):
            e.epoch_accumulate(sigma, eta, True)
            e.epoch_merge()
        w = e.get_weights()
        assert not np.array_equal(w, w0)
        _both_paths(e, c, x, w, fam, worst, c["id"] + " after epochs")
        e.set_weights(w0)
        _both_paths(e, c, x, e.get_weights(), fam, worst, c["id"] + " after set_weights")
    finally:
        e.close()
    return worst


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_case(c):
    run_half_case(c)


# ------------------------------------------------------------------------------------------------ the stage fold
@pytest.mark.parametrize("X,Y,D,prec,env,later", [(8, 16, 24, "bf16", {}, 64 + 12), (8, 16, 96, "f16", P(1), 64 + 12),
                                                  (16, 16, 160, "f16", P(1), 128 + 12), (64, 64, 129, "bf16", dict(NOWIDE, **P(1)), 256 + 12),
                                                  (64, 64, 200, "f16", {}, 32 + 12), (64, 64, 777, "bf16", P(1), 32 + 12)],
                         ids=["k16", "k16-one-part", "tiled4x2x2", "tiled8x2x4", "wide", "wide-one-part"])
def test_equal_units_in_two_stages_of_one_lane_go_to_the_lower_unit(X, Y, D, prec, env, later):
    """The regression case of the stage fold: unit 15 (quad 3, register 3 of its tile: a HIGH index code) is repeated in the
    next stage / unit block at quad 3, register 0 (code 0) -- the same lane holds both, and rows equal to that unit score
    them exactly alike.  A fold that compares whole keys lets the later stage's lower code win wherever one workgroup
    scans both stages (one part; several parts put them in different workgroups, whose 64-bit merge carries the unit)."""
    K = X * Y
    x, w0 = make_half_data("int", 120, K, D, 5)
    w0[later] = w0[15]
    x[:60] = w0[15]
    fam = family_of(half_paths(X, Y, D, len(x), prec, "euclidean", env))
    with case_env(env):
        e = engine(X, Y, D, precision=prec)
    try:
        e.set_weights(w0)
        ids = e.bmu(x)
        assert (ids[:60] == 15).all(), "rows equal to units 15 and %d pick %s" % (later, sorted(set(ids[:60].tolist())))
        check_half(ids, x, e.get_weights(), prec, "euclidean", KEY_ULPS[fam], True, fam)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ streamed epoch
@pytest.mark.parametrize("shape,prec", [((20, 24, 96), "bf16"), ((64, 64, 200), "f16"), ((9, 9, 300), "bf16")])
def test_streamed_chunks_are_picked_with_their_own_offset(shape, prec):
    """A streamed epoch: B is per chunk, the chunks differ in scale by 8 and 1/8.  The picks are not returned, but with a
    neighbourhood narrower than a unit (sigma 0.05: exp(-200) = 0 in float32) the denominator is the histogram of the
    picks.  From each chunk's reference with THAT chunk's B: a row whose only admissible unit is k must count for k, and
    k cannot count more rows than admit it."""
    X, Y, D = shape
    K = X * Y
    fam = family_of(half_paths(X, Y, D, 300, prec, "euclidean"))
    x, w0 = make_half_data("blobs", 900, K, D, 77)
    chunks = [x[:300], x[300:557] * F32(8), x[557:] * F32(0.125)]
    with case_env({}):
        e = engine(X, Y, D, precision=prec)
    try:
        e.set_weights(w0)
        w = e.get_weights()
        e.stream_epoch_accumulate(chunks, 0.05, 0.5, True)
        den = e.epoch_fetch(want_bmu=False)[1].astype(np.float64)
        # h(bmu, bmu) = eta-weighted 1: the denominator is a multiple of one weight; normalise by the total
        assert den.sum() > 0
        counts = den / den.sum() * len(x)
        assert np.abs(counts - np.rint(counts)).max() < 1e-3, "the denominator is not a histogram"
        lo, hi = np.zeros(K), np.zeros(K)
        for ch in chunks:
            s, E = half_scores(ch, w, prec, "euclidean", KEY_ULPS[fam])
            adm = (s - E) <= (s + E).min(axis=1, keepdims=True)
            single = adm.sum(1) == 1
            lo += np.bincount(np.argmax(adm, 1)[single], minlength=K)
            hi += adm.sum(0)
        c = np.rint(counts)
        bad = np.flatnonzero((c < lo) | (c > hi))
        assert len(bad) == 0, "unit %d counts %d rows, the chunks' references allow %d .. %d" % (bad[0], c[bad[0]], lo[bad[0]], hi[bad[0]])
        print("streamed %s: %d of %d rows decided by the bound" % (fam, int(lo.sum()), len(x)))
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ canary
@pytest.mark.parametrize("c", [_case(20, 24, 96, 600, "bf16", data="offset300", env={"SOM_VERIFY": "64"}),
                               _case(9, 9, 300, 600, "f16", data="offset300", env={"SOM_VERIFY": "64"}),
                               _case(64, 64, 900, 300, "bf16", data="offset300", env={"SOM_VERIFY": "64"}),
                               _case(64, 64, 200, 600, "f16", data="offset300", env={"SOM_VERIFY": "64"})],
                         ids=["k16", "tiled4x2x2", "tiled8x2x4", "wide"])
def test_canary_accepts_what_the_reference_admits(c):
    """SOM_VERIFY re-scores strided rows of every launch in float32 with a tolerance of its own: on un-centred rows it must
    not raise on picks this reference admits."""
    worst = {}
    run_half_case(c, worst)                                  # (a SomHipError of the canary fails the test)
    with case_env(c["env"]):
        e = engine(c["X"], c["Y"], c["D"], precision=c["prec"])
    try:
        x, w0 = make_half_data(c["data"], c["n"], c["X"] * c["Y"], c["D"], case_seed(c))
        e.set_weights(w0)
        e.bmu(x)
        launches, rows = e.verify_stats()
        assert launches >= 1 and rows >= 1, "the canary did not run"
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ measurements
def test_does_the_mfma_flush_subnormal_half_inputs():
    """Nobody had measured it: one 16x16x32 f16 MFMA on subnormal inputs (2^-20 times 2^10, 32 products).  Either answer is
    inside half_ref's allowance; the test prints which one the hardware gives."""
    with case_env({}):
        e = engine(4, 4, 8, precision="f16")
    try:
        a = np.full((16, 32), 2.0 ** -20, np.float16)
        b = np.full((32, 16), 2.0 ** 10, np.float16)
        d = e.debug_mfma16(a, b, np.zeros((16, 16), F32), f16=True)
        kept, flushed = 32 * 2.0 ** -10, 0.0
        assert (d == kept).all() or (d == flushed).all(), d
        print("v_mfma_f32_16x16x32_f16 on subnormal inputs: %s" % ("KEPT (no flush)" if (d == kept).all() else "FLUSHED to zero"))
    finally:
        e.close()


def test_zz_report_worst_ratios():
    """Prints the worst err/bound per kernel family over the cases that ran before it in this process."""
    for fam in sorted(WORST):
        print("worst err/bound %s: %s" % (fam, ", ".join("%s %.3g" % kv for kv in sorted(WORST[fam].items()))))
