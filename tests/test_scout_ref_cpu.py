"""tests/scout_ref.py on its own (no GPU): the float64 model of the row sample against a brute-force double loop, the margins of
the three builders and the 1 % cap on undecided pairs at every shape tests/test_gpu_default_plan.py runs, named mutants of the
row-sample kernel that the [sure, sure + maybe] check must reject, and the sample tiles' index map."""
import numpy as np
import pytest

from tests import scout_ref as R
from tests import skip_ref as S

F32, F64 = np.float32, np.float64
SHAPES = sorted(R.SHAPES)
NARROW = [s for s in SHAPES if s[2] <= 128]


def geometry32(w, perm):
    C1, r1, _ = S.geometry(w, perm, 0)
    return C1.astype(F32), r1.astype(F32)


# ------------------------------------------------------------------------------------------------------ the model itself
@pytest.mark.parametrize("X,Y,D,N", [(16, 16, 7, 300), (24, 16, 12, 128), (16, 24, 5, 77), (32, 16, 33, 1000)])
def test_rowneed_ref_equals_a_double_loop(X, Y, D, N):
    rng = np.random.RandomState(X + D + N)
    w = rng.randn(X * Y, D).astype(F32)
    x = (w[rng.randint(X * Y, size=N)] + 0.3 * rng.randn(N, D)).astype(F32)
    x[R.sample_rows(N)[3], 0] = np.nan                      # a NaN row among the sampled ones
    C, r = geometry32(w, S.patch_order(X, Y))
    r = r.copy()
    r[2] = -1.0                                             # a slot without units
    G = S.n_groups(X * Y)
    n = min(128, N)
    step = N // n
    sure = maybe = 0
    for b in range(n):
        row = x[b * step + step // 2].astype(F64)
        live = [g for g in range(G) if r[g] >= 0]
        if np.isnan(row).any():
            sure += len(live)
            continue
        d = {g: float(np.sqrt(sum((row[k] - float(C[g, k])) ** 2 for k in range(D)))) for g in live}
        m = min(d[g] + float(r[g]) for g in live)
        for g in live:
            s = d[g] - float(r[g]) - m
            tau = (D + 4) * 2.0 ** -24 * (d[g] + float(r[g]) + m)
            if s <= -tau:
                sure += 1
            elif abs(s) < tau:
                maybe += 1
    assert R.rowneed_ref(x, C, r, G) == (sure, maybe)
    # (and the float32 emulation of the device's count lies in the model's interval)
    assert sure <= R.rowneed_f32(x, C, r, G) <= sure + maybe


def test_the_sampled_rows_are_the_kernels():
    for N in (128, 129, 255, 256, 65791, 65792, 70001, 147000):
        idx = R.sample_rows(N)
        step = N // 128
        assert len(idx) == 128 and idx[0] == step // 2 and idx[-1] == 127 * step + step // 2 < N
    assert list(R.sample_rows(5)) == [0, 1, 2, 3, 4]


# ------------------------------------------------------------------------------------------------------ the builders' margins
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_margins_of_the_three_builders_and_the_cap_on_undecided_pairs(shape):
    """commit: need < 0.3 (the row sample declines above 0.9); rows_decline: need > 0.97; tiles_decline: need in 0.55 .. 0.85
    with exactly 40 structured rows among the sampled ones; undecided pairs <= 1 % of the sampled pairs everywhere."""
    b = R.build(*shape)
    perm = b["perm"]
    need = {}
    for name in ("commit", "rows_decline", "tiles_decline"):
        w, x = b[name]
        need[name], sure, maybe, pairs = R.predicted_need(w, x, perm)
        print(shape, name, "need %.4f sure %d maybe %d of %d" % (need[name], sure, maybe, pairs))
        assert maybe <= 0.01 * pairs, (name, maybe, pairs)
    assert need["commit"] < 0.3
    assert need["rows_decline"] > 0.97
    assert 0.55 < need["tiles_decline"] < 0.85
    assert len(b["structured"]) == 40 and set(b["structured"]) <= set(R.sample_rows(b["N"]))
    N, K, D = b["N"], shape[0] * shape[1], shape[2]
    assert float(N) * K * D >= 3.0e11, "not worth a scout: the forecast would not run"
    if shape == (192, 192, 128):
        # one row fewer: 256 tiles, no sample tiles -- the row sample alone commits the plan (another step, other rows)
        w, x = b["commit"]
        assert R.predicted_need(w, x[:65791], perm)[0] < 0.3 and 65791 // 256 == 256
    # the undecided pairs with a NaN row at a sampled index as well
    bn = R.build(*shape, nan_row=True)
    for name in ("commit", "tiles_decline"):
        w, x = bn[name]
        assert np.isnan(x[bn["nan_at"]]).any() and bn["nan_at"] in set(R.sample_rows(N))
        _, sure, maybe, pairs = R.predicted_need(w, x, perm)
        assert maybe <= 0.01 * pairs


@pytest.mark.parametrize("shape", NARROW, ids=lambda s: "%dx%dx%d" % s)
def test_the_tiles_margins(shape):
    """commit: the model's level-1 share of the sample tiles, from above, < 0.5 (the tiles decline above 0.8).  tiles_decline:
    every unstructured row ALONE keeps > 0.95 of the 16-unit blocks, from below -- and every tile holds such rows."""
    b = R.build(*shape)
    w, x = b["commit"]
    passes = [x] if shape != (128, 128, 128) else [x, x[:73728]]   # (as one pass of 574 tiles, and pass 0 of two)
    for xs in passes:
        share = R.tile_share_ref(xs, w, b["perm"])
        print(shape, len(xs), "commit: level-1 share of the sample tiles <= %.4f" % share)
        assert share < 0.5
    w, x = b["tiles_decline"]
    N = b["N"]
    rows = np.setdiff1d(np.arange(0, N, N // 256), b["structured"])
    per_row = R.row_block_share_ref(x, w, b["perm"], rows)
    print(shape, "tiles_decline: an unstructured row keeps %.4f .. %.4f of the blocks" % (per_row.min(), per_row.max()))
    assert per_row.min() > 0.95
    # 40 structured rows cannot fill a tile: every tile of 256 rows holds an unstructured one
    assert len(b["structured"]) < R.TILE


# ------------------------------------------------------------------------------------------------------ the mutants
@pytest.mark.parametrize("data", ["commit", "tiles_decline"])
@pytest.mark.parametrize("shape", NARROW, ids=lambda s: "%dx%dx%d" % s)
def test_the_interval_rejects_every_mutant_of_the_row_sample(shape, data):
    """Each mutant, emulated in float32 as a model of the device's count, falls outside [sure, sure + maybe]; the unmutated
    emulation falls inside.  dead_slots runs on a copy of the radii with every seventh slot marked empty (level 1 of a real map
    has none: slot g holds units whenever 64 g < K); nan_nothing on the rows with a NaN row; min256 needs more than 256 groups."""
    b = R.build(*shape)
    bn = R.build(*shape, nan_row=True)
    w, x = b[data]
    xn = bn[data][1]
    C, r = geometry32(w, b["perm"])
    G = S.n_groups(len(w))
    sure, maybe = R.rowneed_ref(x, C, r, G)
    assert sure <= R.rowneed_f32(x, C, r, G) <= sure + maybe
    rd = r.copy()
    rd[::7] = -1.0
    for mutant in R.MUTANTS:
        if mutant == "min256" and G <= 256:
            continue
        xs, rs = (xn if mutant == "nan_nothing" else x), (rd if mutant == "dead_slots" else r)
        lo, may = R.rowneed_ref(xs, C, rs, G)
        assert lo <= R.rowneed_f32(xs, C, rs, G) <= lo + may, mutant
        got = R.rowneed_f32(xs, C, rs, G, mutant)
        print(shape, data, mutant, "counts %d against [%d, %d]" % (got, lo, lo + may))
        assert not (lo <= got <= lo + may), mutant


# ------------------------------------------------------------------------------------------------------ the sample tiles' map
@pytest.mark.parametrize("tiles_all,st", [(257, 2), (383, 2), (384, 3), (574, 4)])
def test_the_sample_tiles_index_map(tiles_all, st):
    got_st, n_st, src = R.sample_tiles_map(tiles_all)
    assert (got_st, n_st) == (st, 128) and len(src) == 128 * 256
    for t in (0, 1, 63, 127):
        for j in (0, 1, 255):
            assert src[t * 256 + j] == t * st * 256 + j
    assert src.max() < tiles_all * 256 and len(np.unique(src)) == len(src)
    assert np.array_equal(np.unique(src // 256), np.arange(128) * st)
