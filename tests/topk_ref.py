"""The oracle and the checks of the k nearest units (som_bmu_topk*, som_unit_rank_counts*, include/somhip.h; csrc/topk.hpp;
XPySom.nearest_units / rank_hits / smoothed_hits).  Shared by tests/test_topk_cpu.py and tests/test_gpu_topk.py (not a conftest).

  topk_lowest(s, k)        the definition: per row the k lowest scores by a stable argsort -- ascending, equal scores (-0.0 == +0.0)
                           to the lower unit id -- of the scores that are < +inf; NaN and +inf never enter, -inf does; a slot
                           nothing fills is -1.  Applied to the float32 matrix `activate()` returns it is the ONLY right answer.
  check_topk(ids, s, E, k) the admissibility check against query_ref.scores' float64 s and bound E, query_ref.check_top2 for k
                           slots: a float32 list is ascending in the float32 scores s~, |s~ - s| <= E, so
                             - the ids are in range and distinct,
                             - slot j's unit a has s~_a <= s~_u for every unit u that no earlier slot holds:
                               s_a <= min_u (s_u + E_u) + E_a  (u over the rest; slot 0: query_ref.pick_ratio),
                             - consecutive slots a, b are in order: s_a - s_b <= E_a + E_b.
  pinned_share(s, E, k)    the share of rows whose first k + 1 float64 scores (all of them, on a map of k units or fewer) are
                           each separated from the next by more than the sum of the two bounds, and whose k-th is separated in the
                           same way from EVERY unit behind it: no float32 evaluation within the bounds can order those rows' lists
                           differently, so on them the float64 order is the only admissible answer (pinned_rows: which rows).
  sdh(rank_counts, s)      Pampalk's smoothed data histogram from rank counts.
  plan(...)                topk_plan (csrc/topk.hpp) restated.
"""
import numpy as np

from tests import density_ref as R
from tests import query_ref as Q

F32, F64 = np.float32, np.float64
TOPK_MAX = 8
KS = (1, 2, 3, 4, 5, 8)                      # both instances of the kernel (4 and 8 slots), each with spare slots and full
PASS_ROWS = 262144                           # TOPK_PASS_ROWS
SEED = R.SEED
MODE_OF = {"euclidean": "part", "euclidean_no_opt": "sq", "cosine": "cosine"}

# the GPU module's cases: the smallest shapes that reach each tail of the scan's tiling (128 rows x 128 units x 32 features)
CASES = [
    R.CASES[0],                                                                 # 1x1-d5: one unit, a row tail
    dict(id="1x8-d4-blobs", X=1, Y=8, D=4, N=260, kind="blobs"),                # k = K = 8, one short tile
    R.CASES[1],                                                                 # 10x20-d37: a 72-unit tail, a feature tail, 8 row tiles
    R.CASES[2],                                                                 # ... offset30: float32's cancellation regime
    R.CASES[3],                                                                 # 9x37-d130: more than four chunks, past 128 features
    R.CASES[4],                                                                 # 10x15-d16-offset300: half a chunk
]
BLOB_CASES = [c for c in CASES if c["kind"] == "blobs"]
TIE_CASES = R.TIE_CASES                                                         # 10x20, d3 and d6, small integers: exact ties everywhere
DUP_CASE = dict(id="10x20-d37-dup40", X=10, Y=20, D=37, N=1000, kind="blobs", dup=40)


def case_data(c):
    """(rows, units) of a case: query_ref's generators with seed 3; `dup`: the first dup units repeated at the end."""
    if "dup" not in c:
        return R.case_data(c)
    x = Q.make_rows(c["kind"], c["N"], c["D"], SEED)
    return x, Q.make_units(c["kind"], x, c["X"] * c["Y"], c["D"], SEED, dup=c["dup"])


def ks_of(c):
    K = c["X"] * c["Y"]
    return [k for k in KS if k <= K]


def topk_lowest(s, k):
    """(n, k) int64: per row the k lowest scores' unit ids, ascending, ties to the lower id, only scores < +inf; -1 = unfilled."""
    s = np.asarray(s)
    n, K = s.shape
    with np.errstate(invalid="ignore"):
        enters = s < np.inf
    key = np.where(enters, s, np.inf)
    order = np.argsort(key, axis=1, kind="stable")[:, :k]
    ids = np.where(np.take_along_axis(enters, order, axis=1), order, -1).astype(np.int64)
    if k > K:
        ids = np.concatenate([ids, np.full((n, k - K), -1, np.int64)], axis=1)
    return ids


def gather(m, ids, fill=np.nan):
    """m[n, ids[n, j]] with `fill` where ids is -1."""
    ids = np.asarray(ids, np.int64)
    out = np.take_along_axis(np.asarray(m), np.maximum(ids, 0), axis=1).astype(np.asarray(m).dtype, copy=True)
    out[ids < 0] = fill
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same_bits_or_nan(a, b):
    """Bit for bit, any NaN equal to any NaN (an unfilled slot's NaN has no prescribed payload)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def check_topk(ids, s, E, k, what=""):
    """Assert the lists admissible (see the module docstring); returns the worst err/bound."""
    ids = np.asarray(ids, np.int64)
    n, K = s.shape
    assert ids.shape == (n, k), "%s: ids are %r, wanted %r" % (what, ids.shape, (n, k))
    assert k <= K, "%s: k = %d on %d units" % (what, k, K)
    assert ((ids >= 0) & (ids < K)).all(), "%s: an id out of range" % what
    srt = np.sort(ids, axis=1)
    twice = np.flatnonzero((srt[:, 1:] == srt[:, :-1]).any(axis=1))
    assert len(twice) == 0, "%s: row %d names a unit twice: %s" % (what, twice[0] if len(twice) else -1, ids[twice[0]] if len(twice) else "")
    if n == 0:
        return 0.0
    r = np.arange(n)
    rest = s + E                                          # what a unit no earlier slot holds may score at most
    worst = np.zeros(n)
    prev_s = prev_e = None
    for j in range(k):
        a = ids[:, j]
        sa, ea = s[r, a], E[r, a]
        rest[r, a] = np.inf                               # (this slot's unit leaves the rest; the last slot of k = K: nothing left, cap +inf)
        cap = rest.min(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            rj = np.where(sa - cap <= 0, 0.0, (sa - cap) / ea)
            if j:
                ro = np.where(prev_s - sa <= 0, 0.0, (prev_s - sa) / (prev_e + ea))
                rj = np.maximum(rj, ro)
        worst = np.maximum(worst, np.where(np.isnan(rj), np.inf, rj))
        prev_s, prev_e = sa, ea
    i = int(np.argmax(worst))
    assert worst[i] <= 1.0, "%s: row %d lists %s with scores %s; the row's lowest are %s: err/bound %.3g" % (
        what, i, ids[i].tolist(), s[i, ids[i]].tolist(), np.sort(s[i])[:k + 1].tolist(), worst[i])
    return float(worst[i])


def pinned_rows(s, E, k):
    """bool (n,): rows on which the float64 order of the first k slots is the only admissible answer."""
    n, K = s.shape
    order = np.argsort(s, axis=1, kind="stable")
    so, eo = np.take_along_axis(s, order, axis=1), np.take_along_axis(E, order, axis=1)
    m = min(k + 1, K)
    ok = np.ones(n, bool)
    for j in range(m - 1):                                # neighbours among the first k + 1
        ok &= so[:, j + 1] - so[:, j] > eo[:, j] + eo[:, j + 1]
    if K > k:                                             # the k-th against every unit behind it
        ok &= so[:, k - 1] + eo[:, k - 1] < (so[:, k:] - eo[:, k:]).min(axis=1)
    return ok


def pinned_share(s, E, k):
    return float(pinned_rows(s, E, k).mean()) if len(s) else 1.0


def sdh(rank_counts, s):
    """Pampalk's smoothed data histogram: rank j (0-based) of s gets (s - j) points, divided by s (s + 1) / 2."""
    c = np.asarray(rank_counts, F64)
    assert c.shape[0] == s
    out = np.zeros(c.shape[1:], F64)
    for j in range(s):
        out += c[j] * ((s - j) / (s * (s + 1) / 2.0))
    return out


def sdh_weights(s):
    return np.array([(s - j) / (s * (s + 1) / 2.0) for j in range(s)])


def plan(n_rows, K, slots, forced=0):
    """topk_plan (csrc/topk.hpp) restated: (row tiles, stages, parts, stages per part)."""
    row_tiles = -(-n_rows // 128)
    stages = -(-K // 128)
    s = forced if forced > 0 else -(-slots // row_tiles)
    s = min(max(s, 1), stages)
    per = -(-stages // s)
    return row_tiles, stages, -(-stages // per), per
