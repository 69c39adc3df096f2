"""CPU restatements of the exact mode's top-2 path (csrc/bmu_exact.hpp "TOP-2", csrc/exact_top2_host.hpp), shared by
tests/test_top2_ref_cpu.py and tests/test_gpu_top2.py (not a conftest).

  settled / pair_settled    the tie test exact_top2_settle_kernel applies to both units of a pair (ex_sqrt_settled): is
                            float32's sqrt'd distance nan_to_num(sqrt(q + |x|^2)) strictly larger at the next float32 above q?
  top2_lowest               the lowest-id top-2 of a score vector (equal values go to the lower id; a NaN never wins)
  group_minima / window_candidates / stored_mask
                            the second-smallest-window rule on a screen-value matrix cut into 64-unit groups: which groups
                            the select kernel takes (within E of the second-smallest group minimum), and which group minima
                            the screen has stored by then (within E of the second-smallest SO FAR of its codebook part)
  top2_fast_path            when a handle's top-2 calls take the screen at all
  top2_paths                the dispatch label of a top-2 call.  tests/query_ref.py's `query_paths` mirror is an existing
                            yardstick and keeps describing the dispatch before this path existed ("f32.res.kgN.top2" for
                            every handle); the label of the new dispatch -- "exact.top2" -- lives HERE
  unsettled_share           the share of rows of a data set the tie test would send to the float32 kernel, with a NumPy
                            float32 product in place of the kernel's fma chain (an estimate for choosing test inputs)

`scores`, `check_top2`, `make_rows`, `make_units` come from tests/query_ref.py.
"""
import numpy as np

from tests.query_ref import F32, check_top2, is_exact, make_rows, make_units, query_paths, scores  # noqa: F401  (re-exported)

EX_GROUP = 64                               # bmu_exact.hpp: units per group


def sqrt_distance(q, xs):
    """float32's nan_to_num(sqrt(q + |x|^2)) (score_f32<SCORE_EUCLID_SQRT>, numpy.nan_to_num: NaN -> 0, +inf -> FLT_MAX)."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(q, F32) + F32(xs)).astype(F32)
        return np.nan_to_num(np.sqrt(t).astype(F32))


def next_up(q):
    """The next float32 above q (-0: the least positive one), elementwise, as ex_sqrt_settled forms it from the bits."""
    b = np.asarray(q, F32).view(np.uint32).astype(np.int64)
    neg = (b & 0x80000000) != 0
    nb = np.where(b == 0x80000000, 1, np.where(neg, b - 1, b + 1))
    return nb.astype(np.uint32).view(F32)


def settled(q, xs):
    """ex_sqrt_settled(q, xs): q finite and the sqrt'd distance strictly larger at the next float32 above q."""
    q = np.asarray(q, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.isfinite(q) & (sqrt_distance(q, xs) < sqrt_distance(next_up(q), xs))


def top2_lowest(v):
    """(first, second): the lowest-id minimum of v and the lowest-id minimum of the rest ('<' scans: a NaN never wins)."""
    order = np.argsort(np.asarray(v), kind="stable")        # (stable: equal values -- -0 and +0 too -- keep their id order; NaN last)
    return int(order[0]), int(order[1])


def pair_settled(q, xs):
    """The float32 top-2 of q (lowest ids) and whether BOTH of its units are settled: then it is the top-2 of the sqrt'd
    distance as well, else the row belongs to the float32 top-2 kernel."""
    b1, b2 = top2_lowest(q)
    ok = bool(settled(np.asarray(q, F32)[b1], xs)) and bool(settled(np.asarray(q, F32)[b2], xs))
    return b1, b2, ok


def group_minima(S, group=EX_GROUP):
    """(n, G) minima of the (n, K) screen values over groups of `group` consecutive units (the last one may be short)."""
    S = np.asarray(S)
    n, K = S.shape
    G = -(-K // group)
    pad = np.full((n, G * group - K), np.inf, S.dtype)
    return np.concatenate([S, pad], axis=1).reshape(n, G, group).min(axis=2)


def second_smallest(gm):
    """Per row the second-smallest entry of gm (n, G); +inf where there is one group only."""
    if gm.shape[1] < 2:
        return np.full(gm.shape[0], np.inf)
    return np.partition(gm, 1, axis=1)[:, 1]


def window_candidates(S, E, group=EX_GROUP):
    """(n, G) bool: the groups the top-2 select takes -- group minimum <= m2 + E, m2 the row's second-smallest group minimum;
    a map of one group: that group."""
    gm = group_minima(S, group)
    if gm.shape[1] == 1:
        return np.ones_like(gm, bool)
    return gm <= (second_smallest(gm) + np.asarray(E).reshape(-1))[:, None]


def stored_mask(S, E, parts=1, group=EX_GROUP):
    """(n, G) bool: the group minima the screen has stored -- walking the groups of each of `parts` contiguous codebook parts
    in order, a minimum is kept where it is within E of the second-smallest minimum of the part SO FAR (before it)."""
    gm = group_minima(S, group)
    n, G = gm.shape
    E = np.asarray(E).reshape(-1)
    out = np.zeros((n, G), bool)
    for p in range(parts):
        m1 = np.full(n, np.inf)
        m2 = np.full(n, np.inf)
        for g in range(G * p // parts, G * (p + 1) // parts):
            f = gm[:, g]
            out[:, g] = f <= m2 + E
            m2 = np.where(f < m1, m1, np.where(f < m2, f, m2))
            m1 = np.minimum(m1, f)
    return out


def top2_fast_path(X, Y, D, precision, distance, env=None):
    """Whether a handle's top-2 calls take the screen (exact_top2_fast): the exact mode engaged on the euclidean images up to
    128 features, at least two units, SOM_EXACT_TOP2 not 0."""
    env = env or {}
    return (is_exact(X, Y, D, precision, distance, env) and distance == "euclidean" and D <= 128 and X * Y >= 2
            and env.get("SOM_EXACT_TOP2", "1") != "0")


def top2_paths(X, Y, D, n, precision, distance, env=None):
    """Labels of what one top-2 call reaches: "exact.top2" (screen, select, two re-score rounds, tie test) where the fast path
    serves -- its unsettled rows still reach the float32 top-2 kernel, whose label query_paths gives -- else that kernel alone."""
    f32 = query_paths(X, Y, D, n, precision, distance, "top2", env)
    return ({"exact.top2"} | f32) if top2_fast_path(X, Y, D, precision, distance, env) else f32


def unsettled_share(x, w, chunk=2048):
    """Share of the rows of x whose float32 top-2 under q = |w|^2 - 2 x.w has an unsettled unit (or a score that is not
    finite).  q by a float32 NumPy product, not the kernel's fma chain: an estimate, good enough to choose test inputs by."""
    x = np.asarray(x, F32)
    w = np.asarray(w, F32)
    wq = (w * w).sum(1, dtype=F32)
    bad = 0
    for s in range(0, len(x), chunk):
        xc = x[s:s + chunk]
        q = (wq[None, :] - F32(2) * (xc @ w.T)).astype(F32)
        xs = (xc * xc).sum(1, dtype=F32)
        idx = np.argsort(q, axis=1, kind="stable")[:, :2]
        r = np.arange(len(xc))
        for j in (0, 1):
            qj = q[r, idx[:, j]]
            with np.errstate(invalid="ignore", over="ignore"):
                t0 = np.nan_to_num(np.sqrt((qj + xs).astype(F32)))
                t1 = np.nan_to_num(np.sqrt((next_up(qj) + xs).astype(F32)))
            ok = np.isfinite(qj) & (t0 < t1)
            if j == 0:
                ok_all = ok
            else:
                ok_all &= ok
        bad += int((~ok_all).sum())
    return bad / max(1, len(x))
