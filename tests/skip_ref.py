"""A float64 model of the exact mode's block skipping (csrc/exact_skip.hpp, csrc/exact_skip_wide.hpp), codebooks built to
defeat it, and named mutants of the model that show those codebooks have teeth.

Shared by tests/test_skip_ref_cpu.py and tests/test_gpu_skip_bound.py (not a conftest).

THE LAYOUT.  Positions come from som_patch_order (host arithmetic, no device): position p holds unit perm[p].  A GROUP is 64
consecutive positions, a SUB-BLOCK 16; the last group of a map whose K is no multiple of 64 holds cnt = K - 64 (G - 1) units
and its sub-block b holds max(0, min(16, cnt - 16 b)).  Level 1 files group g under slot g, level 2 files sub-block b of
group g under slot 16 (g >> 2) + 4 (g & 3) + b (sixteen consecutive slots = the sub-blocks of four consecutive groups); the
level-2 table has 16 ceil(G / 4) slots.  A slot without units has centroid 0 and radius -1.

THE TEST.  With c, r the float64 centroid and radius (max |w - c|) of a block and u any unit ("the row's last unit"),
U(x) = |x - w_u|^2 under the CURRENT codebook bounds the squared distance to the BMU, and a block whose every unit is
farther than that may be skipped:  keep  <=>  |x - c| <= sqrt(U) + r.  A row's BMU block is always kept (triangle
inequality); the device's test is this one with every quantity rounded outwards, so it keeps at least what the model keeps.

THE BUILDERS are deterministic in their seed and return a dict: x rows, wA / wB the codebooks before and after the move
(float32, (K, D)), bmu the float64 BMUs under wB, last the rows' last units, adv the adversarial rows, moved the units
mutant 1 leaves out, margin the rows' second-best / best squared distance.

  moved_units   wA is a smooth sheet (unit (i, j) at (i, j, 0, ...) plus noise of norm 0.01); wB moves a few units -- at
                positions 0, 15, 16, 47, 63 of their groups, and the last position of a partial last group -- to height 3
                above sheet positions far from their own group.  Adversarial rows lie within 0.02 of those points: their
                last unit (the BMU under wA) is the sheet unit below, their BMU under wB the moved unit, whose group's
                centroid stays far away.  One more kind: the unit at position 63 lands 0.02 from where the unit at position
                0 was, on the ray from its own sub-block's centroid, and rows within 0.001 of that vacated spot have the
                unit that left as their last unit -- only U under wB bounds them.  Filler rows lie near ordinary sheet
                units: tiles are full and most blocks really are skippable.
  collinear     a row sits on the ray from a group's centroid through its farthest unit k, delta beyond k; a helper unit
                u (taken from the map's last group) is put at distance (1 + eps) delta from the row and planted as its last
                unit: the test keeps k's group with a relative slack of eps delta / (r + delta).

THE MUTANTS (of the model, by name): `omit` the radius leaves the moved units out; `stale` centroids and radii of wA;
`stale_seed` U under wA; `slot` a sub-block's centroid and radius filed under the next sub-block's slot of its group;
`tail` the units of a partial group beyond 16 floor(cnt / 16) ignored; and for the collinear rows, whose group has four
corners equally far from its centroid, `shrink` every radius times (1 - eps / 8)."""
import ctypes as C

import numpy as np

F32, F64 = np.float32, np.float64
GROUP, SUB = 64, 16
HEIGHT = 3.0
POSITIONS = (0, 15, 16, 47, 63)
MUTANTS = ("omit", "stale", "stale_seed", "slot", "tail", "shrink")
COLLINEAR_EPS = (2.0 ** -2, 2.0 ** -5, 2.0 ** -8, 2.0 ** -12)


# ------------------------------------------------------------------------------------------------------ the layout
def patch_order(X, Y, sub44=True):
    """position -> unit (som_patch_order); sub44=False: every group's units ascending (SOM_EXACT_SUB44=0)."""
    from xpysom_dask_amd import _lib
    perm = np.full(X * Y, -1, np.int32)
    assert _lib.load().som_patch_order(X, Y, perm.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    if not sub44:
        for p in range(0, len(perm), GROUP):
            perm[p:p + GROUP].sort()
    return perm


def n_groups(K):
    return -(-K // GROUP)


def n_slots(K, level):
    G = n_groups(K)
    return G if level == 0 else 16 * (-(-G // 4))


def slot_of(g, b):
    return 16 * (g >> 2) + 4 * (g & 3) + b


def block_positions(K, level, slot):
    """The positions (patch order) of the units filed under `slot` of `level` (0: groups, 1: sub-blocks); empty: none."""
    if level == 0:
        return np.arange(min(K, GROUP * slot), min(K, GROUP * slot + GROUP))
    g, b = 4 * (slot >> 4) + ((slot >> 2) & 3), slot & 3
    return np.arange(min(K, GROUP * g + SUB * b), min(K, GROUP * g + SUB * b + SUB))


# ------------------------------------------------------------------------------------------------------ the model
def geometry(w, perm, level, omit=(), tail=False):
    """(C (n_slots, D), r (n_slots,), csq (n_slots,)) in float64.  omit: units the RADIUS leaves out (mutant `omit`);
    tail: the units of a partial group beyond 16 floor(cnt / 16) are ignored altogether (mutant `tail`)."""
    w = np.asarray(w, F32).astype(F64)
    K, D = w.shape
    ns = n_slots(K, level)
    Cc, r = np.zeros((ns, D)), np.full(ns, -1.0)
    omit = set(int(u) for u in omit)
    cnt_last = K - GROUP * (n_groups(K) - 1)
    for s in range(ns):
        pos = block_positions(K, level, s)
        if tail and len(pos) and pos[0] // GROUP == n_groups(K) - 1:
            pos = pos[pos < GROUP * (n_groups(K) - 1) + SUB * (cnt_last // SUB)]
        if not len(pos):
            continue
        units = perm[pos]
        Cc[s] = w[units].mean(0)
        far = [u for u in units if int(u) not in omit]
        r[s] = np.sqrt(((w[far] - Cc[s]) ** 2).sum(1)).max() if far else 0.0
    return Cc, r, (Cc * Cc).sum(1)


def seed_bound(x, w, last):
    """U = |x - w_last|^2 in float64."""
    x, w = np.asarray(x, F32).astype(F64), np.asarray(w, F32).astype(F64)
    return ((x - w[np.asarray(last)]) ** 2).sum(1)


def keep(x, U, Cc, r):
    """(n, n_slots) bool: |x - c| <= sqrt(U) + r; an empty slot (r < 0) is never kept.  (1e-12: the float64 rounding of the
    three norms -- the triangle inequality itself has no slack to give on a collinear row)"""
    x = np.asarray(x, F32).astype(F64)
    d2 = np.maximum((x * x).sum(1)[:, None] - 2.0 * x @ Cc.T + (Cc * Cc).sum(1)[None, :], 0.0)
    # (the expanded form loses digits where x is near c: recompute those entries from the difference)
    d = np.sqrt(d2)
    near = d2 < 1e-6 * (x * x).sum(1)[:, None]
    for i, s in zip(*np.nonzero(near)):
        d[i, s] = np.sqrt(((x[i] - Cc[s]) ** 2).sum())
    return (d <= (np.sqrt(U)[:, None] + r[None, :]) * (1.0 + 1e-12)) & (r[None, :] >= 0.0)


def plan(case, mutant=None, levels=2):
    """The model's plan of a built case (or of one of its mutants): (keep1 (n, G), keep2 (n, 16 ceil(G / 4)) or None)."""
    assert mutant is None or mutant in MUTANTS
    x, perm = case["x"], case["perm"]
    w_geo = case["wA"] if mutant == "stale" else case["wB"]
    U = seed_bound(x, case["wA"] if mutant == "stale_seed" else case["wB"], case["last"])
    kw = dict(omit=case["moved"] if mutant == "omit" else (), tail=mutant == "tail")
    C1, r1, _ = geometry(w_geo, perm, 0, **kw)
    f = 1.0 - case["eps"] / 8.0 if mutant == "shrink" else 1.0
    keep1 = keep(x, U, C1, r1 * f)
    if levels < 2:
        return keep1, None
    C2, r2, _ = geometry(w_geo, perm, 1, **kw)
    if mutant == "slot":
        src = np.arange(len(r2))
        src = (src & ~3) | ((src + 1) & 3)                   # slot (g, b) holds sub-block b + 1's centroid and radius
        C2, r2 = C2[src], r2[src]
    return keep1, keep(x, U, C2, r2 * f)


def bmu_block_kept(case, keep1, keep2):
    """Per row: does the plan keep the block that holds the row's float64 BMU (its group, and its sub-block where level 2 ran)?"""
    inv = np.empty(len(case["perm"]), np.int64)
    inv[case["perm"]] = np.arange(len(case["perm"]))
    pos = inv[case["bmu"]]
    g, b = pos >> 6, (pos >> 4) & 3
    rows = np.arange(len(pos))
    ok = keep1[rows, g]
    if keep2 is not None:
        ok = ok & keep2[rows, slot_of(g, b)]
    return ok


def shares(case, keep1, keep2):
    """(kept share of the (row, group) pairs, kept share of the (row, 16-unit block) pairs: level 2 under level 1)."""
    K = len(case["perm"])
    G = n_groups(K)
    s1 = keep1[:, :G].mean()
    if keep2 is None:
        return float(s1), float(s1)
    blocks = sum(int((keep1[:, g] & keep2[:, slot_of(g, b)]).sum()) for g in range(G) for b in range(4)
                 if len(block_positions(K, 1, slot_of(g, b))))
    total = len(keep1) * sum(1 for g in range(G) for b in range(4) if len(block_positions(K, 1, slot_of(g, b))))
    return float(s1), blocks / total


def applicable(case, mutant, levels=2):
    K = len(case["perm"])
    if mutant == "slot":
        return levels >= 2 and case["kind"] == "moved_units"
    if mutant == "tail":
        return case["kind"] == "moved_units" and K % GROUP != 0 and (K % GROUP) % SUB != 0
    if mutant == "shrink":
        return case["kind"] == "collinear"
    return case["kind"] == "moved_units"


# ------------------------------------------------------------------------------------------------------ the builders
def bmu64(x, w):
    """(ids, second-best / best squared distance) in float64, by differences (no cancellation), in row chunks."""
    x, w = np.asarray(x, F32).astype(F64), np.asarray(w, F32).astype(F64)
    ids, ratio = np.empty(len(x), np.int64), np.empty(len(x))
    wq = (w * w).sum(1)
    for s in range(0, len(x), 512):
        xs = x[s:s + 512]
        d2 = (xs * xs).sum(1)[:, None] - 2.0 * xs @ w.T + wq[None, :]
        # (candidates from the expanded form, the two best re-evaluated from the differences)
        top = np.argpartition(d2, 8, axis=1)[:, :9] if w.shape[0] > 9 else np.tile(np.arange(w.shape[0]), (len(xs), 1))
        dd = ((xs[:, None, :] - w[top]) ** 2).sum(2)
        o = np.argsort(dd, axis=1, kind="stable")
        ids[s:s + 512] = top[np.arange(len(xs)), o[:, 0]]
        best, second = dd[np.arange(len(xs)), o[:, 0]], dd[np.arange(len(xs)), o[:, 1]]
        with np.errstate(divide="ignore"):
            ratio[s:s + 512] = np.where(best > 0, second / np.where(best > 0, best, 1.0), np.inf)
    return ids, ratio


def sheet(X, Y, D, rng):
    """Unit (i, j) at (i, j, 0, ...) plus noise of norm 0.01."""
    assert D >= 3
    w = np.zeros((X * Y, D))
    w[:, 0] = np.repeat(np.arange(X), Y)
    w[:, 1] = np.tile(np.arange(Y), X)
    noise = rng.randn(X * Y, D)
    w += 0.01 * noise / np.sqrt((noise * noise).sum(1, keepdims=True))
    return w.astype(F32)


def _ball(rng, n, D, radius):
    v = rng.randn(n, D)
    return radius * rng.uniform(0.3, 1.0, size=(n, 1)) * v / np.sqrt((v * v).sum(1, keepdims=True))


def _far_unit(wA, centre, taken, rng, reach):
    """A sheet unit about `reach` away from `centre` (float64 features 0, 1), not in `taken`."""
    d = np.sqrt(((wA[:, :2].astype(F64) - centre[:2]) ** 2).sum(1))
    for width in (1.0, 2.0, 4.0, 8.0, 1e9):
        cand = [u for u in np.flatnonzero(np.abs(d - reach) <= width) if int(u) not in taken]
        if cand:
            return int(cand[rng.randint(len(cand))])
    raise AssertionError("no sheet unit left")


def moved_units(X, Y, D, n, seed, sub44=True, rows_per_point=32):
    rng = np.random.RandomState(seed)
    K = X * Y
    G = n_groups(K)
    perm = patch_order(X, Y, sub44)
    wA = sheet(X, Y, D, rng)
    full = [g for g in range(G) if GROUP * (g + 1) <= K]
    assert full, "the map has no whole group"
    cen = np.array([wA[perm[GROUP * g:GROUP * g + GROUP]].astype(F64).mean(0) for g in full])
    # the groups the moved units leave: one each on a map of many groups, ONE for all of them on a small map (a group that lost a
    # unit has a radius of tens: every such group is one no row nearby can skip)
    if len(full) >= 16:
        for _ in range(1000):
            gs = [full[i] for i in rng.choice(len(full), len(POSITIONS), replace=False)]
            if np.sqrt(((cen[full.index(gs[0])] - cen[full.index(gs[-1])]) ** 2).sum()) >= 16.0:
                break
        else:
            raise AssertionError("no pair of far groups")
    else:
        gs = [full[rng.randint(len(full))]] * len(POSITIONS)
    places = [(g, p) for g, p in zip(gs, POSITIONS)]
    if K % GROUP:
        places.append((G - 1, K - GROUP * (G - 1) - 1))       # the last position of the partial group
    moved = [int(perm[GROUP * g + p]) for g, p in places]
    taken = set(moved)
    wB = wA.astype(F64).copy()
    x_adv, targets = [], []
    span = np.sqrt(float(X - 1) ** 2 + float(Y - 1) ** 2)
    for (g, p), m in zip(places, moved):
        c_g = wA[perm[GROUP * g:min(K, GROUP * g + GROUP)]].astype(F64).mean(0)
        far = np.sqrt(((wA[:, :2].astype(F64) - c_g[:2]) ** 2).sum(1)).max()
        reach = min(30.0, 0.65 * far, 0.75 * span)
        s = _far_unit(wA, c_g, taken | set(targets), rng, reach)
        targets.append(s)
        wB[m] = wA[s].astype(F64)
        wB[m, 2] += HEIGHT
    wB32 = wB.astype(F32)
    # the vacated spot: the unit at position 63 (alone among the moved units in its sub-block) lands 0.02 from where the unit at
    # position 0 was, on the ray from the rest of its sub-block through the rows there
    ma, mb = moved[len(POSITIONS) - 1], moved[0]
    ga = places[len(POSITIONS) - 1][0]
    others = perm[GROUP * ga + 48:GROUP * ga + 63]
    o = wA[others].astype(F64).mean(0)
    x_b = (wA[mb].astype(F64) + _ball(rng, rows_per_point // 2, D, 0.001)).astype(F32)
    ray = x_b[0].astype(F64) - o
    wB32[ma] = (x_b[0].astype(F64) - 0.02 * ray / np.sqrt((ray * ray).sum())).astype(F32)
    for m in moved:
        if m != ma:
            x_adv.append((wB32[m].astype(F64) + _ball(rng, rows_per_point, D, 0.02)).astype(F32))
    x_adv.append(x_b)
    x_adv = np.concatenate(x_adv)
    n_fill = n - len(x_adv)
    assert n_fill > 0, "more adversarial rows than rows"
    # (every fifth unit gets no filler row: units no row reaches keep den == 0 through a merge with a narrow neighbourhood)
    plain = np.array([u for u in range(K) if u not in taken and u % 5 != 0])
    x_fill = (wA[plain[rng.randint(len(plain), size=n_fill)]].astype(F64) + _ball(rng, n_fill, D, 0.02)).astype(F32)
    x = np.concatenate([x_adv, x_fill])
    order = rng.permutation(n)
    x = np.ascontiguousarray(x[order])
    adv = np.sort(np.flatnonzero(order < len(x_adv)))
    bmu, margin = bmu64(x, wB32)
    last, _ = bmu64(x, wA)
    return dict(kind="moved_units", X=X, Y=Y, D=D, x=x, wA=wA, wB=wB32, bmu=bmu, last=last.astype(np.int32), adv=adv,
                moved=moved, margin=margin, perm=perm)


def collinear(X, Y, D, n, eps, seed, sub44=True, delta=0.25):
    rng = np.random.RandomState(seed)
    K = X * Y
    G = n_groups(K)
    assert K % GROUP == 0 and G >= 4
    perm = patch_order(X, Y, sub44)
    wA = sheet(X, Y, D, rng)
    wB = wA.copy()
    helpers = list(perm[GROUP * (G - 1):])                   # the last group gives its units away
    x_adv, last, ks = [], [], []
    for g in range(G - 1):
        units = perm[GROUP * g:GROUP * g + GROUP]
        wg = wA[units].astype(F64)
        c = wg.mean(0)
        dist = np.sqrt(((wg - c) ** 2).sum(1))
        k = int(units[np.argmax(dist)])
        ray = (wA[k].astype(F64) - c) / dist.max()
        xr = (wA[k].astype(F64) + delta * ray).astype(F32)
        dk = np.sqrt(((xr.astype(F64) - wA[k].astype(F64)) ** 2).sum())
        u = int(helpers.pop())
        up = np.zeros(D)
        up[2] = 1.0
        wB[u] = (xr.astype(F64) + (1.0 + eps) * dk * up).astype(F32)
        x_adv.append(xr)
        last.append(u)
        ks.append(k)
    x_adv = np.array(x_adv, F32)
    n_fill = n - len(x_adv)
    plain = perm[:GROUP * (G - 1)]
    fill_u = plain[rng.randint(len(plain), size=n_fill)]
    x_fill = (wA[fill_u].astype(F64) + _ball(rng, n_fill, D, 0.02)).astype(F32)
    x = np.concatenate([x_adv, x_fill])
    last = np.concatenate([np.array(last), fill_u])
    order = rng.permutation(n)
    x, last = np.ascontiguousarray(x[order]), last[order]
    adv = np.sort(np.flatnonzero(order < len(x_adv)))
    bmu, margin = bmu64(x, wB)
    return dict(kind="collinear", X=X, Y=Y, D=D, x=x, wA=wA, wB=wB, bmu=bmu, last=last.astype(np.int32), adv=adv, moved=ks,
                margin=margin, perm=perm, eps=eps)


def collinear_slack(case):
    """Per adversarial row: (sqrt(U) + r - |x - c|) / |x - c| for the group of its BMU."""
    C1, r1, _ = geometry(case["wB"], case["perm"], 0)
    inv = np.empty(len(case["perm"]), np.int64)
    inv[case["perm"]] = np.arange(len(case["perm"]))
    a = case["adv"]
    g = inv[case["bmu"][a]] >> 6
    x = case["x"][a].astype(F64)
    d = np.sqrt(((x - C1[g]) ** 2).sum(1))
    U = seed_bound(case["x"][a], case["wB"], case["last"][a])
    return (np.sqrt(U) + r1[g] - d) / d


def f32_window(x, w, ids_a, ids_b):
    """The float32 kernel's own window on the scores of two units per row (tests/query_ref.py, mode 'part':
    E = gamma(D + 2) (2 |x|.|w| + |w|^2)), summed over the two: a float64 margin above it is one the float32 kernel resolves."""
    from tests.query_ref import gamma
    x, w = np.asarray(x, F32).astype(F64), np.asarray(w, F32).astype(F64)
    D = x.shape[1]

    def E(ids):
        wk = w[np.asarray(ids)]
        return gamma(D + 2) * (2.0 * (np.abs(x) * np.abs(wk)).sum(1) + (wk * wk).sum(1))
    return E(ids_a) + E(ids_b)


def undecided(b):
    """Rows whose float64 margin (second-best minus best squared distance) does not exceed the float32 window of the two units."""
    xs, ws = b["x"].astype(F64), b["wB"].astype(F64)
    d2 = (xs * xs).sum(1)[:, None] - 2.0 * xs @ ws.T + (ws * ws).sum(1)[None, :]
    d2[np.arange(len(xs)), b["bmu"]] = np.inf
    second = np.argmin(d2, axis=1)
    gap = ((xs - ws[second]) ** 2).sum(1) - ((xs - ws[b["bmu"]]) ** 2).sum(1)
    return gap <= f32_window(b["x"], b["wB"], b["bmu"], second)


# ------------------------------------------------------------------------------------------------------ the case table
def _case(kind, X, Y, D, n, env=None, eps=None, check="full", note=""):
    c = dict(kind=kind, X=X, Y=Y, D=D, n=n, env=dict(env or {}), eps=eps, check=check)
    c["id"] = "%s-%dx%dx%d-n%d%s%s" % (kind, X, Y, D, n, "-eps2^%d" % int(np.log2(eps)) if eps else "",
                                      "".join("-%s%s" % kv for kv in sorted(c["env"].items())) or "-default")
    return c


SKIP2 = {"SOM_EXACT_SKIP": "2"}
# check: "full" = the planned launch must skip (run < total); "ids" = ids only (the default policy may decline the plan)
CASES = [
    _case("moved_units", 64, 64, 32, 3072, SKIP2),
    _case("moved_units", 64, 64, 32, 3072, {}, check="ids"),
    _case("moved_units", 64, 64, 3, 3072, SKIP2),
    _case("moved_units", 16, 16, 7, 1536, SKIP2),
    _case("moved_units", 33, 17, 128, 2048, SKIP2),          # 9 groups, the last of 49 units; 2 x 8 strips
    _case("moved_units", 70, 3, 100, 1536, SKIP2),           # 4 groups, the last of 18 units
    _case("moved_units", 35, 15, 16, 1536, SKIP2),           # 9 groups, the last of 13 units
    _case("moved_units", 72, 64, 128, 3072, SKIP2),
    _case("moved_units", 64, 64, 32, 3072, dict(SKIP2, SOM_EXACT_SUBBLOCKS="0")),
    _case("moved_units", 64, 64, 32, 3072, dict(SKIP2, SOM_EXACT_SUB44="0")),
    _case("moved_units", 33, 17, 128, 2500 + 37, dict(SKIP2, SOM_EXACT_PASS_ROWS="1024")),
    _case("moved_units", 64, 64, 200, 2048, SKIP2),          # the wide path: one level
    _case("moved_units", 64, 72, 129, 2048, SKIP2),
    _case("moved_units", 64, 64, 800, 1536, SKIP2),
    *[_case("collinear", 32, 32, 8, 1536, SKIP2, eps=e) for e in COLLINEAR_EPS],
]
# the eps whose COLLINEAR rows the float64 reference decides (the float64 margin above the float32 window on 90 % of them or
# more; the filler rows are always decided and do not count): tests/test_skip_ref_cpu.py checks the list against the reference
# alone -- 0 and 1 of the 15 collinear rows are left out at 2^-2 and 2^-5, 11 and 15 at 2^-8 and 2^-12
COLLINEAR_F64_EPS = (2.0 ** -2, 2.0 ** -5)
COLLINEAR_F64_CAP = 0.10


def levels_of(c):
    """Levels the plan of a case runs: one beyond 128 features and with SOM_EXACT_SUBBLOCKS=0."""
    return 1 if c["D"] > 128 or c["env"].get("SOM_EXACT_SUBBLOCKS") == "0" else 2


def case_seed(c):
    return (c["X"] * 7919 + c["Y"] * 131 + c["D"] * 17 + c["n"]) % 100003


_BUILT = {}


def build(c):
    """The case's data, built once per process and shared (never written to)."""
    sub44 = c["env"].get("SOM_EXACT_SUB44") != "0"
    key = (c["kind"], c["X"], c["Y"], c["D"], c["n"], c["eps"], sub44)
    if key not in _BUILT:
        if c["kind"] == "moved_units":
            b = moved_units(c["X"], c["Y"], c["D"], c["n"], case_seed(c), sub44)
        else:
            b = collinear(c["X"], c["Y"], c["D"], c["n"], c["eps"], case_seed(c), sub44)
        for v in b.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _BUILT[key] = b
    return _BUILT[key]
