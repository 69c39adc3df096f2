"""A float64 model of the exact mode's FORECAST under the default switches (csrc/exact_host.hpp: launch_bmu_exact,
exact_sample_tiles; csrc/exact_skip.hpp: exact_scout_rowneed_kernel, exact_sample_tiles_kernel), and data built so that each of
its three outcomes -- commit, the row sample declines, the sample tiles decline -- is decided by what the device COUNTS, with a
margin shown here on the CPU.  No GPU.  Shared by tests/test_scout_ref_cpu.py and tests/test_gpu_default_plan.py (not a conftest).

THE ROW SAMPLE.  n = min(128, N) rows, row b * step + step // 2 with step = N // n, one workgroup each.  Per row, over the group
slots with r_g >= 0:  m = min_g (|x - c_g| + r_g);  group g is NEEDED iff not (|x - c_g| - r_g > m).  A row with a NaN needs every
live group (every comparison with a NaN is false).  need = needed pairs / (rows * n_groups).

TAU.  The kernel works in float32 on float32 inputs (the rows, the device's own centroids and radii -- all exact here), u = 2^-24:
  t_k = fl(x_k - c_k) = (x_k - c_k)(1 + d1), |d1| <= u;  q = the fma chain q <- fma(t_k, t_k, q) over D terms, all >= 0:
  q^ = sum t_k^2 (1 + th_k) with |th_k| <= gamma_D for the chain (one rounding per fma, at most D of them on any term) and
  (1 + d1)^2 for the subtraction: |q^ - q| <= (D + 2) u q to first order.  d^ = sqrtf(q^) (correctly rounded):
  |d^ - d| <= ((D + 2) / 2 + 1) u d = (D / 2 + 2) u d.
  The threshold m^ = min_g fl(d^_g + r_g): |m^ - m| <= (D / 2 + 2) u d' + u (d' + r') <= (D / 2 + 3) u m for the g' that gives it
  (a minimum of perturbed values is within the largest perturbation of the minimum).
  The tested quantity fl(d^_g - r_g): |.. - (d_g - r_g)| <= (D / 2 + 2) u d_g + u |d_g - r_g| <= (D / 2 + 3) u (d_g + r_g).
  So the device's (d - r) - m differs from the exact one by at most (D / 2 + 3) u (d_g + r_g + m) to first order.  The model takes
  TAU = (D + 4) u (d_g + r_g + m): at least twice that at every D, which holds the second-order terms ((D u)^2 <= 6e-11 here)
  with room to spare.  A pair whose exact (d_g - r_g) - m lies within TAU of zero may go either way: `maybe`; a pair at or below
  -TAU is needed whatever the rounding: `sure`.  The device's count lies in [sure, sure + maybe].

THE SAMPLE TILES.  A pass of tiles_all = n // 256 whole tiles (> 256 of them) gives every st-th tile of its sorted order, st =
tiles_all // 128, n_st = min(128, tiles_all // st): position t * 256 + j of the sample is position t * st * 256 + j of the pass.

THE DATA (deterministic in their arguments, built once per process, never written to):
  commit         a codebook on the float32 trajectory of a batch SOM (train_f32: the benchmark's schedule, normalised random
                 start, 6 epochs, the BMU search and the codebooks in float32 -- NumPy, so that the CPU suite holds the very
                 codebook the GPU tests run) and rows of the same mixture: MIXTURE, 16 blobs ~ N(0, 12^2 I) with unit noise.
                 (With the benchmark's 64 blobs of spread 3 a map of 128 x 128 units gives every blob four groups' worth of
                 units, nearly every group straddles two blobs and the centroid-only bound of the row sample needs half to three
                 quarters of them, however long the schedule: measured here, need 0.50 .. 0.77 at these shapes.)
  rows_decline   a normalised random codebook (units on the unit sphere) and rows ~ N(0, I): every group's centroid is near the
                 origin with a radius near 1, no row can tell the groups apart.
  tiles_decline  the rows_decline rows and codebook, EXCEPT: the units of the last trained_groups(K) groups of the patch order are
                 the trained codebook's own units there, brought to the shell's scale (radius 1 about their mean) and put
                 FAR_SHIFT from the origin -- trained units beside an isotropic shell they stay clear of -- and the rows at
                 exactly 40 of the 128 sampled indices are the rows of the mixture nearest to those units, moved with them.
                 (At their own scale, some hundred from the origin, the largest unit is 150 times the shell's: the screen's error
                 windows grow with max |w|, every shell unit becomes a candidate and every row falls back to the float32 kernel
                 -- correct ids, but not the path under test.)  Those 40 rows need a few
                 trained groups and no shell group; the other 88 need every shell group and no trained one: need ~ 0.69, and
                 since every 256-row tile holds unstructured rows, every tile keeps (nearly) every shell block: est ~ 0.97.
                 (On the trained codebook alone rows ~ N(0, I) need a small part of the groups -- its groups are compact and far
                 apart, a far row tells them apart --, so the plain variant cannot hold the unstructured rows' need near 1.)"""
import numpy as np

from oracle import som_oracle as O
from tests import skip_ref as S

F32, F64 = np.float32, np.float64
U24 = 2.0 ** -24
TILE = 256
N_SAMPLE = 128
TRAIN_ROWS = 4096
TRAIN_EPOCHS = 6
MIXTURE = dict(centres=16, spread=12.0)
FAR_SHIFT = 4.0
N_STRUCTURED = 40
NAN_BLOCK = 77
MUTANTS = ("no_half_step", "plus_r", "dead_slots", "nan_nothing", "min256")

# shape -> rows (the GPU cases of tests/test_gpu_default_plan.py; every one is worth a scout: N K D >= 3e11)
SHAPES = {
    (192, 192, 128): 65792,      # 257 tiles, st = 2: the smallest pass with sample tiles
    (192, 192, 126): 70001,      # the row sample's scalar branch (D & 3), a partial last tile, dp != D
    (128, 128, 128): 147000,     # 574 tiles, st = 4; two passes of 288 tiles under SOM_EXACT_PASS_ROWS=73728
    (256, 256, 64): 72000,       # 1 024 groups: four turns of the row sample's loops
    (128, 128, 136): 135000,     # beyond 128 features: the row sample only
}


# ------------------------------------------------------------------------------------------------------ the row sample
def sample_rows(N):
    n = min(N_SAMPLE, N)
    step = N // n
    return np.arange(n, dtype=np.int64) * step + step // 2


def _dist64(xs, C):
    """|x - c| for every (row, centroid), by differences."""
    return np.sqrt(((xs[:, None, :] - C[None, :, :]) ** 2).sum(2))


def rowneed_ref(x, C, r, n_groups):
    """(sure, maybe): needed (row, group) pairs whatever the float32 rounding, and pairs within TAU of the threshold."""
    x = np.asarray(x, F32)
    D = x.shape[1]
    xs = x[sample_rows(len(x))].astype(F64)
    C = np.asarray(C, F32).astype(F64)[:n_groups]
    r = np.asarray(r, F32).astype(F64)[:n_groups]
    live = r >= 0.0
    sure = maybe = 0
    for row in xs:
        if np.isnan(row).any():
            sure += int(live.sum())
            continue
        d = _dist64(row[None, :], C)[0]
        m = (d + r)[live].min()
        s = d - r - m
        tau = (D + 4) * U24 * (d + r + m)
        sure += int(((s <= -tau) & live).sum())
        maybe += int(((np.abs(s) < tau) & live).sum())
    return sure, maybe


def rowneed_f32(x, C, r, n_groups, mutant=None):
    """A float32 NumPy emulation of the device's count (not bit for bit: NumPy sums pairwise), or of a named MUTANT of the kernel."""
    assert mutant is None or mutant in MUTANTS
    x = np.asarray(x, F32)
    N = len(x)
    n = min(N_SAMPLE, N)
    step = N // n
    idx = np.arange(n) * step + (0 if mutant == "no_half_step" else step // 2)
    C = np.asarray(C, F32)[:n_groups]
    r = np.asarray(r, F32)[:n_groups]
    live = np.ones(n_groups, bool) if mutant == "dead_slots" else r >= 0
    count = 0
    for row in x[idx]:
        t = row[None, :] - C
        with np.errstate(invalid="ignore"):
            d = np.sqrt((t * t).sum(1, dtype=F32)).astype(F32)
        if np.isnan(d).any():
            count += 0 if mutant == "nan_nothing" else int(live.sum())
            continue
        first = live.copy()
        if mutant == "min256":
            first[256:] = False
        m = (d + r)[first].min()
        test = (d + r) if mutant == "plus_r" else (d - r)
        count += int((~(test > m) & live).sum())
    return count


# ------------------------------------------------------------------------------------------------------ the sample tiles
def sample_tiles_map(tiles_all):
    """(st, n_st, src): src[p] is the position of the pass that position p of the sample copies."""
    st = tiles_all // N_SAMPLE
    n_st = min(N_SAMPLE, tiles_all // st)
    p = np.arange(n_st * TILE, dtype=np.int64)
    return st, n_st, (p // TILE) * st * TILE + p % TILE


def tile_share_ref(x, w, perm):
    """The model's level-1 share of the sample tiles of ONE pass over x, from above: rows sorted (stably) by their nearest group
    centroid, every st-th tile taken, U = the squared distance to the best unit of the row's nearest group (the device picks among
    the units of every group a tile's keys name: its U is no larger), a tile keeps the union of what its rows keep."""
    x64 = np.asarray(x, F32).astype(F64)
    w64 = np.asarray(w, F32).astype(F64)
    K = len(w64)
    G = S.n_groups(K)
    C1, r1, _ = S.geometry(w, perm, 0)
    xq = (x64 * x64).sum(1)
    d2 = xq[:, None] - 2.0 * x64 @ C1.T + (C1 * C1).sum(1)[None, :]
    near = np.argmin(d2, axis=1)
    order = np.argsort(near, kind="stable")
    st, n_st, src = sample_tiles_map(len(x) // TILE)
    rows = order[src]
    xs, g = x64[rows], near[rows]
    Usq = np.empty(len(rows))
    for gg in np.unique(g):
        sel = np.flatnonzero(g == gg)
        wg = w64[perm[S.GROUP * gg:min(K, S.GROUP * gg + S.GROUP)]]
        Usq[sel] = ((xs[sel][:, None, :] - wg[None, :, :]) ** 2).sum(2).min(1)
    dc = np.sqrt(np.maximum(d2[rows], 0.0))
    keep = dc <= np.sqrt(Usq)[:, None] + r1[None, :]
    tiles = keep.reshape(n_st, TILE, G).any(1)
    return float(tiles.mean())


def row_block_share_ref(x, w, perm, rows):
    """The share of the 16-unit blocks the plan must keep for each of `rows` ALONE, from below: U = the squared distance to the
    row's float64 BMU (no unit gives a smaller bound), both levels.  A tile keeps at least what any one of its rows keeps."""
    xs = np.asarray(x, F32)[rows]
    ids, _ = S.bmu64(xs, w)
    U = S.seed_bound(xs, w, ids)
    C1, r1, _ = S.geometry(w, perm, 0)
    C2, r2, _ = S.geometry(w, perm, 1)
    k1, k2 = S.keep(xs, U, C1, r1), S.keep(xs, U, C2, r2)
    G = S.n_groups(len(w))
    slots = np.array([[S.slot_of(g, b) for b in range(4)] for g in range(G)])
    blocks = k1[:, :G, None] & k2[:, slots]
    return blocks.reshape(len(xs), -1).mean(1)


# ------------------------------------------------------------------------------------------------------ the builders
def bmu_f32(x, w):
    """argmin_k |w_k|^2 - 2 x.w_k in float32, in row chunks."""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    wq = (w * w).sum(1)
    ids = np.empty(len(x), np.int64)
    for s in range(0, len(x), 512):
        ids[s:s + 512] = np.argmin(wq[None, :] - 2.0 * (x[s:s + 512] @ w.T), axis=1)
    return ids


def random_codebook(X, Y, D, seed=1234):
    rs = np.random.RandomState(seed)
    w = rs.rand(X, Y, D) * 2 - 1
    return (w / np.linalg.norm(w, axis=-1, keepdims=True)).astype(F32).reshape(X * Y, D)


def train_f32(X, Y, D, rows, T=TRAIN_EPOCHS, seed=1234):
    """T epochs of the batch SOM on `rows` from a normalised random codebook: sigma from min(X, Y) / 2 to 1 (exponential), Gaussian
    neighbourhood; the BMU search and every epoch's codebook in float32 (the neighbourhood sums in float64)."""
    w = random_codebook(X, Y, D, seed)
    rows = np.asarray(rows, F32)
    for t in range(T):
        sig = float(O.exponential_decay(min(X, Y) / 2.0, 1.0, t, T))
        ids = bmu_f32(rows, w)
        sums = np.zeros((X * Y, D))
        np.add.at(sums, ids, rows.astype(F64))
        cnt = np.bincount(ids, minlength=X * Y).astype(F64)
        gx = np.exp(-((np.arange(X)[:, None] - np.arange(X)[None, :]) ** 2) / (2.0 * sig * sig))
        gy = np.exp(-((np.arange(Y)[:, None] - np.arange(Y)[None, :]) ** 2) / (2.0 * sig * sig))
        num = np.matmul(gy, (gx @ sums.reshape(X, Y * D)).reshape(X, Y, D))
        den = gy @ (gx @ cnt.reshape(X, Y)).T
        den = den.T.reshape(X * Y)
        num = num.reshape(X * Y, D)
        ok = den > 1e-30
        w = np.where(ok[:, None], num / np.where(ok, den, 1.0)[:, None], w.astype(F64)).astype(F32)
    return w


def trained_groups(K):
    """Groups of the tiles_decline codebook that hold trained units: 1 / 36 of them."""
    return max(4, S.n_groups(K) // 36)


_BUILT = {}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def build(X, Y, D, N=None, nan_row=False):
    """dict: perm; commit = (w, x); rows_decline = (w, x); tiles_decline = (w, x); structured (the 40 replaced row indices).
    nan_row: the commit and tiles_decline rows with a NaN in the row at the sampled index of block NAN_BLOCK (an unstructured one)."""
    N = SHAPES[(X, Y, D)] if N is None else N
    key = (X, Y, D, N, nan_row)
    if key in _BUILT:
        return _BUILT[key]
    if nan_row:
        b = dict(build(X, Y, D, N))
        at = int(sample_rows(N)[NAN_BLOCK])
        assert at not in set(b["structured"].tolist())
        for name in ("commit", "tiles_decline"):
            w, x = b[name]
            x = x.copy()
            x[at, D // 2] = np.nan
            x.setflags(write=False)
            b[name] = (w, x)
        b["nan_at"] = at
        _BUILT[key] = b
        return b
    from xpysom_dask_amd.synthetic import gaussian_blobs
    K = X * Y
    perm = S.patch_order(X, Y)
    xm = gaussian_blobs(N, D, seed=7, **MIXTURE)
    wt = train_f32(X, Y, D, xm[:TRAIN_ROWS])
    wr = random_codebook(X, Y, D, seed=99)
    xr = np.random.RandomState(5).randn(N, D).astype(F32)
    # tiles_decline: trained units beside the shell, and 40 sampled rows that belong to them
    tu = perm[K - S.GROUP * trained_groups(K):]             # (the LAST groups: beyond the first turn of the row sample's loops)
    # (brought to the shell's scale: radius 1 about their mean, FAR_SHIFT from the origin along (1, .., 1) / sqrt(D))
    c0 = wt[tu].astype(F64).mean(0)
    sc = np.sqrt(((wt[tu].astype(F64) - c0) ** 2).sum(1)).max()
    place = lambda v: ((v.astype(F64) - c0) / sc + (FAR_SHIFT / np.sqrt(D)) * np.ones(D)).astype(F32)
    wd = wr.copy()
    wd[tu] = place(wt[tu])
    ids = bmu_f32(xm[:16384], wt[tu])                        # (the nearest of the trained units that were kept)
    dist = np.sqrt(((xm[:16384].astype(F64) - wt[tu][ids].astype(F64)) ** 2).sum(1))
    mine = np.argsort(dist, kind="stable")[:N_STRUCTURED]    # the mixture rows closest to those units
    # (block NAN_BLOCK stays unstructured: the NaN row of build(.., nan_row=True))
    blocks = np.sort(np.random.RandomState(11).choice(np.delete(np.arange(N_SAMPLE), NAN_BLOCK), N_STRUCTURED, replace=False))
    at = sample_rows(N)[blocks]
    xd = xr.copy()
    xd[at] = place(xm[mine])
    b = _freeze(dict(X=X, Y=Y, D=D, N=N, perm=perm, structured=at))
    for w_, x_ in ((wt, xm), (wr, xr), (wd, xd)):
        w_.setflags(write=False)
        x_.setflags(write=False)
    b["commit"], b["rows_decline"], b["tiles_decline"] = (wt, xm), (wr, xr), (wd, xd)
    _BUILT[key] = b
    return b


def predicted_need(w, x, perm):
    """(need from the float64 geometry of the codebook, sure, maybe, pairs)."""
    G = S.n_groups(len(w))
    C1, r1, _ = S.geometry(w, perm, 0)
    sure, maybe = rowneed_ref(x, C1.astype(F32), r1.astype(F32), G)
    pairs = min(N_SAMPLE, len(x)) * G
    return (sure + 0.5 * maybe) / pairs, sure, maybe, pairs
