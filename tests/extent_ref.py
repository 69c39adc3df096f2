"""Helpers of the row-extent tests: row sets of more than 2^31 elements (2^32 bytes) and more than 2^24 rows on one unit.

Shared by tests/test_extent_cpu.py and tests/test_gpu_extent.py (not a conftest).  Importing it needs no GPU.

Every kernel that walks rows forms `row * pitch` as an offset.  An `int` product wraps at 2^31 elements, an `unsigned` byte
offset at 2^32 bytes, a row id kept in 24 bits (or a float32 count) at 2^24 rows.  None of these can be reached by a small
shape, so the GPU module builds its rows in HBM and keeps everything row-sized there:

  boundary_windows   the rows to look at closely: the first and last `width` rows, the rows around element `elems`, around
                     byte `bytes_` of the float32 image (pitch D floats) and of the 16-bit image (pitch dp halves), and a
                     fixed stride over everything
  rows_on_device     seeded blobs around the points of a map-shaped sheet, written slab by slab; nothing of size N * D ever
                     exists in float64
  forced_bmus        a multiplicative hash of the row index: a wrapped index lands on another unit
  the references     plain float64 torch expressions, one slab of at most 2^20 rows at a time: the score matrix with
                     query_ref.scores' bound E (`scores_t`), the admissible-pick and top-2 inequalities of query_ref restated
                     on tensors (`pick_ratio_t`, `top2_ratio_t`), the distance of a row to a given unit (`row_distances_t`),
                     and the per-unit segment sums S, |S|, c by index_add_ (`segment_sums_t`), which go to
                     update_ref.accumulate through `reference_from_sums`; the weighted and the masked forms of these
                     (missing_ref's split, masked scores and augmented rows [x~ | m]), monitor_ref's row metrics
                     (`row_metrics_t`) and project_ref's label counts and value sums (`label_counts_t`, `value_sums_t`).  tests/test_extent_cpu.py holds each of them equal
                     to the NumPy form it restates.
  the model engine   a NumPy stand-in that reads its rows through an offset function, and four named mutants of it -- what a
                     missing cast would compute.  No mutant is ever built for or run on a device: a wrapped offset there reads
                     out of bounds.  The CPU module shows that each check fails on its mutant above the (emulated) boundary
                     and passes below it.

None of this shares code with csrc/.
"""
import numpy as np

from oracle import som_oracle as O
from tests import query_ref as Q
from tests import update_ref as U

F32, F64 = np.float32, np.float64
SLAB = 1 << 20
STRIDE = 4099                       # the stride sample: a prime, so it visits every residue of every tile and chunk size
GRID, SPACING, SPREAD = (8, 4), 12.0, 0.75   # the data sets' sheet of centres, and how far a unit sits from its centre
MIN_BEYOND = 65536                  # rows that must lie wholly beyond the element boundary, or a case proves nothing
HASH, HASH2, HASH3 = 2654435761, 0x2C1B3C6D, 0x297A2D39   # Knuth's multiplicative constant, two more odd ones below 2^30


def half_pitch(D):
    """Feature stride of the 16-bit row image: D rounded up to 32 (csrc/somhip.hip, h->dp)."""
    return -(-D // 32) * 32


# ------------------------------------------------------------------------------------------------------ the windows
def boundary_windows(N, D, elems=2 ** 31, bytes_=2 ** 32, itemsize=4, width=4096):
    """{name: (lo, hi)} row windows [lo, hi) plus "stride": the step of the sample over all rows.

    first / last: `width` rows each.  elems: `width` rows centred on the row that holds element `elems` of the float32 image
    (it straddles the boundary when elems % D != 0).  bytes_f32 / bytes_half: the same around byte `bytes_` of the float32
    image and of the 16-bit image.  Asserts every window inside [0, N) and at least MIN_BEYOND rows wholly beyond `elems`."""
    assert N > 0 and D > 0 and width > 0
    assert N >= 2 * width, "N = %d is too small for two windows of %d rows" % (N, width)
    first_beyond = -(-elems // D)                                    # the first row whose every element is >= elems
    assert N - first_beyond >= MIN_BEYOND, "N = %d leaves %d rows wholly beyond element %d (pitch %d); %d are needed" % (
        N, max(0, N - first_beyond), elems, D, MIN_BEYOND)
    half = width // 2
    out = {"first": (0, width), "last": (N - width, N)}
    for name, row in (("elems", elems // D), ("bytes_f32", bytes_ // (D * itemsize)), ("bytes_half", bytes_ // (half_pitch(D) * 2))):
        out[name] = (row - half, row - half + width)
    for name, (lo, hi) in out.items():
        assert 0 <= lo < hi <= N, "window %s = [%d, %d) leaves [0, %d)" % (name, lo, hi, N)
    out["stride"] = STRIDE
    return out


def window_rows(win, N):
    """The sorted distinct row indices (int64) of every window and of the stride sample."""
    parts = [np.arange(lo, hi, dtype=np.int64) for k, (lo, hi) in sorted((k, v) for k, v in win.items() if k != "stride")]
    parts.append(np.arange(0, N, win["stride"], dtype=np.int64))
    return np.unique(np.concatenate(parts))


def rows_beyond(rows, D, boundary_elems):
    """How many of `rows` lie wholly beyond element `boundary_elems`."""
    return int((np.asarray(rows, np.int64) * D >= boundary_elems).sum())


# ------------------------------------------------------------------------------------------------------ data
def _gen(device, seed):
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    return g


def sheet_centres(D, seed, grid=GRID, spacing=SPACING):
    """float32 (gx * gy, D) CPU tensor: the points spacing * (I u + J v) of a flat gx x gy sheet about the origin, u and v two
    seeded orthonormal directions -- a map-shaped data set, so that a codebook laid along it has the topology of a trained
    map and the exact mode's block bounds can exclude blocks (units thrown at random centres defeat every bound)."""
    import torch
    g = _gen("cpu", seed)
    a = torch.randn(2, D, generator=g, dtype=torch.float64)
    u = a[0] / a[0].norm()
    v = a[1] - (a[1] @ u) * u
    v = v / v.norm()
    gx, gy = grid
    I = (torch.arange(gx, dtype=torch.float64) - (gx - 1) / 2).repeat_interleave(gy)
    J = (torch.arange(gy, dtype=torch.float64) - (gy - 1) / 2).repeat(gx)
    return (spacing * (I[:, None] * u[None, :] + J[:, None] * v[None, :])).float()


def rows_on_device(N, D, seed, kind="blobs", device="cuda", grid=GRID, slab=SLAB):
    """(x float32 (N, D) on `device`, c float32 (gx * gy, D)): kind "blobs", the centres of sheet_centres plus unit noise,
    written slab by slab from one seeded generator.  The noise makes row r unrelated to every other row, rows r - 2^31/D,
    r - 2^30/D and r - 2^32/D among them: a kernel that reads one of those for r picks another unit."""
    import torch
    if kind != "blobs":
        raise ValueError(kind)
    c = sheet_centres(D, seed, grid).to(device)
    g = _gen(device, seed)
    x = torch.empty((N, D), dtype=torch.float32, device=device)
    for s in range(0, N, slab):
        n = min(slab, N - s)
        which = torch.randint(0, len(c), (n,), generator=g, device=device)
        x[s:s + n] = c[which] + torch.randn(n, D, generator=g, device=device, dtype=torch.float32)
    return x, c


def punch_on_device(x, seed, share=0.03, empty_rows=(), slab=SLAB):
    """A copy of the rows with about `share` of the features NaN (seeded, slab by slab) and every row of `empty_rows` NaN
    throughout: the rows of a handle with missing values."""
    import torch
    g = _gen(x.device, seed)
    out = x.clone()
    for s in range(0, len(x), slab):
        hole = torch.rand(out[s:s + slab].shape, generator=g, device=x.device) < share
        out[s:s + slab][hole] = float("nan")
    if len(empty_rows):
        out[torch.as_tensor(np.asarray(empty_rows, np.int64), device=x.device)] = float("nan")
    return out


def codebook_near(c, X, Y, seed, grid=GRID, spread=SPREAD):
    """float32 (X * Y, D) NumPy codebook: unit (i, j) sits `spread` away (per feature) from the centre of its own part of the
    sheet, (i gx // X, j gy // Y), so that every centre is shared by neighbouring units that compete for its rows -- the BMUs
    spread over the whole map and the scores are close enough for a subtly wrong score to change picks, yet few rows are
    float32 near-ties."""
    import torch
    g = _gen("cpu", seed)
    cc = c.detach().cpu().double()
    gx, gy = grid
    k = torch.arange(X * Y)
    own = (torch.div(k, Y, rounding_mode="floor") * gx // X) * gy + (k % Y) * gy // Y
    w = cc[own] + spread * torch.randn(X * Y, cc.shape[1], generator=g, dtype=torch.float64)
    return w.float().numpy()


def forced_bmus(N, K, device="cpu"):
    """int32 (N,) tensor: mix(r) mod K with mix = hash_mix below, a multiplicative hash of the row index formed in int64 (three
    multiplications modulo 2^32 with xor-shifts between them, so that high bits of r reach the low bits of the result).  Row r
    and row r mod 2^24 (or r - 2^31 / D) get different units: a wrapped or truncated row index moves a row's contribution to
    another unit."""
    import torch
    return (hash_mix(torch.arange(N, dtype=torch.int64, device=device)) % K).to(torch.int32)


def hash_mix(r):
    """int64 in, int64 in [0, 2^32) out; works on torch tensors and NumPy arrays alike (every product stays below 2^63)."""
    h = (r * HASH) & 0xFFFFFFFF
    h = h ^ (h >> 16)
    h = (h * HASH2) & 0xFFFFFFFF
    h = h ^ (h >> 13)
    h = (h * HASH3) & 0xFFFFFFFF
    return h ^ (h >> 16)


def slab_rows(K):
    """Rows per slab of an (n, K) float64 score matrix: at most SLAB, and at most 2^27 entries (1 GiB) a matrix."""
    return max(1, min(SLAB, (1 << 27) // max(1, K)))


def slabs(N, slab=SLAB, every=1):
    """(start, stop) of every `every`-th slab of at most `slab` rows."""
    return [(s, min(N, s + slab)) for i, s in enumerate(range(0, N, slab)) if i % every == 0]


# ------------------------------------------------------------------------------------------------------ float64 references
def scores_t(x, w, mode):
    """query_ref.scores for the modes part / sq / sqrt as torch float64 expressions: (s, E) of shape (n, K)."""
    import torch
    x, w = x.double(), w.double()
    D = w.shape[1]
    c = x @ w.T
    S = x.abs() @ w.abs().T
    Xq = (x * x).sum(1)[:, None]
    Wq = (w * w).sum(1)[None, :]
    part = Wq - 2 * c
    if mode == "part":
        return part, Q.gamma(D + 2) * (2 * S + Wq)
    sq = part + Xq
    Esq = Q.gamma(D + 3) * (2 * S + Wq + Xq)
    if mode == "sq":
        return sq, Esq
    if mode != "sqrt":
        raise ValueError(mode)
    sq = torch.clamp(sq, min=0.0)
    return torch.sqrt(sq), torch.sqrt(Esq) + 2 * Q.U * torch.sqrt(sq + Esq)


def widen_for_sqrt(s, E):
    """The 'sq' bound for picks made on float32 square roots (the quantization mode), NumPy or torch.  query_ref's own bound
    of that mode carries sqrt(E_sq) and decides almost no row of close units.  A correctly rounded float32 sqrt is monotone
    and fl(sqrt a) <= fl(sqrt b) gives sqrt(a) (1 - u) <= sqrt(b) (1 + u), so a <= b ((1 + u) / (1 - u))^2 <= b (1 + 5 u):
    the pick k of the rounded roots has s~_k <= s~_j (1 + 5 u) for every j, and with |s~ - s| <= E
        s_k - E_k <= (s_j + E_j) (1 + 5 u) = s_j + E'_j,    E' = E + 5 u (s + E).
    A kernel that takes the argmin before the root satisfies the same with room to spare."""
    return s, E + 5 * Q.U * (s + E)


def pick_ratio_t(ids, s, E):
    """query_ref.pick_ratio on tensors: per row, how far the pick's score sits above min_j (s_j + E_j) in units of its own
    bound (<= 1: admissible); an id outside [0, K) is infinitely wrong."""
    import torch
    ids = ids.long()
    bad = (ids < 0) | (ids >= s.shape[1])
    safe = torch.where(bad, torch.zeros_like(ids), ids)[:, None]
    cap = (s + E).min(dim=1).values
    over = s.gather(1, safe)[:, 0] - cap
    r = torch.where(over <= 0, torch.zeros_like(over), over / E.gather(1, safe)[:, 0])
    return torch.where(bad, torch.full_like(r, float("inf")), r)


def undecided_t(s, E):
    """Rows whose admissible set holds more than one unit (float32 near-ties): the pick bound does not decide them."""
    cap = (s + E).min(dim=1, keepdim=True).values
    return ((s <= cap + E).sum(dim=1) > 1)


def top2_ratio_t(i1, i2, s, E):
    """query_ref.check_top2's three inequalities on tensors (K >= 2, inexact data): per row the largest of the best's pick
    ratio, the second's ratio against the row without the best, and the order ratio; ids out of range or equal: inf."""
    import torch
    i1, i2 = i1.long(), i2.long()
    K = s.shape[1]
    bad = (i1 < 0) | (i1 >= K) | (i2 < 0) | (i2 >= K) | (i1 == i2)
    z = torch.zeros_like(i1)
    a, b = torch.where(bad, z, i1)[:, None], torch.where(bad, z, i2)[:, None]
    worst = pick_ratio_t(a[:, 0], s, E)
    s_wo = (s + E).scatter(1, a, float("inf"))
    cap2 = s_wo.min(dim=1).values
    s1, s2 = s.gather(1, a)[:, 0], s.gather(1, b)[:, 0]
    e1, e2 = E.gather(1, a)[:, 0], E.gather(1, b)[:, 0]
    zero = torch.zeros_like(s1)
    r2 = torch.where(s2 - cap2 <= 0, zero, (s2 - cap2) / e2)
    r3 = torch.where(s1 - s2 <= 0, zero, (s1 - s2) / (e1 + e2))
    worst = torch.maximum(worst, torch.maximum(r2, r3))
    return torch.where(bad, torch.full_like(worst, float("inf")), worst)


def row_distances_t(x, w, ids, masked=False):
    """diag_ref.row_distances / monitor_ref.row_distances on tensors: |x_n - w[ids_n]| in float64; masked: over the features
    of the row that are not NaN (none: 0)."""
    import torch
    d = x.double() - w.double()[ids.long()]
    sq = d * d
    if masked:
        sq = torch.where(torch.isnan(sq), torch.zeros_like(sq), sq)
    return torch.sqrt(sq.sum(1))


def split_t(x):
    """missing_ref.split on tensors: (x~, m) in float64 -- x where observed and 0 where NaN; 1 where observed, else 0."""
    import torch
    seen = ~torch.isnan(x)
    return torch.where(seen, x, torch.zeros_like(x)).double(), seen.double()


def masked_scores_t(x, w):
    """missing_ref.masked_scores on tensors: s = c2 - 2 c1 and E = gamma(D + 3) (2 sum |x~ w| + sum m w^2), (n, K)."""
    xt, m = split_t(x)
    w = w.double()
    c1 = xt @ w.T
    c2 = m @ (w * w).T
    S = xt.abs() @ w.abs().T
    return c2 - 2 * c1, Q.gamma(w.shape[1] + 3) * (2 * S + c2)


def segment_sums_t(x, bmu, K, weights=None, slab=SLAB, lanes=256, masked=False):
    """(S (K, D), A (K, D), c (K,)) float64 NumPy arrays: per unit the sum of its rows, of their absolute values and their
    number (weights: of w x, w |x| and w; a row of weight 0 is absent), by index_add_ in float64, a slab at a time.  Row n of a
    slab adds into copy n % lanes of the table and the copies are summed afterwards: the same sums, without millions of
    atomic additions on one address when a single unit owns every row.  masked: the sums of the augmented rows [x~ | m] of
    missing_ref, 2 D wide -- the first D columns of S are the numerator's sums, the last D the per-feature counts."""
    import torch
    N, D = x.shape
    if masked:
        D = 2 * D
    S = torch.zeros((K, D), dtype=torch.float64, device=x.device)
    A = torch.zeros_like(S)
    c = torch.zeros(K, dtype=torch.float64, device=x.device)
    for s, e in slabs(N, slab):
        xs = torch.cat(split_t(x[s:e]), dim=1) if masked else x[s:e].double()
        b = bmu[s:e].long()
        if weights is None:
            ws = torch.ones(e - s, dtype=torch.float64, device=x.device)
        else:
            ws = weights[s:e].double()
            keep = ws != 0
            xs, b, ws = xs[keep], b[keep], ws[keep]
            xs = xs * ws[:, None]
        key = (torch.arange(len(b), device=x.device) % lanes) * K + b
        for total, rows in ((S, xs), (A, xs.abs()), (c, ws)):
            part = torch.zeros((lanes * K,) + tuple(rows.shape[1:]), dtype=torch.float64, device=x.device)
            part.index_add_(0, key, rows)
            total += part.view((lanes, K) + tuple(rows.shape[1:])).sum(0)
    return S.cpu().numpy(), A.cpu().numpy(), c.cpu().numpy()


def reference_from_sums(S, A, c, X, Y, eta, sigma, wide, std_coeff=0.5):
    """update_ref.reference_update's (num, den, mag_num, mag_den) from per-unit sums over all K units (a unit without rows
    has zeros and adds nothing): the gaussian rectangular neighbourhood of the oracle, through update_ref.accumulate."""
    K = X * Y
    fn = O.NEIGHBOURHOODS["gaussian"]
    eta_t = F64(eta) if wide else float(eta)

    def h_of(u):
        return fn(X, Y, std_coeff, False, u // Y, u % Y, sigma, wide) * eta_t

    S, A, c = np.asarray(S, F64), np.asarray(A, F64), np.asarray(c, F64)
    units = np.flatnonzero((c != 0) | (A != 0).any(axis=1))
    return U.accumulate(S[units], A[units], c[units], units, K, h_of)


def qe_sum_t(x, w, ids, slab=SLAB, masked=False):
    """sum_n |x_n - w[ids_n]| in float64 over every row, a slab at a time (query_ref.qe_reference times N; masked:
    missing_ref.qe_reference times N)."""
    tot = 0.0
    for s, e in slabs(len(x), slab):
        tot += float(row_distances_t(x[s:e], w, ids[s:e], masked).sum())
    return tot


def check_qe_t(qe, x, w, ids, what="", masked=False):
    """query_ref.check_qe (masked: missing_ref.check_qe) with the float64 mean taken on tensors; returns err / bound."""
    ref = qe_sum_t(x, w, ids, masked=masked) / len(x)
    bound = Q.gamma(w.shape[1] + 10) * ref
    err = abs(float(qe) - ref)
    ratio = 0.0 if err == 0 else (err / bound if bound > 0 else float("inf"))
    assert ratio <= 1.0, "%s: QE %r, float64 mean distance to the ids %r (bound %r)" % (what, qe, ref, bound)
    return ratio


def check_picks_all_rows(ids, x, w, mode, what="", every=1, max_undecided=0.01):
    """Every pick of every `every`-th slab admissible under query_ref's bound; returns (worst ratio, undecided share, rows
    checked).  The undecided share -- rows the bound cannot decide -- must stay below max_undecided, so that a failure cannot
    hide among near-ties."""
    worst, undecided, seen = 0.0, 0, 0
    for s, e in slabs(len(x), slab_rows(len(w)), every=every):
        if mode == "quant":                                # the quantization mode: query_ref's sqrt bound as it stands ...
            sc, E = scores_t(x[s:e], w, "sqrt")
            r0 = pick_ratio_t(ids[s:e], sc, E)
            assert float(r0.max()) <= 1.0, "%s: row %d is outside query_ref's sqrt bound" % (what, s + int(r0.argmax()))
            sc, E = widen_for_sqrt(*scores_t(x[s:e], w, "sq"))   # ... and the bound that decides the rows
        elif mode == "masked":
            sc, E = masked_scores_t(x[s:e], w)
        else:
            sc, E = scores_t(x[s:e], w, mode)
        r = pick_ratio_t(ids[s:e], sc, E)
        m = float(r.max())
        if m > 1.0:
            i = int(r.argmax())
            raise AssertionError("%s: row %d picks unit %d, the row's best is unit %d, err/bound %.3g" % (
                what, s + i, int(ids[s + i]), int(sc[i].argmin()), m))
        worst = max(worst, m)
        undecided += int(undecided_t(sc, E).sum())
        seen += e - s
    share = undecided / max(1, seen)
    assert share <= max_undecided, "%s: the bound leaves %.3g of the rows undecided" % (what, share)
    return worst, share, seen


def check_top2_all_rows(i1, i2, x, w, what="", every=1):
    """query_ref.check_top2's inequalities (mode sqrt) on every row of every `every`-th slab; returns the worst ratio."""
    worst = 0.0
    for s, e in slabs(len(x), slab_rows(len(w)), every=every):
        sc, E = scores_t(x[s:e], w, "sqrt")
        r = top2_ratio_t(i1[s:e], i2[s:e], sc, E)
        m = float(r.max())
        if m > 1.0:
            i = int(r.argmax())
            raise AssertionError("%s: row %d pair (%d, %d): err/bound %.3g" % (what, s + i, int(i1[s + i]), int(i2[s + i]), m))
        worst = max(worst, m)
    return worst


def row_metrics_t(x, w, ids, prev=None, masked=False, slab=SLAB):
    """monitor_ref.row_metrics on tensors (no sample weights): dict(sum_wd, sum_w, rows, changed), changed -1 without prev."""
    n = len(x)
    return {"sum_wd": qe_sum_t(x, w, ids, slab, masked), "sum_w": float(n), "rows": n,
            "changed": -1 if prev is None else int((prev.long() != ids.long()).sum())}


def label_counts_t(ids, labels, K, C):
    """project_ref.label_counts_model on tensors: int64 (K, C) NumPy array, one bincount over unit * C + label of the rows
    whose label lies in [0, C)."""
    import torch
    ids, labels = ids.long(), labels.long()
    ok = (labels >= 0) & (labels < C)
    return torch.bincount(ids[ok] * C + labels[ok], minlength=K * C).reshape(K, C).cpu().numpy()


def value_sums_t(ids, values, K, slab=SLAB, lanes=256):
    """project_ref.value_sums_model and abs_sums on tensors: (count int64, sum, sumsq, sum |v|) per (unit, column), (K, C)
    NumPy arrays, over the values that are not NaN; float64 index_add_ a slab at a time, spread over `lanes` copies of the
    table like segment_sums_t.  (The sums are float64 sums in some order, not math.fsum: they differ from the model by at
    most project_ref.gamma(m) sum |v|, like the device's.)"""
    import torch
    N, C = values.shape
    dev = values.device
    out = [torch.zeros((K, C), dtype=torch.float64, device=dev) for _ in range(4)]
    for s, e in slabs(N, slab):
        v = values[s:e].double()
        seen = ~torch.isnan(v)
        v = torch.where(seen, v, torch.zeros_like(v))
        key = (torch.arange(e - s, device=dev) % lanes) * K + ids[s:e].long()
        for total, rows in zip(out, (seen.double(), v, v * v, v.abs())):
            part = torch.zeros((lanes * K, C), dtype=torch.float64, device=dev)
            part.index_add_(0, key, rows)
            total += part.view(lanes, K, C).sum(0)
    count, tot, sq, sa = (t.cpu().numpy() for t in out)
    return count.astype(np.int64), tot, sq, sa


# ------------------------------------------------------------------------------------------------------ the model engine
def offset_exact(r, D):
    return r * D


def offset_mod(modulus):
    """A row offset that wraps at `modulus` elements: what an `int` (2^31) or `unsigned` byte (2^32 / itemsize) product does."""
    def off(r, D):
        return (r * D) % modulus
    return off


class ModelEngine:
    """A NumPy stand-in for the engine that reads its rows from the flat float32 image through `offset(r, D)` and sorts rows
    by unit under `id_bits`-bit row ids; `count_dtype` is the type its per-unit count is accumulated in, one row at a time.
    The correct engine: offset_exact, 64 id bits, float64 counts."""

    def __init__(self, x, offset=offset_exact, id_bits=64, count_dtype=F64):
        x = np.ascontiguousarray(x, F32)
        self.N, self.D = x.shape
        self.flat = x.reshape(-1)
        self.offset, self.id_bits, self.count_dtype = offset, id_bits, count_dtype

    def rows(self, r):
        r = np.asarray(r, np.int64)
        start = np.asarray(self.offset(r, self.D), np.int64)
        return self.flat[start[:, None] + np.arange(self.D)[None, :]]

    def bmu(self, w, r=None):
        """Picks (float64 argmin of |w|^2 - 2 x.w) of rows `r` (default: all)."""
        r = np.arange(self.N) if r is None else r
        return np.argmin(Q.scores(self.rows(r), w, "part")[0], axis=1).astype(np.int32)

    def segment_sums(self, bmu, K):
        """(S, c): per unit the float64 sum of its rows as the engine reads them after its sort, and its count."""
        bmu = np.asarray(bmu, np.int64)
        order = np.argsort(bmu, kind="stable")
        ids = order if self.id_bits >= 63 else order & ((1 << self.id_bits) - 1)
        xs = self.rows(ids).astype(F64)
        S = np.zeros((K, self.D))
        np.add.at(S, bmu[order], xs)
        c = np.zeros(K)
        for k in range(K):
            n = int((bmu == k).sum())
            c[k] = float(np.add.accumulate(np.ones(n, self.count_dtype), dtype=self.count_dtype)[-1]) if n else 0.0
        return S, c


def mutants(elems, bytes_, itemsize=4, id_bits=24, count_dtype=F32):
    """{name: ModelEngine keyword arguments} of the four named defects."""
    return {
        "offset_mod_elems": dict(offset=offset_mod(elems)),
        "offset_mod_bytes": dict(offset=offset_mod(bytes_ // itemsize)),
        "sort_id_truncated": dict(id_bits=id_bits),
        "count_sequential_low_precision": dict(count_dtype=count_dtype),
    }
