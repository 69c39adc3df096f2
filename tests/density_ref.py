"""A float64 model of the data density per unit (som_unit_density*, include/somhip.h; csrc/density.hpp; XPySom.density_map) and
the band its float32 arithmetic must stay in.  Shared by tests/test_density_cpu.py and tests/test_gpu_density.py (not a conftest).

The kernel counts, per radius r_j and unit k, the rows with sq(n, k) <= r2_j, where r2_j = float32(r_j * r_j) (the product in
double), x' = fl32(x - c), w' = fl32(w - c) for the pivot c, and sq is the float32 GEMM form of |x' - w'|^2.  The model forms x' and
w' exactly as the kernel does (an IEEE subtraction is deterministic) and takes `s, E = query_ref.scores(x', w', "sq")`: s the
float64 value and E = gamma(D + 3) (2 S + Wq + Xq) the bound on any float32 evaluation of it whose two norms are fixed-order
float32 sums of the rounded squares and whose cross term is a float32 fma chain.  With u = 2^-24, per radius and unit

    lo = #{ n : s + E <  r2 (1 - 2u) }        rows the kernel MUST count
    hi = #{ n : s - E <= r2 (1 + 2u) }        rows the kernel MAY count

and a result P is admissible when lo <= P <= hi for every unit.  The band must not be wide enough to hide a failure:
`band_share` is sum_k (hi - lo) / (N K) per radius, and the tests hold it to at most 0.5 % on the reference alone.
A row holding a NaN or an infinity has s = NaN or inf against every unit and is in neither count."""
import numpy as np

from tests import query_ref as Q

F32, F64 = np.float32, np.float64
U = Q.U
MAX_SHARE = 0.005

# the GPU module's band cases: the smallest shapes that reach every tail of the scan's tiling (128 units x 128 rows x 32 features)
CASES = [
    dict(id="1x1-d5-blobs", X=1, Y=1, D=5, N=517, kind="blobs"),               # one unit, a row tail
    dict(id="10x20-d37-blobs", X=10, Y=20, D=37, N=1000, kind="blobs"),        # two unit tiles with a 72-unit tail, a feature tail, 8 row tiles
    dict(id="10x20-d37-offset30", X=10, Y=20, D=37, N=1000, kind="offset30"),  # ... on rows the un-centred form cannot resolve
    dict(id="9x37-d130-blobs", X=9, Y=37, D=130, N=700, kind="blobs"),         # more than four chunks, past the resident kernels' 128 features
    dict(id="10x15-d16-offset300", X=10, Y=15, D=16, N=600, kind="offset300"),  # half a chunk
]
TIE_CASES = [dict(id="ties-d%d" % D, X=10, Y=20, D=D, N=1000, kind="int") for D in (3, 6)]
TIE_RADII = (0, 1, 2, 3, 5, 7)
SEED = 3


def case_data(c):
    """(rows, units) of a case: query_ref's generators with seed 3."""
    x = Q.make_rows(c["kind"], c["N"], c["D"], SEED)
    w = Q.make_units(c["kind"], x, c["X"] * c["Y"], c["D"], SEED)
    return x, w


def midrange(w):
    """The pivot XPySom.density_map passes: float32((min_k w_kd + max_k w_kd) / 2) of the float32 codebook."""
    w = np.asarray(w, F32).reshape(-1, np.shape(w)[-1]).astype(F64)
    return ((w.min(axis=0) + w.max(axis=0)) / 2).astype(F32)


def r2_of(radii):
    """float32(r * r) with the product formed in double, of the float32 radii."""
    r = np.asarray(radii, F32).reshape(-1).astype(F64)
    return (r * r).astype(F32)


def centred(x, w, pivot):
    """(x', w') as the kernel forms them: one float32 subtraction per element; pivot None: the operands as they are."""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    if pivot is None:
        return x, w
    c = np.asarray(pivot, F32)
    with np.errstate(invalid="ignore"):
        return (x - c).astype(F32), (w - c).astype(F32)


def model(x, w, pivot):
    """(s, E): the float64 squared distances of the centred operands and the bound on the kernel's float32 value of each."""
    xc, wc = centred(x, w, pivot)
    with np.errstate(invalid="ignore", over="ignore"):
        return Q.scores(xc, wc, "sq")


def band(s, E, radii):
    """(lo, hi), int64 (R, K) each: what the kernel must count and what it may count."""
    r2 = r2_of(radii).astype(F64)
    with np.errstate(invalid="ignore"):
        lo = np.stack([(s + E < t * (1 - 2 * U)).sum(axis=0) for t in r2]).astype(np.int64)
        hi = np.stack([(s - E <= t * (1 + 2 * U)).sum(axis=0) for t in r2]).astype(np.int64)
    return lo, hi


def band_share(lo, hi, n):
    """Per radius: the share of the (row, unit) pairs the band leaves undecided."""
    return (hi - lo).sum(axis=1) / float(max(1, n) * lo.shape[1])


def percentile_radii(s):
    """The GPU cases' radii from the model's distances: 0, their 1st, 5th, 20th, 50th and 90th percentile, twice the maximum."""
    d = np.sqrt(np.maximum(s[np.isfinite(s)], 0.0))
    return np.array([0.0] + [np.percentile(d, p) for p in (1, 5, 20, 50, 90)] + [2 * d.max()], F32)


def check_counts(got, lo, hi, what=""):
    """Assert lo <= got <= hi everywhere; returns how many (radius, unit) entries the band left open."""
    got = np.asarray(got)
    assert got.dtype == np.int64 and got.shape == lo.shape, "%s: %s %r, wanted int64 %r" % (what, got.dtype, got.shape, lo.shape)
    bad = np.argwhere((got < lo) | (got > hi))
    assert len(bad) == 0, "%s: %d entries outside the band, first radius %d unit %d: %d not in [%d, %d]" % (
        what, len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], lo[tuple(bad[0])], hi[tuple(bad[0])])
    return int((hi > lo).sum())


def brute_counts(x, w, pivot, radii, inclusive=True):
    """The count from the (n, K, D) float64 differences of the centred operands, in row chunks."""
    xc, wc = centred(x, w, pivot)
    xc, wc = xc.astype(F64), wc.astype(F64)
    r2 = r2_of(radii).astype(F64)
    out = np.zeros((len(r2), len(wc)), np.int64)
    step = max(1, (1 << 22) // max(1, wc.size))
    for a in range(0, len(xc), step):
        with np.errstate(invalid="ignore"):
            d2 = ((xc[a:a + step, None, :] - wc[None, :, :]) ** 2).sum(axis=2)
            for j, t in enumerate(r2):
                out[j] += ((d2 <= t) if inclusive else (d2 < t)).sum(axis=0)
    return out


def plan(n_rows, K, slots, forced=0):
    """density_plan (csrc/density.hpp) restated: (unit tiles, row tiles, slabs, row tiles per slab)."""
    unit_tiles = -(-K // 128)
    row_tiles = -(-n_rows // 128)
    s = forced if forced > 0 else -(-slots // unit_tiles)
    s = min(max(s, 1), row_tiles)
    per = -(-row_tiles // s)
    return unit_tiles, row_tiles, -(-row_tiles // per), per
