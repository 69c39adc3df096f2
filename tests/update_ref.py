"""A direct-form float64 reference of the neighbourhood update, and a pure-Python mirror of the host's dispatch.

Shared by tests/test_update_ref_cpu.py, tests/test_gpu_update_ref.py and tests/fuzz/fuzz_update.py (not a conftest).

`reference_update` restates xpysom.py:420-443 without the library's separable algebra: the segment sums of the rows
per distinct BMU, the neighbourhood h(b -> k) taken straight from oracle.som_oracle.NEIGHBOURHOODS (so it carries the
reference's float32 / float64 evaluation, the hexagonal coordinates and the mexican hat's double mask), then
num = H^T S and den = H^T c in float64.  It shares no table, term or class offset with csrc/update.hpp.

`update_paths` returns the kernel instances one epoch of the library reaches (csrc/somhip.hip and csrc/update.hpp,
functions named below), on an ordinary handle or one with missing values, so the GPU modules can show that their case
lists reach every one of them.
"""
import numpy as np

from oracle import som_oracle as O

F32, F64 = np.float32, np.float64
TOL = 1e-5                  # elementwise, relative to the magnitude sum (G4's ceiling; ~1e-7 per f32 MFMA chain)
UNDERFLOW = 2.0 ** -120     # below this fraction of an array's largest magnitude: an absolute test at that level
CHUNK_ENTRIES = 1 << 24     # entries of H (distinct BMUs x units) evaluated at once


def oracle_key(neighbourhood, topology):
    return neighbourhood + "_hex" if topology == "hexagonal" else neighbourhood


def segment_sums(data, bmu):
    """(units, S, |S|, c): the distinct BMUs in ascending order, the float64 sums of their rows, of the rows'
    absolute values, and their row counts (a stable sort, then np.add.reduceat over the runs)."""
    x = np.asarray(data, F64)
    bmu = np.asarray(bmu, np.int64)
    if len(bmu) == 0:
        return np.zeros(0, np.int64), np.zeros((0, x.shape[1])), np.zeros((0, x.shape[1])), np.zeros(0)
    order = np.argsort(bmu, kind="stable")
    sb = bmu[order]
    starts = np.flatnonzero(np.r_[True, sb[1:] != sb[:-1]])
    xs = x[order]
    S = np.add.reduceat(xs, starts, axis=0)
    A = np.add.reduceat(np.abs(xs), starts, axis=0)
    c = np.diff(np.r_[starts, len(sb)]).astype(F64)
    return sb[starts], S, A, c


def _mexican_hat_abs_terms(X, Y, std_coeff, compact, ci, cj, sigma, wide, hexagonal):
    """exp(-p/d) + exp(-p/d) * 2p/d, float64, (n, X, Y): the sum of the absolute values of the two terms the mexican
    hat is the difference of, with the p the reference forms (neighborhoods.py:57-97, masked where it masks)."""
    sigma = F64(sigma) if wide else float(sigma)
    d = 2 * std_coeff ** 2 * sigma ** 2
    if hexagonal:
        nx, ny, cx, cy = O._generic_terms(X, Y, np.asarray(ci), np.asarray(cj))
        px = np.power(nx - cx, 2, dtype=F32)
        py = np.power(ny - cy, 2, dtype=F32)
        if compact:
            px *= np.logical_and(nx > cx - sigma, nx < cx + sigma)
            px *= np.logical_and(ny > cy - sigma, ny < cy + sigma)
        p = (px + py).transpose((0, 2, 1))
    else:
        ni, nj = np.arange(X)[None, :], np.arange(Y)[None, :]
        ci, cj = np.asarray(ci)[:, None], np.asarray(cj)[:, None]
        px = np.power(ni - ci, 2, dtype=F32)
        py = np.power(nj - cj, 2, dtype=F32)
        if compact:
            px *= O._support(ni, ci, sigma)
            px *= O._support(nj, cj, sigma)
        p = px[:, :, None] + py[:, None, :]
    p = p.astype(F64)
    e = np.exp(-p / d)
    return e + e * (2 * p / d)


def accumulate(S, A, c, units, K, h_of, habs_of=None):
    """num = H^T S, den = H^T c, mag_num = |H|^T |S|, mag_den = |H|^T c in float64, H = h_of(chunk of units)
    ((n, K) rows of h(b -> k)), evaluated CHUNK_ENTRIES at a time.  habs_of (default |h_of|) gives the magnitude rows."""
    D = S.shape[1]
    num, mag_num = np.zeros((K, D)), np.zeros((K, D))
    den, mag_den = np.zeros(K), np.zeros(K)
    step = max(1, CHUNK_ENTRIES // max(K, 1))
    for s in range(0, len(units), step):
        u = units[s:s + step]
        H = np.asarray(h_of(u), F64).reshape(len(u), K)
        Ha = np.abs(H) if habs_of is None else np.asarray(habs_of(u), F64).reshape(len(u), K)
        num += H.T @ S[s:s + step]
        den += H.T @ c[s:s + step]
        mag_num += Ha.T @ A[s:s + step]
        mag_den += Ha.T @ c[s:s + step]
    return num, den, mag_num, mag_den


def reference_update(data, bmu, X, Y, eta, sigma, *, wide, neighbourhood="gaussian", topology="rectangular",
                     compact=False, std_coeff=0.5):
    """(num (K, D), den (K,), mag_num (K, D), mag_den (K,)), float64, of one update with the BMUs `bmu` (unit ids
    i * Y + j) -- the direct form of xpysom.py:420-443 over distinct BMUs.

    h(b -> k) is oracle.som_oracle.NEIGHBOURHOODS[...] times eta, exactly as O.update forms it (float32 or float64 as
    the reference evaluates it), promoted to float64.  The magnitudes bound a float32 evaluation's rounding:
    mag_num = |H|^T |S| and mag_den = |H|^T c.  The mexican hat is the exception: h crosses zero and is the
    DIFFERENCE of exp(-p/d) and exp(-p/d) * 2p/d, and any evaluation rounds in proportion to those terms, not to
    their difference (which is zero on the ring p = d/2).  Its |H| is therefore |eta| * (exp(-p/d) + exp(-p/d) * 2p/d)
    with the p the reference forms, masked where it masks."""
    K = X * Y
    units, S, A, c = segment_sums(data, bmu)
    fn = O.NEIGHBOURHOODS[oracle_key(neighbourhood, topology)]
    eta_t = F64(eta) if wide else float(eta)

    def h_of(u):
        return fn(X, Y, std_coeff, compact, u // Y, u % Y, sigma, wide) * eta_t

    habs_of = None
    if neighbourhood == "mexican_hat":
        def habs_of(u):
            return abs(float(eta)) * _mexican_hat_abs_terms(X, Y, std_coeff, compact, u // Y, u % Y, sigma, wide,
                                                             topology == "hexagonal")
    return accumulate(S, A, c, units, K, h_of, habs_of)


# ------------------------------------------------------------------------------------------------------ the checks
def accum_bound(mag):
    """The error an accumulator element may carry: TOL * mag, and for elements whose magnitude is below
    UNDERFLOW * max(mag) -- where float32 tables underflow -- the absolute UNDERFLOW * max(mag)."""
    mag = np.asarray(mag, F64)
    floor = UNDERFLOW * (mag.max() if mag.size else 0.0)
    return np.where(mag >= floor, TOL * mag, floor)


def accum_ratio(got, ref, mag):
    """(worst err / accum_bound, flat index of it) over one accumulator.  A non-finite element counts as infinitely
    wrong."""
    got, ref, mag = (np.asarray(a, F64).ravel() for a in (got, ref, mag))
    bound = accum_bound(mag)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r[~np.isfinite(got)] = np.inf
    if r.size == 0:
        return 0.0, -1
    i = int(np.argmax(r))
    return float(r[i]), i


def check_accumulators(num, den, ref, what=""):
    """Assert the engine's float32 (num (K, D), den (K,)) against reference_update's output; returns the worst ratio."""
    rnum, rden, mnum, mden = ref
    K, D = rnum.shape
    num = np.asarray(num).reshape(K, D)
    den = np.asarray(den).reshape(K)
    a, ia = accum_ratio(num, rnum, mnum)
    b, ib = accum_ratio(den, rden, mden)
    assert a <= 1.0, "%s num: err/bound %.3g at unit %d feature %d: got %r, ref %r, mag %r" % (
        what, a, ia // D, ia % D, float(num.flat[ia]), rnum.flat[ia], mnum.flat[ia])
    assert b <= 1.0, "%s den: err/bound %.3g at unit %d: got %r, ref %r, mag %r" % (
        what, b, ib, float(den[ib]), rden[ib], mden[ib])
    return max(a, b)


def check_merge(w_old, w_new, num, den, ref, mexican, what=""):
    """The merge after an accumulate: bit for bit float32(num / den) of the engine's own accumulators where den != 0 and
    the old row where den == 0; against the reference on units with |den_ref| >= 1e-30 (mexican hat: also above 1e-3 of
    the largest |den_ref|, fuzz_train.py), |W' - W_ref| <= (e_num + |W_ref| * e_den) / |den_ref| -- the first-order
    error of a quotient whose numerator and denominator carry the errors check_accumulators allows them,
    e = accum_bound(mag): TOL * (mag_num + |W_ref| * mag_den) / |den_ref| except where an element of the numerator
    underflows (a unit far from every row of the data but near a zero row has num ~ 1e-48: float32 holds 0 there).
    Returns the worst ratio."""
    rnum, rden, mnum, mden = ref
    K, D = rnum.shape
    w_old, w_new = np.asarray(w_old, F32).reshape(K, D), np.asarray(w_new, F32).reshape(K, D)
    num, den = np.asarray(num, F32).reshape(K, D), np.asarray(den, F32).reshape(K)
    nz = den != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.where(nz[:, None], num / den[:, None], w_old).astype(F32)
    bad = np.flatnonzero((want.view(np.uint32) != w_new.view(np.uint32)).any(1))
    assert len(bad) == 0, "%s merge: %d units differ from float32(num/den) / the old row, first unit %d (den %r)" % (
        what, len(bad), bad[0], float(den[bad[0]]))
    ad = np.abs(rden)
    ok = ad >= 1e-30
    if mexican and ad.size:
        ok &= ad > 1e-3 * ad.max()
    if not ok.any():
        return 0.0
    wr = rnum[ok] / rden[ok, None]
    bound = (accum_bound(mnum)[ok] + np.abs(wr) * accum_bound(mden)[ok, None]) / ad[ok, None]
    err = np.abs(w_new[ok].astype(F64) - wr)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    i = int(np.argmax(r))
    worst = float(r.flat[i])
    assert worst <= 1.0, "%s merge vs reference: err/bound %.3g at unit %d feature %d" % (
        what, worst, np.flatnonzero(ok)[i // D], i % D)
    return worst


# ------------------------------------------------------------------------------------------ the host's dispatch
def _cdiv(a, b):
    return -(-a // b)


def seg_waves_per_block(D1p):
    """update.hpp:239-243 (the workgroup's partial slots must fit 64 KiB of LDS)."""
    nw = 16
    while nw > 1 and 2 * nw * (D1p + 1) * 4 > 64 * 1024:
        nw >>= 1
    return nw


def sort_path(K, n):
    """'counting' or 'radix': the sort by unit that n rows take on a map of K units in a scratch that was sized for them (a fresh
    resident set, a first query, a first streamed chunk) -- the suite's ONE restatement of csrc/unit_sort.hpp's rule (sizes +
    counting), pinned against the library by tests/test_unit_sort_cpu.py: counting up to CS_MAX_K = 8 192 units with at least
    2 CS_BLOCK = 2 048 rows and a table of at most 2^21 counts, else radix.  A scratch grown by earlier, larger calls holds the
    table its capacity allowed; the clauses on n then decide alone."""
    return "counting" if K <= 8192 and n >= 2048 and _cdiv(n, 1024) * K <= (1 << 21) else "radix"


def update_paths(X, Y, D, neighbourhood, topology, compact, N, masked=False):
    """The branches one epoch of N rows reaches on an X x Y x D map, as labels (somhip.hip: launch_leftmul,
    run_transform_stage1 / run_transform_stage2, band_ranges_from, som_create, seg_reserve, launch_runsum, segsum_rows;
    update.hpp: seg_waves_per_block).  The SOM_LM_ROWS / SOM_NO_BANDS hooks are not modelled here:
    tests/test_gpu_transform_bands.py owns them.

      s1.* / s2.*        stage 1 / stage 2 of the transform (launch_leftmul): tile64 / tile128 (the 64-row tile when the
                         stage has <= 64 output rows or the launch carries band ranges, else the 128-row tile), wrap
                         (a toroidal handle with ranges: leftmul_wrap_f32_kernel in place of leftmul_f32_kernel),
                         narrow2 / narrow4 / narrow_none (leftmul_narrow_f32_kernel on a last column tile of 1..4 / 5..8
                         columns), rows1 / rows2 / rows3+ (128-row blocks), last1 (the last block holds one row)
      s2.per_column / s2.whole_rows   stage 2 batched over map columns when the row width UD % 128 == 0
      bands.on / off     nonzero bands of the tables: a side > 32 (LM_TILE), and never for the swapped order
      swapped.on / off   mexican hat + compact support, rectangular: the row stage first
      hex.classes0/3/4   parity classes of the hexagonal terms
      seg.waves{16,8,4,2,1}, seg.vec2 / seg.vec1   the run sum's workgroup (seg_waves_per_block(D1p)) and D's parity
                         at level 0 (launch_runsum)
      sort.counting / sort.radix      sort_path: unit_sort.hpp's rule (seg_reserve, sort_rows_by_unit)
      runsum.upper / runsum.single    whether level 0 leaves more than one workgroup (segsum_rows)

    masked: a handle created with SOM_MISSING_NAN.  Its rows are [S | C | count], UD = 2 D wide, through the whole chain
    (h->UD, h->D1p = round_up(UD + 1, 4)); only level 0 of the run sum, which reads the data's rows, still sees D.
    """
    out = set()
    UD = 2 * D if masked else D
    D1p = _cdiv(UD + 1, 4) * 4
    mex = neighbourhood == "mexican_hat"
    nt = (4 if compact else 2) if mex else 1
    classes = 0
    if topology == "hexagonal" and neighbourhood != "bubble":
        classes = 4 if compact else 3
        nt *= classes
    swapped = mex and compact and topology == "rectangular"
    torus = topology == "toroidal"
    bands = (X > 32 or Y > 32) and not swapped
    nyb, nxb = _cdiv(Y, 128), _cdiv(X, 128)

    def leftmul(stage, Ro, C, row_blocks, ranges):
        rem = C % 128
        wide = _cdiv(C, 128)
        if 0 < rem <= 8:
            wide -= 1
            out.add(stage + (".narrow2" if rem <= 4 else ".narrow4"))
        else:
            out.add(stage + ".narrow_none")
        if wide > 0:
            out.add(stage + (".tile64" if Ro <= 64 or ranges else ".tile128"))
            if torus and ranges:
                out.add(stage + ".wrap")
        out.add(stage + (".rows1" if row_blocks == 1 else ".rows2" if row_blocks == 2 else ".rows3+"))
        if Ro > 128 and Ro % 128 == 1:
            out.add(stage + ".last1")

    if swapped:
        leftmul("s1", X, Y * D1p, nxb, False)
        leftmul("s2", Y, D1p, nyb, False)
    else:
        leftmul("s1", Y, UD, nyb, bands)
        per_column = UD % 128 == 0
        out.add("s2.per_column" if per_column else "s2.whole_rows")
        leftmul("s2", X, UD if per_column else Y * D1p, nxb, bands)
    out.add("bands.on" if bands else "bands.off")
    out.add("swapped.on" if swapped else "swapped.off")
    out.add("hex.classes%d" % classes)
    if N > 0:
        K = X * Y
        nw = seg_waves_per_block(D1p)
        out.add("seg.waves%d" % nw)
        out.add("seg.vec2" if D % 2 == 0 else "seg.vec1")
        out.add("sort." + sort_path(K, N))
        out.add("runsum.upper" if _cdiv(N, nw * 32) > 1 else "runsum.single")
    return out


# every label the GPU case list of tests/test_gpu_update_ref.py must reach
ALL_LABELS = ({"%s.%s" % (s, b) for s in ("s1", "s2")
               for b in ("tile64", "tile128", "narrow2", "narrow4", "narrow_none", "rows1", "rows2", "rows3+", "last1")}
              | {"s2.per_column", "s2.whole_rows", "bands.on", "bands.off", "swapped.on", "swapped.off",
                 "hex.classes0", "hex.classes3", "hex.classes4", "seg.waves16", "seg.waves8", "seg.waves4", "seg.waves2",
                 "seg.waves1", "seg.vec2", "seg.vec1", "sort.counting", "sort.radix", "runsum.upper", "runsum.single"})
# what a toroidal handle adds (that grid has no toroidal family: tests/test_gpu_torus.py and the masked grid reach them)
TORUS_LABELS = {"s1.wrap", "s2.wrap"}


# ------------------------------------------------------------------------------------------ case construction
FAMILIES = {      # family -> (neighbourhood, topology, compact)
    "gaussian": ("gaussian", "rectangular", False),
    "gaussian_compact": ("gaussian", "rectangular", True),
    "mexican_hat": ("mexican_hat", "rectangular", False),
    "mexican_hat_compact": ("mexican_hat", "rectangular", True),      # square maps only
    "bubble": ("bubble", "rectangular", False),
    "triangle": ("triangle", "rectangular", False),
    "triangle_compact": ("triangle", "rectangular", True),
    "hex_gaussian": ("gaussian", "hexagonal", False),
    "hex_gaussian_compact": ("gaussian", "hexagonal", True),
    "hex_mexican_hat": ("mexican_hat", "hexagonal", False),
    "hex_mexican_hat_compact": ("mexican_hat", "hexagonal", True),
    "hex_bubble": ("bubble", "hexagonal", False),
}
OFF_LATTICE = 5 / (1 + 2 / 3)               # 3 plus or minus one ulp
RUNS = (1, 31, 32, 33, 511, 512, 513, 4097)


def edge_units(X, Y):
    """First and last rows and columns, corners, both sides of every 128-unit block boundary on both axes, both
    parities of the hexagonal rows (columns 0 / 1 and Y-2 / Y-1)."""
    def side(n):
        v = {0, 1, n - 2, n - 1} | {b + o for b in range(128, n, 128) for o in (-1, 0)}
        return sorted(i for i in v if 0 <= i < n)
    return np.array([i * Y + j for i in side(X) for j in side(Y)], np.int64)


def make_bmu(pattern, X, Y, N, rs):
    """Forced BMUs (N,) int32 of a pattern: spread / edges / skewed / sparse (see tests/test_gpu_update_ref.py)."""
    K = X * Y
    if pattern == "spread":                         # every unit at least once
        b = np.concatenate([rs.permutation(K), rs.randint(0, K, max(0, N - K))])[:N] if N >= K else rs.randint(0, K, N)
    elif pattern == "edges":
        e = edge_units(X, Y)
        b = e[rs.randint(0, len(e), N)]
    elif pattern == "sparse":                       # <= 8 distinct units
        u = rs.choice(K, size=min(K, int(rs.randint(1, 9))), replace=False)
        b = u[rs.randint(0, len(u), N)]
    elif pattern == "skewed":                       # one unit >= 40 %, runs of RUNS rows, the rest on <= 200 units
        units = rs.permutation(K)
        big = int(np.ceil(0.4 * N))
        parts = [np.full(big, units[0])]
        left, used = N - big, 1
        for L in RUNS:
            if L <= left and used < K:
                parts.append(np.full(L, units[used]))
                used += 1
                left -= L
        if left > 0:
            pool = units[used:used + 200] if used < K else units[:1]
            parts.append(pool[rs.randint(0, len(pool), left)])
        b = rs.permutation(np.concatenate(parts))
    else:
        raise ValueError(pattern)
    return np.asarray(b, np.int32)


def make_data(N, D, scale, seed):
    """Gaussian blobs times `scale`, about one row in 50 (at least one when N > 1) zero."""
    rs = np.random.RandomState(seed)
    x = O.gaussian_blobs(N, D, seed=seed).astype(F64) * scale
    if N > 1:
        z = rs.rand(N) < 0.02
        z[rs.randint(0, N)] = True
        x[z] = 0
    return x.astype(F32)


# ------------------------------------------------------------------------------------------ running a case on the engine
def run_forced_case(case, engine_cls=None):
    """One teacher-forced accumulate + merge on the engine, checked against reference_update; then repeatability and,
    with more than one map-row block, staged == monolithic.  Returns {"accum": worst ratio, "merge": worst ratio}."""
    if engine_cls is None:
        from xpysom_dask_amd.engine import HipEngine as engine_cls
    neigh, topo, compact = FAMILIES[case["family"]]
    X, Y, D, N = case["X"], case["Y"], case["D"], case["N"]
    rs = np.random.RandomState(case["seed"])
    bmu = make_bmu(case["pattern"], X, Y, N, rs)
    data = make_data(N, D, case["scale"], case["seed"])
    w0 = (O.default_codebook(X, Y, D, case["seed"]) * case["scale"]).astype(F32).reshape(X * Y, D)
    sigma, eta, wide = case["sigma"], case["eta"], case["wide"]
    e = engine_cls(X, Y, D, neighborhood=neigh, topology=topo, compact_support=compact, std_coeff=case["std"],
                   precision="f32")
    try:
        e.set_weights(w0)
        e.set_data(data)
        e.epoch_accumulate_forced(bmu, sigma, eta, wide)
        num, den, _ = e.epoch_fetch(want_bmu=False)
        e.epoch_accumulate_forced(bmu, sigma, eta, wide)
        num2, den2, _ = e.epoch_fetch(want_bmu=False)
        assert np.array_equal(num.view(np.uint32), num2.view(np.uint32)) and \
            np.array_equal(den.view(np.uint32), den2.view(np.uint32)), "%s: a second forced accumulate differs" % case["id"]
        e.epoch_merge()
        w1 = e.get_weights()
        if e.epoch_block_count() > 1:
            e.set_weights(w0)
            e.epoch_accumulate(sigma, eta, wide)
            mnum, mden, mbmu = e.epoch_fetch()
            e.epoch_accumulate_begin(sigma, eta, wide)
            for blk in range(e.epoch_block_count()):
                e.epoch_accumulate_block(blk)
            snum, sden, sbmu = e.epoch_fetch()
            assert np.array_equal(mbmu, sbmu), "%s: staged BMUs differ" % case["id"]
            assert np.array_equal(mnum.view(np.uint32), snum.view(np.uint32)) and \
                np.array_equal(mden.view(np.uint32), sden.view(np.uint32)), "%s: staged != monolithic" % case["id"]
    finally:
        e.close()
    ref = reference_update(data, bmu, X, Y, eta, sigma, wide=wide, neighbourhood=neigh, topology=topo, compact=compact,
                           std_coeff=case["std"])
    a = check_accumulators(num, den, ref, case["id"])
    m = check_merge(w0, w1, num, den, ref, neigh == "mexican_hat", case["id"])
    return {"accum": a, "merge": m}


def case_id(c):
    return "%s-%dx%dx%d-n%d-%s-s%s%s" % (c["family"], c["X"], c["Y"], c["D"], c["N"], c["pattern"], repr(c["sigma"]),
                                          "-wide" if c["wide"] else "")


def random_case(rs, seed, max_entries=3e7, max_flops=4e10):
    """A random forced case for the fuzzer: sides 1..320, D from the layout list, every family, std_coeff, sigma on /
    one ulp off the lattice, wide, pattern and N -- redrawn until K x distinct BMUs fits the CPU reference's budget."""
    while True:
        fam = str(rs.choice(sorted(FAMILIES)))
        X, Y = int(rs.randint(1, 321)), int(rs.randint(1, 321))
        if rs.rand() < 0.3:                                   # near the tile and block edges
            X = int(rs.choice([63, 64, 65, 127, 128, 129, 255, 256, 257, 300]))
        if fam == "mexican_hat_compact":
            Y = X
        D = int(rs.choice([1, 3, 6, 24, 100, 128, 136, 256, 507, 508, 784, 1020]))
        N = int(rs.choice([1, 2, 2047, 2048, 5000, 30011, 100003]))
        pattern = str(rs.choice(["spread", "edges", "skewed", "sparse"]))
        K = X * Y
        distinct = {"spread": min(K, N), "edges": len(edge_units(X, Y)), "sparse": 8, "skewed": 209}[pattern]
        distinct = min(distinct, N, K)
        if K * distinct > max_entries or 4.0 * K * distinct * (D + 1) > max_flops or N * D > 4e7 or K * D > 3e7:
            continue
        base = float(rs.choice([1.0, 1.5, 2.0, 3.0, max(1.0, max(X, Y) / 2.0)]))
        sigma = float(rs.choice([base, OFF_LATTICE, np.nextafter(base, 0.0), np.nextafter(base, 10.0 * base)]))
        c = dict(family=fam, X=X, Y=Y, D=D, N=N, pattern=pattern, sigma=sigma,
                 std=float(rs.choice([0.25, 0.5, 1.0])), wide=bool(rs.rand() < 0.5), eta=float(rs.choice([0.5, 0.1, 1.0])),
                 scale=float(rs.choice([1e-3, 1.0, 1e3])), seed=seed)
        c["id"] = case_id(c)
        return c
