"""The Chebyshev BMU search (csrc/bmu_chebyshev.hpp) beside the Manhattan one (csrc/bmu_pairwise.hpp) on the same build: both
do two floating-point operations per (row, unit, feature) triple -- a "pair" below -- on the vector ALU.  One process, device
rows, a seeded codebook of rows plus noise; per shape and distance 1 warm-up call of som_bmu_device, then the median of CB_REPS
calls (wall clock per call, the ids' copy to the host inside it).  The shader clock the device reports (pp_dpm_sclk) is sampled
over a further second of back-to-back calls; the share of peak is against  CUs x 4 SIMDs x 16 lanes x that clock  at ONE instruction per pair.
A third shape lies beyond the input_len the Manhattan kernel accepts.  Writes CB_OUT (default profiles/chebyshev.json) and a
table next to it (.md).
    CB_REPS=11 python tools/chebyshev_bench.py"""
import glob, json, os, re, statistics, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xpysom_dask_amd.engine import HipEngine, SomHipError
from xpysom_dask_amd.synthetic import gaussian_blobs

REPS = max(3, int(os.environ.get("CB_REPS", "11")))
OUT = os.environ.get("CB_OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "chebyshev.json"))
SHAPES = [(64, 64, 32, 100000), (256, 256, 128, 65536), (64, 64, 3000, 4096)]
CUS = torch.cuda.get_device_properties(0).multi_processor_count


def sclk_mhz():
    """the highest shader clock any GPU of the host reports as current (the busy one), or None"""
    best = None
    for p in glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"):
        try:
            m = re.search(r"(\d+)Mhz \*", open(p).read())
        except OSError:
            continue
        if m:
            best = max(best or 0, int(m.group(1)))
    return best


def timed(fn):
    fn()                                                             # warm-up: allocations, code objects
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter(); out = fn(); ts.append(1e3 * (time.perf_counter() - t0))
    # the clock: the timed calls of a small shape are over before the device's report moves, so sample it over a second of
    # back-to-back calls of the same shape (the first 0.3 s, while the clock still climbs, are not sampled)
    clocks, t0 = [], time.perf_counter()
    while time.perf_counter() - t0 < 1.0:
        fn()
        if time.perf_counter() - t0 > 0.3:
            c = sclk_mhz()
            if c:
                clocks.append(c)
    return out, {"ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "sclk_mhz": statistics.median(clocks) if clocks else None}


res = {"reps": REPS, "cus": CUS, "method": "one process, device rows, 1 warm-up, median of reps of som_bmu_device, wall clock per call incl. the ids' copy; "
       "sclk_mhz: median of pp_dpm_sclk samples over a further second of back-to-back calls; peak = cus x 64 lanes x sclk at one instruction per pair", "shapes": []}
for X, Y, D, N in SHAPES:
    data = gaussian_blobs(N, D, seed=1234, centre_seed=1234)
    rs = np.random.RandomState(1234)
    w = (data[rs.randint(0, N, X * Y)] + rs.normal(0.0, 0.5, (X * Y, D))).astype(np.float32)
    dev = torch.from_numpy(data).cuda(); torch.cuda.synchronize()
    row = {"map": [X, Y, D], "rows": N, "pairs": float(N) * X * Y * D}
    for dist in ("chebyshev", "manhattan"):
        e = HipEngine(X, Y, D, distance=dist, precision="f32"); e.set_weights(w)
        try:
            ids, r = timed(lambda: e.bmu_device(dev.data_ptr(), N))
        except SomHipError as err:
            row[dist] = {"refused": str(err)}
            print("%d x %d x %d, %d rows, %-9s refused: %s" % (X, Y, D, N, dist, err), flush=True)
            continue
        finally:
            e.close()
        r["pairs_per_s"] = row["pairs"] / (r["ms"] * 1e-3)
        if r["sclk_mhz"]:
            r["share_of_peak"] = r["pairs_per_s"] / (CUS * 64 * r["sclk_mhz"] * 1e6)
        r["distinct_ids"] = int(len(np.unique(ids)))
        row[dist] = r
        print("%d x %d x %d, %d rows, %-9s %10.3f ms (min %.3f)  %.3e pairs/s  sclk %s MHz  share of peak %s" % (
            X, Y, D, N, dist, r["ms"], r["min_ms"], r["pairs_per_s"], r["sclk_mhz"], "%.3f" % r["share_of_peak"] if "share_of_peak" in r else "-"), flush=True)
    if "ms" in row["manhattan"]:
        row["manhattan_over_chebyshev"] = row["manhattan"]["ms"] / row["chebyshev"]["ms"]
    res["shapes"].append(row)
    del dev
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
with open(os.path.splitext(OUT)[0] + ".md", "w") as f:
    f.write("# The Chebyshev BMU search beside the Manhattan one\n\n`tools/chebyshev_bench.py`: MI355X, one GPU (%d CUs), device rows, 1 warm-up, "
            "median of %d calls of `som_bmu_device`\n(wall clock, the ids' copy inside), one process, both distances on the same build.  A pair is one "
            "(row, unit, feature) triple;\nthe share of peak is against CUs x 4 SIMDs x 16 lanes x the sampled shader clock at one VALU instruction "
            "per pair\n(the kernel issues 1.5: two `v_sub_f32` and one `v_max3_f32` per two pairs).\n\n" % (CUS, REPS))
    f.write("| shape, rows | distance | ms per call (min - max) | pairs/s | sclk MHz | share of peak | manhattan / chebyshev |\n|---|---|---|---|---|---|---|\n")
    for row in res["shapes"]:
        for dist in ("chebyshev", "manhattan"):
            r = row[dist]
            name = "%d x %d x %d, %d" % (*row["map"], row["rows"])
            if "refused" in r:
                f.write("| %s | %s | refused: %s | | | | |\n" % (name, dist, r["refused"]))
                continue
            f.write("| %s | %s | %.3f (%.3f - %.3f) | %.3e | %s | %s | %s |\n" % (
                name, dist, r["ms"], r["min_ms"], r["max_ms"], r["pairs_per_s"], r["sclk_mhz"] or "not reported",
                "%.3f" % r["share_of_peak"] if "share_of_peak" in r else "-",
                "x %.2f" % row["manhattan_over_chebyshev"] if dist == "chebyshev" and "manhattan_over_chebyshev" in row else ""))
print(json.dumps({k: v for k, v in res.items() if k != "method"}), flush=True)
