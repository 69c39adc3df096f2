"""The Tanimoto BMU search (csrc/bmu_tanimoto.hpp) beside the nearest existing float32 GEMM-form search, 'cosine' on a
precision='f32' handle (csrc/bmu_f32_tiled.hpp beyond 128 features, csrc/bmu_f32_res.hpp up to 128), on the same build and the
same device rows: both do 2 N K D float32 MFMA operations.  One process, count-like rows near units of a count-like codebook;
per shape and distance 1 warm-up call of som_bmu_device, then the median of TB_REPS calls (wall clock per call, the row norms'
pass and the ids' copy to the host inside it).  The share of peak is against  CUs x 256 flop/clock x the shader clock the
device reports (pp_dpm_sclk), sampled over a further second of back-to-back calls.  Writes TB_OUT (default
profiles/tanimoto.json) and a table next to it (.md).
    TB_REPS=11 python tools/tanimoto_bench.py"""
import glob, json, os, re, statistics, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xpysom_dask_amd.engine import HipEngine

REPS = max(3, int(os.environ.get("TB_REPS", "11")))
OUT = os.environ.get("TB_OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tanimoto.json"))
SHAPES = [(64, 64, 2048, 65536), (256, 256, 128, 65536)]
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
    clocks, t0 = [], time.perf_counter()
    while time.perf_counter() - t0 < 1.0:                            # (the first 0.3 s, while the clock still climbs, are not sampled)
        fn()
        if time.perf_counter() - t0 > 0.3:
            c = sclk_mhz()
            if c:
                clocks.append(c)
    return out, {"ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "sclk_mhz": statistics.median(clocks) if clocks else None}


res = {"reps": REPS, "cus": CUS, "method": "one process, device rows, 1 warm-up, median of reps of som_bmu_device, wall clock per call incl. the row "
       "norms and the ids' copy; sclk_mhz: median of pp_dpm_sclk samples over a further second of calls; peak = cus x 256 flop/clock x sclk", "shapes": []}
for X, Y, D, N in SHAPES:
    rs = np.random.RandomState(1234)
    w = (rs.randint(1, 4, (X * Y, D)) * (rs.rand(X * Y, D) < 0.15)).astype(np.float32)
    data = np.empty((N, D), np.float32)
    for s in range(0, N, 8192):                                      # rows near units: a unit's counts with 5 % of them dropped
        pick = rs.randint(0, X * Y, min(8192, N - s))
        data[s:s + len(pick)] = w[pick] * (rs.rand(len(pick), D) > 0.05)
    dev = torch.from_numpy(data).cuda(); torch.cuda.synchronize()
    row = {"map": [X, Y, D], "rows": N, "flop": 2.0 * N * X * Y * D}
    for dist in ("tanimoto", "cosine"):
        e = HipEngine(X, Y, D, distance=dist, precision="f32"); e.set_weights(w + (0.0 if dist == "tanimoto" else 1e-3))
        try:
            ids, r = timed(lambda: e.bmu_device(dev.data_ptr(), N))
        finally:
            e.close()
        r["tflops"] = row["flop"] / (r["ms"] * 1e-3) / 1e12
        if r["sclk_mhz"]:
            r["share_of_peak"] = r["tflops"] * 1e12 / (CUS * 256 * r["sclk_mhz"] * 1e6)
        r["distinct_ids"] = int(len(np.unique(ids)))
        row[dist] = r
        print("%d x %d x %d, %d rows, %-9s %10.3f ms (min %.3f)  %.1f TFLOP/s  sclk %s MHz  share of peak %s" % (
            X, Y, D, N, dist, r["ms"], r["min_ms"], r["tflops"], r["sclk_mhz"], "%.3f" % r["share_of_peak"] if "share_of_peak" in r else "-"), flush=True)
    row["tanimoto_over_cosine"] = row["tanimoto"]["ms"] / row["cosine"]["ms"]
    res["shapes"].append(row)
    del dev
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
with open(os.path.splitext(OUT)[0] + ".md", "w") as f:
    f.write("# The Tanimoto BMU search beside the float32 cosine search\n\n`tools/tanimoto_bench.py`: MI355X, one GPU (%d CUs), device rows, 1 warm-up, "
            "median of %d calls of `som_bmu_device`\n(wall clock, the row norms' pass and the ids' copy inside), one process, both distances on "
            "`precision='f32'` handles of the same build.\nBoth do 2 N K D float32 MFMA operations; the share of peak is against CUs x 256 flop/clock x "
            "the sampled shader clock.\n\n" % (CUS, REPS))
    f.write("| shape, rows | distance | ms per call (min - max) | TFLOP/s | sclk MHz | share of float32 MFMA peak | tanimoto / cosine (time) |\n|---|---|---|---|---|---|---|\n")
    for row in res["shapes"]:
        for dist in ("tanimoto", "cosine"):
            r = row[dist]
            f.write("| %d x %d x %d, %d | %s | %.3f (%.3f - %.3f) | %.1f | %s | %s | %s |\n" % (
                *row["map"], row["rows"], dist, r["ms"], r["min_ms"], r["max_ms"], r["tflops"], r["sclk_mhz"] or "not reported",
                "%.3f" % r["share_of_peak"] if "share_of_peak" in r else "-", "x %.2f" % row["tanimoto_over_cosine"] if dist == "tanimoto" else ""))
print(json.dumps({k: v for k, v in res.items() if k != "method"}), flush=True)
