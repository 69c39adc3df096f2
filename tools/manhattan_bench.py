"""The register-tiled Manhattan BMU search (csrc/bmu_manhattan.hpp) beside the one-thread-a-row kernel it replaces
(bmu_pairwise_kernel, reached by SOM_MANHATTAN_TILED=0 on the same build) and beside the Chebyshev search on the same rows.
One process, device rows, a seeded codebook of rows plus noise; per shape and kernel 1 warm-up call of som_bmu_device, then
the median of MB_REPS calls (wall clock per call, the ids' copy to the host inside it).  A pair is one (row, unit, feature)
triple: Manhattan issues two VALU instructions a pair, Chebyshev 1.5, so by instruction count Manhattan's pair rate is 0.75 of
Chebyshev's.  Writes MB_OUT (default profiles/manhattan.json); profiles/manhattan.md is written by hand from it.
    MB_REPS=11 python tools/manhattan_bench.py"""
import json, os, statistics, sys, time, numpy as np, torch
os.environ["SOM_TEST_HOOKS"] = "1"                                   # SOM_MANHATTAN_TILED is a test hook
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xpysom_dask_amd.engine import HipEngine, SomHipError
from xpysom_dask_amd.synthetic import gaussian_blobs

REPS = max(3, int(os.environ.get("MB_REPS", "11")))
OUT = os.environ.get("MB_OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "manhattan.json"))
SHAPES = [(64, 64, 32, 100000), (256, 256, 128, 65536), (64, 64, 3000, 4096), (64, 64, 4096, 4096)]
KERNELS = [("manhattan_tiled", "manhattan", "1"), ("manhattan_pairwise", "manhattan", "0"), ("chebyshev", "chebyshev", "1")]


def timed(fn):
    fn()                                                             # warm-up: allocations, code objects
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter(); out = fn(); ts.append(1e3 * (time.perf_counter() - t0))
    return out, {"ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


res = {"reps": REPS, "cus": torch.cuda.get_device_properties(0).multi_processor_count, "shapes": [],
       "method": "one process, device rows, 1 warm-up, median of reps of som_bmu_device, wall clock per call incl. the ids' copy"}
for X, Y, D, N in SHAPES:
    data = gaussian_blobs(N, D, seed=1234, centre_seed=1234)
    rs = np.random.RandomState(1234)
    w = (data[rs.randint(0, N, X * Y)] + rs.normal(0.0, 0.5, (X * Y, D))).astype(np.float32)
    dev = torch.from_numpy(data).cuda(); torch.cuda.synchronize()
    row = {"map": [X, Y, D], "rows": N, "pairs": float(N) * X * Y * D}
    ids = {}
    for name, dist, tiled in KERNELS:
        os.environ["SOM_MANHATTAN_TILED"] = tiled                    # (read once, when the engine is created)
        e = HipEngine(X, Y, D, distance=dist, precision="f32"); e.set_weights(w)
        try:
            ids[name], r = timed(lambda: e.bmu_device(dev.data_ptr(), N))
        except SomHipError as err:
            row[name] = {"refused": str(err)}
            print("%d x %d x %d, %d rows, %-18s refused: %s" % (X, Y, D, N, name, err), flush=True)
            continue
        finally:
            e.close()
        r["pairs_per_s"] = row["pairs"] / (r["ms"] * 1e-3)
        row[name] = r
        print("%d x %d x %d, %d rows, %-18s %10.3f ms (min %.3f)  %.3e pairs/s" % (X, Y, D, N, name, r["ms"], r["min_ms"], r["pairs_per_s"]), flush=True)
    if "manhattan_pairwise" in ids:
        row["pairwise_over_tiled"] = row["manhattan_pairwise"]["ms"] / row["manhattan_tiled"]["ms"]
        row["same_ids"] = bool(np.array_equal(ids["manhattan_pairwise"], ids["manhattan_tiled"]))
    row["tiled_pair_rate_over_chebyshev"] = row["chebyshev"]["ms"] / row["manhattan_tiled"]["ms"]   # (the model: 0.75)
    res["shapes"].append(row)
    del dev
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps({k: v for k, v in res.items() if k != "method"}), flush=True)
