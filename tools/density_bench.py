"""The density scan (som_unit_density_device, csrc/density.hpp) beside the float32 BMU search over the same rows: one process, a
256 x 256 x 128 map (a codebook of rows plus noise), DB_ROWS device-resident rows of the benchmark's blobs; 1 warm-up call, then
the median of DB_REPS calls each, every call closed by som_sync.  Measured: som_unit_density_device at 1 and at 8 radii (the
codebook's midrange as pivot), and som_bmu_device on a precision='f32' handle -- existing code, the same 2 N K D float32 MFMA work.
Wall clock per call (it includes the counts' / the ids' copy to the host) and the time of the scan kernel alone on the stream
(the SOM_K_BMU event pair).  Writes DB_OUT (default profiles/density.json) and a table next to it (.md).
    DB_ROWS=1048576 DB_REPS=11 python tools/density_bench.py"""
import json, os, statistics, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xpysom_dask_amd.engine import HipEngine
from xpysom_dask_amd.synthetic import gaussian_blobs

X = Y = 256; D = 128
N = int(os.environ.get("DB_ROWS", str(1 << 20))); REPS = max(3, int(os.environ.get("DB_REPS", "11")))
OUT = os.environ.get("DB_OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "density.json"))
data = gaussian_blobs(N, D, seed=1234, centre_seed=1234)
rs = np.random.RandomState(1234)
w = (data[rs.randint(0, N, X * Y)] + rs.normal(0.0, 0.5, (X * Y, D))).astype(np.float32)
w64 = w.astype(np.float64)
pivot = ((w64.min(axis=0) + w64.max(axis=0)) / 2).astype(np.float32)
# radii: percentiles of the distances of a sample of rows to a sample of units (float64, host)
sx, sw = data[rs.randint(0, N, 1024)].astype(np.float64), w64[rs.randint(0, X * Y, 1024)]
dist = np.sqrt(np.maximum((sx * sx).sum(1)[:, None] - 2 * sx @ sw.T + (sw * sw).sum(1)[None, :], 0.0))
radii8 = np.percentile(dist, (0.1, 0.5, 1, 2, 5, 10, 20, 50)).astype(np.float32)
dev = torch.from_numpy(data).cuda(); torch.cuda.synchronize()


def timed(e, fn):
    fn(); e.sync()                                                  # warm-up: allocations, operand images
    e.profile_reset(); e.profile_enable(True)
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter(); out = fn(); e.sync(); ts.append(1e3 * (time.perf_counter() - t0))
    e.profile_enable(False)
    return out, {"ms": statistics.median(ts), "min_ms": min(ts), "scan_kernel_ms": e.profile_get("bmu")[0] / REPS}


e = HipEngine(X, Y, D, precision="f32"); e.set_weights(w)
res = {"map": [X, Y, D], "rows": N, "reps": REPS, "radii": [float(r) for r in radii8],
       "method": "one process, 1 warm-up, median of reps, wall clock per call closed by som_sync; scan_kernel_ms: the SOM_K_BMU event pair"}
p1, res["density_r1"] = timed(e, lambda: e.unit_density_device(dev.data_ptr(), N, pivot, radii8[6:7]))
p8, res["density_r8"] = timed(e, lambda: e.unit_density_device(dev.data_ptr(), N, pivot, radii8))
ids, res["bmu_f32"] = timed(e, lambda: e.bmu_device(dev.data_ptr(), N))
e.close()
assert np.array_equal(p1[0], p8[6]), "one radius differs from its row of the eight-radius call"
res["median_share_per_radius"] = [float(np.median(p8[j]) / N) for j in range(8)]
for k in ("density_r1", "density_r8"):
    res["ratio_%s_over_bmu_f32" % k[8:]] = res[k]["ms"] / res["bmu_f32"]["ms"]
    res["ratio_%s_over_bmu_f32_kernel" % k[8:]] = res[k]["scan_kernel_ms"] / res["bmu_f32"]["scan_kernel_ms"]
flops = 2.0 * N * X * Y * D
for k in ("density_r1", "density_r8", "bmu_f32"):
    res[k]["scan_tflops"] = flops / (res[k]["scan_kernel_ms"] * 1e-3) / 1e12
    print("%-11s %9.3f ms per call (min %.3f), the scan kernel %9.3f ms = %.1f TFLOP/s" % (
        k, res[k]["ms"], res[k]["min_ms"], res[k]["scan_kernel_ms"], res[k]["scan_tflops"]), flush=True)
print("density / float32 search: %.3f at 1 radius, %.3f at 8 (wall); %.3f and %.3f (scan kernels)" % (
    res["ratio_r1_over_bmu_f32"], res["ratio_r8_over_bmu_f32"], res["ratio_r1_over_bmu_f32_kernel"], res["ratio_r8_over_bmu_f32_kernel"]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
with open(os.path.splitext(OUT)[0] + ".md", "w") as f:
    f.write("# Density scan beside the float32 BMU search\n\n`tools/density_bench.py`: %d x %d x %d map, %d device rows, 1 warm-up, median of %d calls, one process.\n\n"
            % (X, Y, D, N, REPS))
    f.write("| call | ms per call | scan kernel ms | TFLOP/s (scan) | / float32 search (wall) | / float32 search (kernel) |\n|---|---|---|---|---|---|\n")
    for k, label in (("bmu_f32", "som_bmu_device, precision f32"), ("density_r1", "som_unit_density_device, 1 radius"),
                     ("density_r8", "som_unit_density_device, 8 radii")):
        f.write("| %s | %.2f | %.2f | %.1f | %.3f | %.3f |\n" % (
            label, res[k]["ms"], res[k]["scan_kernel_ms"], res[k]["scan_tflops"], res[k]["ms"] / res["bmu_f32"]["ms"],
            res[k]["scan_kernel_ms"] / res["bmu_f32"]["scan_kernel_ms"]))
