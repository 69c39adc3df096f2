"""The k nearest units (som_bmu_topk_device / som_unit_rank_counts_device, csrc/topk.hpp) beside the float32 BMU search over the same
rows: one process, a 256 x 256 x 128 map (a codebook of rows plus noise), TB_ROWS device-resident rows of the benchmark's blobs;
1 warm-up call, then the median of TB_REPS calls each, every call closed by som_sync.  Measured:
  som_bmu_topk_device at k = 1, 4 and 8, ids only and with distances (the (n, k) lists' copy to the host is inside the call);
  som_unit_rank_counts_device at k = 8 (the lists stay on the device);
  som_bmu_device on a precision='f32' handle -- existing code, the same 2 N K D float32 MFMA work: the yardstick;
  activate() + np.argsort on TB_HOST_ROWS host rows -- what a user has today (the (n, K) matrix through the host).
Wall clock per call and the time of the call's kernels on the stream (the SOM_K_BMU event pairs: scan, merge, distances, counts).
Writes TB_OUT (default profiles/topk.json) and a table next to it (.md).
    TB_ROWS=1048576 TB_REPS=11 python tools/topk_bench.py"""
import json, os, statistics, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xpysom_dask_amd.engine import HipEngine
from xpysom_dask_amd.synthetic import gaussian_blobs

X = Y = 256; D = 128
N = int(os.environ.get("TB_ROWS", str(1 << 20))); REPS = max(3, int(os.environ.get("TB_REPS", "11")))
HOST_ROWS = int(os.environ.get("TB_HOST_ROWS", "4096"))
OUT = os.environ.get("TB_OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "topk.json"))
data = gaussian_blobs(N, D, seed=1234, centre_seed=1234)
rs = np.random.RandomState(1234)
w = (data[rs.randint(0, N, X * Y)] + rs.normal(0.0, 0.5, (X * Y, D))).astype(np.float32)
dev = torch.from_numpy(data).cuda(); torch.cuda.synchronize()


def timed(e, fn, reps=REPS):
    fn(); e.sync()                                                  # warm-up: allocations, operand images
    e.profile_reset(); e.profile_enable(True)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); e.sync(); ts.append(1e3 * (time.perf_counter() - t0))
    e.profile_enable(False)
    return out, {"ms": statistics.median(ts), "min_ms": min(ts), "kernels_ms": e.profile_get("bmu")[0] / reps}


e = HipEngine(X, Y, D, precision="f32"); e.set_weights(w)
res = {"map": [X, Y, D], "rows": N, "reps": REPS, "host_rows": HOST_ROWS,
       "method": "one process, 1 warm-up, median of reps, wall clock per call closed by som_sync; kernels_ms: the SOM_K_BMU event pairs"}
lists = {}
for k in (1, 4, 8):
    lists[k], res["topk_k%d_ids" % k] = timed(e, lambda: e.bmu_topk_device(dev.data_ptr(), N, k, score=False, dist=False))
    _, res["topk_k%d_dist" % k] = timed(e, lambda: e.bmu_topk_device(dev.data_ptr(), N, k, score=False, dist=True))
counts, res["rank_counts_k8"] = timed(e, lambda: e.unit_rank_counts_device(dev.data_ptr(), N, 8))
ids, res["bmu_f32"] = timed(e, lambda: e.bmu_device(dev.data_ptr(), N))
host = data[:HOST_ROWS]
today, res["activate_argsort_host"] = timed(e, lambda: np.argsort(e.distance_matrix(host), axis=1, kind="stable")[:, :8], reps=3)
e.close()
# cross-checks: slot 0 is the search's id, a shorter list heads the longer, the counts are the lists', today's route agrees
assert np.array_equal(lists[8][0][:, 0], ids), "slot 0 differs from som_bmu_device"
assert np.array_equal(lists[1][0][:, 0], ids) and np.array_equal(lists[4][0], lists[8][0][:, :4])
assert np.array_equal(counts, np.stack([np.bincount(lists[8][0][:, j], minlength=X * Y) for j in range(8)]))
assert np.array_equal(today, lists[8][0][:HOST_ROWS]), "activate + argsort differs from the lists"
base = res["bmu_f32"]
keys = [k for k in res if k.startswith("topk_") or k.startswith("rank_")]
for k in keys:
    res["ratio_%s_over_bmu_f32" % k] = res[k]["ms"] / base["ms"]
    res["ratio_%s_over_bmu_f32_kernels" % k] = res[k]["kernels_ms"] / base["kernels_ms"]
res["activate_argsort_host"]["us_per_row"] = 1e3 * res["activate_argsort_host"]["ms"] / HOST_ROWS
res["topk_k8_dist"]["us_per_row"] = 1e3 * res["topk_k8_dist"]["ms"] / N
res["ratio_host_route_over_topk_k8_dist_per_row"] = res["activate_argsort_host"]["us_per_row"] / res["topk_k8_dist"]["us_per_row"]
flops = 2.0 * N * X * Y * D
labels = [("bmu_f32", "som_bmu_device, precision f32")]
labels += [("topk_k%d_%s" % (k, v), "som_bmu_topk_device, k = %d, %s" % (k, "ids" if v == "ids" else "ids + distances")) for k in (1, 4, 8) for v in ("ids", "dist")]
labels += [("rank_counts_k8", "som_unit_rank_counts_device, k = 8")]
for k, label in labels:
    res[k]["kernels_tflops"] = flops / (res[k]["kernels_ms"] * 1e-3) / 1e12
    print("%-46s %9.3f ms per call (min %.3f), kernels %9.3f ms = %.1f TFLOP/s, x %.3f (wall) x %.3f (kernels)" % (
        label, res[k]["ms"], res[k]["min_ms"], res[k]["kernels_ms"], res[k]["kernels_tflops"], res[k]["ms"] / base["ms"],
        res[k]["kernels_ms"] / base["kernels_ms"]), flush=True)
print("activate() + argsort, %d host rows: %.1f ms = %.2f us per row; top-8 with distances: %.4f us per row (x %.0f)" % (
    HOST_ROWS, res["activate_argsort_host"]["ms"], res["activate_argsort_host"]["us_per_row"], res["topk_k8_dist"]["us_per_row"],
    res["ratio_host_route_over_topk_k8_dist_per_row"]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
with open(os.path.splitext(OUT)[0] + ".md", "w") as f:
    f.write("# The k nearest units beside the float32 BMU search\n\n`tools/topk_bench.py`: %d x %d x %d map, %d device rows, 1 warm-up, median of %d calls, one process.\n\n"
            % (X, Y, D, N, REPS))
    f.write("| call | ms per call | kernels ms | TFLOP/s (kernels) | / float32 search (wall) | / float32 search (kernels) |\n|---|---|---|---|---|---|\n")
    for k, label in labels:
        f.write("| %s | %.2f | %.2f | %.1f | %.3f | %.3f |\n" % (
            label, res[k]["ms"], res[k]["kernels_ms"], res[k]["kernels_tflops"], res[k]["ms"] / base["ms"], res[k]["kernels_ms"] / base["kernels_ms"]))
    f.write("\n`activate()` + `np.argsort` on %d host rows (what a user had): %.1f ms, %.2f us per row; `som_bmu_topk_device` at k = 8 with distances: %.4f us per row, x %.0f.\n"
            % (HOST_ROWS, res["activate_argsort_host"]["ms"], res["activate_argsort_host"]["us_per_row"], res["topk_k8_dist"]["us_per_row"],
               res["ratio_host_route_over_topk_k8_dist_per_row"]))
