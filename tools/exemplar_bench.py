"""The k nearest rows of every unit (som_unit_nearest_rows_device, csrc/exemplar.hpp) beside the float32 BMU search over the same rows:
one process, device-resident rows of the benchmark's blobs, a codebook of rows plus noise; 1 warm-up call, then the median of
EB_REPS calls each, every call closed by som_sync.  Two workloads: a 256 x 256 x 128 map with EB_ROWS rows, a 64 x 64 x 32 map
with 100 000.  Measured per workload:
  som_unit_nearest_rows_device at k = 1 and 8, ids + scores + distances (the (K, k) lists' copy to the host is inside the call);
  som_bmu_device on a precision='f32' handle -- existing code, the same 2 N K D float32 MFMA work: the yardstick.
Wall clock per call and the time of the call's kernels on the stream (the SOM_K_BMU event pairs: scan, merge, distances).
Writes EB_OUT (default profiles/exemplars.md); a "## Reading" section already in that file is kept.
    EB_ROWS=1048576 EB_REPS=11 python tools/exemplar_bench.py"""
import os, statistics, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xpysom_dask_amd.engine import HipEngine
from xpysom_dask_amd.synthetic import gaussian_blobs

REPS = max(3, int(os.environ.get("EB_REPS", "11")))
OUT = os.environ.get("EB_OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "exemplars.md"))
WORKLOADS = [(256, 256, 128, int(os.environ.get("EB_ROWS", str(1 << 20)))), (64, 64, 32, 100000)]


def timed(e, fn):
    fn(); e.sync()                                                  # warm-up: allocations, operand images
    e.profile_reset(); e.profile_enable(True)
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter(); out = fn(); e.sync(); ts.append(1e3 * (time.perf_counter() - t0))
    e.profile_enable(False)
    return out, {"ms": statistics.median(ts), "min_ms": min(ts), "kernels_ms": e.profile_get("bmu")[0] / REPS}


lines = ["# The k nearest rows of every unit beside the float32 BMU search\n",
         "`tools/exemplar_bench.py`: device rows, 1 warm-up, median of %d calls, one process.\n" % REPS]
for X, Y, D, N in WORKLOADS:
    data = gaussian_blobs(N, D, seed=1234, centre_seed=1234)
    rs = np.random.RandomState(1234)
    w = (data[rs.randint(0, N, X * Y)] + rs.normal(0.0, 0.5, (X * Y, D))).astype(np.float32)
    dev = torch.from_numpy(data).cuda(); torch.cuda.synchronize()
    e = HipEngine(X, Y, D, precision="f32"); e.set_weights(w)
    res, lists = {}, {}
    for k in (1, 8):
        lists[k], res["som_unit_nearest_rows_device, k = %d" % k] = timed(e, lambda: e.unit_nearest_rows_device(dev.data_ptr(), N, k))
    bmu, base = timed(e, lambda: e.bmu_device(dev.data_ptr(), N))
    e.close()
    # cross-checks: the shorter list heads the longer; every slot is filled; a list ascends by score
    assert np.array_equal(lists[1][0], lists[8][0][:, :1]) and (lists[8][0] >= 0).all()
    assert (np.diff(lists[8][1], axis=1) >= 0).all(), "a list does not ascend by score"
    flops = 2.0 * N * X * Y * D
    lines += ["## %d x %d x %d map, %d rows\n" % (X, Y, D, N),
              "| call | ms per call | kernels ms | TFLOP/s (kernels) | / float32 search (wall) | / float32 search (kernels) |\n|---|---|---|---|---|---|"]
    for label, r in [("som_bmu_device, precision f32", base)] + list(res.items()):
        row = "| %s | %.2f | %.2f | %.1f | %.3f | %.3f |" % (label, r["ms"], r["kernels_ms"], flops / (r["kernels_ms"] * 1e-3) / 1e12,
                                                          r["ms"] / base["ms"], r["kernels_ms"] / base["kernels_ms"])
        lines.append(row); print(row, flush=True)
    lines.append("")
    del dev
reading = ""
if os.path.exists(OUT):
    old = open(OUT).read()
    reading = old[old.index("## Reading"):] if "## Reading" in old else ""
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n" + reading)
