"""The map diagnostics on rows that live in HBM: som_bmu_distances_device and som_unit_stats_device next to their yardstick,
som_quantization_error_device, over the DB_ROWS device-resident rows the map was trained on (the benchmark's blobs) on the
256 x 256 x 128 map in precision 'exact' after the benchmark's 25-epoch schedule.  One process, 1 warm-up call, then the median of
DB_REPS calls each (wall clock per call, including the results' copy to the host), with the time the calls' kernel families
spent on the stream (som_profile_*: `bmu` the search, `segsum` the sort by unit + the per-unit reduction, `prep` the operands).
quantization_error_device's code is the parent's: it times the pass the two new calls build on.  bmu_distances adds one 4 B/row
write and the copy of ids and distances to the host; unit_stats adds a sort of the (unit, row) pairs and one pass over the
distances.  Writes a JSON document (DB_OUT, default profiles/unit_stats.json) and a summary (DB_MD, default
profiles/unit_stats.md); `unit_stats_within_budget` says whether unit_stats cost at most quantization_error's time plus the
0.36 ms README gives for the update's whole steady-state cost at this size.
    DB_ROWS=1048576 DB_REPS=11 python tools/diag_bench.py"""
import json, math, os, statistics, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xpysom_dask_amd.decays import exponential_decay
from xpysom_dask_amd.engine import HipEngine
from xpysom_dask_amd.synthetic import gaussian_blobs

X = Y = 256; D = 128
N = int(os.environ.get("DB_ROWS", str(1 << 20))); T = int(os.environ.get("DB_EPOCHS", "25"))
REPS = max(3, int(os.environ.get("DB_REPS", "11")))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("DB_OUT", os.path.join(ROOT, "profiles", "unit_stats.json"))
MD = os.environ.get("DB_MD", os.path.splitext(OUT)[0] + ".md")
UPDATE_BUDGET_MS = 0.36                                             # README: the update's steady-state cost at this size
data = gaussian_blobs(N, D, seed=1234, centre_seed=1234)
rs = np.random.RandomState(1234)
w = rs.rand(X, Y, D) * 2 - 1; w /= np.linalg.norm(w, axis=-1, keepdims=True)
dev = torch.from_numpy(data).cuda(); torch.cuda.synchronize()        # the benchmark's own rows
e = HipEngine(X, Y, D, precision="exact"); e.set_data_device(dev.data_ptr(), N, keepalive=dev); e.set_weights(w.astype(np.float32))
for t in range(T):
    e.epoch(exponential_decay(128, 1, t, T), exponential_decay(0.5, 0.01, t, T), True)
e.sync()


def timed(fn):
    fn(); e.sync()                                                  # warm-up: allocations, operand images
    e.profile_reset(); e.profile_enable(True)
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter(); out = fn(); e.sync(); ts.append(1e3 * (time.perf_counter() - t0))
    e.profile_enable(False)
    kern = {k: e.profile_get(k)[0] / REPS for k in ("bmu", "screen", "segsum", "prep")}
    return out, {"median_ms": statistics.median(ts), "min_ms": min(ts), "stream_ms": kern}


ptr = dev.data_ptr()
res = {"map": [X, Y, D], "rows": N, "epochs": T, "reps": REPS, "precision": "exact",
       "method": "1 warm-up, median of reps, wall clock per call incl. the results' copy to the host"}
qe, res["quantization_error_device"] = timed(lambda: e.quantization_error_device(ptr, N))
(ids, dist), res["bmu_distances_device"] = timed(lambda: e.bmu_distances_device(ptr, N))
(cnt, tot, sq, mx), res["unit_stats_device"] = timed(lambda: e.unit_stats_device(ptr, N))
rows, rows_sqrt = e.qe_stats()
res["qe_rows"], res["qe_rows_sqrt"] = rows, rows_sqrt
# the three calls describe the same rows
res["quantization_error"] = qe
res["mean_of_unit_sums"] = math.fsum(tot.tolist()) / N
res["agree_1e-12"] = bool(abs(res["mean_of_unit_sums"] - qe) <= 1e-12 * abs(qe))
res["counts_equal_bincount"] = bool(np.array_equal(cnt, np.bincount(ids, minlength=X * Y)))
res["units_hit"] = int((cnt > 0).sum()); res["largest_unit_rows"] = int(cnt.max())
q, b, u = (res[k]["median_ms"] for k in ("quantization_error_device", "bmu_distances_device", "unit_stats_device"))
res["bmu_distances_over_qe_ms"], res["unit_stats_over_qe_ms"] = b - q, u - q
res["update_budget_ms"] = UPDATE_BUDGET_MS
res["unit_stats_within_budget"] = bool(u <= q + UPDATE_BUDGET_MS)
e.close()
for k in ("quantization_error_device", "bmu_distances_device", "unit_stats_device"):
    r = res[k]
    print("%-26s %.3f ms (min %.3f; on the stream: bmu %.3f, of it the screen %.3f, segsum %.3f, prep %.3f)"
          % (k, r["median_ms"], r["min_ms"], r["stream_ms"]["bmu"], r["stream_ms"]["screen"], r["stream_ms"]["segsum"], r["stream_ms"]["prep"]), flush=True)
print("QE %.9g | mean of the unit sums %.9g | agree to 1e-12: %s | counts equal bincount: %s | unit_stats within QE + %.2f ms: %s"
      % (qe, res["mean_of_unit_sums"], res["agree_1e-12"], res["counts_equal_bincount"], UPDATE_BUDGET_MS, res["unit_stats_within_budget"]), flush=True)
assert res["agree_1e-12"] and res["counts_equal_bincount"]
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
with open(MD, "w") as f:
    f.write("# Map diagnostics on device rows: timings\n\n")
    f.write("`tools/diag_bench.py`: %d x %d x %d map, precision `exact`, after the benchmark's %d-epoch schedule, on the %d device rows it\n"
            "trained on.  One process, 1 warm-up call, then the median of %d calls; wall clock per call including the results' copy to the\n"
            "host.  `quantization_error_device` is unchanged code: it times the pass the two new calls build on.\n\n" % (X, Y, D, T, N, REPS))
    f.write("| call | median ms | min ms | stream: bmu | of it screen | stream: segsum (sort + per-unit pass) |\n|---|---|---|---|---|---|\n")
    for k in ("quantization_error_device", "bmu_distances_device", "unit_stats_device"):
        r = res[k]
        f.write("| `%s` | %.3f | %.3f | %.3f | %.3f | %.3f |\n" % (k, r["median_ms"], r["min_ms"], r["stream_ms"]["bmu"], r["stream_ms"]["screen"], r["stream_ms"]["segsum"]))
    f.write("\n- `bmu_distances_device` over `quantization_error_device`: %+.3f ms (one 4 B/row write, %d MB of ids and distances to the host).\n"
            % (res["bmu_distances_over_qe_ms"], 8 * N >> 20))
    f.write("- `unit_stats_device` over `quantization_error_device`: %+.3f ms (the sort of the pairs, one pass over the distances, four\n"
            "  K-entry copies); the yardstick is QE's time + %.2f ms, the update's whole steady-state cost at this size: %s.\n"
            % (res["unit_stats_over_qe_ms"], UPDATE_BUDGET_MS, "within it" if res["unit_stats_within_budget"] else "EXCEEDED"))
    f.write("- The three calls agree: the mean of the unit sums equals `quantization_error` to 1e-12 (%s), the counts equal `bincount` of\n"
            "  the ids (%s); %d of %d units win rows, the largest %d.\n"
            % (res["agree_1e-12"], res["counts_equal_bincount"], res["units_hit"], X * Y, res["largest_unit_rows"]))
