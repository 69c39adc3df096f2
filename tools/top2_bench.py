"""topographic_error's top-2 search on rows that live in HBM: som_bmu_top2_device and XPySom.topographic_error over
the TB_ROWS device-resident rows the map was trained on (the benchmark's blobs) on the 256 x 256 x 128 map after the
benchmark's 25-epoch schedule --
with the default settings (precision 'exact': the screen's second-smallest window + two float32 re-score rounds) and under
SOM_EXACT_TOP2=0 (the float32 top-2 kernel for every row: the kernel and launch before the fast path existed).  One process,
1 warm-up call, then the median of TB_REPS calls each; `winner` on the same rows with every block run (SOM_EXACT_SKIP=0)
and the top-2 row counters for context; small row counts (TB_SMALL) for the break-even against the single float32 launch.
topographic_error's figure includes the host's adjacency pass over the pairs (NumPy; reported as host_adjacency_ms = its
time less bmu_top2_device's), the same on both sides.  Writes one JSON document (TB_OUT, default profiles/top2_query.json);
`acceptance_third` says whether the default path took at most a third of the off switch's time.
    TB_ROWS=1048576 TB_REPS=11 python tools/top2_bench.py"""
import json, os, statistics, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xpysom_dask_amd import XPySom
from xpysom_dask_amd.decays import exponential_decay
from xpysom_dask_amd.engine import HipEngine
from xpysom_dask_amd.synthetic import gaussian_blobs

X = Y = 256; D = 128
N = int(os.environ.get("TB_ROWS", str(1 << 20))); T = int(os.environ.get("TB_EPOCHS", "25"))
REPS = max(10, int(os.environ.get("TB_REPS", "11")))
OUT = os.environ.get("TB_OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "top2_query.json"))
data = gaussian_blobs(N, D, seed=1234, centre_seed=1234)
SMALL = [int(v) for v in os.environ.get("TB_SMALL", "256,1024,4096,16384,65536").split(",") if v]
rs = np.random.RandomState(1234)
w = rs.rand(X, Y, D) * 2 - 1; w /= np.linalg.norm(w, axis=-1, keepdims=True)
tr = HipEngine(X, Y, D, precision="exact"); tr.set_data(data); tr.set_weights(w.astype(np.float32))
for t in range(T):
    tr.epoch(exponential_decay(128, 1, t, T), exponential_decay(0.5, 0.01, t, T), True)
wt = tr.get_weights(); tr.close()
dev = torch.from_numpy(data).cuda(); torch.cuda.synchronize()        # the benchmark's own rows


def model(**env):
    os.environ.update({k: str(v) for k, v in env.items()})
    som = XPySom(X, Y, D, precision="exact"); som._weights = wt.reshape(X, Y, D); som._upload_weights()
    for k in env:
        del os.environ[k]
    return som


def timed(e, fn, reps=None):
    reps = reps or REPS
    fn(); e.sync()                                                  # warm-up: allocations, operand images
    e.profile_reset(); e.profile_enable(True)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); e.sync(); ts.append(1e3 * (time.perf_counter() - t0))
    e.profile_enable(False)
    kern = {k: e.profile_get(k)[0] / reps for k in ("bmu", "screen", "prep")}
    return out, statistics.median(ts), min(ts), kern


fast, off, full = model(), model(SOM_EXACT_TOP2=0), model(SOM_EXACT_SKIP=0)
res = {"map": [X, Y, D], "rows": N, "epochs": T, "reps": REPS, "method": "1 warm-up, median of reps, wall clock per call incl. the ids' copy to the host"}
for name, som in (("default", fast), ("SOM_EXACT_TOP2=0", off)):
    e = som._engine()
    pair, med, best, kern = timed(e, lambda: e.bmu_top2_device(dev.data_ptr(), N))
    te, med_te, best_te, _ = timed(e, lambda: som.topographic_error(dev))
    rows, rows_f32 = e.exact_top2_stats()
    small = {str(n): timed(e, lambda: e.bmu_top2_device(dev.data_ptr(), n))[1] for n in SMALL if n <= N}
    res[name] = {"small_rows_ms": small, "host_adjacency_ms": med_te - med,"bmu_top2_device_ms": med, "bmu_top2_device_min_ms": best, "topographic_error_ms": med_te, "topographic_error_min_ms": best_te,
                 "stream_ms": kern, "topographic_error": te, "top2_rows": rows, "top2_rows_f32": rows_f32, "pair": pair}
    print("%-18s bmu_top2_device %.3f ms (min %.3f; on the stream: BMU family %.3f, of it the screen %.3f) | topographic_error %.3f ms = %.6f | rows %d, to the float32 kernel %d"
          % (name, med, best, kern["bmu"], kern["screen"], med_te, te, rows, rows_f32), flush=True)
a, b = res["default"].pop("pair"), res["SOM_EXACT_TOP2=0"].pop("pair")
res["ids_equal"] = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
res["topographic_error_equal"] = res["default"]["topographic_error"] == res["SOM_EXACT_TOP2=0"]["topographic_error"]
e = full._engine()
ids, med_w, best_w, kern_w = timed(e, lambda: e.bmu_device(dev.data_ptr(), N))
res["winner_every_block"] = {"bmu_device_ms": med_w, "min_ms": best_w, "stream_ms": kern_w, "first_ids_equal": bool(np.array_equal(ids, a[0]))}
res["ratio_default_over_off"] = res["default"]["bmu_top2_device_ms"] / res["SOM_EXACT_TOP2=0"]["bmu_top2_device_ms"]
res["ratio_topographic_error"] = res["default"]["topographic_error_ms"] / res["SOM_EXACT_TOP2=0"]["topographic_error_ms"]
res["acceptance_third"] = bool(res["ratio_default_over_off"] <= 1.0 / 3.0)
print("small row counts, default vs off (ms): " + ", ".join("%s: %.3f vs %.3f" % (n, res["default"]["small_rows_ms"][n], res["SOM_EXACT_TOP2=0"]["small_rows_ms"][n])
                                                             for n in res["default"]["small_rows_ms"]), flush=True)
print("winner, every block: %.3f ms | default / off: %.3f (bmu_top2_device), %.3f (topographic_error) | ids equal %s"
      % (med_w, res["ratio_default_over_off"], res["ratio_topographic_error"], res["ids_equal"]), flush=True)
assert res["ids_equal"] and res["topographic_error_equal"]
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
