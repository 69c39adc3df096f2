"""The codebook initialisers on rows that live in HBM, measured three ways.  One process, 1 warm-up, then the median of IB_REPS runs.
  1. the two moments passes (som_row_moments_device: the sums, then the sums and the Gram matrix about the mean) on IB_ROWS x 128
     and 250 000 x 784 device rows, each beside its own floor: the larger of the bytes read over the HBM bandwidth and
     2 n D^2 / 2 flops over the float32 MFMA peak (6.29 TB/s and 155 TFLOP/s, both as measured on this part)
  2. XPySom.linear_weights_init end to end on the IB_ROWS x 128 device rows against the only route there was before it: the rows
     copied to the host, np.cov, eigh and a Python loop over the units (timed once: it takes seconds)
  3. the benchmark's 25-epoch schedule at 256 x 256 x 128 on its blob rows from the seeded default codebook and from
     linear_weights_init: per-epoch times, blocks run per epoch (som_exact_skip_stats), the quantization error after epochs 5, 10
     and 25 (taken in a second, untimed run of the same schedule, so that the queries do not sit in the timed one)
Writes profiles/linear_init.json and profiles/linear_init.md (IB_OUT: another stem).
    IB_ROWS=1048576 IB_REPS=11 python tools/init_bench.py"""
import json, os, statistics, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xpysom_dask_amd import XPySom
from xpysom_dask_amd.decays import exponential_decay
from xpysom_dask_amd.engine import HipEngine
from xpysom_dask_amd.synthetic import gaussian_blobs

X = Y = 256; D = 128
N = int(os.environ.get("IB_ROWS", str(1 << 20))); T = int(os.environ.get("IB_EPOCHS", "25"))
N2, D2 = int(os.environ.get("IB_ROWS2", "250000")), 784
REPS = max(3, int(os.environ.get("IB_REPS", "11")))
OUT = os.environ.get("IB_OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "linear_init"))
HBM_BPS, MFMA_F32_FLOPS = 6.29e12, 155e12


def median_ms(fn, sync):
    fn(); sync()                                                    # warm-up: allocations
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter(); fn(); sync(); ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts)


res = {"reps": REPS, "method": "one process, 1 warm-up, median of reps, wall clock per call incl. the results' copy to the host",
       "floor_constants": {"hbm_bytes_per_s": HBM_BPS, "mfma_f32_flops": MFMA_F32_FLOPS}}

# ---- 1. the moments passes ----
res["moments"] = []
for n, d in ((N, D), (N2, D2)):
    rows = torch.from_numpy(np.random.RandomState(7).standard_normal((n, d)).astype(np.float32) + 3.0).cuda(); torch.cuda.synchronize()
    e = HipEngine(4, 4, d, precision="f32")
    _, s1, _ = e.row_moments_device(rows.data_ptr(), n, None, None, False)
    pivot = (s1 / n).astype(np.float32)
    sums = median_ms(lambda: e.row_moments_device(rows.data_ptr(), n, None, None, False), e.sync)
    full = median_ms(lambda: e.row_moments_device(rows.data_ptr(), n, None, pivot, True), e.sync)
    read_ms = 1e3 * n * d * 4 / HBM_BPS
    flop_ms = 1e3 * n * d * d / MFMA_F32_FLOPS
    # the second call runs the sums kernel again and then the Gram kernel: two reads of the rows
    r = {"rows": n, "features": d, "sums_pass_ms": sums[0], "sums_pass_min_ms": sums[1], "gram_pass_ms": full[0], "gram_pass_min_ms": full[1],
         "floor_sums_ms": read_ms, "floor_gram_ms": max(2 * read_ms, flop_ms), "floor_gram_bytes_ms": 2 * read_ms, "floor_gram_flops_ms": flop_ms}
    r["sums_fraction_of_floor"] = r["floor_sums_ms"] / sums[0]
    r["gram_fraction_of_floor"] = r["floor_gram_ms"] / full[0]
    res["moments"].append(r)
    print("moments %d x %d: sums %.3f ms (floor %.3f, %.0f %%) | sums + gram %.3f ms (floor %.3f, %.0f %%)"
          % (n, d, sums[0], read_ms, 100 * r["sums_fraction_of_floor"], full[0], r["floor_gram_ms"], 100 * r["gram_fraction_of_floor"]), flush=True)
    e.close(); del rows

# ---- 2. linear_weights_init end to end against the host route ----
data = gaussian_blobs(N, D, seed=1234, centre_seed=1234)
dev = torch.from_numpy(data).cuda(); torch.cuda.synchronize()
som = XPySom(X, Y, D, precision="exact", random_seed=1234)
lin = median_ms(lambda: som.linear_weights_init(dev), som._engine().sync)
w_lin = som._weights.copy()
t0 = time.perf_counter()
host = dev.cpu().numpy()
t_copy = time.perf_counter()
cov = np.cov(np.transpose(host))
t_cov = time.perf_counter()
lam, vec = np.linalg.eigh(cov)
mean = host.mean(axis=0, dtype=np.float64)
w_host = np.empty((X, Y, D), np.float32)
a1, a2 = np.sqrt(lam[-1]) * vec[:, -1], np.sqrt(lam[-2]) * vec[:, -2]
for i, c1 in enumerate(np.linspace(-1, 1, X)):
    for j, c2 in enumerate(np.linspace(-1, 1, Y)):
        w_host[i, j] = mean + c1 * a1 + c2 * a2
t1 = time.perf_counter()
res["linear_weights_init"] = {"rows": N, "features": D, "map": [X, Y], "device_ms": lin[0], "device_min_ms": lin[1],
                              "host_route_ms": 1e3 * (t1 - t0), "host_route_copy_ms": 1e3 * (t_copy - t0), "host_route_cov_ms": 1e3 * (t_cov - t_copy),
                              "host_route_eigh_and_loop_ms": 1e3 * (t1 - t_cov), "host_route_runs": 1}
res["linear_weights_init"]["device_is_faster"] = bool(lin[0] < 1e3 * (t1 - t0))
# (the two routes agree up to the sign of an axis, which the host route here does not fix: compare the spans)
res["linear_weights_init"]["corner_span_rel_diff"] = float(abs(np.linalg.norm(w_host[-1, 0] - w_host[0, 0]) - np.linalg.norm(w_lin[-1, 0] - w_lin[0, 0]))
                                                           / np.linalg.norm(w_lin[-1, 0] - w_lin[0, 0]))
print("linear_weights_init %d x %d on device rows: %.3f ms | host route (copy %.0f + np.cov %.0f + eigh and loop %.0f) %.0f ms"
      % (N, D, lin[0], 1e3 * (t_copy - t0), 1e3 * (t_cov - t_copy), 1e3 * (t1 - t_cov), 1e3 * (t1 - t0)), flush=True)
assert res["linear_weights_init"]["device_is_faster"]
del host, cov

# ---- 3. the schedule from both codebooks ----
rs = np.random.RandomState(1234)                                    # the seeded default codebook, as bench.py draws it
w0 = rs.rand(X, Y, D) * 2 - 1; w0 /= np.linalg.norm(w0, axis=-1, keepdims=True)
sched = [(exponential_decay(min(X, Y) / 2, 1, t, T), exponential_decay(0.5, 0.01, t, T)) for t in range(T)]
res["schedule"] = {"map": [X, Y, D], "rows": N, "epochs": T}
for name, w in (("default", w0.astype(np.float32)), ("linear_weights_init", w_lin)):
    runs = []
    for rep in range(REPS):
        e = HipEngine(X, Y, D, precision="exact"); e.set_weights(w); e.set_data_device(dev.data_ptr(), N, keepalive=dev); e.sync()
        ms, blocks = [], []
        for sig, eta in sched:
            b0 = e.exact_skip_stats()
            t0 = time.perf_counter(); e.epoch(sig, eta, True); e.sync(); ms.append(1e3 * (time.perf_counter() - t0))
            b1 = e.exact_skip_stats()
            blocks.append([b1[0] - b0[0], b1[1] - b0[1]])
        runs.append((ms, blocks)); e.close()
    e = HipEngine(X, Y, D, precision="exact"); e.set_weights(w); e.set_data_device(dev.data_ptr(), N, keepalive=dev)
    qe = {"0": e.quantization_error_device(dev.data_ptr(), N)}
    for t, (sig, eta) in enumerate(sched):
        e.epoch(sig, eta, True)
        if t + 1 in (5, 10, 25):
            qe[str(t + 1)] = e.quantization_error_device(dev.data_ptr(), N)
    e.close()
    per_epoch = [statistics.median(r[0][t] for r in runs) for t in range(T)]
    share = [statistics.median(r[1][t][0] / max(r[1][t][1], 1) for r in runs) for t in range(T)]
    res["schedule"][name] = {"epoch_ms": per_epoch, "blocks_run_share": share, "blocks_run_last_run": [b[0] for b in runs[-1][1]],
                             "blocks_total_per_epoch": runs[-1][1][0][1], "total_ms": sum(per_epoch), "quantization_error": qe}
    print("%-20s 25 epochs %.2f ms | first epochs %s | executed share %s | QE %s"
          % (name, sum(per_epoch), " ".join("%.2f" % v for v in per_epoch[:6]), " ".join("%.2f" % v for v in share[:6]),
             " ".join("%s: %.4f" % kv for kv in qe.items())), flush=True)

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT + ".json", "w") as f:
    json.dump(res, f, indent=1, sort_keys=True); f.write("\n")
L, S = res["linear_weights_init"], res["schedule"]
with open(OUT + ".md", "w") as f:
    f.write("# Codebook initialisers on device rows (tools/init_bench.py)\n\n%s.\n\n" % res["method"].capitalize())
    f.write("## The two moments passes\n\n| rows x features | sums pass ms | floor ms | share | sums + Gram pass ms | floor ms (bytes / flops) | share |\n|---|---|---|---|---|---|---|\n")
    for r in res["moments"]:
        f.write("| %d x %d | %.3f | %.3f | %.0f %% | %.3f | %.3f (%.3f / %.3f) | %.0f %% |\n" % (
            r["rows"], r["features"], r["sums_pass_ms"], r["floor_sums_ms"], 100 * r["sums_fraction_of_floor"], r["gram_pass_ms"],
            r["floor_gram_ms"], r["floor_gram_bytes_ms"], r["floor_gram_flops_ms"], 100 * r["gram_fraction_of_floor"]))
    f.write("\nFloor: the larger of the bytes read over %.2f TB/s and n D^2 flops over %.0f TFLOP/s.  Not gated.\n\n" % (HBM_BPS / 1e12, MFMA_F32_FLOPS / 1e12))
    f.write("## linear_weights_init end to end, %d x %d device rows, %d x %d map\n\n" % (N, D, X, Y))
    f.write("| route | ms |\n|---|---|\n| device moments + host eigh | %.3f |\n| copy to host %.0f + np.cov %.0f + eigh and per-unit loop %.0f (one run) | %.0f |\n\n"
            % (L["device_ms"], L["host_route_copy_ms"], L["host_route_cov_ms"], L["host_route_eigh_and_loop_ms"], L["host_route_ms"]))
    f.write("## The %d-epoch schedule at %d x %d x %d from both codebooks\n\n| epoch | default ms | share of blocks run | linear ms | share of blocks run |\n|---|---|---|---|---|\n" % (T, X, Y, D))
    for t in range(T):
        f.write("| %d | %.3f | %.3f | %.3f | %.3f |\n" % (t, S["default"]["epoch_ms"][t], S["default"]["blocks_run_share"][t],
                                                      S["linear_weights_init"]["epoch_ms"][t], S["linear_weights_init"]["blocks_run_share"][t]))
    f.write("| sum | %.3f | | %.3f | |\n\n" % (S["default"]["total_ms"], S["linear_weights_init"]["total_ms"]))
    f.write("| quantization error after epoch | default | linear |\n|---|---|---|\n")
    for k in S["default"]["quantization_error"]:
        f.write("| %s | %.6f | %.6f |\n" % (k, S["default"]["quantization_error"][k], S["linear_weights_init"]["quantization_error"][k]))
