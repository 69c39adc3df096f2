"""precision='exact' beyond 800 features (the GM instance of the two-sided tiling, csrc/bmu_bf16_tiled.hpp) beside what served
these shapes before: one process, 256 x 256 maps (a codebook of rows plus noise) at 1024 and 2048 features, EL_ROWS device-resident
Gaussian-blob rows (drawn on the device); 1 warm-up call, then the median of EL_REPS calls, every call closed by som_sync, the
codebook set back before every call.  Per feature count:
  exact          the epoch (som_epoch) and the BMU launch (som_bmu_device): wall clock, the launch's kernels on the stream
                 (SOM_K_BMU) and the screen kernel alone (SOM_K_SCREEN); the rest of the launch -- select, re-score, finalize,
                 fallback -- is the difference (the library times no finer families); candidate groups per row, fallback rows;
  exact_long0    the same calls on a handle created under SOM_EXACT_LONG=0: the float32 kernels, what these shapes ran before;
  f16            som_bmu_device on a precision='f16' handle: the same MFMA work with the argmin epilogue.
Writes EL_OUT (default profiles/exact_long.json) and a table next to it (.md).
    EL_ROWS=250000 EL_REPS=11 python tools/exact_long_bench.py"""
import json, os, statistics, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["SOM_TEST_HOOKS"] = "1"                                 # (SOM_EXACT_LONG is a developer switch)
from xpysom_dask_amd.engine import HipEngine

X = Y = 256
N = int(os.environ.get("EL_ROWS", "250000")); REPS = max(3, int(os.environ.get("EL_REPS", "11")))
DIMS = [int(d) for d in os.environ.get("EL_DIMS", "1024,2048").split(",")]
OUT = os.environ.get("EL_OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "exact_long.json"))


def timed(e, w, fn):
    def once():
        e.set_weights(w); e.sync()
        t0 = time.perf_counter(); out = fn(); e.sync()
        return out, 1e3 * (time.perf_counter() - t0)
    once()                                                          # warm-up: allocations, operand images
    e.profile_reset(); e.profile_enable(True)
    ts = [once() for _ in range(REPS)]
    e.profile_enable(False)
    return ts[-1][0], {"ms": statistics.median(t for _, t in ts), "min_ms": min(t for _, t in ts),
                       "bmu_kernels_ms": e.profile_get("bmu")[0] / REPS, "screen_ms": e.profile_get("screen")[0] / REPS}


res = {"map": [X, Y], "rows": N, "reps": REPS,
       "method": "one process, 1 warm-up, median of reps, wall clock per call closed by som_sync; *_kernels_ms / screen_ms: event pairs on the stream"}
for D in DIMS:
    g = torch.Generator(device="cuda"); g.manual_seed(1234 + D)
    centres = 3.0 * torch.randn(64, D, device="cuda", generator=g)
    dev = centres[torch.randint(0, 64, (N,), device="cuda", generator=g)] + torch.randn(N, D, device="cuda", generator=g)
    pick = torch.randint(0, N, (X * Y,), device="cuda", generator=g)
    w = (dev[pick] + 0.5 * torch.randn(X * Y, D, device="cuda", generator=g)).cpu().numpy()
    torch.cuda.synchronize()
    r, ids = {}, {}
    for name, prec, env in (("exact", "exact", None), ("exact_long0", "exact", "0"), ("f16", "f16", None)):
        if env is not None:
            os.environ["SOM_EXACT_LONG"] = env
        e = HipEngine(X, Y, D, precision=prec)
        os.environ.pop("SOM_EXACT_LONG", None)
        e.set_weights(w)
        ids[name], r[name + "_bmu"] = timed(e, w, lambda: e.bmu_device(dev.data_ptr(), N))
        if prec == "exact":
            rows, fb, _ = e.exact_stats()
            r[name + "_bmu"].update(screened_rows=rows, fallback_rows_per_call=fb / (REPS + 1),
                                    candidate_groups_per_row=float(e.exact_last_counts(min(N, 65536)).mean()) if rows else None)
            e.set_data_device(dev.data_ptr(), N, keepalive=dev)
            _, r[name + "_epoch"] = timed(e, w, lambda: e.epoch(4.0, 0.1, True))
        e.close()
    assert np.array_equal(ids["exact"], ids["exact_long0"]), "the screen left the float32 BMUs"
    assert r["exact_bmu"]["screened_rows"] == (REPS + 1) * N and r["exact_long0_bmu"]["screened_rows"] == 0
    r["f16_agrees_with_f32"] = float((ids["f16"] == ids["exact"]).mean())
    r["ratio_exact_epoch_over_f32_epoch"] = r["exact_epoch"]["ms"] / r["exact_long0_epoch"]["ms"]
    r["ratio_exact_bmu_over_f32_bmu"] = r["exact_bmu"]["ms"] / r["exact_long0_bmu"]["ms"]
    r["ratio_screen_over_f16_kernels"] = r["exact_bmu"]["screen_ms"] / r["f16_bmu"]["bmu_kernels_ms"]
    r["screen_tflops"] = 2.0 * N * X * Y * D / (r["exact_bmu"]["screen_ms"] * 1e-3) / 1e12
    res["D%d" % D] = r
    print(D, json.dumps(r, sort_keys=True), flush=True)
    del dev, centres
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
with open(os.path.splitext(OUT)[0] + ".md", "w") as f:
    f.write("# precision='exact' beyond 800 features: the tiled group-minimum screen\n\n`tools/exact_long_bench.py`: %d x %d maps, %d device rows, "
            "1 warm-up, median of %d calls, one process.  `exact, SOM_EXACT_LONG=0` is what these shapes ran before (the float32 kernels).  "
            "The library times the whole BMU launch and its screen kernel; select, re-score, finalize and fallback are the difference, "
            "not measured apart.\n\n" % (X, Y, N, REPS))
    f.write("| features | call | wall ms | BMU launch kernels ms | screen ms | launch - screen ms | candidate groups / row | fallback rows / call |\n|---|---|---|---|---|---|---|---|\n")
    for D in DIMS:
        r = res["D%d" % D]
        for k, label in (("exact_epoch", "exact, epoch"), ("exact_bmu", "exact, som_bmu_device"), ("exact_long0_epoch", "exact, SOM_EXACT_LONG=0, epoch"),
                         ("exact_long0_bmu", "exact, SOM_EXACT_LONG=0, som_bmu_device"), ("f16_bmu", "f16, som_bmu_device")):
            v = r[k]
            f.write("| %d | %s | %.2f | %.2f | %.2f | %.2f | %s | %s |\n" % (
                D, label, v["ms"], v["bmu_kernels_ms"], v["screen_ms"], v["bmu_kernels_ms"] - v["screen_ms"],
                "%.2f" % v["candidate_groups_per_row"] if v.get("candidate_groups_per_row") is not None else "-",
                "%.1f" % v["fallback_rows_per_call"] if "fallback_rows_per_call" in v else "-"))
    f.write("\n")
    for D in DIMS:
        r = res["D%d" % D]
        f.write("%d features: exact epoch / float32 epoch = %.3f; exact BMU launch / float32 = %.3f; screen / f16 tiled kernel = %.3f (%.0f TFLOP/s); "
                "f16 ids equal to float32's on %.4f of the rows.\n\n" % (D, r["ratio_exact_epoch_over_f32_epoch"], r["ratio_exact_bmu_over_f32_bmu"],
                                                                        r["ratio_screen_over_f16_kernels"], r["screen_tflops"], r["f16_agrees_with_f32"]))
