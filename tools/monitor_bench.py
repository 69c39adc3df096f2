"""What the training monitor costs: 256 x 256 x 128 map, precision 'exact', MB_ROWS blob rows resident in HBM (the benchmark's
generator), the benchmark's MB_EPOCHS-epoch schedule, through the product's own epoch driver (distributed.epoch).

  unmonitored / monitored   schedules alternate in one process, MB_REPS times each; per schedule the mean epoch time of epochs
                            5 ... T-1 (host clock between two stream synchronisations around that span), and the spread over the
                            repetitions.  The monitored schedule's records are checked to be identical across repetitions, and its
                            codebook to equal the unmonitored one bit for bit.
  old way                   the same curve without the monitor: a loop of train(rows, T, iter_beg=t, iter_end=t+1) with a
                            quantization_error(rows) between the epochs, on the same device rows.  It uses nothing this tool's
                            feature added, so it runs unchanged on a tree from before the monitor (MB_MODE=old).
  quantization_error        one call on the same device rows after the schedule, median of 5: what a second BMU search costs

MB_MODE = all (default) | monitored (the monitored schedule alone, MB_REPS times: the run to put under a kernel trace) | old.
Writes a JSON document to MB_OUT (default profiles/monitor.json under the tree) and prints a summary.
    MB_ROWS=1048576 MB_EPOCHS=25 MB_REPS=3 python tools/monitor_bench.py"""
import json, os, statistics, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xpysom_dask_amd import XPySom
from xpysom_dask_amd import distributed as D
from xpysom_dask_amd.decays import exponential_decay
from xpysom_dask_amd.engine import HipEngine
from xpysom_dask_amd.synthetic import gaussian_blobs

X = Y = 256; DIM = 128
N = int(os.environ.get("MB_ROWS", str(1 << 20))); T = int(os.environ.get("MB_EPOCHS", "25")); FIRST = min(5, T - 1)
REPS = max(1, int(os.environ.get("MB_REPS", "3"))); MODE = os.environ.get("MB_MODE", "all")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("MB_OUT", os.path.join(ROOT, "profiles", "monitor.json"))
data = gaussian_blobs(N, DIM, seed=1234, centre_seed=1234)
rs = np.random.RandomState(1234)
w0 = rs.rand(X, Y, DIM) * 2 - 1; w0 /= np.linalg.norm(w0, axis=-1, keepdims=True); w0 = w0.astype(np.float32)
dev = torch.from_numpy(data).cuda(); torch.cuda.synchronize()
res = {"map": [X, Y, DIM], "rows": N, "epochs": T, "mean_over_epochs": [FIRST, T - 1], "reps": REPS, "precision": "exact"}


def schedule(monitored):
    """One schedule on a fresh engine: (mean ms of epochs FIRST ... T-1, records, final codebook)."""
    e = HipEngine(X, Y, DIM, precision="exact")
    try:
        e.set_weights(w0); e.set_data_device(dev.data_ptr(), N, keepalive=dev)
        if monitored:
            e.monitor(True)
        recs = []
        for t in range(T):
            if t == FIRST:
                e.sync(); t0 = time.perf_counter()
            sig, eta = exponential_decay(128, 1, t, T), exponential_decay(0.5, 0.01, t, T)
            if monitored:
                m = {}; D.epoch(e, sig, eta, True, metrics=m); recs.append(m)
            else:
                D.epoch(e, sig, eta, True)
        e.sync(); ms = 1e3 * (time.perf_counter() - t0) / (T - FIRST)
        return ms, recs, e.get_weights()
    finally:
        e.close()


def old_way():
    """The curve the old way: (mean ms of iterations FIRST ... T-1 incl. their quantization_error call, the curve)."""
    som = XPySom(X, Y, DIM, sigma=128, random_seed=1234, precision="exact")
    som._weights = w0.copy()
    curve = []
    for t in range(T):
        if t == FIRST:
            torch.cuda.synchronize(); t0 = time.perf_counter()
        som.train(dev, T, iter_beg=t, iter_end=t + 1)
        curve.append(float(som.quantization_error(dev)))
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / (T - FIRST), curve


def spread(v):
    return {"mean_ms": statistics.mean(v), "min_ms": min(v), "max_ms": max(v), "all_ms": v}


if MODE in ("all", "monitored"):
    schedule(False)                                                 # warm-up: first allocations, first launches of every kernel
    un, mo, recs, w_un, w_mo = [], [], None, None, None
    for r in range(REPS):
        if MODE == "all":
            ms, _, w_un = schedule(False); un.append(ms)
        ms, rr, w_mo = schedule(True); mo.append(ms)
        assert recs is None or rr == recs, "two monitored schedules returned different records"
        recs = rr
    res["monitored"] = spread(mo)
    res["records"] = recs
    print("monitored   %.3f ms / epoch (min %.3f, max %.3f)" % (res["monitored"]["mean_ms"], min(mo), max(mo)), flush=True)
    if MODE == "all":
        assert np.array_equal(w_un.view(np.uint32), w_mo.view(np.uint32)), "the monitor changed the trained codebook"
        res["unmonitored"] = spread(un)
        res["added_ms"] = res["monitored"]["mean_ms"] - res["unmonitored"]["mean_ms"]
        print("unmonitored %.3f ms / epoch (min %.3f, max %.3f); the monitor adds %.3f ms" % (res["unmonitored"]["mean_ms"], min(un), max(un), res["added_ms"]), flush=True)
if MODE in ("all", "old"):
    old_way()                                                       # warm-up
    olds = [old_way() for _ in range(REPS)]
    res["old_way"] = spread([o[0] for o in olds]); res["old_way_curve"] = olds[-1][1]
    print("old way     %.3f ms / iteration (train of one epoch + quantization_error)" % res["old_way"]["mean_ms"], flush=True)
    som = XPySom(X, Y, DIM, sigma=128, random_seed=1234, precision="exact"); som._weights = w0.copy(); som.train(dev, T)
    ts = []
    for _ in range(6):
        torch.cuda.synchronize(); t0 = time.perf_counter(); som.quantization_error(dev); ts.append(1e3 * (time.perf_counter() - t0))
    res["quantization_error_call_ms"] = statistics.median(ts[1:])
    print("quantization_error(device rows) %.3f ms" % res["quantization_error_call_ms"], flush=True)
if MODE == "all":
    yard = res["unmonitored"]["mean_ms"] + res["quantization_error_call_ms"]
    res["yardstick_ms"] = yard
    res["monitored_below_yardstick"] = bool(res["monitored"]["mean_ms"] < yard)
    print("monitored epoch %.3f ms against an unmonitored epoch + one quantization_error call = %.3f ms: %s"
          % (res["monitored"]["mean_ms"], yard, "below" if res["monitored_below_yardstick"] else "NOT below"), flush=True)
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True); f.write("\n")
