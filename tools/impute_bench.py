"""Missing values, the completed rows, on rows that live in HBM: som_impute_device (the masked search + the fill of
csrc/impute.hpp) next to its yardstick, a hipMemcpyAsync device-to-device copy of the same N * D * 4 bytes, and next to the
route it replaces, XPySom.quantization + np.where on the host with the copies that route needs.  IB_ROWS device rows (the
benchmark's blobs) with 30 % of the values NaN on a 256 x 256 map trained on them for IB_EPOCHS epochs with missing='nan', at
D = 128 and again at D = 16.  One process, 1 warm-up call, then the median of IB_REPS calls each.
  search        som_bmu_device: wall clock, and the time of its kernels on the stream (som_profile_*, `bmu`)
  fill          som_impute_device out of place and in place: wall clock (search + fill + the ids' copy), and the fill kernel
                alone on the stream (`fill`: hipEvents around the one launch) -- the figure to hold against the copy
  copy          hipMemcpyAsync(device to device), N * D * 4 bytes, hipEvents around it on a stream of its own
  host route    quantization(rows) + np.where(isnan(rows), ., rows) + the upload of the result: wall clock (IB_HOST_REPS calls)
The in-place calls start from a fresh copy of the rows each (made outside the timed part).  Every result is compared, bit for
bit, with where(isnan(x), W[ids], x) formed by torch on the device.  Writes IB_OUT (default profiles/impute.json) and a summary
(IB_MD, default profiles/impute.md).
    IB_ROWS=1048576 IB_REPS=11 python tools/impute_bench.py"""
import ctypes as C, json, os, statistics, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xpysom_dask_amd import XPySom, _lib
from xpysom_dask_amd.synthetic import gaussian_blobs

X = Y = 256
N = int(os.environ.get("IB_ROWS", str(1 << 20))); T = int(os.environ.get("IB_EPOCHS", "3"))
REPS = max(3, int(os.environ.get("IB_REPS", "11"))); HOST_REPS = max(1, int(os.environ.get("IB_HOST_REPS", str(REPS))))
DIMS = [int(d) for d in os.environ.get("IB_DIMS", "128,16").split(",")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("IB_OUT", os.path.join(ROOT, "profiles", "impute.json"))
MD = os.environ.get("IB_MD", os.path.splitext(OUT)[0] + ".md")
hip = C.CDLL(_lib.torch_lib_file("libamdhip64.so") or "libamdhip64.so")
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
HIP_D2D = 3


def med(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def run(D):
    data = gaussian_blobs(N, D, seed=1234, centre_seed=1234)
    data[np.random.RandomState(77).rand(N, D) < 0.3] = np.nan
    x = torch.from_numpy(data).cuda(); torch.cuda.synchronize()
    s = XPySom(X, Y, D, sigma=16.0, learning_rate=0.5, random_seed=5, missing="nan", precision="exact")
    s.train(x, T)
    e = s._upload_weights()
    ptr, nbytes = x.data_ptr(), N * D * 4
    out, work = torch.empty_like(x), torch.empty_like(x)

    def calls(fn, slots, before=None, reps=REPS):
        """wall clock per call and, per slot, the time of that kernel family on the stream per call"""
        wall, stream = [], {k: [] for k in slots}
        for i in range(reps + 1):
            if before:
                before()
            torch.cuda.synchronize(); e.sync(); e.profile_reset(); e.profile_enable(True)
            t0 = time.perf_counter(); r = fn(); e.sync(); dt = 1e3 * (time.perf_counter() - t0)
            e.profile_enable(False)
            if i:                                                   # (call 0 is the warm-up: allocations)
                wall.append(dt)
                for k in slots:
                    stream[k].append(e.profile_get(k)[0])
        return r, {"wall": med(wall), **{"stream_" + k: med(v) for k, v in stream.items()}}

    res = {"features": D, "bytes": nbytes, "holes_share": float(np.isnan(data).mean())}
    ids_s, res["search"] = calls(lambda: e.bmu_device(ptr, N), ("bmu",))
    ids_o, res["impute_out_of_place"] = calls(lambda: e.impute_device(ptr, N, out.data_ptr()), ("bmu", "fill"))
    ids_p, res["impute_in_place"] = calls(lambda: e.impute_device(work.data_ptr(), N, work.data_ptr()), ("bmu", "fill"),
                                          before=lambda: work.copy_(x))
    # the yardstick: one device-to-device copy of the same bytes
    st = torch.cuda.Stream(); a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dst, ts = torch.empty_like(x), []
    for i in range(REPS + 1):
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            a.record(st)
            assert hip.hipMemcpyAsync(dst.data_ptr(), ptr, nbytes, HIP_D2D, C.c_void_p(st.cuda_stream)) == 0
            b.record(st)
        st.synchronize()
        if i:
            ts.append(a.elapsed_time(b))
    res["copy_d2d"] = med(ts)
    assert torch.equal(dst.view(torch.int32), x.view(torch.int32))

    def host_route():
        q = s.quantization(x)                                       # ids to the host, an (N, D) gather from the host codebook
        xh = x.cpu().numpy()
        r = torch.from_numpy(np.where(np.isnan(xh), q, xh)).cuda(); torch.cuda.synchronize()
        return r
    hr, ts = None, []
    for i in range(HOST_REPS + 1):
        t0 = time.perf_counter(); hr = host_route(); dt = 1e3 * (time.perf_counter() - t0)
        if i:
            ts.append(dt)
    res["host_route"] = {"wall": med(ts), "reps": HOST_REPS}
    t0 = time.perf_counter(); py = s.impute(x, out=out); res["xpysom_impute_wall_ms"] = 1e3 * (time.perf_counter() - t0)
    # every route returns the same rows
    w = torch.from_numpy(np.asarray(s.get_weights(), np.float32).reshape(X * Y, D)).cuda()
    want = torch.where(torch.isnan(x), w[torch.from_numpy(ids_o).cuda().long()], x).view(torch.int32)
    res["ids_equal_search"] = bool(np.array_equal(ids_s, ids_o) and np.array_equal(ids_o, ids_p))
    res["bits_equal"] = bool(torch.equal(out.view(torch.int32), want) and torch.equal(work.view(torch.int32), want)
                             and torch.equal(py.view(torch.int32), want))
    res["host_route_equal"] = bool(torch.equal(hr.view(torch.int32), want))
    res["nan_left"] = int(torch.isnan(out).sum())
    f, c = res["impute_out_of_place"]["stream_fill"]["median_ms"], res["copy_d2d"]["median_ms"]
    res["fill_over_copy"] = f / c
    res["fill_in_place_over_copy"] = res["impute_in_place"]["stream_fill"]["median_ms"] / c
    res["fill_GBps_read_plus_write"] = 2 * nbytes / f / 1e6
    res["copy_GBps_read_plus_write"] = 2 * nbytes / c / 1e6
    res["fill_within_2x_copy"] = bool(f <= 2 * c)
    print("D = %d: search %.3f ms (stream %.3f) | fill on the stream: out of place %.4f ms, in place %.4f ms | copy %.4f ms | "
          "fill / copy %.2f | impute wall %.3f ms | host route %.1f ms | bits equal %s, ids equal %s, host route equal %s" % (
              D, res["search"]["wall"]["median_ms"], res["search"]["stream_bmu"]["median_ms"], f,
              res["impute_in_place"]["stream_fill"]["median_ms"], c, res["fill_over_copy"],
              res["impute_out_of_place"]["wall"]["median_ms"], res["host_route"]["wall"]["median_ms"], res["bits_equal"],
              res["ids_equal_search"], res["host_route_equal"]), flush=True)
    assert res["bits_equal"] and res["ids_equal_search"] and res["nan_left"] == 0
    e.close()
    return res


doc = {"map": [X, Y], "rows": N, "epochs": T, "reps": REPS, "precision": "exact", "missing": "nan",
       "method": "1 warm-up, median of reps; wall clock per call incl. the ids' copy to the host; stream_*: hipEvent time of the "
                 "kernel family per call; copy_d2d: hipEvents around one hipMemcpyAsync",
       "cases": [run(D) for D in DIMS]}
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(doc, f, indent=1, sort_keys=True)
    f.write("\n")
with open(MD, "w") as f:
    f.write("# `impute` on device rows: timings\n\n")
    f.write("`tools/impute_bench.py`: %d x %d map, `missing='nan'`, precision `exact`, trained for %d epochs on the %d device rows it\n"
            "then completes (the benchmark's blobs, 30 %% of the values NaN).  One process, 1 warm-up call, then the median of %d calls\n"
            "(minimum - maximum).  `stream`: hipEvent time of the kernels on the engine's stream; the copy is one `hipMemcpyAsync`\n"
            "device to device of the same N x D x 4 bytes between two events.  Raw figures: `profiles/impute.json`.\n\n" % (X, Y, T, N, REPS))
    f.write("| D | bytes | masked search, stream ms | fill out of place, stream ms | fill in place, stream ms | d2d copy ms | fill / copy |"
            " `som_impute_device` wall ms | host route wall ms |\n|---|---|---|---|---|---|---|---|---|\n")
    for r in doc["cases"]:
        g = lambda k, sub: "%.4f (%.4f - %.4f)" % (r[k][sub]["median_ms"], r[k][sub]["min_ms"], r[k][sub]["max_ms"])
        f.write("| %d | %d MB | %s | %s | %s | %.4f (%.4f - %.4f) | %.2f, in place %.2f | %s | %s |\n" % (
            r["features"], r["bytes"] >> 20, g("search", "stream_bmu"), g("impute_out_of_place", "stream_fill"),
            g("impute_in_place", "stream_fill"), r["copy_d2d"]["median_ms"], r["copy_d2d"]["min_ms"], r["copy_d2d"]["max_ms"],
            r["fill_over_copy"], r["fill_in_place_over_copy"], g("impute_out_of_place", "wall"), g("host_route", "wall")))
    f.write("\n")
    for r in doc["cases"]:
        f.write("- D = %d: the out-of-place fill moves %.0f GB/s (rows read + rows written; the copy: %.0f GB/s), and reads the ids and\n"
                "  the holes' codebook values on top; within twice the copy's time: %s.  The host route (`quantization` + `np.where`, the\n"
                "  rows down and the result up) returns the same bits: %s.  `XPySom.impute(rows, out=...)`, one call: %.1f ms.\n" % (
                    r["features"], r["fill_GBps_read_plus_write"], r["copy_GBps_read_plus_write"],
                    "yes" if r["fill_within_2x_copy"] else "NO", r["host_route_equal"], r["xpysom_impute_wall_ms"]))
