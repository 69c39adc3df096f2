"""Sparse rows (som_bmu_csr, the sparse epoch; csrc/sparse.hpp) beside the dense float32 search over the same rows made dense: one
process, a 64 x 64 map, input_len 8192, SB_ROWS rows on a (stratified) random support at densities of 0.1 %, 1 % and 10 %; 1 warm-up, then the median
of SB_REPS calls, every call closed by som_sync.  Measured per density:
  som_bmu_csr                  wall clock (the host check and the upload of the CSR arrays are inside the call) and the kernels on the
                               stream (the SOM_K_BMU event pairs: transpose, scan, merge) -- the rows are device-resident for those
  the sparse epoch             som_epoch_accumulate + som_epoch_merge over resident CSR rows; search, segment sum, transform and merge
                               apart (the SOM_K_* event pairs)
  the skewed epoch             the same with a codebook under which ONE unit wins every row: the segment sum's known worst case
  som_bmu_device, 'f32'        the dense float32 MFMA search over the same rows as a 2 GB device array: the comparison
and one row at input_len 50 000, 1 % density, where the dense form is not attempted.  The search's achieved rate is 4 nnz K bytes (its
cache-read model) over the scan's time.  Writes SB_OUT (default profiles/sparse.json) and a table next to it (.md).
    SB_ROWS=65536 SB_REPS=11 python tools/sparse_bench.py"""
import json, os, statistics, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xpysom_dask_amd.engine import HipEngine

X = Y = 64; K = X * Y
N = int(os.environ.get("SB_ROWS", "65536")); REPS = max(3, int(os.environ.get("SB_REPS", "11")))
OUT = os.environ.get("SB_OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sparse.json"))
FAMILIES = ("bmu", "segsum", "kron", "merge")


def make_csr(n, D, density, seed):
    """n rows of round(density * D) entries each on a stratified random support (one column drawn from each of as many equal
    strata of the columns: distinct and ascending by construction), values uniform in (0, 1]"""
    rs = np.random.RandomState(seed)
    per = max(1, int(round(density * D)))
    cols = ((np.arange(per, dtype=np.int64) * D // per)[None, :] + rs.randint(0, D // per, (n, per))).astype(np.int32)
    vals = (1.0 - rs.rand(n, per)).astype(np.float32)
    return np.arange(0, n * per + 1, per, dtype=np.int64), cols.reshape(-1), vals.reshape(-1)


def timed(e, fn, reps=REPS):
    fn(); e.sync()                                                  # warm-up: allocations, the transposed codebook's buffer
    e.profile_reset(); e.profile_enable(True)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); e.sync(); ts.append(1e3 * (time.perf_counter() - t0))
    e.profile_enable(False)
    r = {"ms": statistics.median(ts), "min_ms": min(ts)}
    r.update({k + "_ms": e.profile_get(k)[0] / reps for k in FAMILIES})
    return out, r


def epoch(e, w, reset=False):
    """reset: every call starts from w again (the upload is outside the kernels' event pairs, inside the wall clock)"""
    def run():
        if reset:
            e.set_weights(w)
        e.epoch_accumulate(np.float64(4.0), 0.5, True); e.epoch_merge()
    e.set_weights(w)
    return timed(e, run)[1]


def one(D, density, dense, reps=REPS):
    csr = make_csr(N, D, density, 1234)
    nnz = int(csr[0][-1])
    rs = np.random.RandomState(5)
    w = rs.rand(K, D).astype(np.float32)
    r = {"input_len": D, "density": density, "nnz": nnz, "model_bytes": 4.0 * nnz * K}
    e = HipEngine(X, Y, D, precision="f32"); e.set_weights(w)
    ids, r["bmu_csr"] = timed(e, lambda: e.bmu_csr(csr), reps)
    r["bmu_csr"]["model_TBps"] = r["model_bytes"] / (r["bmu_csr"]["bmu_ms"] * 1e-3) / 1e12
    e.set_data_csr(csr)
    r["epoch"] = epoch(e, w)
    skew = np.full((K, D), -50.0, np.float32); skew[K // 2] = 0.0   # positive rows: unit K / 2 scores 0, every other unit more
    r["epoch_skewed"] = epoch(e, skew, reset=True)
    r["epoch_skewed"]["top_unit_share"] = float(np.bincount(e.epoch_fetch()[2], minlength=K).max() / N)
    if dense:
        e.set_weights(w)
        x = torch.zeros((N, D), dtype=torch.float32, device="cuda")
        rows = torch.from_numpy(np.repeat(np.arange(N), np.diff(csr[0]))).cuda()
        x[rows, torch.from_numpy(csr[1].astype(np.int64)).cuda()] = torch.from_numpy(csr[2]).cuda()
        torch.cuda.synchronize()
        dense_ids, r["bmu_dense_f32"] = timed(e, lambda: e.bmu_device(x.data_ptr(), N), reps)
        r["ids_differ_from_dense"] = int((dense_ids != ids).sum())
        r["sparse_over_dense_kernels"] = r["bmu_csr"]["bmu_ms"] / r["bmu_dense_f32"]["bmu_ms"]
        del x
    e.close()
    print(json.dumps(r), flush=True)
    return r


res = {"map": [X, Y], "rows": N, "reps": REPS,
       "method": "one process, 1 warm-up, median of reps, wall clock per call closed by som_sync; *_ms: the SOM_K_* event pairs per call",
       "cases": [one(8192, d, True) for d in (0.001, 0.01, 0.1)] + [one(50000, 0.01, False, max(3, REPS // 2))]}
# the density at which the two searches cross: log-linear between the measured densities on either side
c = res["cases"][:3]
res["crossover_density"] = None
for a, b in zip(c, c[1:]):
    ra, rb = a["sparse_over_dense_kernels"], b["sparse_over_dense_kernels"]
    if (ra - 1) * (rb - 1) <= 0 and ra != rb:
        t = (0 - np.log(ra)) / (np.log(rb) - np.log(ra))
        res["crossover_density"] = float(np.exp(np.log(a["density"]) + t * (np.log(b["density"]) - np.log(a["density"]))))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
with open(os.path.splitext(OUT)[0] + ".md", "w") as f:
    f.write("# Sparse rows beside the dense float32 search\n\n`tools/sparse_bench.py`: %d x %d map, %d rows, 1 warm-up, median of %d calls, one process; "
            "kernel times are event pairs on the stream.\n\n" % (X, Y, N, REPS))
    f.write("| input_len | density | nnz | sparse search ms | 4 nnz K model TB/s | dense f32 search ms | sparse / dense | som_bmu_csr wall ms | epoch: search | segment sum | transform | merge | skewed segment sum ms |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
    for r in res["cases"]:
        d = r.get("bmu_dense_f32")
        f.write("| %d | %g | %d | %.2f | %.2f | %s | %s | %.1f | %.2f | %.2f | %.2f | %.2f | %.2f |\n" % (
            r["input_len"], r["density"], r["nnz"], r["bmu_csr"]["bmu_ms"], r["bmu_csr"]["model_TBps"],
            "%.2f" % d["bmu_ms"] if d else "not attempted", "%.3f" % r["sparse_over_dense_kernels"] if d else "-", r["bmu_csr"]["ms"],
            r["epoch"]["bmu_ms"], r["epoch"]["segsum_ms"], r["epoch"]["kron_ms"], r["epoch"]["merge_ms"], r["epoch_skewed"]["segsum_ms"]))
    f.write("\nCrossover density (sparse search = dense float32 search, log-linear between the measured points): %s.\n" % (
        "%.3g" % res["crossover_density"] if res["crossover_density"] else "none inside the measured range"))
