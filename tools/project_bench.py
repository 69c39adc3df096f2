"""The label and value maps on rows that live in HBM: som_unit_label_counts_device (16 classes) and som_unit_value_sums_device (1
and 16 columns) next to their floor, som_bmu_device on the same rows -- the search itself, which every one of them runs first --
and next to what they replace, XPySom.labels_map on the same rows as a host array (unchanged code: one BMU call in n_parallel
chunks, one host argsort, a Counter per unit).  The PB_ROWS device-resident rows the 256 x 256 x 128 map was trained on (the
benchmark's blobs), precision 'exact', after the benchmark's 25-epoch schedule.  One process, 1 warm-up call, then the median of
PB_REPS calls each (wall clock per call, including the results' copy to the host), with the time the calls' kernel families spent
on the stream (som_profile_*: `bmu` the search, `segsum` the sort by unit + heads + the per-unit pass, `prep` the operands).
Writes a JSON document (PB_OUT, default profiles/unit_labels.json) and a summary (PB_MD, default profiles/unit_labels.md).
    PB_ROWS=1048576 PB_REPS=11 python tools/project_bench.py"""
import json, os, statistics, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xpysom_dask_amd import XPySom
from xpysom_dask_amd.decays import exponential_decay
from xpysom_dask_amd.engine import HipEngine
from xpysom_dask_amd.synthetic import gaussian_blobs

X = Y = 256; D = 128; CLASSES = 16
N = int(os.environ.get("PB_ROWS", str(1 << 20))); T = int(os.environ.get("PB_EPOCHS", "25"))
REPS = max(3, int(os.environ.get("PB_REPS", "11")))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("PB_OUT", os.path.join(ROOT, "profiles", "unit_labels.json"))
MD = os.environ.get("PB_MD", os.path.splitext(OUT)[0] + ".md")
data = gaussian_blobs(N, D, seed=1234, centre_seed=1234)
rs = np.random.RandomState(1234)
w = rs.rand(X, Y, D) * 2 - 1; w /= np.linalg.norm(w, axis=-1, keepdims=True)
labels = rs.randint(0, CLASSES, N).astype(np.int32)
values = rs.normal(0, 1, (N, CLASSES)).astype(np.float32)
dev = torch.from_numpy(data).cuda()                                  # the benchmark's own rows
dl, dv16, dv1 = torch.from_numpy(labels).cuda(), torch.from_numpy(values).cuda(), torch.from_numpy(np.ascontiguousarray(values[:, :1])).cuda()
torch.cuda.synchronize()
e = HipEngine(X, Y, D, precision="exact"); e.set_data_device(dev.data_ptr(), N, keepalive=dev); e.set_weights(w.astype(np.float32))
for t in range(T):
    e.epoch(exponential_decay(128, 1, t, T), exponential_decay(0.5, 0.01, t, T), True)
e.sync()
trained = e.get_weights().reshape(X, Y, D)


def timed(fn, sync, profile=None):
    fn(); sync()                                                    # warm-up: allocations, operand images
    if profile:
        profile.profile_reset(); profile.profile_enable(True)
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter(); out = fn(); sync(); ts.append(1e3 * (time.perf_counter() - t0))
    r = {"median_ms": statistics.median(ts), "min_ms": min(ts)}
    if profile:
        profile.profile_enable(False)
        r["stream_ms"] = {k: profile.profile_get(k)[0] / REPS for k in ("bmu", "screen", "segsum", "prep")}
    return out, r


ptr = dev.data_ptr()
res = {"map": [X, Y, D], "rows": N, "epochs": T, "reps": REPS, "precision": "exact", "classes": CLASSES,
       "method": "1 warm-up, median of reps, wall clock per call incl. the results' copy to the host; one process"}
DEVICE = ("predict (som_bmu_device)", "label_counts_device, 16 classes", "value_sums_device, 1 column", "value_sums_device, 16 columns")
ids, res[DEVICE[0]] = timed(lambda: e.bmu_device(ptr, N), e.sync, e)
counts, res[DEVICE[1]] = timed(lambda: e.label_counts_device(ptr, dl.data_ptr(), N, CLASSES), e.sync, e)
one, res[DEVICE[2]] = timed(lambda: e.value_sums_device(ptr, dv1.data_ptr(), N, 1), e.sync, e)
wide, res[DEVICE[3]] = timed(lambda: e.value_sums_device(ptr, dv16.data_ptr(), N, CLASSES), e.sync, e)
e.close()
# the calls describe the same rows
hits = np.bincount(ids, minlength=X * Y)
res["counts_equal_bincount"] = bool(np.array_equal(counts, np.bincount(ids.astype(np.int64) * CLASSES + labels, minlength=X * Y * CLASSES).reshape(X * Y, CLASSES))
                                    and np.array_equal(one[0][:, 0], hits) and np.array_equal(wide[0], np.repeat(hits[:, None], CLASSES, axis=1)))
res["first_column_same_bits"] = bool(np.array_equal(one[1][:, 0], wide[1][:, 0]) and np.array_equal(one[2][:, 0], wide[2][:, 0]))
res["units_hit"] = int((hits > 0).sum()); res["largest_unit_rows"] = int(hits.max())
# what they replace: labels_map on the same rows as a host array
som = XPySom(X, Y, D, precision="exact"); som._weights = trained
lm, res["labels_map, host rows"] = timed(lambda: som.labels_map(data, labels), lambda: None)
res["labels_map_agrees"] = bool(all(counts[i * Y + j, c] == m for (i, j), ctr in lm.items() for c, m in ctr.items())
                                and sum(sum(ctr.values()) for ctr in lm.values()) == N)
floor = res[DEVICE[0]]["median_ms"]
for k in DEVICE:
    r = res[k]
    r["over_predict_ms"] = r["median_ms"] - floor
    r["search_share_of_stream"] = r["stream_ms"]["bmu"] / max(1e-9, r["stream_ms"]["bmu"] + r["stream_ms"]["segsum"] + r["stream_ms"]["prep"])
    print("%-36s %.3f ms (min %.3f; on the stream: bmu %.3f, of it the screen %.3f, segsum %.3f, prep %.3f)"
          % (k, r["median_ms"], r["min_ms"], r["stream_ms"]["bmu"], r["stream_ms"]["screen"], r["stream_ms"]["segsum"], r["stream_ms"]["prep"]), flush=True)
r = res["labels_map, host rows"]
print("%-36s %.1f ms (min %.1f)" % ("labels_map, host rows", r["median_ms"], r["min_ms"]))
print("counts equal bincount: %s | column 0 alone and among 16: same bits: %s | labels_map agrees: %s"
      % (res["counts_equal_bincount"], res["first_column_same_bits"], res["labels_map_agrees"]), flush=True)
assert res["counts_equal_bincount"] and res["labels_map_agrees"]
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
with open(MD, "w") as f:
    f.write("# Label and value maps on device rows: timings\n\n")
    f.write("`tools/project_bench.py`: %d x %d x %d map, precision `exact`, after the benchmark's %d-epoch schedule, on the %d device rows it\n"
            "trained on; %d random class codes, standard-normal values.  One process, 1 warm-up call, then the median of %d calls; wall\n"
            "clock per call including the results' copy to the host.  `predict` is the search every other call runs first: the floor.\n"
            "`labels_map` is unchanged code, on the same rows as a host array (its own upload in `n_parallel` chunks included).\n\n"
            % (X, Y, D, T, N, CLASSES, REPS))
    f.write("| call | median ms | min ms | over predict | stream: bmu | of it screen | stream: segsum (sort + heads + per-unit pass) | search's share of the stream time |\n"
            "|---|---|---|---|---|---|---|---|\n")
    for k in DEVICE:
        r = res[k]
        f.write("| `%s` | %.3f | %.3f | %+.3f | %.3f | %.3f | %.3f | %.0f %% |\n" % (
            k, r["median_ms"], r["min_ms"], r["over_predict_ms"], r["stream_ms"]["bmu"], r["stream_ms"]["screen"], r["stream_ms"]["segsum"],
            100 * r["search_share_of_stream"]))
    r = res["labels_map, host rows"]
    f.write("| `labels_map`, host rows | %.1f | %.1f | | | | | |\n" % (r["median_ms"], r["min_ms"]))
    f.write("\n- The calls agree: the label counts and the value counts equal `bincount` of `predict`'s ids (%s); column 0 summed alone and\n"
            "  among 16 columns differs in lane layout, so its sums need not share bits (same bits in this run: %s); `labels_map`'s Counters equal the\n"
            "  label counts entry for entry (%s).  %d of %d units win rows, the largest %d.\n"
            % (res["counts_equal_bincount"], res["first_column_same_bits"], res["labels_map_agrees"], res["units_hit"], X * Y, res["largest_unit_rows"]))
    f.write("- `predict` copies %d MB of ids to the host; `label_counts` %d MB of counts, `unit_means` with 16 columns %d MB into three fresh\n"
            "  pageable arrays: what a call costs over `predict` beyond its `segsum` time on the stream is that copy.\n"
            % (4 * N >> 20, 8 * X * Y * CLASSES >> 20, 24 * X * Y * CLASSES >> 20))
