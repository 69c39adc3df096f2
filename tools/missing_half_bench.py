"""What the 16-bit masked search (`missing='nan', missing_search='bf16' | 'f16'`; csrc/bmu_masked_half.hpp) takes beside the float32
masked search, on the same handle, rows and codebook, and how often the two name the same unit.

Method (tools/missing_bench.py's): one process per shape, started here with a time limit of its own (MH_LIMIT seconds; a shape
that fails or runs out of time ends the tool).  Per shape two masked handles hold the benchmark's blobs, once complete and once
with 30 % of the values NaN, and one unmasked precision='f16' handle holds the complete rows; all start from the same seeded
codebook.  After MH_WARM warm-up epochs per (handle, search) the searches take turns -- set_missing_search between rounds --,
MH_ROUNDS rounds of MH_EPOCHS `som_epoch` calls each under som_profile_enable(1) (hipEvent pairs per kernel family): the median
over the rounds of SOM_K_BMU per epoch, with minimum and maximum, and of SOM_K_PREP (the 16-bit searches' image kernel).
Agreement: the share of the first MH_AGREE rows whose pick equals the float32 masked pick, on the seeded codebook and on the
codebook the float32-search schedule leaves.  Model: 3 * 2 N K D flop on the 16-bit pipe per search.

    shapes   256 x 256 x 128 with 65 536 and 1 048 576 rows, 64 x 64 x 32 with 100 000 rows (MH_SHAPES="X,Y,D,N;...")
    gate     float32 masked SOM_K_BMU over the 16-bit searches' at 256 x 256 x 128: accepted at >= 4

Writes profiles/missing_half.json and profiles/missing_half.md (MH_OUT: another stem).
    python tools/missing_half_bench.py"""
import json, os, statistics, subprocess, sys, numpy as np
TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TREE)

SHAPES = os.environ.get("MH_SHAPES", "64,64,32,100000;256,256,128,65536;256,256,128,1048576").split(";")
WARM, ROUNDS, EPOCHS, AGREE, LIMIT = (int(os.environ.get(k, d)) for k, d in (
    ("MH_WARM", "2"), ("MH_ROUNDS", "5"), ("MH_EPOCHS", "3"), ("MH_AGREE", "65536"), ("MH_LIMIT", "420")))
OUT = os.environ.get("MH_OUT", os.path.join(TREE, "profiles", "missing_half"))
SEARCHES = ("f32", "bf16", "f16")
SIGMA, ETA, GATE = 2.0, 0.5, 4.0
# the compiler's resource report of the new instances (hipcc -O3, gfx950): VGPRs, AGPRs, scratch bytes, static + dynamic LDS bytes
REGISTERS = [("bmu_masked_half_kernel<1>", 90, 0, 0, 24576), ("bmu_masked_half_kernel<2>", 160, 0, 0, 49152),
             ("bmu_masked_half_kernel<3>", 226, 0, 0, 73728), ("bmu_masked_half_kernel<4>", 256, 68, 0, 98304),
             ("bmu_masked_half_stream_kernel", 218, 0, 0, 24576), ("prep_masked_half_kernel", 28, 0, 0, 0)]


def stat(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def run_shape(spec):
    from xpysom_dask_amd.engine import HipEngine
    from xpysom_dask_amd.synthetic import gaussian_blobs
    X, Y, D, N = (int(v) for v in spec.split(","))
    data = gaussian_blobs(N, D, seed=1234, centre_seed=1234)
    holes = data.copy()
    holes[np.random.RandomState(1).rand(N, D) < 0.3] = np.nan
    rs = np.random.RandomState(1234)
    w = rs.rand(X, Y, D) * 2 - 1
    w = (w / np.linalg.norm(w, axis=-1, keepdims=True)).astype(np.float32)
    handles = {"complete": (HipEngine(X, Y, D, precision="f32", missing="nan"), data, SEARCHES),
               "holes30": (HipEngine(X, Y, D, precision="f32", missing="nan"), holes, SEARCHES),
               "unmasked_f16": (HipEngine(X, Y, D, precision="f16"), data, (None,))}
    del holes

    def epochs(e, ms, n, timed):
        if ms is not None:
            e.set_missing_search(ms)
        e.set_weights(w)
        if timed:
            e.profile_reset()
            e.profile_enable(True)
        for _ in range(n):
            e.epoch(SIGMA, ETA, True)
        e.sync()
        if timed:
            e.profile_enable(False)
            return tuple(e.profile_get(k)[0] / n for k in ("bmu", "prep"))

    for e, rows, searches in handles.values():
        e.set_weights(w)
        e.set_data(rows)
        for ms in searches:
            epochs(e, ms, WARM, False)
    per = {h: {ms: ([], []) for ms in s} for h, (_, _, s) in handles.items()}
    for _ in range(ROUNDS):
        for h, (e, _, searches) in handles.items():
            for ms in searches:
                b, p = epochs(e, ms, EPOCHS, True)
                per[h][ms][0].append(b)
                per[h][ms][1].append(p)
    block = {h: {str(ms): {"bmu": stat(v[0]), "prep": stat(v[1])} for ms, v in d.items()} for h, d in per.items()}
    for h in ("complete", "holes30"):
        e, rows, _ = handles[h]
        t = {ms: block[h][ms]["bmu"]["median_ms"] for ms in SEARCHES}
        block[h]["f32_over"] = {ms: t["f32"] / t[ms] for ms in ("bf16", "f16")}
        block[h]["tflops_16bit"] = {ms: 6.0 * N * X * Y * D / (t[ms] * 1e9) for ms in ("bf16", "f16")}
        epochs(e, "f32", EPOCHS, False)
        trained, q = e.get_weights(), rows[:AGREE]
        share = {}
        for name, cb in (("seeded", w), ("trained", trained)):
            e.set_weights(cb)
            ids = {}
            for ms in SEARCHES:
                e.set_missing_search(ms)
                ids[ms] = e.bmu(q)
            share[name] = {ms: float((ids[ms] == ids["f32"]).mean()) for ms in ("bf16", "f16")}
        block[h]["same_pick_as_f32"] = share
    for e, _, _ in handles.values():
        e.close()
    return block


def markdown(res):
    out = ["# 16-bit masked BMU search (`missing_search`)", "", res["method"], "",
           "SOM_K_BMU per epoch, ms: median (min - max) over the rounds; `x f32`: the float32 masked search's median over this one's.", ""]
    for name, b in res["shapes"].items():
        out += ["## %s" % name, "", "| rows | search | SOM_K_BMU ms | SOM_K_PREP ms | x f32 | TFLOP/s (3 * 2 N K D) | same pick: seeded | trained |", "|---|---|---|---|---|---|---|---|"]
        for h in ("complete", "holes30"):
            for ms in SEARCHES:
                s, p = b[h][ms]["bmu"], b[h][ms]["prep"]["median_ms"]
                extra = "| 1 | | | |" if ms == "f32" else "| %.2f | %.0f | %.4f | %.4f |" % (
                    b[h]["f32_over"][ms], b[h]["tflops_16bit"][ms], b[h]["same_pick_as_f32"]["seeded"][ms], b[h]["same_pick_as_f32"]["trained"][ms])
                out.append("| %s | %s | %.3f (%.3f - %.3f) | %.4f %s" % (h, ms, s["median_ms"], s["min_ms"], s["max_ms"], p, extra))
        s = b["unmasked_f16"]["None"]["bmu"]
        out += ["| complete | unmasked precision='f16' | %.3f (%.3f - %.3f) | | | | | |" % (s["median_ms"], s["min_ms"], s["max_ms"]), ""]
    gated = [(n, h, ms, b[h]["f32_over"][ms]) for n, b in res["shapes"].items() if n.startswith("256x256x128") for h in ("complete", "holes30") for ms in ("bf16", "f16")]
    if gated:
        worst = min(gated, key=lambda g: g[3])
        out += ["## Gate", "", "Accepted at a ratio of %.0f or more at 256 x 256 x 128.  Smallest measured: x %.2f (%s, %s, %s): %s." % (
            GATE, worst[3], worst[0], worst[1], worst[2], "met" if worst[3] >= GATE else "MISSED"), ""]
    out += ["## Registers", "", "| kernel (both operand types) | VGPRs | AGPRs | scratch bytes | LDS bytes |", "|---|---|---|---|---|"]
    out += ["| %s | %d | %d | %d | %d |" % r for r in REGISTERS]
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        print(json.dumps(run_shape(sys.argv[2])))
        sys.exit(0)
    res = {"method": "%d warm-up epochs per (handle, search), then %d rounds of %d som_epoch calls per (handle, search) in turn; hipEvent time per "
                     "family and epoch; median (min, max) over the rounds; sigma %.1f, eta %.1f; agreement on the first %d rows"
                     % (WARM, ROUNDS, EPOCHS, SIGMA, ETA, AGREE), "shapes": {}}
    for spec in SHAPES:
        X, Y, D, N = spec.split(",")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", spec], capture_output=True, text=True, timeout=LIMIT)
        if p.returncode != 0:
            sys.exit("shape %s failed (exit %d): %s" % (spec, p.returncode, p.stderr[-2000:]))
        res["shapes"]["%sx%sx%s_n%s" % (X, Y, D, N)] = json.loads(p.stdout.strip().splitlines()[-1])
        print(spec, "done", flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT + ".json", "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    with open(OUT + ".md", "w") as f:
        f.write(markdown(res))
    print(markdown(res))
