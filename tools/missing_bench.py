"""What the missing-value mode (`missing='nan'`) costs, kernel family by kernel family, and what the unmasked float32 search takes
beside it.  One process; every handle holds the same rows (the benchmark's blobs; the masked handles once complete and once with
30 % of the values missing) and starts from the same seeded codebook.  After MB_WARM warm-up epochs per handle the handles take
turns, MB_ROUNDS rounds of MB_EPOCHS `som_epoch` calls each with `som_profile_enable(1)` (hipEvent pairs around every kernel
family): per handle and family the median over the rounds of the time per epoch, with the rounds' minimum and maximum.

    shapes     64 x 64 x 32 with 100 000 rows; 256 x 256 x 128 with 65 536 rows (MB_SHAPES="X,Y,D,N;...")
    handles    f32            precision 'f32', no missing values: the search the masked kernel is compared with
               masked         missing='nan', complete rows
               masked_holes   missing='nan', 30 % of the values NaN
    ratios     SOM_K_BMU of the masked handles over the f32 handle's (MB_PARENT_JSON: also over the figure a run of this tool
               with MB_F32_ONLY=1 took in another tree, e.g. the parent commit's); SOM_K_SEGSUM / KRON / MERGE likewise

MB_F32_ONLY=1 measures the f32 handle alone and uses nothing the mode added; MB_TREE names the tree whose package to import
(default: this file's).  Writes one JSON document (MB_OUT, default profiles/missing_values.json) and prints a table.
    python tools/missing_bench.py"""
import json, os, statistics, sys, numpy as np
TREE = os.environ.get("MB_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TREE)
from xpysom_dask_amd.engine import HipEngine
from xpysom_dask_amd.synthetic import gaussian_blobs

SHAPES = [tuple(int(v) for v in s.split(",")) for s in os.environ.get("MB_SHAPES", "64,64,32,100000;256,256,128,65536").split(";")]
WARM, ROUNDS, EPOCHS = (int(os.environ.get(k, d)) for k, d in (("MB_WARM", "3"), ("MB_ROUNDS", "7"), ("MB_EPOCHS", "4")))
F32_ONLY = os.environ.get("MB_F32_ONLY") == "1"
OUT = os.environ.get("MB_OUT", os.path.join(TREE, "profiles", "missing_values_f32_only.json" if F32_ONLY else "missing_values.json"))
FAMILIES = ("bmu", "segsum", "kron", "merge")
SIGMA, ETA = 2.0, 0.5

res = {"method": "%d warm-up epochs, then %d rounds of %d som_epoch calls per handle in turn; hipEvent time per family and epoch; "
                 "median (min, max) over the rounds; sigma %.1f, eta %.1f" % (WARM, ROUNDS, EPOCHS, SIGMA, ETA), "shapes": {}}
parent = json.load(open(os.environ["MB_PARENT_JSON"])) if os.environ.get("MB_PARENT_JSON") else None
for X, Y, D, N in SHAPES:
    name = "%dx%dx%d_n%d" % (X, Y, D, N)
    data = gaussian_blobs(N, D, seed=1234, centre_seed=1234)
    holes = data.copy()
    holes[np.random.RandomState(1).rand(N, D) < 0.3] = np.nan
    rs = np.random.RandomState(1234)
    w = rs.rand(X, Y, D) * 2 - 1
    w = (w / np.linalg.norm(w, axis=-1, keepdims=True)).astype(np.float32)
    handles = {"f32": (HipEngine(X, Y, D, precision="f32"), data)}
    if not F32_ONLY:
        handles["masked"] = (HipEngine(X, Y, D, precision="f32", missing="nan"), data)
        handles["masked_holes"] = (HipEngine(X, Y, D, precision="f32", missing="nan"), holes)
    for e, rows in handles.values():
        e.set_weights(w)
        e.set_data(rows)
        for _ in range(WARM):
            e.epoch(SIGMA, ETA, True)
        e.sync()
    per = {h: {k: [] for k in FAMILIES} for h in handles}
    for _ in range(ROUNDS):
        for h, (e, _) in handles.items():
            e.set_weights(w)
            e.profile_reset()
            e.profile_enable(True)
            for _ in range(EPOCHS):
                e.epoch(SIGMA, ETA, True)
            e.sync()
            e.profile_enable(False)
            for k in FAMILIES:
                per[h][k].append(e.profile_get(k)[0] / EPOCHS)
    block = {h: {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in fam.items()} for h, fam in per.items()}
    if not F32_ONLY:
        codebooks = {h: e.get_weights() for h, (e, _) in handles.items()}
        block["masked_codebook_finite"] = bool(np.isfinite(codebooks["masked"]).all() and np.isfinite(codebooks["masked_holes"]).all())
        block["ratio_over_f32"] = {h: {k: block[h][k]["median_ms"] / block["f32"][k]["median_ms"] for k in FAMILIES} for h in ("masked", "masked_holes")}
        if parent is not None and name in parent["shapes"]:
            pf = parent["shapes"][name]["f32"]["bmu"]
            block["other_tree_f32_bmu"] = pf
            block["bmu_ratio_over_other_tree_f32"] = {h: block[h]["bmu"]["median_ms"] / pf["median_ms"] for h in ("masked", "masked_holes")}
    for e, _ in handles.values():
        e.close()
    res["shapes"][name] = block
    for h in handles:
        print("%-18s %-13s " % (name, h) + "  ".join("%s %.4f (%.4f - %.4f)" % (k, block[h][k]["median_ms"], block[h][k]["min_ms"], block[h][k]["max_ms"])
                                                     for k in FAMILIES), flush=True)
    if not F32_ONLY:
        for h in ("masked", "masked_holes"):
            print("%-18s %-13s over f32: " % (name, h) + "  ".join("%s x %.2f" % (k, block["ratio_over_f32"][h][k]) for k in FAMILIES) +
                  ("  | bmu over the other tree's f32: x %.2f" % block["bmu_ratio_over_other_tree_f32"][h] if "other_tree_f32_bmu" in block else ""), flush=True)
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
