"""Query fuzz: random maps, rows, distances and precisions through the checks of tests/test_gpu_query_ref.py (the float64
reference and bounds of tests/query_ref.py); prints the worst err/bound per call."""
import os
import sys
import time
import warnings

sys.path.insert(0, '.')
os.environ.setdefault("SOM_TEST_HOOKS", "1")
import numpy as np  # noqa: E402

from tests.test_gpu_query_ref import ALL_CALLS, _case, run_query_case  # noqa: E402

warnings.filterwarnings("ignore")
rs = np.random.RandomState(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
n_cases = int(sys.argv[2]) if len(sys.argv) > 2 else 100
bad = 0
worst = {}
t0 = time.time()
for case in range(n_cases):
    X, Y = int(rs.randint(1, 40)), int(rs.randint(1, 40))
    D = int(rs.choice([1, 3, 8, 9, 16, 17, 32, 33, 64, 65, 100, 128, 129, 265, 266, 300]))
    n = int(rs.choice([1, 2, 127, 128, 129, 255, 257, 1000]))
    prec = str(rs.choice(["f32", "exact", "bf16", "f16"]))
    dist = str(rs.choice(["euclidean", "euclidean", "euclidean_no_opt", "cosine", "manhattan", "norm_p", "norm_p_no_opt"]))
    if prec in ("bf16", "f16") and dist not in ("euclidean", "cosine"):
        prec = "f32"
    data = str(rs.choice(["blobs", "offset30", "offset300", "int"]))
    p, p_real = int(rs.choice([2, 3, 4, 16])), float(rs.choice([0.0, 0.0, 2.5]))
    env = {"SOM_F32_PARTS": str(rs.choice([1, 2, 256]))} if rs.rand() < 0.5 else {}
    if dist in ("manhattan", "norm_p", "norm_p_no_opt"):
        calls = ("bmu",)
    elif dist == "euclidean":
        calls = ALL_CALLS if prec in ("f32", "exact") else ("top2", "dist", "dist_q", "f64", "qe")
    else:
        calls = ("bmu", "dist") if prec == "f32" else ("dist",)
    c = _case(X, Y, D, n, prec=prec, dist=dist, data=data, calls=calls, env=env, p=p, p_real=p_real,
              dup=int(rs.choice([0, 0, min(3, X * Y - 1)])))
    os.environ.pop("SOM_F32_PARTS", None)
    os.environ.update(env)
    try:
        run_query_case(c, worst)
    except Exception as ex:                      # noqa: BLE001
        bad += 1
        print("FAIL case %d: %s: %s" % (case, c["id"], repr(ex)[:400]), flush=True)
print("worst err/bound: " + ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))
print(f"{n_cases} cases, {bad} failures, {time.time()-t0:.1f} s")
