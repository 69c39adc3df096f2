"""16-bit BMU fuzz: random maps, rows, precisions, distances, data kinds and part counts through the checks of
tests/test_gpu_half_ref.py (the float64 reference on rounded operands and the bounds of tests/half_ref.py), query and
resident path each; prints the worst err/bound per kernel family."""
import os
import sys
import time
import warnings

sys.path.insert(0, '.')
os.environ.setdefault("SOM_TEST_HOOKS", "1")
import numpy as np  # noqa: E402

from tests.test_gpu_half_ref import _case, run_half_case  # noqa: E402

warnings.filterwarnings("ignore")
rs = np.random.RandomState(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
n_cases = int(sys.argv[2]) if len(sys.argv) > 2 else 60
bad = 0
worst = {}
t0 = time.time()
for case in range(n_cases):
    big = rs.rand() < 0.3
    X, Y = (int(rs.randint(60, 70)), int(rs.randint(64, 70))) if big else (int(rs.randint(1, 40)), int(rs.randint(1, 40)))
    D = int(rs.choice([1, 3, 8, 9, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 257, 300, 512, 777, 800, 801, 900]))
    n = int(rs.choice([1, 2, 127, 128, 129, 255, 256, 257, 700]))
    prec = str(rs.choice(["bf16", "f16"]))
    dist = str(rs.choice(["euclidean", "euclidean", "cosine"]))
    data = str(rs.choice(["blobs", "offset30", "offset300", "int", "tiny", "huge"]))
    if dist == "cosine" or (data == "huge" and prec != "f16"):
        data = "blobs"
    env = {}
    if rs.rand() < 0.5:
        env["SOM_BF16_PARTS"] = str(rs.choice([1, 2, 3, 7, 64]))
    if rs.rand() < 0.25:
        env["SOM_BF16_WIDE"] = "0"
    c = _case(X, Y, D, n, prec, dist, data, env=env, dup=int(rs.choice([0, 0, min(5, X * Y - 1)])))
    try:
        run_half_case(c, worst)
    except Exception as ex:                      # noqa: BLE001
        bad += 1
        print("FAIL case %d: %s: %s" % (case, c["id"], repr(ex)[:400]), flush=True)
for fam in sorted(worst):
    print("worst err/bound %s: %s" % (fam, ", ".join("%s %.3g" % kv for kv in sorted(worst[fam].items()))))
print(f"{n_cases} cases, {bad} failures, {time.time()-t0:.1f} s")
