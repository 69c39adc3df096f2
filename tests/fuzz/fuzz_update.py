"""Update-path fuzz: teacher-forced accumulates + merges of the C ABI against the direct-form float64 reference
(tests/update_ref.py) on random configurations -- map sides 1..320, D from the layout list (narrow tiles, per-column
stage 2, 16 / 8 / 4 waves of the segment sum), every neighbourhood family, std_coeff, sigma on and one ulp off the
lattice, the neighbourhood's dtype, the BMU pattern and the row count.  The checks are the GPU module's
(tests/test_gpu_update_ref.py): elementwise accumulators, the merge bit for bit and against the reference,
repeatability, staged == monolithic."""
import sys, time, warnings
import numpy as np
sys.path.insert(0, '.')
from tests.update_ref import random_case, run_forced_case

warnings.filterwarnings("ignore")
seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
rs = np.random.RandomState(seed)
n_cases = int(sys.argv[2]) if len(sys.argv) > 2 else 100
bad = 0
worst = {}
t0 = time.time()
for case in range(n_cases):
    c = random_case(rs, seed * 100003 + case, max_entries=1e7, max_flops=1e10)
    try:
        r = run_forced_case(c)
        w = worst.setdefault(c["family"], 0.0)
        worst[c["family"]] = max(w, r["accum"], r["merge"])
    except Exception as ex:                      # noqa: BLE001
        bad += 1
        print("FAIL case %d: %s std=%s eta=%s scale=%s: %s" % (case, c["id"], c["std"], c["eta"], c["scale"], repr(ex)[:400]),
              flush=True)
for fam in sorted(worst):
    print("worst err/bound %-26s %.3g" % (fam, worst[fam]))
print(f"{n_cases} cases, {bad} failures, {time.time()-t0:.1f} s")
