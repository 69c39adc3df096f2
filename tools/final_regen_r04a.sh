#!/bin/bash
# round 4, first call: the PMC summaries of the c3 launches on THIS build (copied into profiles/ on the box so that the bench
# lines that follow cite a summary of their own build), then the c3 / c2 bench lines (the driver's own flags for c3)
set -e
TAG=r04
tools/pmc_all.sh $TAG 1048576 > gpurun_out/${TAG}_pmc_c3.log 2>&1
tools/pmc_all.sh $TAG 65536 > gpurun_out/${TAG}_pmc_b64k.log 2>&1
cp gpurun_out/${TAG}_pmc_traffic_rows1048576.json gpurun_out/${TAG}_pmc_traffic_rows65536.json profiles/
cp gpurun_out/${TAG}_kernel_stats_rows1048576.csv gpurun_out/${TAG}_kernel_stats_rows65536.csv profiles/
cp gpurun_out/${TAG}_dispatches_rows1048576.csv gpurun_out/${TAG}_dispatches_rows65536.csv profiles/
python3 bench.py --full --steps 20 --warmup 5 > profiles/${TAG}_bench_c3.json
python3 bench.py --full --workload c2 > profiles/${TAG}_bench_c2.json
for w in c3 c2; do python3 - <<PY
import json
d = json.loads(open("profiles/${TAG}_bench_$w.json").read().strip().splitlines()[-1])
r = d["roofline"]
print("$w", round(d["ms_per_step"], 3), "ms", round(d["value"] / 1e6, 2), "M/s frac", round(r["frac"], 4), "traffic", r.get("traffic"), (r.get("traffic_source") or {}).get("same_build"), (r.get("batch65536") or {}).get("epoch_ms"))
PY
done
