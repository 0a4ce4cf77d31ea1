#!/bin/bash
# Final evidence of the round for the committed tree: kernel stats (2D / 3D) and the two bench lines.
R=$GRAFT_REPO_ROOT; cd $R
bash tools/lab/collect_r03.sh stats > gpurun_out/collect_stats.log 2>&1; tail -3 gpurun_out/collect_stats.log
O=${BENCH_OUT:-/tmp/r3_finalize}; mkdir -p $O
python3 bench.py --full > $O/r3_bench_final4.json 2> $O/r3_bench_final4.err
python3 bench.py --full --config 3d --steps 20 --warmup 5 > $O/r3_bench3d_final4.json 2> $O/r3_bench3d_final4.err
python3 - $O/r3_bench_final4.json $O/r3_bench3d_final4.json <<'P'
import json, sys
for f in sys.argv[1:]:
    d = json.load(open(f)); print(f, d["ms_per_step"], d["value"], d["roofline"]["frac"], d["roofline"]["top_kernel"]["frac"], [(e["dtype"], e["ms_per_step"]) for e in d.get("extra_configs", [])])
P
