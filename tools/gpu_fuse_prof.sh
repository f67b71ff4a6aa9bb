#!/bin/bash
# Runs ON THE GPU BOX: kernel times of the sampler queue (fused MCMC step vs likelihood + walk_step) by rocprofv3
# Usage: tools/gpu_fuse_prof.sh [output directory, wiped first; default prof_out/prof_fuse]
export TMPDIR=/tmp
o=${1:-prof_out/prof_fuse}
rm -rf $o; mkdir -p $o
rocprofv3 --kernel-trace --stats --output-format csv -d $o/a -- python3 bench.py --full --steps 5 --warmup 2 --repeats 3 --cpu-seconds 0.5 --sustained-seconds 0 > $o/a.log 2>&1
f=$(find $o/a -name "*kernel_stats.csv" | head -1)
python3 - <<PY
import csv
for r in csv.DictReader(open("$f")):
    n = r["Name"]
    if "em_logl" in n or "walk" in n:
        print(n[:90].ljust(92), r["Calls"], r["AverageNs"], r["MinNs"])
PY
