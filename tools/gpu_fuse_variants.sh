#!/bin/bash
# Runs ON THE GPU BOX: the fused MCMC step's kernel time for measurement builds (build_dbg/lib_<name>.so)
export TMPDIR=/tmp
for n in "$@"; do
  export NMMA_HIP_LIB=$PWD/build_dbg/lib_$n.so
  o=prof_out/prof_fuse_$n
  rm -rf $o; mkdir -p $o
  rocprofv3 --kernel-trace --stats --output-format csv -d $o -- python3 bench.py --full --steps 5 --warmup 2 --repeats 3 --cpu-seconds 0.5 --sustained-seconds 0 > $o.log 2>&1
  f=$(find $o -name "*kernel_stats.csv" | head -1)
  python3 - <<PY
import csv
for r in csv.DictReader(open("$f")):
    n = r["Name"]
    if "em_logl" in n and n.split(">")[0].rstrip().endswith(", 8"):
        print("$n".ljust(10), n[:50], r["Calls"], "avg", r["AverageNs"], "min", r["MinNs"])
PY
done
