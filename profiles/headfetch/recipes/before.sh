#!/bin/bash
# The parent alone, before anything is changed: stamps with the boundary split at four lengths (a stamped library of the
# parent with the split applied: libamc_stamps_prev.so; the parent library: bash tools/ab_prev_lib.sh <parent>), then the
# kernel trace of the short-image bench.  Every run under its own time limit; nothing is started after a failure.
set -o pipefail
R=$PWD
O=${OUT:-profiles/headfetch}/before
mkdir -p $O
L=$PWD/pycolmap_amd/csrc/_obj/libamc_stamps_prev.so
P=$PWD/pycolmap_amd/csrc/_obj/libamc_prev.so
for r in 512 1024 2048 4096; do
  timeout -k 10 120 python tools/scan_stamps.py --images 64 --rows $r --run 4 --lib $L > $O/stamps_parent_run4_$r.json 2> $O/stamps_parent_run4_$r.err || { echo "stamps $r failed rc=$?"; tail -5 $O/stamps_parent_run4_$r.err; exit 1; }
  cat $O/stamps_parent_run4_$r.json
done
timeout -k 10 120 python tools/scan_stamps.py --images 64 --rows 512 --run 1 --lib $L > $O/stamps_parent_run1_512.json 2> $O/stamps_parent_run1_512.err || { echo "stamps run1 failed"; exit 1; }
cat $O/stamps_parent_run1_512.json
cd $O && AMC_LIB_PATH=$P timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d rocprof_parent -o parent -- python $R/bench.py --gpus 1 --images 2000 --feats 512 --steps 3 --warmup 1 > bench_parent_trace.json 2> bench_parent_trace.err || { echo "trace failed rc=$?"; tail -5 bench_parent_trace.err; exit 1; }
cat bench_parent_trace.json | cut -c1-1500
f=$(find rocprof_parent -name '*kernel_stats.csv' | head -1); head -8 $f
find rocprof_parent -type f ! -name '*kernel_stats.csv' -delete
