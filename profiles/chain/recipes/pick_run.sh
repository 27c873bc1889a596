#!/bin/bash
# The run length: the headline alternating parent / AMC_SCAN_RUN = 1 (off) / 2 / 4 / 8, twice, in one call
# (bash tools/ab_prev_lib.sh <parent> first).  OUT: where the runs go.  Stops at the first run that fails.
set -o pipefail
O=${OUT:-profiles/chain}/pick
mkdir -p $O
P=$PWD/pycolmap_amd/csrc/_obj/libamc_prev.so
[ -f $P ] || { echo "no parent library"; exit 2; }
H="python bench.py --gpus 1 --steps 20 --warmup 5"
for i in 1 2; do
  AMC_LIB_PATH=$P timeout -k 10 150 $H > $O/head_parent$i.json 2> $O/head_parent$i.err || { echo "parent$i failed rc=$?"; exit 1; }
  for r in 1 2 4 8; do
    AMC_SCAN_RUN=$r timeout -k 10 150 $H > $O/head_run${r}_$i.json 2> $O/head_run${r}_$i.err || { echo "run$r $i failed rc=$?"; exit 1; }
  done
done
python profiles/chain/recipes/pick_summary.py $O
