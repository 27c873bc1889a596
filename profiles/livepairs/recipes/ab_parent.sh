#!/bin/bash
# A/B against the parent commit's library (bash tools/ab_prev_lib.sh <parent> first): the headline alternating
# parent / new three times, then (FULL=1) the full line once each way.  OUT: where the runs go.
# Every run under its own time limit, chained with &&: nothing is started after a fault, an abort or a time-out.
set -o pipefail
OUT=${OUT:-profiles/livepairs}
O=$OUT/ab
mkdir -p $O
P=$PWD/pycolmap_amd/csrc/_obj/libamc_prev.so
[ -f $P ] || { echo "no parent library"; exit 2; }
H="python bench.py --gpus 1 --steps 20 --warmup 5"
F="python bench.py --full --no-db --no-config3 --no-config4"
AMC_LIB_PATH=$P timeout -k 10 120 $H > $O/head_parent1.json 2> $O/head_parent1.err &&
timeout -k 10 120 $H > $O/head_new1.json 2> $O/head_new1.err &&
AMC_LIB_PATH=$P timeout -k 10 120 $H > $O/head_parent2.json 2> $O/head_parent2.err &&
timeout -k 10 120 $H > $O/head_new2.json 2> $O/head_new2.err &&
AMC_LIB_PATH=$P timeout -k 10 120 $H > $O/head_parent3.json 2> $O/head_parent3.err &&
timeout -k 10 120 $H > $O/head_new3.json 2> $O/head_new3.err &&
echo headline done
rc=$?
if [ $rc -eq 0 ] && [ -n "$FULL" ]; then
AMC_LIB_PATH=$P timeout -k 10 400 $F > $O/full_parent1.json 2> $O/full_parent1.err && echo f1 &&
timeout -k 10 400 $F > $O/full_new1.json 2> $O/full_new1.err && echo f2
rc=$?
fi
echo "ab rc=$rc"
python profiles/scan128/recipes/ab_summary.py $O $OUT/bench_ab_parent.json
exit $rc
