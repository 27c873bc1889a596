#!/bin/bash
# A/B against the parent commit's library (bash tools/ab_prev_lib.sh <parent> first), as profiles/livepairs/recipes/
# ab_parent.sh: the headline alternating parent / new three times, the full line once each way, then --dump-outputs
# from both libraries compared byte for byte.  OUT: where the runs go.
# Every run under its own time limit, chained with &&: nothing is started after a fault, an abort or a time-out.
set -o pipefail
OUT=${OUT:-profiles/chain}
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
echo headline done &&
AMC_LIB_PATH=$P timeout -k 10 400 $F > $O/full_parent1.json 2> $O/full_parent1.err && echo f1 &&
timeout -k 10 400 $F > $O/full_new1.json 2> $O/full_new1.err && echo f2 &&
AMC_LIB_PATH=$P timeout -k 10 120 python bench.py --gpus 1 --steps 2 --warmup 1 --dump-outputs $OUT/dump_parent > $OUT/dump_parent.json 2> $OUT/dump_parent.err &&
timeout -k 10 120 python bench.py --gpus 1 --steps 2 --warmup 1 --dump-outputs $OUT/dump_new > $OUT/dump_new.json 2> $OUT/dump_new.err &&
for f in $(ls $OUT/dump_parent); do cmp $OUT/dump_parent/$f $OUT/dump_new/$f && echo "cmp equal: $f $(stat -c %s $OUT/dump_new/$f) bytes"; done > $OUT/dump_cmp.txt 2>&1
rc=$?
echo "ab rc=$rc"
cat $OUT/dump_cmp.txt
rm -rf $OUT/dump_parent $OUT/dump_new $OUT/dump_parent.json $OUT/dump_new.json $OUT/dump_parent.err $OUT/dump_new.err
python profiles/scan128/recipes/ab_summary.py $O $OUT/bench_ab_parent.json
exit $rc
