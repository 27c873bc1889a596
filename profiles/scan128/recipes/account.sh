#!/bin/bash
# The account of an item's clocks: (1) the unit rungs of the ladder on the benchmark's bytes (LADDER_DATA=7) and on the
# SIFT-like bytes already on file, (2) the stamped diagnostic build on 8 images x 4096 rows (grid capped, so that
# workgroups scan several items) and on 64 images at the full grid, (3) one counters-only pass of the headline with a
# kernel filter on the scan and one of the ladder's unit rungs on the benchmark's bytes.
# Before: hipcc --offload-arch=gfx950 -O3 -o tools/bin/ubench_ladder tools/ubench_ladder.hip; bash tools/scan_stamps_build.sh
set -o pipefail
O=${OUT:-profiles/scan128}
mkdir -p $O
L=tools/bin/ubench_ladder
SQ="SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_I8 GRBM_GUI_ACTIVE"
: > $O/ladder_units_bench_bytes.txt
LADDER_UNITS=1 LADDER_DATA=7 timeout -k 10 120 $L >> $O/ladder_units_bench_bytes.txt 2>&1 &&
LADDER_UNITS=1 LADDER_DATA=1 timeout -k 10 120 $L >> $O/ladder_units_bench_bytes.txt 2>&1 &&
LADDER_UNITS=1 LADDER_DATA=7 timeout -k 10 120 $L >> $O/ladder_units_bench_bytes.txt 2>&1 &&
grep -E "data mode|64-row|128-row" $O/ladder_units_bench_bytes.txt &&
timeout -k 10 180 python tools/scan_stamps.py --images 8 --rows 4096 --grid 14 > $O/stamps_8x4096_grid14.json 2> $O/stamps_8.err && cat $O/stamps_8x4096_grid14.json &&
timeout -k 10 180 python tools/scan_stamps.py --images 64 --rows 4096 > $O/stamps_64x4096.json 2> $O/stamps_64.err && cat $O/stamps_64x4096.json &&
{ timeout -k 10 60 rocprofv3 -L 2>/dev/null | grep -o -E "SQ_WAVE_CYCLES|SQ_BUSY_CYCLES|SQ_WAIT_ANY|SQ_WAIT_INST_ANY|SQ_WAIT_INST_LDS|SQ_ACTIVE_INST_ANY|SQ_VALU_MFMA_BUSY_CYCLES|SQ_INSTS_VALU_MFMA_I8|GRBM_GUI_ACTIVE|SQ_LDS_BANK_CONFLICT" | sort | uniq -c > $O/counter_names_checked.txt; cat $O/counter_names_checked.txt; } &&
rm -rf /tmp/acc_k /tmp/acc_l &&
timeout -k 10 300 rocprofv3 --pmc $SQ --kernel-include-regex "match_mfma_kernel" --output-format csv -d /tmp/acc_k -- python bench.py --gpus 1 --steps 3 --warmup 1 > $O/bench_line_under_wave_counters.json 2> /tmp/acc_k.err &&
{ f=$(find /tmp/acc_k -name "*counter_collection.csv" | head -1); [ -n "$f" ] && python profiles/scan16/recipes/pmc_csv_sum.py $f match_mfma > $O/pmc_wave_cycles_kernel.txt && cat $O/pmc_wave_cycles_kernel.txt; } &&
LADDER_UNITS=1 LADDER_DATA=7 timeout -k 10 300 rocprofv3 --pmc $SQ --kernel-include-regex "ladder16u" --output-format csv -d /tmp/acc_l -- $L > $O/ladder_under_wave_counters.log 2>&1 &&
{ f=$(find /tmp/acc_l -name "*counter_collection.csv" | head -1); [ -n "$f" ] && python profiles/scan16/recipes/pmc_csv_sum.py $f ladder16u > $O/pmc_wave_cycles_ladder.txt && cat $O/pmc_wave_cycles_ladder.txt; }
rc=$?
echo "account rc=$rc"
[ $rc -ne 0 ] && tail -5 $O/stamps_8.err $O/stamps_64.err /tmp/acc_k.err 2>/dev/null
exit $rc
