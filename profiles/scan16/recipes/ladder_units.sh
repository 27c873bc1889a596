#!/bin/bash
# the unit rungs of tools/ubench_ladder.hip: both data modes, then one counters-only pass
set -o pipefail
O=${OUT:-profiles/scan16}
mkdir -p $O
L=tools/bin/ubench_ladder
: > $O/ladder_units_v3.txt
LADDER_UNITS=1 LADDER_DATA=1 timeout -k 10 120 $L >> $O/ladder_units_v3.txt 2>&1 &&
LADDER_UNITS=1 LADDER_DATA=0 timeout -k 10 120 $L >> $O/ladder_units_v3.txt 2>&1 &&
LADDER_UNITS=1 LADDER_DATA=1 timeout -k 10 120 $L >> $O/ladder_units_v3.txt 2>&1 &&
LADDER_UNITS=1 LADDER_DATA=0 timeout -k 10 120 $L >> $O/ladder_units_v3.txt 2>&1 &&
cat $O/ladder_units_v3.txt &&
rm -rf /tmp/lpmc && LADDER_UNITS=1 LADDER_DATA=1 timeout -k 10 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_LDS_BANK_CONFLICT -d /tmp/lpmc --output-format csv -- $L > $O/ladder_units_pmc_v3.log 2>&1
rc=$?
echo "pmc rc=$rc"
tail -5 $O/ladder_units_pmc_v3.log
f=$(find /tmp/lpmc -name "*counter_collection.csv" | head -1)
[ -n "$f" ] && python profiles/scan16/recipes/pmc_csv_sum.py $f > $O/ladder_units_pmc_v3.txt && cat $O/ladder_units_pmc_v3.txt
exit $rc
