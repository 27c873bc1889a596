#!/bin/bash
# before / after: kernel trace with stats, one counters-only pass each (a run of its own, no tracing), the output dumps
# compared byte for byte, and the randomised stress.  Parent library: bash tools/ab_prev_lib.sh <parent> first.
set -o pipefail
O=${OUT:-profiles/scan128}
mkdir -p $O
P=$PWD/pycolmap_amd/csrc/_obj/libamc_prev.so
B="python bench.py --gpus 1 --steps 3 --warmup 1"
one() {  # $1 = tag, env already set
  tag=$1
  rm -rf /tmp/kt_$tag /tmp/pmc_$tag /tmp/dump_$tag
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/kt_$tag -- $B > $O/bench_line_under_rocprofv3_$tag.json 2> /tmp/kt_$tag.err || return 1
  f=$(find /tmp/kt_$tag -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cp $f $O/rocprofv3_kernel_stats_$tag.csv && head -6 $f
  timeout -k 10 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_I8 GRBM_GUI_ACTIVE SQ_LDS_BANK_CONFLICT SQ_WAVE_CYCLES SQ_WAIT_ANY --output-format csv -d /tmp/pmc_$tag -- $B > $O/bench_line_under_pmc_$tag.json 2> /tmp/pmc_$tag.err || return 1
  f=$(find /tmp/pmc_$tag -name "*counter_collection.csv" | head -1); [ -n "$f" ] && python profiles/scan16/recipes/pmc_csv_sum.py $f match_mfma > $O/pmc_scan_$tag.txt && cat $O/pmc_scan_$tag.txt
  timeout -k 10 120 $B --dump-outputs /tmp/dump_$tag > /dev/null 2>&1 || return 1
}
AMC_LIB_PATH=$P one parent && one new &&
{ for f in /tmp/dump_parent/*.npy; do cmp $f /tmp/dump_new/$(basename $f) && echo "byte-equal: $(basename $f) $(stat -c %s $f) bytes" || exit 1; done; } | tee $O/dump_cmp.txt &&
timeout -k 10 400 python tools/stress_match.py --rounds 10 2>&1 | tail -4 | tee $O/stress_match.txt
exit $?
