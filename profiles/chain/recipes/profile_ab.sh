#!/bin/bash
# Stamps with runs off and with R = 4 (bash tools/scan_stamps_build.sh first), the kernel trace with stats (tracing only,
# no counters in that run) parent then new (bash tools/ab_prev_lib.sh <parent> first), the randomised stress with the
# host's choice and with R forced to 4 and 8, smoke.  OUT: where the files go.
# Every run under its own time limit, chained with &&: nothing is started after a fault, an abort or a time-out.
set -o pipefail
O=${OUT:-profiles/chain}
mkdir -p $O
P=$PWD/pycolmap_amd/csrc/_obj/libamc_prev.so
B="python bench.py --gpus 1 --steps 3 --warmup 1"
one() {  # $1 = tag, env already set
  tag=$1
  rm -rf /tmp/kt_$tag
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/kt_$tag -- $B > $O/bench_line_under_rocprofv3_$tag.json 2> /tmp/kt_$tag.err || return 1
  f=$(find /tmp/kt_$tag -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cp $f $O/rocprofv3_kernel_stats_$tag.csv && head -3 $f | cut -c1-200
}
timeout -k 10 200 python tools/scan_stamps.py --images 64 --rows 4096 --run 1 > $O/stamps_run1.json 2> $O/stamps_run1.err && cat $O/stamps_run1.json &&
timeout -k 10 200 python tools/scan_stamps.py --images 64 --rows 4096 --run 4 > $O/stamps_run4.json 2> $O/stamps_run4.err && cat $O/stamps_run4.json &&
AMC_LIB_PATH=$P one parent && one new &&
timeout -k 10 400 python tools/stress_match.py --rounds 10 2>&1 | tail -2 | tee $O/stress_match.txt &&
AMC_SCAN_RUN=4 timeout -k 10 400 python tools/stress_match.py --rounds 10 2>&1 | tail -2 | tee $O/stress_match_run4.txt &&
AMC_SCAN_RUN=8 timeout -k 10 400 python tools/stress_match.py --rounds 10 --seed 1 2>&1 | tail -2 | tee $O/stress_match_run8.txt &&
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -3 | tee $O/smoke.txt
