#!/bin/bash
# before / after: kernel trace with stats (tracing only, no counters in that run), parent then new; the output dumps
# compared byte for byte; the randomised stress.  Parent library: bash tools/ab_prev_lib.sh <parent> first.
# Every run under its own time limit, chained with &&: nothing is started after a fault, an abort or a time-out.
set -o pipefail
O=${OUT:-profiles/livepairs}
mkdir -p $O
P=$PWD/pycolmap_amd/csrc/_obj/libamc_prev.so
B="python bench.py --gpus 1 --steps 3 --warmup 1"
one() {  # $1 = tag, env already set
  tag=$1
  rm -rf /tmp/kt_$tag /tmp/dump_$tag
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/kt_$tag -- $B > $O/bench_line_under_rocprofv3_$tag.json 2> /tmp/kt_$tag.err || return 1
  f=$(find /tmp/kt_$tag -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cp $f $O/rocprofv3_kernel_stats_$tag.csv && head -4 $f
  timeout -k 10 120 $B --dump-outputs /tmp/dump_$tag > /dev/null 2>&1 || return 1
}
AMC_LIB_PATH=$P one parent && one new &&
{ for f in /tmp/dump_parent/*.npy; do cmp $f /tmp/dump_new/$(basename $f) && echo "byte-equal: $(basename $f) $(stat -c %s $f) bytes" || exit 1; done; } | tee $O/dump_cmp.txt &&
timeout -k 10 400 python tools/stress_match.py --rounds 10 2>&1 | tail -4 | tee $O/stress_match.txt
exit $?
