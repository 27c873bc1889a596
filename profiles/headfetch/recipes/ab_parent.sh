#!/bin/bash
# The tree against the parent library (bash tools/ab_prev_lib.sh <parent>; bash tools/scan_stamps_build.sh): the new
# tests, stamps, the short-image bench and the headline alternating parent / new three times, outputs byte for byte on
# both shapes, the GPU suite, smoke.  Every run under its own time limit; nothing is started after a failure.
set -o pipefail
O=$PWD/${OUT:-profiles/headfetch}/ab
mkdir -p $O
P=$PWD/pycolmap_amd/csrc/_obj/libamc_prev.so
L=$PWD/pycolmap_amd/csrc/_obj/libamc_stamps.so
timeout -k 10 300 python -m pytest tests/test_match_scan_epilogue_gpu.py tests/test_match_scan_chain_gpu.py -q -x -m gpu -p no:cacheprovider > $O/pytest_epilogue.txt 2>&1 || { echo "epilogue tests failed rc=$?"; tail -40 $O/pytest_epilogue.txt; exit 1; }
tail -2 $O/pytest_epilogue.txt
for r in 512 4096; do
  timeout -k 10 120 python tools/scan_stamps.py --images 64 --rows $r --run 4 --lib $L > $O/stamps_new_run4_$r.json 2> $O/stamps_new_run4_$r.err || { echo "stamps $r failed rc=$?"; tail -5 $O/stamps_new_run4_$r.err; exit 1; }
  python -c "
import json
d=json.load(open('$O/stamps_new_run4_$r.json')); f=d['forward_scan']
print($r,'item',f['clocks_per_item_c_median'],'share',f['boundary_share_b_over_c_median'],'bnd kept',f['boundary_clocks_kept_x_median'],'loaded',f['boundary_clocks_loaded_x_median'],f['boundary_split_clocks_median'])"
done
H="python bench.py --gpus 1 --images 2000 --feats 512 --steps 20 --warmup 5"
HH="python bench.py --gpus 1 --steps 20 --warmup 5"
for k in 1 2 3; do
  AMC_LIB_PATH=$P timeout -k 10 120 $H > $O/s512_parent_$k.json 2> $O/s512_parent_$k.err &&
  timeout -k 10 120 $H > $O/s512_new_$k.json 2> $O/s512_new_$k.err &&
  AMC_LIB_PATH=$P timeout -k 10 150 $HH > $O/head_parent_$k.json 2> $O/head_parent_$k.err &&
  timeout -k 10 150 $HH > $O/head_new_$k.json 2> $O/head_new_$k.err || { echo "bench round $k failed rc=$?"; tail -5 $O/*.err | tail -20; exit 1; }
done
python - <<PY
import json
def line(f):
    d=json.loads(open(f).read().strip().splitlines()[-1]); return (d["ms_per_step"], round(d["roofline"]["avg_kernel_ms"],4), round(d["roofline"]["frac"],4))
for n in ("s512_parent","s512_new","head_parent","head_new"):
    print(n, [line("$O/%s_%d.json"%(n,k)) for k in (1,2,3)])
PY
for shape in "" "--images 2000 --feats 512"; do
  tag=$( [ -z "$shape" ] && echo head || echo s512 )
  AMC_LIB_PATH=$P timeout -k 10 150 python bench.py --gpus 1 $shape --steps 2 --warmup 1 --dump-outputs $O/dump_parent_$tag > /dev/null 2> $O/dump_parent_$tag.err &&
  timeout -k 10 150 python bench.py --gpus 1 $shape --steps 2 --warmup 1 --dump-outputs $O/dump_new_$tag > /dev/null 2> $O/dump_new_$tag.err || { echo "dump $tag failed"; exit 1; }
  for f in $(ls $O/dump_parent_$tag); do cmp $O/dump_parent_$tag/$f $O/dump_new_$tag/$f && echo "cmp equal: $tag $f $(stat -c %s $O/dump_new_$tag/$f) bytes"; done >> $O/dump_cmp.txt 2>&1
  rm -rf $O/dump_parent_$tag $O/dump_new_$tag $O/dump_parent_$tag.err $O/dump_new_$tag.err
done
cat $O/dump_cmp.txt
timeout -k 10 700 python -m pytest tests -m gpu -q -p no:cacheprovider > $O/pytest_gpu.txt 2>&1; rc=$?
tail -4 $O/pytest_gpu.txt
[ $rc -eq 0 ] || { echo "gpu suite rc=$rc"; grep -E "^(FAILED|ERROR)" $O/pytest_gpu.txt | head -20; exit 1; }
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.txt 2>&1 || { echo "smoke failed rc=$?"; tail -10 $O/smoke.txt; exit 1; }
cat $O/smoke.txt
