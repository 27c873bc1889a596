# usage: bash tools/diag_run.sh prev base ...   bench.py's headline (matching only) on libamc.so (base) or on
# pycolmap_amd/csrc/_obj/libamc_prev.so (prev: tools/ab_prev_lib.sh, tools/ab_build.sh), one line per name in the order given
R=$(cd "$(dirname "$0")/.." && pwd)   # the repository root; bench.py is run from the current directory, which is meant to be it
for v in "$@"; do
  if [ $v = base ]; then unset AMC_LIB_PATH; elif [ $v = prev ]; then export AMC_LIB_PATH=$R/pycolmap_amd/csrc/_obj/libamc_prev.so; else echo "diag_run.sh: $v is neither base nor prev" >&2; exit 2; fi
  timeout 200 python bench.py --steps 3 --warmup 1 --no-cpu-baseline --verify-pairs 0 --no-pipeline --no-dense --no-ragged --no-db 2>/dev/null | tail -1 | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('$v', d['ms_per_step'], d['roofline']['frac'], d['roofline']['avg_kernel_ms'])"
done
