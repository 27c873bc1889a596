# A second build of the verification kernels beside the product's: libamc_<name>.so under pycolmap_amd/csrc/_obj/ with
# extra flags on tvg_e.hip, tvg_fh.hip and amc_verify.hip - the instrumented builds (-DAMC_TVG_PROF, -DAMC_TVG_LODIAG: the
# counters AMC_TVG_PROFILE=1 prints) or an edited working tree against the built product; select with AMC_LIB_PATH.
#   bash tools/variant_build_tvg.sh prof "-DAMC_TVG_PROF"
set -e
cd "$(dirname "$0")/../pycolmap_amd/csrc"
NAME=$1; shift
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -I../../include $*"
VAR="tvg_e tvg_fh amc_verify"
for f in $VAR; do
  /opt/rocm/bin/hipcc $FLAGS -c $f.hip -o _obj/${f}_$NAME.o
done
OBJS=""
for o in $(python -c "import sys; sys.path.insert(0, '../..'); from pycolmap_amd.build import HIP_SOURCES; print(' '.join(n[:-4] for n in HIP_SOURCES))"); do
  case " $VAR " in *" $o "*) OBJS="$OBJS _obj/${o}_$NAME.o";; *) OBJS="$OBJS _obj/$o.o";; esac
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o _obj/libamc_$NAME.so $OBJS
ls -la _obj/libamc_$NAME.so
