# Timing-diagnostic builds of the match kernel (results are WRONG by construction; only their
# kernel time is of interest).  libamc_diag<N>.so under pycolmap_amd/csrc/_obj/, selected with
# AMC_LIB_PATH.  N bit 0: no row-block epilogue; bit 1: no VALU epilogue inside the scan.
set -e
cd "$(dirname "$0")/../pycolmap_amd/csrc"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -I../../include"
STEMS=$(python -c "import sys; sys.path.insert(0, '../..'); from pycolmap_amd.build import HIP_SOURCES; print(' '.join(n[:-4] for n in HIP_SOURCES))")
for n in "$@"; do
  /opt/rocm/bin/hipcc $FLAGS -DAMC_DIAG=$n -c match_mfma.hip -o _obj/match_mfma_diag$n.o
  OBJS=""
  for o in $STEMS; do if [ $o = match_mfma ]; then OBJS="$OBJS _obj/match_mfma_diag$n.o"; else OBJS="$OBJS _obj/$o.o"; fi; done
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o _obj/libamc_diag$n.so $OBJS
done
ls -la _obj/*.so
