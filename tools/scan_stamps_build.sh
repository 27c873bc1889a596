# The diagnostic library of tools/scan_stamps.hip: the product's own objects (python -m pycolmap_amd.build first) with
# match_mfma.o replaced by the stamped build of the same source -> pycolmap_amd/csrc/_obj/libamc_stamps.so.
# Prints the stamped kernels' resource usage (no scratch and at most 256 VGPRs, or its clocks mean nothing).
set -e
cd "$(dirname "$0")/.."
O=pycolmap_amd/csrc/_obj
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math"
/opt/rocm/bin/hipcc $FLAGS -Rpass-analysis=kernel-resource-usage -c tools/scan_stamps.hip -o $O/scan_stamps.o 2>&1 |
    grep -A9 "Function Name: _ZN3amc17match_mfma_kernel" | grep -E "Function Name|VGPRs:|Scratch|Occupancy|SGPRs:"
OBJS=$(ls $O/*.o | grep -v -E "/(match_mfma|scan_stamps|.*_prev)\.o$")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $O/libamc_stamps.so $OBJS $O/scan_stamps.o
ls -la $O/libamc_stamps.so
