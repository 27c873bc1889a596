// scan_stamps.hip - the match scan with s_memtime stamps (match_mfma.hip, AMC_SCAN_STAMPS): where an item's clocks go
// between the loop and the kernel.  This unit replaces match_mfma.o in a diagnostic library (tools/scan_stamps_build.sh
// -> pycolmap_amd/csrc/_obj/libamc_stamps.so); tools/scan_stamps.py runs a match through it and reads the sums.
#define AMC_SCAN_STAMPS 1
#include "../pycolmap_amd/csrc/match_mfma.hip"

// dst: 2 (MODE) x max_wg x kSegsPerItem (waves of a workgroup, 4) x kStampDwords (16) dwords; returns the number of dwords, or -1.  reset != 0 zeroes the sums first
// and copies nothing.
extern "C" __attribute__((visibility("default"))) int amc_scan_stamps_read(uint32_t* dst, int reset) {
    const size_t bytes = sizeof(uint32_t) * 2 * amc::kStampMaxWG * amc::kSegsPerItem * amc::kStampDwords;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (reset) {
        void* p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(amc::g_scan_stamps)) != hipSuccess) return -1;
        return hipMemset(p, 0, bytes) == hipSuccess ? 0 : -1;
    }
    if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(amc::g_scan_stamps), bytes) != hipSuccess) return -1;
    return (int)(bytes / sizeof(uint32_t));
}
