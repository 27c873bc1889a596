// scan_run.h - the host's choice of the forward scan's run length (match_mfma.hip, "Runs"; amc_match.hip, prepare()).
// Plain C++: tests/shim/scan_run_shim.cc builds it for the host.
#pragma once
#include <cstddef>
#include <cstdint>

namespace amc {

constexpr int kScanRunAuto = 4;  // the run length of a batch whose groups share their X lists (profiles/chain/README.md)
// A run is what the scan's queue hands out, so a launch ends on up to one run per workgroup of uneven work instead of one
// item.  Runs are used where that tail is small: at least this many runs per workgroup.
constexpr size_t kScanRunMinPerWorkgroup = 64;

// slot1_at(q): image 1 of the batch's mfma pairs in forward order (by streamed image, then by image 1); grp: ngrp + 1
// cuts of that order, one group per streamed image; items: the launch's items (an upper bound will do), workgroups: the
// scan's grid.  A run keeps X rows in registers from one group to the next, which only happens where item t of both
// groups holds the same segments: where the shorter of two consecutive groups' X lists is a prefix of the longer.  An
// exhaustive batch is like that at every cut but the one where the pair list was carved; sequential windows and
// loop-closure votes are not.  Runs are used where at least three cuts in four are.
// forced: AMC_SCAN_RUN - 0 auto, 1 off, 2 / 4 / 8 that run length whatever the batch looks like (anything else: auto).
// (slot1_at: a callable, so that a caller with the pairs and the order at hand need not copy ten million entries)
template <class Slot1At>
inline int choose_scan_run_by(Slot1At slot1_at, const uint32_t* grp, size_t ngrp, size_t items, size_t workgroups,
                              int forced) {
    if (forced == 1 || forced == 2 || forced == 4 || forced == 8) return forced;
    if (ngrp < 2 || items < kScanRunMinPerWorkgroup * kScanRunAuto * workgroups) return 1;
    const size_t cuts = ngrp - 1, allowed = cuts / 4;
    size_t bad = 0;
    for (size_t g = 0; g + 1 < ngrp; ++g) {
        const size_t a = grp[g], b = grp[g + 1], e = grp[g + 2];
        const size_t n = b - a < e - b ? b - a : e - b;
        size_t k = 0;
        while (k < n && slot1_at(a + k) == slot1_at(b + k)) ++k;
        if ((k < n || n == 0) && ++bad > allowed) return 1;
    }
    return kScanRunAuto;
}
inline int choose_scan_run(const uint32_t* slot1, const uint32_t* grp, size_t ngrp, size_t items, size_t workgroups,
                           int forced) {
    return choose_scan_run_by([slot1](size_t q) { return slot1[q]; }, grp, ngrp, items, workgroups, forced);
}

}  // namespace amc
