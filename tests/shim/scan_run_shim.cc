// Host build of pycolmap_amd/csrc/scan_run.h for tests/test_scan_run_cpu.py: the run length the host chooses for a
// batch's forward scan.
#include "../../pycolmap_amd/csrc/scan_run.h"

extern "C" {
int sr_choose(const unsigned* slot1, const unsigned* grp, unsigned long ngrp, unsigned long items,
              unsigned long workgroups, int forced) {
    return amc::choose_scan_run(slot1, grp, ngrp, items, workgroups, forced);
}
int sr_auto() { return amc::kScanRunAuto; }
unsigned long sr_min_runs_per_workgroup() { return amc::kScanRunMinPerWorkgroup; }
}
