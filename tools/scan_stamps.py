#!/usr/bin/env python3
"""Where an item's clocks go in the match scan: runs one exhaustive match through the stamped diagnostic library
(tools/scan_stamps_build.sh) and reports, as medians over workgroups, the share of an item's clocks spent at chunk
crossings (a / c) and at the item boundary (b / c), and the boundary's split: from the end of the scan to the next item's
top wait (its loads issued, this item decoded and stored), then the wait itself; the rest is the way to the first MFMA.  The stamps are described in match_mfma.hip (AMC_SCAN_STAMPS).
Needs a GPU; not in the test suite.

    bash tools/scan_stamps_build.sh && python tools/scan_stamps.py --images 8 --rows 4096 --grid 28

--grid caps the scan's workgroups (AMC_SCAN_GRID; two of them share a CU): 8 images are 224 items of four segments,
fewer than the workgroups of a full grid (two per CU) take, and an item boundary only exists where a workgroup scans
more than one item.  A workgroup's clocks run while its CU partner scans too: compare clocks per item with TWICE the
clocks of an item of the same four segments scanned alone."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "pycolmap_amd", "csrc", "_obj", "libamc_stamps.so")
MAX_WG, WAVES, DWORDS = 1024, 4, 16  # kStampMaxWG, kSegsPerItem, kStampDwords (match_mfma.hip, amc_internal.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--grid", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3, help="matches run before the sums are read (the first is discarded)")
    ap.add_argument("--run", type=int, default=0, help="AMC_SCAN_RUN: 0 auto, 1 off, 2 / 4 / 8 forced")
    ap.add_argument("--lib", default=LIB, help="a stamped library of another revision (default: the tree's own)")
    args = ap.parse_args()
    lib_path = os.path.abspath(args.lib)
    if not os.path.exists(lib_path):
        sys.exit("no diagnostic library: bash tools/scan_stamps_build.sh")
    os.environ["AMC_LIB_PATH"] = lib_path
    if args.grid:
        os.environ["AMC_SCAN_GRID"] = str(args.grid)
    if args.run:
        os.environ["AMC_SCAN_RUN"] = str(args.run)
    import torch
    import bench
    from pycolmap_amd import _capi, synth

    arena = bench.make_arena_torch(args.images, args.rows, 1234, torch.device("cuda:0")).cpu().numpy()
    s1, s2 = synth.exhaustive_pairs(args.images)
    lib = ctypes.CDLL(lib_path)
    lib.amc_scan_stamps_read.argtypes = [ctypes.c_void_p, ctypes.c_int]
    buf = np.zeros((2, MAX_WG, WAVES, DWORDS), np.uint32)
    with _capi.Context(0) as ctx:
        ctx.reserve_slots(args.images)
        for k in range(args.images):
            ctx.upload_descriptors(k, arena[k])
        for r in range(args.repeat):
            if r == 1 or args.repeat == 1:
                assert lib.amc_scan_stamps_read(None, 1) == 0
            _, _, st = ctx.match_pairs(s1, s2, kernel="mfma")
        assert lib.amc_scan_stamps_read(buf.ctypes.data, 0) == buf.size
    out = {"images": args.images, "rows": args.rows, "grid_cap": args.grid, "matches_summed": max(1, args.repeat - 1),
           "pairs_mfma": int(st["pairs_mfma"]), "scan_run": int(st["scan_run"])}
    for mode, name in ((0, "forward_scan"), (1, "reverse_scan")):
        s = buf[mode].astype(np.float64)
        wg_a, wg_b, wg_c, wg_n, tail_a, tail_c, wg_kept, wg_bk, wg_bl = [], [], [], [], [], [], [], [], []
        sp = {k: [] for k in ("issue_all", "wait_all", "issue_kept", "wait_kept", "issue_loaded", "wait_loaded")}
        for wg in range(MAX_WG):
            w = s[wg][s[wg][:, 3] > 0]
            if len(w):
                wg_a.append(float(np.mean(w[:, 0] / w[:, 2])))
                wg_b.append(float(np.mean(w[:, 1] / w[:, 2])))
                wg_c.append(float(np.mean(w[:, 2] / w[:, 3])))
                wg_n.append(float(w[0, 3]))
                # boundaries of items that kept their X rows (run entries with kRunSameX), and of the others
                wg_kept.append(float(np.mean(w[:, 9] / w[:, 3])))
                k, l = w[w[:, 9] > 0], w[w[:, 3] > w[:, 9]]
                if len(k):
                    wg_bk.append(float(np.mean(k[:, 8] / k[:, 9])))
                if len(l):
                    wg_bl.append(float(np.mean((l[:, 1] - l[:, 8]) / (l[:, 3] - l[:, 9]))))
                # the boundary's split: scan end -> at the top wait (loads issued, item decoded) -> wait passed
                sp["issue_all"].append(float(np.mean(w[:, 10] / w[:, 3])))
                sp["wait_all"].append(float(np.mean(w[:, 11] / w[:, 3])))
                if len(k):
                    sp["issue_kept"].append(float(np.mean(k[:, 12] / k[:, 9])))
                    sp["wait_kept"].append(float(np.mean(k[:, 13] / k[:, 9])))
                if len(l):
                    sp["issue_loaded"].append(float(np.mean((l[:, 10] - l[:, 12]) / (l[:, 3] - l[:, 9]))))
                    sp["wait_loaded"].append(float(np.mean((l[:, 11] - l[:, 13]) / (l[:, 3] - l[:, 9]))))
            t = s[wg][s[wg][:, 7] > 0]
            if len(t):
                tail_a.append(float(np.mean(t[:, 5])))
                tail_c.append(float(np.mean(t[:, 6])))
        med = lambda v: round(float(np.median(v)), 5) if len(v) else None
        out[name] = {"workgroups_with_a_boundary": len(wg_a), "items_with_successor_per_workgroup_median": med(wg_n),
                     "crossings_share_a_over_c_median": med(wg_a), "crossings_share_min_max": [med([min(wg_a)]), med([max(wg_a)])] if wg_a else None,
                     "boundary_share_b_over_c_median": med(wg_b), "boundary_share_min_max": [med([min(wg_b)]), med([max(wg_b)])] if wg_b else None,
                     "clocks_per_item_c_median": med(wg_c), "items_that_kept_x_share_median": med(wg_kept),
                     "boundary_clocks_kept_x_median": med(wg_bk), "boundary_clocks_loaded_x_median": med(wg_bl),
                     "boundary_clocks_median": med([b * c for b, c in zip(wg_b, wg_c)]),
                     "boundary_split_clocks_median": {k: med(v) for k, v in sp.items()},
                     "last_item_crossing_clocks_median": med(tail_a), "last_item_clocks_median": med(tail_c)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
