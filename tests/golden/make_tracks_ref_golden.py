"""Freeze the CPU reference of track completion and track merging (tests/tracks_ref/tracks_ref.cc, written from DESIGN.md
section 18) into tests/golden/tracks_ref_v1.npz: for every flat case of tests/tracks_cases.py the digest of the result,
for a few small cases the result arrays themselves, and for every scene of SCENES, every operation and both id lists the
digest of the sequential result with its counts.  The GPU tests compare the library with the live reference and with
this file; tests/test_tracks_cpu.py checks that the reference still reproduces it.

    python tests/golden/make_tracks_ref_golden.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import tracks_cases as k  # noqa: E402

OUT = Path(__file__).resolve().parent / "tracks_ref_v1.npz"
WITH_ARRAYS = ("c/sizes", "c/nonfinite", "c/threshold", "m/chain_5", "m/mixed")
OPS, IDS = ("complete", "merge", "both"), ("all", "subset")


def main():
    data = {"cases": np.array(sorted(k.ALL_CASES)), "scenes": np.array(sorted(k.SCENES))}
    for name in sorted(k.ALL_CASES):
        res = k.reference(name)
        data[f"{name}/digest"] = np.array(k.digest(name, res))
        if name in WITH_ARRAYS:
            for key in (k.COMPLETE_KEYS if name.startswith("c/") else k.MERGE_KEYS):
                data[f"{name}/{key}"] = np.asarray(res[key])
    for name in sorted(k.SCENES):
        for op in OPS:
            for ids in IDS:
                counts, points, _, _, _ = k.scene_reference(name, op, ids)
                data[f"scene/{name}/{op}/{ids}/digest"] = np.array(k.state_digest(sum(counts), points))
                data[f"scene/{name}/{op}/{ids}/counts"] = np.asarray(counts, np.int64)
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(k.ALL_CASES)} cases, {len(k.SCENES)} scenes)")


if __name__ == "__main__":
    main()
