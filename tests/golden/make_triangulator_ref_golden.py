"""Freeze the incremental triangulator's CPU reference (tests/triangulator_ref/triangulator_ref.cc, written from DESIGN.md
section 17) into tests/golden/triangulator_ref_v1.npz: for every flat case of tests/triangulator_cases.py the digest of
the result, for CASES the result arrays themselves, and for every scene of SCENES the digest of the sequential result
with its per-image counts.  The GPU tests compare the library with the live reference and with this file;
tests/test_triangulator_cpu.py checks that the reference still reproduces it.

    python tests/golden/make_triangulator_ref_golden.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import triangulator_cases as tc  # noqa: E402

OUT = Path(__file__).resolve().parent / "triangulator_ref_v1.npz"


def main():
    data = {"cases": np.array(sorted(tc.CASES)), "edge_cases": np.array(sorted(tc.EDGE_CASES)), "scenes": np.array(sorted(tc.SCENES))}
    for name in sorted(tc.ALL_CASES):
        res = tc.reference(name)
        data[f"{name}/digest"] = np.array(tc.digest(res))
        if name in tc.CASES:
            for k in tc.RESULT_KEYS:
                data[f"{name}/{k}"] = np.asarray(res[k])
    for name in sorted(tc.SCENES):
        counts, points, _, _, _ = tc.scene_reference(name)
        data[f"scene/{name}/digest"] = np.array(tc.scene_digest(counts, points))
        data[f"scene/{name}/counts"] = np.asarray(counts, np.int64)
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(tc.ALL_CASES)} cases, {len(tc.SCENES)} scenes)")


if __name__ == "__main__":
    main()
