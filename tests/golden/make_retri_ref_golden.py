"""Freeze the CPU reference of retriangulate (tests/retri_ref/retri_ref.cc, written from DESIGN.md section 19) into
tests/golden/retri_ref_v1.npz: for every flat case of tests/retri_cases.py the digest of the result, for a few small cases
the result arrays themselves, and for every scene of SCENES the digest of the sequential result after two calls with the
calls' counts.  The GPU tests compare the library with the live reference and with this file;
tests/test_retriangulate_cpu.py checks that the reference still reproduces it.

    python tests/golden/make_retri_ref_golden.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import retri_cases as k  # noqa: E402

OUT = Path(__file__).resolve().parent / "retri_ref_v1.npz"
WITH_ARRAYS = ("mixed", "rounds_2", "nan_point", "continue_at_threshold", "ratio_fifth_runs", "filled_pair_skipped",
               "filled_pair_runs")


def main():
    data = {"cases": np.array(sorted(k.ALL_CASES)), "scenes": np.array(sorted(k.SCENES))}
    for name in sorted(k.ALL_CASES):
        res = k.reference(name)
        data[f"{name}/digest"] = np.array(k.digest(res))
        if name in WITH_ARRAYS:
            for key in k.RESULT_KEYS:
                data[f"{name}/{key}"] = np.asarray(res[key])
    for name in sorted(k.SCENES):
        calls, _ = k.scene_reference(name)
        data[f"scene/{name}/digest"] = np.array(k.state_digest(calls[1][0], calls[1][1], calls[1][4]))
        data[f"scene/{name}/counts"] = np.asarray([c[0] for c in calls], np.int64)
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(k.ALL_CASES)} cases, {len(k.SCENES)} scenes)")


if __name__ == "__main__":
    main()
