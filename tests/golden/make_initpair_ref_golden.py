"""Freeze the CPU reference of the two-view triangulation of image pairs (tests/initpair_ref/initpair_ref.cc, written from
DESIGN.md section 21) into tests/golden/initpair_ref_v1.npz: for every flat case of tests/initpair_cases.py the digest of the
result and, for the small cases, the result arrays themselves.  Also measures the largest difference of xyz and of the
angle between the reference and the numpy restatement over initpair_cases.RESTATEMENT_CASES and writes it, doubled as the
margin, into tests/ref2/initpair_deviation_budget.json.  The GPU tests compare the library with the live reference and with
the fixture; tests/test_initial_pair_cpu.py checks that the reference still reproduces both files.

    python tests/golden/make_initpair_ref_golden.py
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import initpair_cases as k  # noqa: E402

OUT = Path(__file__).resolve().parent / "initpair_ref_v1.npz"
BUDGET = ROOT / "tests" / "ref2" / "initpair_deviation_budget.json"
FIELDS = ("accepted", "xyz", "tri_angle")
MAX_ARRAY = 300  # results up to this many correspondences are stored whole


def main():
    data = {"cases": np.array(sorted(k.CASES))}
    for name in sorted(k.CASES):
        res = k.reference(name)
        data[f"{name}/digest"] = np.array(k.digest(res))
        if len(res["accepted"]) <= MAX_ARRAY:
            for f in FIELDS:
                data[f"{name}/{f}"] = np.asarray(res[f])
    np.savez_compressed(OUT, **data)
    worst = k.measure_deviation()
    BUDGET.write_text(json.dumps({f: {"measured_max_abs_difference": v, "margin": 2.0 * v} for f, v in worst.items()} |
                                 {"over": "every correspondence of initpair_cases.RESTATEMENT_CASES",
                                  "rule": "the margin is twice the measured difference: the restatement solves the DLT with an SVD, the reference with a "
                                          "Jacobi eigen decomposition of A^T A; accepted is compared where the restatement's angle and depths are "
                                          "farther than the margin from their thresholds"}, indent=1, sort_keys=True) + "\n")
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(k.CASES)} cases); deviation {worst} -> {BUDGET}")


if __name__ == "__main__":
    main()
