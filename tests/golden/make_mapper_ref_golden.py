"""Freeze the CPU reference of the mapper (tests/mapper_ref/mapper_ref.cc, written from DESIGN.md section 20) into
tests/golden/mapper_ref_v1.npz: for every flat case of tests/mapper_cases.py the digest of the result, for the small cases
the result arrays themselves, and for every scene the digest of the reference's loop of find_next_images,
register_next_image and find_local_bundle with the number of its steps.  Also measures the largest angle difference
between the reference and the numpy restatement over the angle cases and writes it, doubled as the margin, into
tests/ref2/mapper_deviation_budget.json.  The GPU tests compare the library with the live reference and with the
fixture; tests/test_mapper_cpu.py checks that the reference still reproduces both files.

    python tests/golden/make_mapper_ref_golden.py
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import mapper_cases as k  # noqa: E402

OUT = Path(__file__).resolve().parent / "mapper_ref_v1.npz"
BUDGET = ROOT / "tests" / "ref2" / "mapper_deviation_budget.json"
VIS_FIELDS = ("num_observations", "num_visible_points3D", "score")
MAX_ARRAY = 300  # results up to this many entries are stored whole


def main():
    data = {"vis_cases": np.array(sorted(k.VIS_CASES)), "angle_cases": np.array(sorted(k.ANGLE_CASES)), "scenes": np.array(k.scene_names())}
    for name in sorted(k.VIS_CASES):
        res = k.vis_reference(name)
        data[f"vis/{name}/digest"] = np.array(k.vis_digest(res))
        if len(res["score"]) <= MAX_ARRAY:
            for f in VIS_FIELDS:
                data[f"vis/{name}/{f}"] = np.asarray(res[f])
    for name in sorted(k.ANGLE_CASES):
        res = k.angle_reference(name)
        data[f"angle/{name}/digest"] = np.array(k.angle_digest(res))
        if len(res["angle"]) <= MAX_ARRAY:
            data[f"angle/{name}/angle"] = np.asarray(res["angle"])
    for name in k.scene_names():
        log, trials, snap = k.scene_loop_reference(name)
        data[f"scene/{name}/digest"] = np.array(k.loop_digest(log, trials, snap))
        data[f"scene/{name}/steps"] = np.array([len(log), sum(1 for e in log if e[2])], np.int64)
    np.savez_compressed(OUT, **data)
    worst = k.measure_angle_difference()
    BUDGET.write_text(json.dumps({"angle": {"measured_max_abs_difference_rad": worst, "margin_rad": 2.0 * worst,
                                            "over": "every shared point's angle and every pair's percentile angle of mapper_cases.ANGLE_CASES",
                                            "rule": "the margin is twice the measured difference: two correct summation orders may differ by that much"}},
                                 indent=1, sort_keys=True) + "\n")
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(k.VIS_CASES)} + {len(k.ANGLE_CASES)} cases, {len(k.scene_names())} scenes); "
          f"angle difference {worst:.3e} rad -> {BUDGET}")


if __name__ == "__main__":
    main()
