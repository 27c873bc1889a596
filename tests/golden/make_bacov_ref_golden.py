"""Freeze the bundle-adjustment covariance reference (tests/bacov_ref) into tests/golden/bacov_ref_v1.npz: per case of
tests/bacov_cases.py the sha256 digest of the result (flags, column map, matrix, point blocks, bit for bit), the scalars
(success, failed column, columns, min_pivot_ratio) as float64, and the matrix's diagonal.  Run from the repository root:
python tests/golden/make_bacov_ref_golden.py
With --budget it writes tests/ref2/bacov_deviation_budget.json instead: the deviations of the reference from the numpy
restatement (tests/ref2/bacov_ref2.py), from section 12.8's covariance and of the relative-pose Jacobian from central
differences, as measured on the CPU it runs on, each with its bound, twice the measured figure."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import bacov_cases  # noqa: E402
import bacov_ref_lib as ref  # noqa: E402


def main():
    cases = bacov_cases.cases()
    out = {"names": np.array([c["name"] for c in cases])}
    for c in cases:
        r = ref.ba_covariance(*c["problem"], options=c["options"], point_const=c["point_const"])
        out[f'{c["name"]}/digest'] = np.array(bacov_cases.digest(r))
        out[f'{c["name"]}/scalars'] = np.array([r["success"], r["failed_column"], r["num_columns"], r["min_pivot_ratio"]],
                                               np.float64)
        out[f'{c["name"]}/diagonal'] = np.diag(r["matrix"]).copy() if r["success"] else np.zeros(0)
    np.savez_compressed(ROOT / "tests" / "golden" / "bacov_ref_v1.npz", **out)


def budget():
    import json
    import platform
    sys.path.insert(0, str(ROOT / "tests" / "ref2"))
    import bacov_ref2
    import test_ba_covariance_cpu as t
    out = {"machine": f"{platform.machine()} CPU, numpy {np.__version__}", "cases": {}}
    for c in bacov_cases.cases():
        if c["expect"] != "ok" or c["m"] == 0:
            continue
        r = ref.ba_covariance(*c["problem"], options=c["options"], point_const=c["point_const"])
        m2, p2 = bacov_ref2.ba_covariance(*c["problem"], options=c["options"], point_const=c["point_const"])
        dev = bacov_ref2.deviation(r, m2, p2)
        out["cases"][c["name"]] = {"measured": dev, "bound": 2.0 * dev, "condition": float(np.linalg.cond(r["matrix"]))}
    for key, dev in (("abspose", t.abspose_deviation()), ("relative_pose_jacobian", t.relative_pose_jacobian_deviation())):
        out[key] = {"measured": dev, "bound": 2.0 * dev}
    t.BUDGET_PATH.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    budget() if "--budget" in sys.argv else main()
