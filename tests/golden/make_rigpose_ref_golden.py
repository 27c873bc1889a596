"""Writes tests/golden/rigpose_ref_v1.npz: the CPU reference (tests/rigpose_ref) on every case of tests/rigpose_cases.py,
one array per case and field ("<case>/<field>").  The fixture freezes the reference: tests/test_rigpose_cpu.py compares
a fresh run with it bit for bit, tests/test_rigpose_gpu.py the GPU.  Run from the repository root after a deliberate
change of DESIGN.md section 13: python tests/golden/make_rigpose_ref_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import rigpose_cases  # noqa: E402
import rigpose_ref_lib as ref  # noqa: E402

FIELDS = ("success", "qvec", "tvec", "num_inliers", "num_all_inliers", "num_trials", "inlier_mask", "covariance")


def main():
    out = {}
    for name, (sc, est, rf, cov) in sorted(rigpose_cases.cases().items()):
        r = ref.estimate(*rigpose_cases.args(sc), est, rf, cov)
        for k in FIELDS:
            if k in r:
                out[f"{name}/{k}"] = np.asarray(r[k])
    path = ROOT / "tests" / "golden" / "rigpose_ref_v1.npz"
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {path.stat().st_size} bytes")


if __name__ == "__main__":
    main()
