"""Freeze the triangulation CPU reference (tests/tri_ref/tri_ref.cc) on seeded batches of tests/tri_cases.py: inputs
and outputs -> tests/golden/tri_ref_v1.npz.  tests/test_triangulation_cpu.py::test_reference_against_frozen_fixture
checks that the reference still computes exactly this.  Run from the repository root:
python tests/golden/make_tri_ref_golden.py"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

CASES = ["clean", "outliers30", "three_obs", "long_trial_caps", "min_tri_angle", "degenerate"]


def main():
    import tri_cases
    import tri_ref_lib as ref
    all_cases = tri_cases.cases()
    out = {}
    for name in CASES:
        sc, opts = all_cases[name]
        xyz, ok, mask, st = ref.triangulate(sc["poses"], sc["offsets"], sc["obs_pose"], sc["obs_xy"], **opts)
        for k in ("poses", "offsets", "obs_pose", "obs_xy"):
            out[f"{name}/{k}"] = sc[k]
        out[f"{name}/options"] = np.frombuffer(json.dumps(opts).encode(), np.uint8)
        out[f"{name}/xyz"] = xyz
        out[f"{name}/success"] = ok
        out[f"{name}/inlier_mask"] = mask
        out[f"{name}/num_inliers"] = st["num_inliers"]
        out[f"{name}/num_trials"] = st["num_trials"]
        print(name, len(ok), "tracks", len(mask), "observations", int(ok.sum()), "successful")
    np.savez_compressed(ROOT / "tests" / "golden" / "tri_ref_v1.npz", **out)


if __name__ == "__main__":
    main()
