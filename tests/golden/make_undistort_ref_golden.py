"""Freeze the undistortion CPU reference (tests/undistort_ref/undistort_ref.cc) on the cases of
tests/undistort_cases.py: per case the undistorted camera and the digest of the warped image, for four small cases the
image itself -> tests/golden/undistort_ref_v1.npz.  tests/test_undistort_cpu.py::test_reference_against_frozen_fixture
checks that the reference still computes exactly this.  Run from the repository root:
python tests/golden/make_undistort_ref_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

FULL = ["PINHOLE-2x2", "OPENCV-max_image_size-3ch", "FOV-max_image_size-1ch", "PINHOLE-roi-1ch"]


def main():
    import undistort_cases as cases
    import undistort_ref_lib as ref
    out = {}
    for name, img, cam, opts in cases.warp_cases():
        und = ref.undistort_camera(cam, **opts)
        warped = ref.warp(img, cam, und)
        out[f"{name}/input_digest"] = np.frombuffer(cases.digest(img).encode(), np.uint8)
        out[f"{name}/size"] = np.array(und[1:3], np.int64)
        out[f"{name}/params"] = und[3]
        out[f"{name}/digest"] = np.frombuffer(cases.digest(warped).encode(), np.uint8)
        if name in FULL:
            out[f"{name}/image"] = warped
        print(name, und[1], "x", und[2], cases.digest(warped)[:12])
    np.savez_compressed(ROOT / "tests" / "golden" / "undistort_ref_v1.npz", **out)


if __name__ == "__main__":
    main()
