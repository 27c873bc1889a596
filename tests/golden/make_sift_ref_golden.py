"""Freeze the SIFT CPU reference (tests/sift_ref/sift_ref.cc) on a few seeded images: tests/golden/sift_ref_v1.npz.
Run from the repository root: python tests/golden/make_sift_ref_golden.py (only when the reference's definitions change
on purpose, with a new file version)."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))
import sift_images as si  # noqa: E402
import sift_ref_lib as ref  # noqa: E402

CASES = {
    "textured_default": (lambda: si.textured(101, 150, 190), {}),
    "noise_first_octave_0": (lambda: si.noise(102, 90, 120), {"first_octave": 0}),
    "textured_l2_upright": (lambda: si.textured(103, 130, 110), {"normalization": 1, "upright": True}),
    "blobs_orient4": (lambda: si.blobs(96, 128, [(30.2, 40.6, 2.5), (80.1, 60.3, 4.0)]), {"max_num_orientations": 4}),
}


def main():
    out = {}
    for name, (make, opts) in CASES.items():
        img = make()
        kp, desc = ref.extract(img, **opts)
        out[f"{name}/image"] = img
        out[f"{name}/keypoints"] = kp
        out[f"{name}/descriptors"] = desc
        print(name, img.shape, len(kp))
    np.savez_compressed(ROOT / "tests" / "golden" / "sift_ref_v1.npz", **out)


if __name__ == "__main__":
    main()
