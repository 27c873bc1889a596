"""Record COLMAP's own extractor for a later comparison with this project's (tests/test_sift_cpu.py::
test_reference_against_colmap_recording).  Needs the real pycolmap 0.6.x (COLMAP 3.9.1, CPU SIFT); writes
tests/golden/sift_colmap_v1.npz with pycolmap.Sift().extract on the images of make_sift_ref_golden.py.  Run from the
repository root on a machine that has that package: python tests/golden/make_sift_reference_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests" / "golden"))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    import pycolmap  # the reference package, not this repository's alias
    if "pycolmap_amd" in getattr(pycolmap, "__doc__", "") or not hasattr(pycolmap, "Sift"):
        raise SystemExit("this needs the real pycolmap 0.6.x, not pycolmap_amd's alias")
    import make_sift_ref_golden as cases
    out = {}
    sift = pycolmap.Sift()  # {peak_threshold: 0.01, first_octave: 0, max_image_size: 7000}
    for name, (make, _) in cases.CASES.items():
        img = make()
        kp, desc = sift.extract(img)
        out[f"{name}/image"] = img
        out[f"{name}/keypoints"] = np.asarray(kp, np.float32)
        out[f"{name}/descriptors"] = np.round(np.asarray(desc) * 512).astype(np.uint8)
        print(name, img.shape, len(kp))
    np.savez_compressed(ROOT / "tests" / "golden" / "sift_colmap_v1.npz", **out)


if __name__ == "__main__":
    main()
