"""Freeze the undistortion CPU reference (tests/undistort_ref/undistort_ref.cc) on the edge list of
tests/undistort_cases.py (edge_cases()): per case the digest of the input, the digest of the warped image and the
number of target pixels inside the source, for six small cases the image itself ->
tests/golden/undistort_ref_edges_v1.npz.  tests/test_undistort_cpu.py::test_edge_reference_against_frozen_fixture
checks that the reference still computes exactly this; tests/test_undistort_gpu.py holds the device to the same
digests.  Run from the repository root: python tests/golden/make_undistort_ref_edges_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

FULL = ["a-tail-5x3-3ch-prepass", "b-narrow-1x9-3ch", "c-warp-253-11x23-3ch", "g-halfxy-1ch", "g-prepass-3ch",
        "h-huge-RADIAL-1e-160-21x15-3ch"]


def main():
    import undistort_cases as cases
    import undistort_ref_lib as ref
    out = {}
    for name, img, cam, dst in cases.edge_cases():
        warped, vals, _ = ref.warp(img, cam, dst, details=True)
        inside = int((vals[..., 0] >= 0).sum())
        out[f"{name}/input_digest"] = np.frombuffer(cases.digest(img).encode(), np.uint8)
        out[f"{name}/digest"] = np.frombuffer(cases.digest(warped).encode(), np.uint8)
        out[f"{name}/inside"] = np.array(inside, np.int64)
        if name in FULL:
            out[f"{name}/image"] = warped
        print(name, dst[1], "x", dst[2], inside, "inside", cases.digest(warped)[:12])
    assert all(f"{name}/image" in out for name in FULL)
    np.savez_compressed(ROOT / "tests" / "golden" / "undistort_ref_edges_v1.npz", **out)


if __name__ == "__main__":
    main()
