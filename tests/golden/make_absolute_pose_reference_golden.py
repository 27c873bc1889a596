"""Record COLMAP's own absolute pose for a later comparison with this project's (tests/test_abspose_cpu.py::
test_agreement_with_recorded_pycolmap).  Needs the real pycolmap 0.6.x (COLMAP 3.9.1); writes
tests/golden/absolute_pose_reference_v1.npz with pycolmap.absolute_pose_estimation on the queries of
tests/golden/abspose_ref_v1.npz (cases of make_abspose_ref_golden.py), one call per query.  Run from the repository
root on a machine that has that package: python tests/golden/make_absolute_pose_reference_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "tests" / "golden")]

import make_abspose_ref_golden as mk  # noqa: E402

MODEL_NAMES = ["SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "OPENCV_FISHEYE", "FULL_OPENCV", "FOV",
               "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE"]
NUM_PARAMS = [3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12]


def main():
    import pycolmap  # the reference package, not this repository's alias
    if "pycolmap_amd" in (getattr(pycolmap, "__doc__", "") or "") or not hasattr(pycolmap, "absolute_pose_estimation"):
        raise SystemExit("this needs the real pycolmap 0.6.x, not pycolmap_amd's alias")
    g = np.load(ROOT / "tests" / "golden" / "abspose_ref_v1.npz")
    out = {}
    for name, (sc, est, rf, cov) in mk.fixture_cases(g).items():
        eo = pycolmap.AbsolutePoseEstimationOptions()
        eo.estimate_focal_length = bool(est.get("estimate_focal_length", 0))
        if "num_focal_length_samples" in est:
            eo.num_focal_length_samples = est["num_focal_length_samples"]
        ro = pycolmap.AbsolutePoseRefinementOptions()
        if "loss_function_scale" in rf:
            ro.loss_function_scale = rf["loss_function_scale"]
        off = sc["offsets"].astype(np.int64)
        nq, n = len(off) - 1, int(off[-1])
        ok, q, t, mask = np.zeros(nq, bool), np.zeros((nq, 4)), np.zeros((nq, 3)), np.zeros(n, bool)
        for i in range(nq):
            m = int(sc["camera_models"][i])
            cam = pycolmap.Camera(model=MODEL_NAMES[m], width=1600, height=1200,
                                  params=sc["camera_params"][i][:NUM_PARAMS[m]])
            sl = slice(off[i], off[i + 1])
            r = pycolmap.absolute_pose_estimation(sc["points2D"][sl], sc["points3D"][sl], cam, eo, ro)
            if r is None:
                continue
            ok[i] = True
            q[i] = r["cam_from_world"].rotation.quat
            t[i] = r["cam_from_world"].translation
            mask[sl] = r["inliers"]
        out.update({f"{name}/success": ok, f"{name}/qvec": q, f"{name}/tvec": t, f"{name}/inlier_mask": mask})
    path = ROOT / "tests" / "golden" / "absolute_pose_reference_v1.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
