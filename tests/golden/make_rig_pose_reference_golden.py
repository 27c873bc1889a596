"""Record COLMAP's own rig absolute pose for a later comparison with this project's.  Needs the real pycolmap 0.6.x
(COLMAP 3.9.1); writes tests/golden/rig_pose_reference_v1.npz with pycolmap.rig_absolute_pose_estimation on the cases of
tests/rigpose_cases.py, one call per case.  The GP3P formulation differs from COLMAP's, so the
comparison this enables is one of poses and masks within a tolerance, not of bits.  Run from the repository root on a
machine that has that package: python tests/golden/make_rig_pose_reference_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

MODEL_NAMES = ["SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "OPENCV_FISHEYE", "FULL_OPENCV", "FOV",
               "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE"]


def main():
    import pycolmap  # the reference package, not this repository's alias
    if "pycolmap_amd" in (getattr(pycolmap, "__doc__", "") or "") or not hasattr(pycolmap, "rig_absolute_pose_estimation"):
        raise SystemExit("this needs the real pycolmap 0.6.x, not pycolmap_amd's alias")
    import rigpose_cases
    out = {}
    for name, (sc, est, rf, cov) in sorted(rigpose_cases.cases().items()):
        eo = pycolmap.RANSACOptions()
        for k, v in est.items():
            setattr(eo, k, v)
        ro = pycolmap.AbsolutePoseRefinementOptions()
        for k, v in rf.items():
            setattr(ro, k, v)
        cams = [pycolmap.Camera(model=MODEL_NAMES[int(m)], width=1600, height=1200, params=p)
                for m, p in zip(sc["camera_models"], sc["camera_params"])]
        rigs = [pycolmap.Rigid3d(pycolmap.Rotation3d(g[:4]), g[4:]) for g in sc["cams_from_rig"]]
        r = pycolmap.rig_absolute_pose_estimation(sc["points2D"], sc["points3D"], [int(i) for i in sc["camera_idxs"]],
                                                  rigs, cams, eo, ro, bool(cov))
        n = len(sc["points2D"])
        out[f"{name}/success"] = np.array([r is not None])
        out[f"{name}/qvec"] = np.asarray(r["rig_from_world"].rotation.quat) if r else np.zeros(4)
        out[f"{name}/tvec"] = np.asarray(r["rig_from_world"].translation) if r else np.zeros(3)
        out[f"{name}/num_inliers"] = np.array([r["num_inliers"] if r else 0])
        out[f"{name}/inlier_mask"] = np.asarray(r["inliers"]) if r else np.zeros(n, bool)
        if r and cov:
            out[f"{name}/covariance"] = np.asarray(r["covariance"])
    path = ROOT / "tests" / "golden" / "rig_pose_reference_v1.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
