"""Writes tests/golden/abspose_ref_v1.npz: a few localisation queries (inputs included) and what the absolute pose CPU
reference (tests/abspose_ref) returns for them, so that a later change of the reference shows up as a diff.

    python tests/golden/make_abspose_ref_golden.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import abspose_cases  # noqa: E402

OUT = ROOT / "tests" / "golden" / "abspose_ref_v1.npz"
FIELDS = ("success", "qvec", "tvec", "num_inliers", "num_trials", "focal_factor", "inlier_mask", "covariance")
INPUTS = ("offsets", "camera_models", "points2D", "points3D")
OPTS = {"outliers40": ({}, {}, True), "focal": (dict(estimate_focal_length=1, num_focal_length_samples=6), {}, False),
        "models": ({}, dict(loss_function_scale=2.0), True), "degenerate": ({}, {}, True)}


def fresh_scenes():
    return {"outliers40": abspose_cases.scene(500, 3, 400, outlier_frac=0.4),
            "focal": abspose_cases.scene(501, 2, 200, outlier_frac=0.2),
            "models": abspose_cases.concat(*[abspose_cases.scene(510 + m, 1, 120, outlier_frac=0.3, model=m)
                                             for m in range(11)]),
            "degenerate": abspose_cases.degenerate()}


def fixture_cases(g=None):
    """name -> (scene, estimation options, refinement options, return_covariance); the scenes from the fixture itself
    when it is given, else freshly generated"""
    out = {}
    scenes = fresh_scenes() if g is None else None
    for name, (est, rf, cov) in OPTS.items():
        if g is None:
            sc = scenes[name]
        else:
            sc = {k: g[f"{name}/in_{k}"] for k in INPUTS}
            sc["camera_params"] = list(g[f"{name}/in_camera_params"])
        out[name] = (sc, est, rf, cov)
    return out


def main():
    import abspose_ref_lib as ref
    arrays = {}
    for name, (sc, est, rf, cov) in fixture_cases().items():
        for k in INPUTS:
            arrays[f"{name}/in_{k}"] = np.asarray(sc[k])
        arrays[f"{name}/in_camera_params"] = np.stack([np.pad(np.asarray(p, np.float64), (0, 12 - len(p)))
                                                       for p in sc["camera_params"]])
        r = ref.estimate(sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"], sc["points3D"], est,
                         rf, cov)
        for k in FIELDS:
            if k in r:
                arrays[f"{name}/{k}"] = np.asarray(r[k])
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
