"""Record COLMAP's own EstimateTriangulation for a later comparison with this project's (tests/test_triangulation_cpu.py::
test_reference_against_pycolmap_recording).  Needs the real pycolmap 0.6.x (COLMAP 3.9.1); writes
tests/golden/tri_pycolmap_v1.npz with pycolmap.estimate_triangulation on the tracks of tests/golden/tri_ref_v1.npz
(cases of make_tri_ref_golden.py), one call per track.  Run from the repository root on a machine that has that
package: python tests/golden/make_triangulation_reference_golden.py"""
import json
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]


def main():
    import pycolmap  # the reference package, not this repository's alias
    if "pycolmap_amd" in (getattr(pycolmap, "__doc__", "") or "") or not hasattr(pycolmap, "estimate_triangulation"):
        raise SystemExit("this needs the real pycolmap 0.6.x, not pycolmap_amd's alias")
    fx = np.load(ROOT / "tests" / "golden" / "tri_ref_v1.npz")
    names = sorted({k.split("/")[0] for k in fx.files})
    out = {}
    for name in names:
        opts = json.loads(bytes(fx[f"{name}/options"]).decode())
        o = pycolmap.EstimateTriangulationOptions()
        o.min_tri_angle = opts.get("min_tri_angle", 0.0)
        for k, v in opts.items():
            if k != "min_tri_angle":
                setattr(o.ransac, k, v)
        poses, off = fx[f"{name}/poses"], fx[f"{name}/offsets"].astype(np.int64)
        op, xy = fx[f"{name}/obs_pose"], fx[f"{name}/obs_xy"]
        xyz = np.zeros((len(off) - 1, 3))
        ok = np.zeros(len(off) - 1, bool)
        mask = np.zeros(len(op), bool)
        for t in range(len(off) - 1):
            sl = slice(off[t], off[t + 1])
            if off[t + 1] - off[t] < 2:
                continue
            pts = [pycolmap.PointData(p, p) for p in xy[sl]]
            ims = [pycolmap.Image(cam_from_world=pycolmap.Rigid3d(poses[p])) for p in op[sl]]
            cams = [pycolmap.Camera(model="SIMPLE_PINHOLE", width=1000, height=1000, params=[1000.0, 500.0, 500.0])] * len(pts)
            r = pycolmap.estimate_triangulation(pts, ims, cams, opions=o)
            if r is not None:
                ok[t] = True
                xyz[t] = r["xyz"]
                mask[sl] = r["inliers"]
        out[f"{name}/xyz"], out[f"{name}/success"], out[f"{name}/inlier_mask"] = xyz, ok, mask
        print(name, int(ok.sum()), "of", len(ok))
    np.savez_compressed(ROOT / "tests" / "golden" / "tri_pycolmap_v1.npz", **out)


if __name__ == "__main__":
    main()
