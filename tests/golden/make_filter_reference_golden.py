"""Record COLMAP's own point filter for a later comparison with this project's (deviations F2 and F3 are
the candidates such a recording would settle).  Needs the real pycolmap 0.6.x (COLMAP 3.9.1); writes
tests/golden/filter_pycolmap_v1.npz: the model of tests/test_filter_gpu.py's FILTER_SCENE is built through the public
Reconstruction methods, and for filter_all_points3D, filter_points3D with an id set, filter_points3D_in_images,
delete_observation on tracks of length 5 and 2, and the two means, the return value and the model afterwards (tracks,
points2D ids, errors) are stored.  Run from the repository root on a machine that has that package:
python tests/golden/make_filter_reference_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))

FILTER_SCENE = dict(seed=300, nimg=5, npts=30, model=2, noise=0.5, outliers=10, tracks="mixed", perturb=0.0)
INVALID = 0xFFFFFFFFFFFFFFFF


def build(pycolmap, sc, names):
    """ba_cases.reconstruction with the given package"""
    r = pycolmap.Reconstruction()
    for c, p in enumerate(sc["camera_params"]):
        r.add_camera(pycolmap.Camera(model=names[sc["models"][c]], width=1000, height=800, params=list(p), camera_id=c + 1))
    tracks = {}
    for i, c in enumerate(sc["image_cameras"]):
        im = pycolmap.Image(name=f"image{i + 1}.png", camera_id=int(c) + 1, id=i + 1)
        im.cam_from_world = pycolmap.Rigid3d(pycolmap.Rotation3d(np.array(sc["qvec"][i])), np.array(sc["tvec"][i]))
        sel = np.flatnonzero(sc["obs_image"] == i)
        im.points2D = pycolmap.ListPoint2D([pycolmap.Point2D(sc["obs_xy"][k]) for k in sel])
        im.registered = True
        for idx, k in enumerate(sel):
            tracks.setdefault(int(sc["obs_point"][k]), []).append(pycolmap.TrackElement(i + 1, idx))
        r.add_image(im)
        r.register_image(i + 1)
    for j in range(len(sc["xyz"])):
        r.add_point3D(sc["xyz"][j], pycolmap.Track(tracks[j]))
    return r


def state(r, out, key):
    ids = sorted(r.points3D)
    out[f"{key}/point_ids"] = np.array(ids, np.uint64)
    out[f"{key}/errors"] = np.array([r.points3D[i].error for i in ids], np.float64)
    out[f"{key}/track_lengths"] = np.array([r.points3D[i].track.length() for i in ids], np.uint32)
    out[f"{key}/tracks"] = np.array([[i, e.image_id, e.point2D_idx] for i in ids for e in r.points3D[i].track.elements],
                                    np.uint64).reshape(-1, 3)
    for iid in sorted(r.images):
        out[f"{key}/points2D/{iid}"] = np.array([p.point3D_id if p.has_point3D() else INVALID for p in r.images[iid].points2D],
                                                np.uint64)
    out[f"{key}/mean_reprojection_error"] = np.float64(r.compute_mean_reprojection_error())
    out[f"{key}/mean_observations_per_reg_image"] = np.float64(r.compute_mean_observations_per_reg_image())


def main():
    import pycolmap  # the reference package, not this repository's alias
    if "pycolmap_amd" in (getattr(pycolmap, "__doc__", "") or ""):
        raise SystemExit("this needs the real pycolmap 0.6.x, not pycolmap_amd's alias")
    import ba_cases
    sc = ba_cases.scene(**FILTER_SCENE)
    out = {}
    calls = {"all": lambda r: r.filter_all_points3D(3.0, 1.5),
             "ids": lambda r: r.filter_points3D(3.0, 1.5, set(sorted(r.points3D)[::3])),
             "in_images": lambda r: r.filter_points3D_in_images(3.0, 1.5, {2}),
             "angle_only": lambda r: r.filter_all_points3D(1e9, 12.0)}
    for key, call in calls.items():
        r = build(pycolmap, sc, ba_cases.MODEL_NAMES)
        state(r, out, f"{key}/before")
        out[f"{key}/returned"] = np.uint64(call(r))
        state(r, out, f"{key}/after")
        print(key, int(out[f"{key}/returned"]), r.num_points3D())
    r = build(pycolmap, sc, ba_cases.MODEL_NAMES)
    for want in (5, 2):
        pid = next(i for i in sorted(r.points3D) if r.points3D[i].track.length() == want)
        e = r.points3D[pid].track.elements[0]
        r.delete_observation(e.image_id, e.point2D_idx)
        state(r, out, f"delete_observation/from_length_{want}")
    np.savez_compressed(ROOT / "tests" / "golden" / "filter_pycolmap_v1.npz", **out)


if __name__ == "__main__":
    main()
