"""Deterministic problems for bundle adjustment with constant points and for BundleAdjustmentConfig / BundleAdjuster
(DESIGN.md 15.12), for tests/test_ba_config_cpu.py, tests/test_ba_config_gpu.py and
tests/golden/make_ba_config_ref_golden.py.  The scenes are tests/ba_cases.py's; a case adds the point mask, extra
constant pose columns and cameras that are constant as a whole.  The shapes are the smallest that reach each path."""
from __future__ import annotations

import numpy as np

import ba_cases

_M = {n: k for k, n in enumerate(ba_cases.MODEL_NAMES)}


def mask(kind, npts):
    """none / all / second (every second point, the odd ones) / third (j % 3 == 1) / only3 (point 3 alone) as a uint8 mask"""
    j = np.arange(npts)
    return {"none": j < 0, "all": j >= 0, "second": j % 2 == 1, "third": j % 3 == 1, "only3": j == 3}[kind].astype(np.uint8)


# name -> (scene arguments with "flags", "pose_const" and "camera_const_all" (camera indices constant as a whole) beside
# them, the mask's kind, solver options)
CASES = {
    # masks
    "all_points_const": (dict(seed=301, nimg=4, npts=30, model=2, noise=0.3), "all", dict(max_num_iterations=4)),
    "all_poses_const": (dict(seed=302, nimg=4, npts=30, model=2, noise=0.3, flags=dict(refine_extrinsics=False)), "second",
                        dict(max_num_iterations=4)),
    "everything_const": (dict(seed=303, nimg=3, npts=12, model=2, noise=0.3,
                              flags=dict(refine_extrinsics=False, refine_focal_length=False, refine_extra_params=False)),
                         "all", dict(max_num_iterations=4)),
    # two cameras of different models, one constant as a whole
    "two_models_one_const": (dict(seed=307, nimg=4, npts=30, noise=0.3, models=[_M["SIMPLE_RADIAL"], _M["OPENCV"]],
                                  image_cameras=[0, 0, 1, 1], camera_const_all=[1]), "third", dict(max_num_iterations=4)),
    # exits with a mask: rejected steps (the minimum scene at another seed: 9 accepted and 3 rejected steps on the
    # reference) and the PCG breakdown of ba_cases.EDGE_CASES["pcg_breakdown"] with point 3 constant (4 of the 80 solves
    # end as a breakdown on the reference); tests/test_ba_config_cpu.py asserts both by the reference's own result
    "rejected_step": (dict(seed=3, nimg=2, npts=8, model=2, noise=0.3), "second", dict(max_num_iterations=12)),
    "pcg_breakdown": (dict(seed=201, nimg=3, npts=12, model=6, noise=0.3, perturb=6.0), "only3",
                      dict(max_num_iterations=80, max_linear_solver_iterations=1)),
}
# constant position subsets {0}, {1, 2}, {0, 1, 2} of image 2 (tangent columns 3 + k)
for _name, _cols in (("0", (3,)), ("12", (4, 5)), ("012", (3, 4, 5))):
    CASES[f"positions_{_name}"] = (dict(seed=304, nimg=4, npts=30, model=2, noise=0.3, pose_const={2: _cols}), "third",
                                   dict(max_num_iterations=3))
# an image with 63, 64 and 65 observations whose points alternate between constant and variable
for _n in (63, 64, 65):
    CASES[f"wave{_n}_alternate"] = (dict(seed=310 + _n, nimg=3, npts=_n, model=1, noise=0.3), "second",
                                    dict(max_num_iterations=3))
# 0, 1, 64, 65 and 257 points (a 256-lane block and one more) with masks of none, all and every second
for _n in (0, 1, 64, 65, 257):
    for _k in ("none", "all", "second"):
        CASES[f"points{_n}_{_k}"] = (dict(seed=320 + _n, nimg=3, npts=_n, model=2, noise=0.3), _k, dict(max_num_iterations=2))
for _l in ("TRIVIAL", "SOFT_L1", "CAUCHY"):
    CASES[f"loss_{_l}"] = (dict(seed=60, nimg=4, npts=60, model=2, noise=1.0, outliers=6), "second",
                           dict(max_num_iterations=4, loss_function_type=_l, loss_function_scale=2.0))


def case_scene(name):
    args = {k: v for k, v in CASES[name][0].items() if k not in ("flags", "pose_const", "camera_const_all")}
    return ba_cases.scene(**args)


def case_problem(name):
    """(positional arguments of Context.bundle_adjust, point mask, options)"""
    args, kind, options = CASES[name]
    sc = case_scene(name)
    pb = list(ba_cases.problem(sc, pose_const=args.get("pose_const"), **args.get("flags", {})))
    for c in args.get("camera_const_all", []):
        pb[2][c, :] = 1
    return tuple(pb), mask(kind, len(sc["xyz"])), options


def permuted(args, pm, seed=5):
    """the problem with its points in another order and the mask permuted with them; order[new] = old"""
    rng = np.random.default_rng(seed)
    n = len(args[7])
    order = rng.permutation(n)
    new_of = np.empty(n, np.int64)
    new_of[order] = np.arange(n)
    out = list(args)
    out[7] = np.asarray(args[7])[order]
    out[9] = new_of[np.asarray(args[9], np.int64)].astype(np.uint32)
    return tuple(out), np.asarray(pm)[order], order


# ---- Reconstruction scenes for BundleAdjustmentConfig / BundleAdjuster ---------------------------------------------------
def _thin(sc, seen):
    """the scene with only the observations (i, j) for which i is in seen(j)"""
    keep = np.array([int(i) in seen(int(j)) for i, j in zip(sc["obs_image"], sc["obs_point"])], bool)
    out = dict(sc)
    for k in ("obs_image", "obs_point", "obs_xy"):
        out[k] = sc[k][keep]
    return out


def local_scene():
    """6 images (0-based 0 .. 5; ids are index + 1), camera 0 for the first five and camera 1 (id 2) for the last; the
    config holds images 1, 2, 3 (ids 2, 3, 4).  Point j (id j + 1) is seen by:
      j % 4 == 0: images 1, 2, 3: only inside, variable
      j % 4 == 1: images 0 .. 4: also outside, constant
      j % 4 == 2: images 2, 3: inside; point 2 (id 3) is listed constant
      j % 4 == 3: images 3, 4: one residual inside and one element outside, constant with a single residual
      point 5 (id 6): images 1, 2, 5 and listed variable: pulls in image 5 and camera 1 as constants
      point 9 (id 10): images 0, 4 only and listed constant: all of its residuals come through constant poses
      point 23 (id 24): image 2 alone: a single-element track (R3), left out"""
    sc = ba_cases.scene(seed=340, nimg=6, npts=24, model=2, cameras="mixed", noise=0.3)

    def seen(j):
        if j == 5:
            return (1, 2, 5)
        if j == 9:
            return (0, 4)
        if j == 23:
            return (2,)
        return {0: (1, 2, 3), 1: (0, 1, 2, 3, 4), 2: (2, 3), 3: (3, 4)}[j % 4]
    return _thin(sc, seen)


def local_config(pc):
    cfg = pc.BundleAdjustmentConfig()
    for iid in (2, 3, 4):
        cfg.add_image(iid)
    cfg.add_variable_point(6)
    cfg.add_constant_point(3)
    cfg.add_constant_point(10)
    cfg.set_constant_cam_positions(3, [0])
    return cfg


def pose_only_scene():
    """refining new images against an existing map: every point constant by listing, images 2 and 3 (ids 3, 4) variable"""
    return ba_cases.scene(seed=341, nimg=5, npts=30, models=[_M["SIMPLE_RADIAL"], _M["OPENCV"]],
                          image_cameras=[0, 0, 1, 1, 0], noise=0.3)


def pose_only_config(pc):
    cfg = pc.BundleAdjustmentConfig()
    cfg.add_image(3)
    cfg.add_image(4)
    for j in range(30):
        cfg.add_constant_point(j + 1)
    cfg.set_constant_cam_intrinsics(2)
    return cfg


def structure_only_scene():
    return ba_cases.scene(seed=342, nimg=4, npts=20, model=1, noise=0.3)


def structure_only_config(pc):
    """structure-only refinement of selected points: no image, the even points listed variable"""
    cfg = pc.BundleAdjustmentConfig()
    for j in range(0, 20, 2):
        cfg.add_variable_point(j + 1)
    return cfg


SCENES = {"local": (local_scene, local_config, dict(max_num_iterations=4)),
          "pose_only": (pose_only_scene, pose_only_config, dict(max_num_iterations=4)),
          "structure_only": (structure_only_scene, structure_only_config, dict(max_num_iterations=3))}


def adjuster(pc, name):
    """(reconstruction, BundleAdjuster) of a scene"""
    make_scene, make_config, solver = SCENES[name]
    o = pc.BundleAdjustmentOptions()
    for k, v in solver.items():
        setattr(o.solver_options, k, v)
    return ba_cases.reconstruction(make_scene()), pc.BundleAdjuster(o, make_config(pc))


FLAT_KEYS = ("camera_models", "camera_params", "camera_const", "image_cameras", "qvec", "tvec", "pose_const", "xyz",
             "obs_image", "obs_point", "obs_xy")


def flat_args(d):
    """Context.bundle_adjust's positional arguments from BundleAdjuster._problem's dict"""
    a = [np.asarray(d[k]) for k in FLAT_KEYS]
    a[0], a[3], a[8], a[9] = a[0].reshape(-1), a[3].reshape(-1), a[8].reshape(-1), a[9].reshape(-1)
    return tuple(a)


def reference_solver(ref):
    """the callable BundleAdjuster._solve_with takes, running the reference module `ref`"""
    def solve(d):
        return ref.bundle_adjust(*flat_args(d), options=dict(d["options"]), point_const=np.asarray(d["point_const"]).reshape(-1))
    return solve


def model_bits(r):
    """every number of the reconstruction as bytes, keyed by kind and id"""
    out = {}
    for cid, c in r.cameras.items():
        out["camera", cid] = np.asarray(c.params, np.float64).tobytes()
    for iid, im in r.images.items():
        out["image", iid] = (np.asarray(im.cam_from_world.rotation.quat, np.float64).tobytes() +
                             np.asarray(im.cam_from_world.translation, np.float64).tobytes())
    for pid, p in r.points3D.items():
        out["point", pid] = np.asarray(p.xyz, np.float64).tobytes()
    return out
