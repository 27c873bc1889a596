"""Absolute pose with the camera refined: refine_absolute_pose and estimate_and_refine_absolute_pose, the names later
pycolmap releases bind for COLMAP's RefineAbsolutePose / EstimateAndRefineAbsolutePose (the reference binding in the
tree, pycolmap 0.6, calls them pose_refinement / absolute_pose_estimation; the spellings are to confirm, DESIGN.md
25.7), and register_next_image_and_refine, the registration of COLMAP's IncrementalMapper::RegisterNextImage with the
intrinsics of a camera that has no registered image yet refined together with the pose.

pose_refinement and absolute_pose_estimation keep refusing refine_focal_length / refine_extra_params (DESIGN.md 12,
A11); the functions here honour them, through Context.refine_poses_and_cameras / estimate_poses_and_cameras (libamc.so,
csrc/absrefine.hip).  The camera is updated in place on success and untouched otherwise."""
from __future__ import annotations

import time

import numpy as np

from . import _capi, _pycolmap

_last = {}


def last_run_stats() -> dict:
    """What the last call of this module did: entry, success, num_correspondences, num_inliers, focal_factor, device_ms,
    kernel_ms, total_ms."""
    return dict(_last)


def _check(cond, what, a, b):
    if not cond:
        raise ValueError(f"[_pose_intrinsics.py] Check Failed: {what} ({a} vs. {b})")


def _rows(obj, cols, name):
    try:
        a = np.ascontiguousarray(obj, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be convertible to an N x {cols} array") from None
    if a.size == 0:
        return np.zeros((0, cols))
    if a.ndim != 2 or a.shape[1] != cols:
        raise ValueError(f"{name} must be an N x {cols} array")
    return a


def _refinement(options):
    if options is None:
        options = _pycolmap.AbsolutePoseRefinementOptions()
    elif isinstance(options, dict):
        options = _pycolmap.AbsolutePoseRefinementOptions(options)
    elif not isinstance(options, _pycolmap.AbsolutePoseRefinementOptions):
        raise TypeError(f"refinement_options: AbsolutePoseRefinementOptions or a dict is needed, not {type(options).__name__}")
    d = options.todict()
    return dict(gradient_tolerance=float(d["gradient_tolerance"]), max_num_iterations=int(d["max_num_iterations"]),
                loss_function_scale=float(d["loss_function_scale"]), refine_focal_length=int(d["refine_focal_length"]),
                refine_extra_params=int(d["refine_extra_params"]), print_summary=int(d["print_summary"]))


def _estimation(options):
    if options is None:
        options = _pycolmap.AbsolutePoseEstimationOptions()
    elif isinstance(options, dict):
        options = _pycolmap.AbsolutePoseEstimationOptions(options)
    elif not isinstance(options, _pycolmap.AbsolutePoseEstimationOptions):
        raise TypeError(f"estimation_options: AbsolutePoseEstimationOptions or a dict is needed, not {type(options).__name__}")
    d = options.todict()
    r = d["ransac"]
    return dict(estimate_focal_length=int(d["estimate_focal_length"]),
                num_focal_length_samples=int(d["num_focal_length_samples"]),
                min_focal_length_ratio=float(d["min_focal_length_ratio"]),
                max_focal_length_ratio=float(d["max_focal_length_ratio"]), max_error=float(r["max_error"]),
                min_inlier_ratio=float(r["min_inlier_ratio"]), confidence=float(r["confidence"]),
                dyn_num_trials_multiplier=float(r["dyn_num_trials_multiplier"]), min_num_trials=int(r["min_num_trials"]),
                max_num_trials=int(r["max_num_trials"]))


def _camera(camera):
    if not isinstance(camera, _pycolmap.Camera):
        raise TypeError(f"camera: a Camera is needed, not {type(camera).__name__}")
    params = np.array(camera.params, np.float64).reshape(-1)
    if params.size > 12:
        raise ValueError(f"camera: {params.size} parameters (at most 12)")
    return int(camera.model), params


def _pose(r):
    return _pycolmap.Rigid3d(_pycolmap.Rotation3d(np.array(r["qvec"][0])), np.array(r["tvec"][0]))


def _record(entry, t0, r, n):
    _last.clear()
    _last.update(entry=entry, success=bool(r["success"][0]), num_correspondences=int(n),
                 num_inliers=int(r["num_inliers"][0]), focal_factor=float(r["focal_factor"][0]),
                 device_ms=float(r["device_ms"]), kernel_ms=float(r["kernel_ms"]),
                 total_ms=(time.perf_counter() - t0) * 1e3)
    _pycolmap._last_stats = dict(_last)


def refine_absolute_pose(cam_from_world, points2D, points3D, inlier_mask, camera, refinement_options=None,
                         return_covariance=False):
    """RefineAbsolutePose on the GPU with refine_focal_length / refine_extra_params honoured.
    Returns None, or {"cam_from_world"[, "covariance"]} (the 6 x 6 pose block of the joint covariance, rotation first).
    camera.params is updated in place on success and untouched on None.  Without a GPU it raises."""
    t0 = time.perf_counter()
    ro = _refinement(refinement_options)
    if not isinstance(cam_from_world, _pycolmap.Rigid3d):
        raise TypeError(f"cam_from_world: a Rigid3d is needed, not {type(cam_from_world).__name__}")
    p2, p3 = _rows(points2D, 2, "points2D"), _rows(points3D, 3, "points3D")
    try:
        mask = np.ascontiguousarray(inlier_mask, dtype=bool).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("inlier_mask must be convertible to a boolean array") from None
    n = p2.shape[0]
    _check(n == p3.shape[0], "points2D.size() == points3D.size()", n, p3.shape[0])
    _check(mask.size == n, "inlier_mask.size() == points2D.size()", mask.size, n)
    model, params = _camera(camera)
    with _capi.Context(0) as ctx:
        r = ctx.refine_poses_and_cameras([0, n], [model], [params], p2, p3, np.array(cam_from_world.rotation.quat),
                                         np.array(cam_from_world.translation), mask, ro, return_covariance)
    _record("refine_absolute_pose", t0, r, n)
    if not r["success"][0]:
        return None
    camera.params = r["camera_params"][0, :params.size].copy()
    out = {"cam_from_world": _pose(r)}
    if return_covariance:
        out["covariance"] = r["covariance"][0].copy()
    return out


def estimate_and_refine_absolute_pose(points2D, points3D, camera, estimation_options=None, refinement_options=None,
                                      return_covariance=False):
    """EstimateAndRefineAbsolutePose on the GPU: LO-RANSAC per focal-length factor, then one joint refinement of the
    RANSAC's pose and the scaled camera.  Returns None, or {"cam_from_world", "num_inliers",
    "inlier_mask"[, "covariance"]}.  The camera is scaled and refined in place on success and untouched on None.
    Without a GPU it raises."""
    t0 = time.perf_counter()
    eo, ro = _estimation(estimation_options), _refinement(refinement_options)
    p2, p3 = _rows(points2D, 2, "points2D"), _rows(points3D, 3, "points3D")
    n = p2.shape[0]
    _check(n == p3.shape[0], "points2D.size() == points3D.size()", n, p3.shape[0])
    model, params = _camera(camera)
    with _capi.Context(0) as ctx:
        r = ctx.estimate_poses_and_cameras([0, n], [model], [params], p2, p3, eo, ro, return_covariance)
    _record("estimate_and_refine_absolute_pose", t0, r, n)
    if not r["success"][0]:
        return None
    camera.params = r["camera_params"][0, :params.size].copy()
    out = {"cam_from_world": _pose(r), "num_inliers": int(r["num_inliers"][0]), "inlier_mask": r["inlier_mask"].copy()}
    if return_covariance:
        out["covariance"] = r["covariance"][0].copy()
    return out


def _registration_solver(estimate):
    """The solver of IncrementalMapper._register_next_image_with that refines the camera with the pose: `estimate` is
    Context.estimate_poses_and_cameras or a function of its form."""
    def solver(d):
        n = len(d["points2D"])
        est = {k: (int(v) if isinstance(v, (bool, np.bool_)) else v) for k, v in dict(d["estimation"]).items()}
        rf = {k: int(bool(v)) for k, v in dict(d["refinement"]).items()}
        r = estimate([0, n], [int(d["camera_model"])], [np.asarray(d["camera_params"], np.float64).reshape(-1)],
                     d["points2D"], d["points3D"], est, rf, False)
        return dict(success=bool(r["success"][0]), qvec=r["qvec"][0], tvec=r["tvec"][0],
                    num_inliers=int(r["num_inliers"][0]), focal_factor=float(r["focal_factor"][0]),
                    inlier_mask=np.asarray(r["inlier_mask"]).astype(np.uint8),
                    camera_params=np.ascontiguousarray(r["camera_params"][0], dtype=np.float64))
    return solver


def register_next_image_and_refine(mapper, options, image_id):
    """IncrementalMapper.register_next_image with the camera refined as COLMAP's RegisterNextImage does it: the
    registration rule's estimation options and its refine_focal_length / refine_extra_params flags (a camera that has a
    registered image keeps its intrinsics) go to Context.estimate_poses_and_cameras, and the refined camera replaces
    the reconstruction's.  Returns what register_next_image returns, with the same trial counting; False (a failed
    refinement included) changes nothing but the trial count.  Without a GPU it raises."""
    with _capi.Context(0) as ctx:
        return mapper._register_next_image_with(options, image_id, _registration_solver(ctx.estimate_poses_and_cameras))


def _register_next_image_and_refine_with(mapper, options, image_id, estimate):
    """register_next_image_and_refine with a function of Context.estimate_poses_and_cameras' form in the library's
    place (test hook)."""
    return mapper._register_next_image_with(options, image_id, _registration_solver(estimate))
