"""ctypes view of libamc.so's C ABI (include/amc.h).

Thin by design: every function here maps 1:1 to an `amc_*` entry point; no computation happens
in Python and there is no fallback — if libamc.so is missing or no gfx950 device is visible the
calls raise.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "libamc.so"

AMC_OK = 0
AMC_E_INVALID, AMC_E_HIP, AMC_E_NOMEM, AMC_E_STATE = -1, -2, -3, -4
KERNEL_AUTO, KERNEL_MFMA, KERNEL_DOT4 = 0, 1, 2
KERNELS = {"auto": KERNEL_AUTO, "mfma": KERNEL_MFMA, "dot4": KERNEL_DOT4}

# every symbol include/amc.h declares (tests check the library exports all of them)
EXPORTED_SYMBOLS = [
    "amc_last_error", "amc_abi_version", "amc_device_count", "amc_ctx_create", "amc_ctx_destroy",
    "amc_ctx_set_stream", "amc_ctx_reserve_slots", "amc_upload_descriptors",
    "amc_upload_descriptors_device", "amc_match_pairs", "amc_match_result_free",
    "amc_match_opts_default", "amc_get_acos_lut",
    "amc_tvg_opts_default", "amc_upload_keypoints", "amc_upload_camera", "amc_verify_pairs",
    "amc_verify_result_free", "amc_upload_points_f64", "amc_ransac_pairs", "amc_ransac_result_free",
    "amc_squared_sampson_error", "amc_match_guided_pairs", "amc_ctx_grow_slots", "amc_pose_pairs",
    "amc_cam_from_img", "amc_match_verify_pairs", "amc_ctx_trim", "amc_ctx_resident_matches",
    "amc_homography_decomposition", "amc_img_from_cam",
    "amc_comm_unique_id", "amc_comm_create", "amc_comm_destroy", "amc_allgather_match_tables", "amc_gathered_tables_free",
    "amc_allgather_pair_records", "amc_gathered_records_free", "amc_allgather_inlier_tables", "amc_ctx_last_timeline",
    "amc_upload_matches",
    "amc_estimate_rig_absolute_poses", "amc_rigpose_result_free",
    "amc_undistort_opts_default", "amc_undistort_camera", "amc_undistort_points", "amc_undistort_images",
    "amc_ba_opts_default", "amc_bundle_adjust", "amc_bundle_adjust_masked",
    "amc_bacov_opts_default", "amc_ba_covariance", "amc_bacov_result_free",
    "amc_filter_opts_default", "amc_filter_points3d", "amc_filter_result_free",
    "amc_triobs_opts_default", "amc_triangulate_observations", "amc_triobs_result_free",
    "amc_complete_opts_default", "amc_complete_tracks", "amc_complete_result_free",
    "amc_merge_opts_default", "amc_merge_tracks", "amc_merge_result_free",
    "amc_retri_opts_default", "amc_retriangulate_pairs", "amc_retri_result_free",
    "amc_image_visibility", "amc_visibility_result_free",
    "amc_pair_angle_opts_default", "amc_shared_point_angles", "amc_pair_angle_result_free",
    "amc_pair_tri_opts_default", "amc_triangulate_pairs", "amc_pair_tri_result_free",
    "amc_patch_match_opts_default", "amc_patch_match", "amc_patch_match_result_free",
    "amc_fusion_opts_default", "amc_fuse_depth_maps", "amc_fusion_result_free",
    "amc_refine_poses_and_cameras", "amc_estimate_poses_and_cameras", "amc_absrefine_result_free",
]
COMM_ID_BYTES = 128
RANSAC_F, RANSAC_H, RANSAC_E = 0, 1, 2
RANSAC_KINDS = {"F": RANSAC_F, "H": RANSAC_H, "E": RANSAC_E}


class _MatchLease:
    """Owns one amc_match_result; frees it when the arrays viewing it are gone."""

    def __init__(self, lib, res):
        self._lib, self._res = lib, res

    def __del__(self):
        try:
            self._lib.amc_match_result_free(C.byref(self._res))
        except Exception:  # interpreter shutdown
            pass


class _VerifyLease:
    """Owns one amc_verify_result; frees it when the arrays viewing it are gone."""

    def __init__(self, lib, res):
        self._lib, self._res = lib, res

    def __del__(self):
        try:
            self._lib.amc_verify_result_free(C.byref(self._res))
        except Exception:  # interpreter shutdown
            pass


class _LeasedArray(np.ndarray):
    """ndarray view that keeps its lease alive (numpy views of it inherit the reference through .base)."""

    @staticmethod
    def wrap(arr, lease):
        out = arr.view(_LeasedArray)
        out._lease = lease
        return out

    def __array_finalize__(self, obj):
        self._lease = getattr(obj, "_lease", None)


class AmcError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"amc error {code}: {msg}")
        self.code = code


class GatheredTables(C.Structure):
    """amc_gathered_tables (include/amc.h)."""
    _fields_ = [("npairs", C.c_size_t), ("offsets", C.POINTER(C.c_uint64)), ("matches", C.POINTER(C.c_uint32)),
                ("matches_device", C.c_void_p), ("num_matches", C.c_uint64), ("rows_sent", C.c_uint64),
                ("rows_received", C.c_uint64), ("world_size", C.c_int32), ("rank", C.c_int32),
                ("sizes_ms", C.c_double), ("meta_ms", C.c_double), ("rows_ms", C.c_double), ("reorder_ms", C.c_double),
                ("download_ms", C.c_double), ("total_ms", C.c_double), ("_priv", C.c_void_p)]


class GatheredRecords(C.Structure):
    """amc_gathered_records (include/amc.h)."""
    _fields_ = [("npairs", C.c_size_t), ("record_bytes", C.c_size_t), ("records", C.c_void_p), ("records_device", C.c_void_p),
                ("bytes_sent", C.c_uint64), ("bytes_received", C.c_uint64), ("world_size", C.c_int32), ("rank", C.c_int32),
                ("total_ms", C.c_double), ("_priv", C.c_void_p)]


class MatchOpts(C.Structure):
    _fields_ = [("max_ratio", C.c_double), ("max_distance", C.c_double),
                ("cross_check", C.c_int32), ("kernel", C.c_int32)]


class MatchResult(C.Structure):
    _fields_ = [("npairs", C.c_size_t), ("offsets", C.POINTER(C.c_uint64)),
                ("matches", C.POINTER(C.c_uint32)), ("num_distances", C.c_uint64),
                ("pairs_mfma", C.c_uint64), ("pairs_dot4", C.c_uint64), ("pairs_guided_grid", C.c_uint64),
                ("device_ms", C.c_double), ("match_kernel_ms", C.c_double),
                ("cross_kernel_ms", C.c_double),
                ("match_kernel_launches", C.c_uint32), ("scan_run", C.c_uint32), ("_priv", C.c_void_p)]


class SiftOpts(C.Structure):  # amc_sift_opts (include/amc_sift.h)
    _fields_ = [("first_octave", C.c_int32), ("num_octaves", C.c_int32), ("octave_resolution", C.c_int32),
                ("peak_threshold", C.c_double), ("edge_threshold", C.c_double), ("max_num_orientations", C.c_int32),
                ("upright", C.c_int32), ("normalization", C.c_int32), ("max_num_features", C.c_int32),
                ("max_image_size", C.c_int32)]


class SiftImage(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("pitch", C.c_int64)]


class SiftResult(C.Structure):
    _fields_ = [("nimages", C.c_size_t), ("offsets", C.POINTER(C.c_uint64)), ("keypoints", C.POINTER(C.c_float)),
                ("descriptors", C.POINTER(C.c_uint8)), ("device_ms", C.c_double), ("stage_ms", C.c_double * 4),
                ("_priv", C.c_void_p)]


class AbsPoseOpts(C.Structure):  # amc_abspose_opts (include/amc_abspose.h)
    _fields_ = [("estimate_focal_length", C.c_int32), ("num_focal_length_samples", C.c_int32),
                ("min_focal_length_ratio", C.c_double), ("max_focal_length_ratio", C.c_double),
                ("max_error", C.c_double), ("min_inlier_ratio", C.c_double), ("confidence", C.c_double),
                ("dyn_num_trials_multiplier", C.c_double), ("min_num_trials", C.c_int64),
                ("max_num_trials", C.c_int64)]


class AbsPoseRefineOpts(C.Structure):  # amc_abspose_refine_opts
    _fields_ = [("gradient_tolerance", C.c_double), ("max_num_iterations", C.c_int64),
                ("loss_function_scale", C.c_double), ("refine_focal_length", C.c_int32),
                ("refine_extra_params", C.c_int32), ("print_summary", C.c_int32)]


class AbsPoseResult(C.Structure):
    _fields_ = [("nqueries", C.c_size_t), ("ncorr", C.c_size_t), ("success", C.POINTER(C.c_uint8)),
                ("qvec", C.POINTER(C.c_double)), ("tvec", C.POINTER(C.c_double)),
                ("num_inliers", C.POINTER(C.c_uint32)), ("num_trials", C.POINTER(C.c_uint64)),
                ("focal_factor", C.POINTER(C.c_double)), ("covariance", C.POINTER(C.c_double)),
                ("inlier_mask", C.POINTER(C.c_uint8)), ("device_ms", C.c_double), ("kernel_ms", C.c_double),
                ("num_batches", C.c_uint32), ("_priv", C.c_void_p)]


class AbsRefineResult(C.Structure):  # amc_absrefine_result (include/amc_absrefine.h)
    _fields_ = [("nqueries", C.c_size_t), ("ncorr", C.c_size_t), ("success", C.POINTER(C.c_uint8)),
                ("qvec", C.POINTER(C.c_double)), ("tvec", C.POINTER(C.c_double)),
                ("num_inliers", C.POINTER(C.c_uint32)), ("num_trials", C.POINTER(C.c_uint64)),
                ("focal_factor", C.POINTER(C.c_double)), ("covariance", C.POINTER(C.c_double)),
                ("inlier_mask", C.POINTER(C.c_uint8)), ("camera_params", C.POINTER(C.c_double)),
                ("device_ms", C.c_double), ("kernel_ms", C.c_double), ("num_batches", C.c_uint32),
                ("_priv", C.c_void_p)]


def abspose_options(estimation=None, refinement=None):
    """amc_abspose_opts / amc_abspose_refine_opts at their defaults (the C defaults, no library needed) with the
    given fields replaced; an unknown field raises ValueError."""
    eo, ro = AbsPoseOpts(), AbsPoseRefineOpts()
    for k, v in dict(estimate_focal_length=0, num_focal_length_samples=30, min_focal_length_ratio=0.1,
                     max_focal_length_ratio=10.0, max_error=12.0, min_inlier_ratio=0.01, confidence=0.9999,
                     dyn_num_trials_multiplier=3.0, min_num_trials=1000, max_num_trials=100000).items():
        setattr(eo, k, v)
    for k, v in dict(gradient_tolerance=1.0, max_num_iterations=100, loss_function_scale=1.0, refine_focal_length=0,
                     refine_extra_params=0, print_summary=0).items():
        setattr(ro, k, v)
    for o, given in ((eo, estimation or {}), (ro, refinement or {})):
        for k, v in given.items():
            if k not in dict(type(o)._fields_):
                raise ValueError(f"unknown absolute pose option {k!r}")
            setattr(o, k, type(getattr(o, k))(v))
    return eo, ro


def abspose_inputs(offsets, camera_models, camera_params, points2D, points3D):
    """The CSR batch of amc_estimate_absolute_poses as contiguous arrays: offsets (Q + 1,) uint64, models (Q,) int32,
    params (Q, 12) float64 (each camera's parameters first), points2D (N, 2), points3D (N, 3)."""
    off = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    if off.size < 1:
        raise ValueError("absolute poses: offsets needs nqueries + 1 entries")
    nq, n = off.size - 1, int(off[-1])
    models = np.ascontiguousarray(camera_models, dtype=np.int32).reshape(-1)
    if models.size != nq or len(camera_params) != nq:
        raise ValueError(f"absolute poses: {nq} queries by offsets, {models.size} camera models, "
                         f"{len(camera_params)} parameter sets")
    prm = np.zeros((nq, 12), np.float64)
    for i, p in enumerate(camera_params):
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        if p.size > 12:
            raise ValueError(f"absolute poses: camera {i} has {p.size} parameters (at most 12)")
        prm[i, :p.size] = p
    p2 = np.ascontiguousarray(points2D, dtype=np.float64).reshape(-1, 2)
    p3 = np.ascontiguousarray(points3D, dtype=np.float64).reshape(-1, 3)
    if p2.shape[0] != n or p3.shape[0] != n:
        raise ValueError(f"absolute poses: {n} correspondences by offsets, {p2.shape[0]} points2D, "
                         f"{p3.shape[0]} points3D")
    return off, models, prm, p2, p3


class BaOpts(C.Structure):  # amc_ba_opts (include/amc_ba.h)
    _fields_ = [("loss_function_type", C.c_int32), ("max_num_iterations", C.c_int32),
                ("max_linear_solver_iterations", C.c_int32), ("max_num_consecutive_invalid_steps", C.c_int32),
                ("loss_function_scale", C.c_double), ("function_tolerance", C.c_double),
                ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double)]


class BaProblem(C.Structure):  # amc_ba_problem
    _fields_ = [("num_cameras", C.c_size_t), ("camera_models", C.c_void_p), ("camera_params", C.c_void_p),
                ("camera_const", C.c_void_p), ("num_images", C.c_size_t), ("image_cameras", C.c_void_p),
                ("qvec", C.c_void_p), ("tvec", C.c_void_p), ("pose_const", C.c_void_p), ("num_points", C.c_size_t),
                ("xyz", C.c_void_p), ("num_observations", C.c_size_t), ("obs_image", C.c_void_p),
                ("obs_point", C.c_void_p), ("obs_xy", C.c_void_p)]


class BaResult(C.Structure):  # amc_ba_result
    _fields_ = [("num_images", C.c_uint64), ("num_points", C.c_uint64), ("num_observations", C.c_uint64),
                ("num_variable_parameters", C.c_uint64), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("num_successful_steps", C.c_uint32), ("num_unsuccessful_steps", C.c_uint32),
                ("num_pcg_iterations", C.c_uint32), ("num_pcg_stops_residual", C.c_uint32),
                ("num_pcg_stops_cap", C.c_uint32), ("termination", C.c_int32), ("host_ms", C.c_double),
                ("device_ms", C.c_double), ("kernel_ms", C.c_double)]


BA_LOSSES = {"TRIVIAL": 0, "SOFT_L1": 1, "CAUCHY": 2}
BA_TERMINATIONS = ("FUNCTION_TOLERANCE", "PARAMETER_TOLERANCE", "GRADIENT_TOLERANCE", "MAX_ITERATIONS", "MIN_RADIUS",
                   "INVALID_STEPS", "NOTHING_TO_REFINE")
BA_PCG_TOLERANCE = 1e-8


def ba_options(options=None) -> "BaOpts":
    """amc_ba_opts at its defaults (COLMAP 3.9.1's BundleAdjustmentOptions, no library needed) with the given fields
    replaced; loss_function_type may be a name; an unknown field raises ValueError."""
    o = BaOpts()
    for k, v in dict(loss_function_type=0, max_num_iterations=100, max_linear_solver_iterations=200,
                     max_num_consecutive_invalid_steps=10, loss_function_scale=1.0, function_tolerance=0.0,
                     gradient_tolerance=0.0, parameter_tolerance=0.0).items():
        setattr(o, k, v)
    for k, v in (options or {}).items():
        if k not in dict(BaOpts._fields_):
            raise ValueError(f"unknown bundle adjustment option {k!r}")
        if k == "loss_function_type" and isinstance(v, str):
            if v.upper() not in BA_LOSSES:
                raise ValueError(f"unknown loss function type {v!r}")
            v = BA_LOSSES[v.upper()]
        setattr(o, k, type(getattr(o, k))(v))
    return o


def ba_inputs(camera_models, camera_params, camera_const, image_cameras, qvec, tvec, pose_const, xyz, obs_image,
              obs_point, obs_xy):
    """The flat problem of amc_bundle_adjust as contiguous arrays (copies: the caller's arrays are not touched):
    models (C,) int32, params (C, 12), camera_const (C, 12) uint8, image_cameras (I,) uint32, qvec (I, 4) x y z w,
    tvec (I, 3), pose_const (I, 6) uint8, xyz (P, 3), obs_image / obs_point (N,) uint32, obs_xy (N, 2)."""
    models = np.array(camera_models, dtype=np.int32).reshape(-1)
    nc = models.size
    if len(camera_params) != nc:
        raise ValueError(f"bundle adjustment: {nc} camera models, {len(camera_params)} parameter sets")
    prm = np.zeros((nc, 12), np.float64)
    for i, p in enumerate(camera_params):
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        if p.size > 12:
            raise ValueError(f"bundle adjustment: camera {i} has {p.size} parameters (at most 12)")
        prm[i, :p.size] = p
    cc = np.ones((nc, 12), np.uint8)
    for i, m in enumerate(camera_const):
        m = np.asarray(m).reshape(-1)
        cc[i, :min(m.size, 12)] = m[:12] != 0
    icam = np.array(image_cameras, dtype=np.int64).reshape(-1)
    ni = icam.size
    q = np.array(qvec, dtype=np.float64).reshape(-1, 4)
    t = np.array(tvec, dtype=np.float64).reshape(-1, 3)
    pc = (np.array(pose_const).reshape(-1, 6) != 0).astype(np.uint8)
    X = np.array(xyz, dtype=np.float64).reshape(-1, 3)
    oi = np.array(obs_image, dtype=np.int64).reshape(-1)
    op = np.array(obs_point, dtype=np.int64).reshape(-1)
    xy = np.array(obs_xy, dtype=np.float64).reshape(-1, 2)
    if q.shape[0] != ni or t.shape[0] != ni or pc.shape[0] != ni or op.size != oi.size or xy.shape[0] != oi.size:
        raise ValueError(f"bundle adjustment: {ni} images by image_cameras, {q.shape[0]} rotations, {t.shape[0]} "
                         f"translations, {pc.shape[0]} pose masks; {oi.size} observations by obs_image, {op.size} "
                         f"point indices, {xy.shape[0]} pixels")
    for name, a in (("image_cameras", icam), ("obs_image", oi), ("obs_point", op)):
        if a.size and (a.min() < 0 or a.max() > 0xffffffff):
            raise ValueError(f"bundle adjustment: {name} has an index outside 0 .. 2^32 - 1")
    return (models, prm, cc, icam.astype(np.uint32), q, t, pc, X, oi.astype(np.uint32), op.astype(np.uint32), xy)


class BacovOpts(C.Structure):  # amc_bacov_opts (include/amc_bacov.h)
    _fields_ = [("loss_function_type", C.c_int32), ("want_points", C.c_int32), ("want_matrix", C.c_int32),
                ("reserved", C.c_int32), ("loss_function_scale", C.c_double), ("damping", C.c_double)]


class BacovResult(C.Structure):  # amc_bacov_result
    _fields_ = [("success", C.c_int32), ("reserved", C.c_int32), ("failed_column", C.c_int64),
                ("num_columns", C.c_uint64), ("num_points", C.c_uint64), ("min_pivot_ratio", C.c_double),
                ("column_owner", C.POINTER(C.c_uint32)), ("column_coord", C.POINTER(C.c_uint32)),
                ("matrix", C.POINTER(C.c_double)), ("point_present", C.POINTER(C.c_uint8)),
                ("point_cov", C.POINTER(C.c_double)), ("host_ms", C.c_double), ("device_ms", C.c_double),
                ("kernel_ms", C.c_double), ("copy_ms", C.c_double), ("phase_ms", C.c_double * 5)]


BACOV_MAX_COLUMNS = 8192  # AMC_BACOV_MAX_COLUMNS
BACOV_PHASES = ("evaluation", "formation", "factor", "inverse", "points")


def bacov_options(options=None) -> "BacovOpts":
    """amc_bacov_opts at its defaults (no library needed) with the given fields replaced; loss_function_type may be a
    name; an unknown field or a value the library would refuse raises ValueError."""
    o = BacovOpts(0, 1, 1, 0, 1.0, 1e-8)
    for k, v in (options or {}).items():
        if k not in dict(BacovOpts._fields_) or k == "reserved":
            raise ValueError(f"ba_covariance: unknown option {k!r}")
        if k == "loss_function_type" and isinstance(v, str):
            if v.upper() not in BA_LOSSES:
                raise ValueError(f"ba_covariance: unknown loss function type {v!r}")
            v = BA_LOSSES[v.upper()]
        setattr(o, k, type(getattr(o, k))(v))
    if not 0 <= o.loss_function_type <= 2:
        raise ValueError(f"ba_covariance: loss_function_type {o.loss_function_type} outside 0 .. 2")
    if not (o.loss_function_scale > 0 and np.isfinite(o.loss_function_scale)):
        raise ValueError(f"ba_covariance: loss_function_scale {o.loss_function_scale} is not positive and finite")
    if not (o.damping >= 0 and np.isfinite(o.damping)):
        raise ValueError(f"ba_covariance: damping {o.damping} is not non-negative and finite")
    return o


def bacov_inputs(camera_models, camera_params, camera_const, image_cameras, qvec, tvec, pose_const, xyz, obs_image,
                 obs_point, obs_xy, point_const=None):
    """ba_inputs' arrays plus the point mask (P,) uint8 or None, for amc_ba_covariance; malformed input is a ValueError
    naming ba_covariance."""
    try:
        arrays = ba_inputs(camera_models, camera_params, camera_const, image_cameras, qvec, tvec, pose_const, xyz,
                           obs_image, obs_point, obs_xy)
    except ValueError as e:
        raise ValueError(f"ba_covariance: {e}") from None
    mask = None
    if point_const is not None:
        mask = np.ascontiguousarray(np.asarray(point_const).reshape(-1) != 0, dtype=np.uint8)
        if mask.size != arrays[7].shape[0]:
            raise ValueError(f"ba_covariance: {arrays[7].shape[0]} points, {mask.size} point_const flags")
    return arrays + (mask,)


class FilterOpts(C.Structure):  # amc_filter_opts (include/amc_filter.h)
    _fields_ = [("max_reproj_error", C.c_double), ("min_tri_angle", C.c_double), ("errors_only", C.c_int32),
                ("reserved", C.c_int32)]


class FilterProblem(C.Structure):  # amc_filter_problem
    _fields_ = [("num_cameras", C.c_size_t), ("camera_models", C.c_void_p), ("camera_params", C.c_void_p),
                ("num_images", C.c_size_t), ("image_cameras", C.c_void_p), ("qvec", C.c_void_p), ("tvec", C.c_void_p),
                ("num_points", C.c_size_t), ("xyz", C.c_void_p), ("track_offsets", C.c_void_p),
                ("obs_image", C.c_void_p), ("obs_xy", C.c_void_p), ("selected", C.c_void_p)]


class FilterResult(C.Structure):  # amc_filter_result
    _fields_ = [("num_points", C.c_uint64), ("num_observations", C.c_uint64), ("num_filtered", C.c_uint64),
                ("obs_sq_error", C.POINTER(C.c_double)), ("obs_deleted", C.POINTER(C.c_uint8)),
                ("point_verdict", C.POINTER(C.c_uint8)), ("point_error", C.POINTER(C.c_double)),
                ("num_batches", C.c_uint32), ("reserved", C.c_uint32), ("host_ms", C.c_double),
                ("device_ms", C.c_double), ("kernel_ms", C.c_double), ("copy_ms", C.c_double),
                ("alloc_ms", C.c_double)]


FILTER_VERDICTS = ("KEPT", "NOT_SELECTED", "SHORT_TRACK", "REPROJECTION", "ANGLE")


def filter_inputs(camera_models, camera_params, image_cameras, qvec, tvec, xyz, track_offsets, obs_image, obs_xy,
                  selected=None):
    """The flat problem of amc_filter_points3d as contiguous arrays (copies: the caller's arrays are not touched):
    models (C,) int32, params (C, 12), image_cameras (I,) uint32, qvec (I, 4) x y z w, tvec (I, 3), xyz (P, 3),
    track_offsets (P + 1,) uint64, obs_image (N,) uint32, obs_xy (N, 2), selected (P,) uint8 or None."""
    models = np.array(camera_models, dtype=np.int32).reshape(-1)
    if len(camera_params) != models.size:
        raise ValueError(f"filter_points3d: {models.size} camera models, {len(camera_params)} parameter sets")
    prm = np.zeros((models.size, 12), np.float64)
    for i, p in enumerate(camera_params):
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        if p.size > 12:
            raise ValueError(f"filter_points3d: camera {i} has {p.size} parameters (at most 12)")
        prm[i, :p.size] = p
    icam = np.array(image_cameras, dtype=np.int64).reshape(-1)
    q = np.array(qvec, dtype=np.float64).reshape(-1, 4)
    t = np.array(tvec, dtype=np.float64).reshape(-1, 3)
    X = np.array(xyz, dtype=np.float64).reshape(-1, 3)
    off = np.array(track_offsets, dtype=np.int64).reshape(-1)
    oi = np.array(obs_image, dtype=np.int64).reshape(-1)
    xy = np.array(obs_xy, dtype=np.float64).reshape(-1, 2)
    if q.shape[0] != icam.size or t.shape[0] != icam.size or off.size != X.shape[0] + 1 or xy.shape[0] != oi.size:
        raise ValueError(f"filter_points3d: {icam.size} images by image_cameras, {q.shape[0]} rotations, {t.shape[0]} "
                         f"translations; {X.shape[0]} points, {off.size} offsets; {oi.size} observations by obs_image, "
                         f"{xy.shape[0]} pixels")
    if off.min() < 0 or int(off[-1]) != oi.size:
        raise ValueError(f"filter_points3d: track_offsets ends at {int(off[-1])}, {oi.size} observations")
    for name, a in (("image_cameras", icam), ("obs_image", oi)):
        if a.size and (a.min() < 0 or a.max() > 0xffffffff):
            raise ValueError(f"filter_points3d: {name} has an index outside 0 .. 2^32 - 1")
    sel = None
    if selected is not None:
        sel = np.ascontiguousarray(np.asarray(selected).reshape(-1) != 0, dtype=np.uint8)
        if sel.size != X.shape[0]:
            raise ValueError(f"filter_points3d: {X.shape[0]} points, {sel.size} selection flags")
    return models, prm, icam.astype(np.uint32), q, t, X, off.astype(np.uint64), oi.astype(np.uint32), xy, sel


class TriobsOpts(C.Structure):  # amc_triobs_opts (include/amc_triobs.h)
    _fields_ = [("create_max_angle_error", C.c_double), ("continue_max_angle_error", C.c_double),
                ("min_angle", C.c_double), ("reserved", C.c_double)]


class TriobsProblem(C.Structure):  # amc_triobs_problem
    _fields_ = [("num_cameras", C.c_size_t), ("camera_models", C.c_void_p), ("camera_params", C.c_void_p),
                ("num_images", C.c_size_t), ("image_cameras", C.c_void_p), ("qvec", C.c_void_p), ("tvec", C.c_void_p),
                ("num_items", C.c_size_t), ("item_offsets", C.c_void_p), ("cand_image", C.c_void_p),
                ("cand_xy", C.c_void_p), ("cand_has_point", C.c_void_p), ("cand_xyz", C.c_void_p),
                ("no_create_two_view", C.c_void_p)]


class TriobsResult(C.Structure):  # amc_triobs_result
    _fields_ = [("num_items", C.c_uint64), ("num_candidates", C.c_uint64), ("num_created", C.c_uint64),
                ("num_continued", C.c_uint64), ("continued", C.POINTER(C.c_int32)),
                ("cand_round", C.POINTER(C.c_uint32)), ("round_offsets", C.POINTER(C.c_uint64)),
                ("round_xyz", C.POINTER(C.c_double)), ("num_batches", C.c_uint32), ("reserved", C.c_uint32),
                ("host_ms", C.c_double), ("device_ms", C.c_double), ("kernel_ms", C.c_double), ("copy_ms", C.c_double),
                ("alloc_ms", C.c_double)]


def triobs_inputs(camera_models, camera_params, image_cameras, qvec, tvec, item_offsets, cand_image, cand_xy,
                  cand_has_point, cand_xyz, no_create_two_view=None):
    """The flat problem of amc_triangulate_observations as contiguous arrays (copies: the caller's arrays are not
    touched): models (C,) int32, params (C, 12), image_cameras (I,) uint32, qvec (I, 4) x y z w, tvec (I, 3),
    item_offsets (T + 1,) uint64, cand_image (N,) uint32, cand_xy (N, 2), cand_has_point (N,) uint8, cand_xyz (N, 3),
    no_create_two_view (T,) uint8 or None."""
    who = "triangulate_observations"
    models = np.array(camera_models, dtype=np.int32).reshape(-1)
    if len(camera_params) != models.size:
        raise ValueError(f"{who}: {models.size} camera models, {len(camera_params)} parameter sets")
    prm = np.zeros((models.size, 12), np.float64)
    for i, p in enumerate(camera_params):
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        if p.size > 12:
            raise ValueError(f"{who}: camera {i} has {p.size} parameters (at most 12)")
        prm[i, :p.size] = p
    icam = np.array(image_cameras, dtype=np.int64).reshape(-1)
    q = np.array(qvec, dtype=np.float64).reshape(-1, 4)
    t = np.array(tvec, dtype=np.float64).reshape(-1, 3)
    off = np.array(item_offsets, dtype=np.int64).reshape(-1)
    ci = np.array(cand_image, dtype=np.int64).reshape(-1)
    xy = np.array(cand_xy, dtype=np.float64).reshape(-1, 2)
    has = np.ascontiguousarray(np.asarray(cand_has_point).reshape(-1) != 0, dtype=np.uint8)
    X = np.array(cand_xyz, dtype=np.float64).reshape(-1, 3)
    if q.shape[0] != icam.size or t.shape[0] != icam.size or off.size < 1 or not (xy.shape[0] == has.size == X.shape[0] == ci.size):
        raise ValueError(f"{who}: {icam.size} images by image_cameras, {q.shape[0]} rotations, {t.shape[0]} translations; "
                         f"{off.size} offsets; {ci.size} candidates by cand_image, {xy.shape[0]} pixels, {has.size} flags, "
                         f"{X.shape[0]} points")
    if off.min() < 0 or int(off[-1]) != ci.size:
        raise ValueError(f"{who}: item_offsets ends at {int(off[-1])}, {ci.size} candidates")
    for name, a in (("image_cameras", icam), ("cand_image", ci)):
        if a.size and (a.min() < 0 or a.max() > 0xffffffff):
            raise ValueError(f"{who}: {name} has an index outside 0 .. 2^32 - 1")
    two = None
    if no_create_two_view is not None:
        two = np.ascontiguousarray(np.asarray(no_create_two_view).reshape(-1) != 0, dtype=np.uint8)
        if two.size != off.size - 1:
            raise ValueError(f"{who}: {off.size - 1} items, {two.size} two-view flags")
    return models, prm, icam.astype(np.uint32), q, t, off.astype(np.uint64), ci.astype(np.uint32), xy, has, X, two


class RetriOpts(C.Structure):  # amc_retri_opts (include/amc_retri.h)
    _fields_ = [("create_max_angle_error", C.c_double), ("re_max_angle_error", C.c_double), ("min_angle", C.c_double),
                ("re_min_ratio", C.c_double)]


class RetriProblem(C.Structure):  # amc_retri_problem
    _fields_ = [("num_cameras", C.c_size_t), ("camera_models", C.c_void_p), ("camera_params", C.c_void_p),
                ("num_images", C.c_size_t), ("image_cameras", C.c_void_p), ("qvec", C.c_void_p), ("tvec", C.c_void_p),
                ("num_obs", C.c_size_t), ("obs_image", C.c_void_p), ("obs_xy", C.c_void_p), ("obs_point", C.c_void_p),
                ("num_points", C.c_size_t), ("point_xyz", C.c_void_p),
                ("num_pairs", C.c_size_t), ("pair_images", C.c_void_p), ("pair_offsets", C.c_void_p),
                ("corr_obs", C.c_void_p), ("corr_two_view", C.c_void_p),
                ("num_rounds", C.c_size_t), ("round_offsets", C.c_void_p)]


class RetriResult(C.Structure):  # amc_retri_result
    _fields_ = [("num_pairs", C.c_uint64), ("num_corrs", C.c_uint64), ("num_pairs_run", C.c_uint64),
                ("num_continued", C.c_uint64), ("num_created", C.c_uint64), ("pair_ran", C.POINTER(C.c_uint8)),
                ("pair_num_tri", C.POINTER(C.c_uint32)), ("corr_action", C.POINTER(C.c_uint8)),
                ("created_offsets", C.POINTER(C.c_uint64)), ("created_xyz", C.POINTER(C.c_double)),
                ("num_launches", C.c_uint32), ("reserved", C.c_uint32),
                ("host_ms", C.c_double), ("device_ms", C.c_double), ("kernel_ms", C.c_double), ("copy_ms", C.c_double),
                ("alloc_ms", C.c_double)]


class VisibilityProblem(C.Structure):  # amc_visibility_problem (include/amc_mapper.h)
    _fields_ = [("num_graph_images", C.c_size_t), ("image_point_offsets", C.c_void_p), ("point2D_point3D", C.c_void_p),
                ("num_candidates", C.c_size_t), ("cand_width", C.c_void_p), ("cand_height", C.c_void_p),
                ("cand_point_offsets", C.c_void_p), ("cand_xy", C.c_void_p), ("corr_offsets", C.c_void_p),
                ("corr_image", C.c_void_p), ("corr_point2D", C.c_void_p)]


class VisibilityResult(C.Structure):  # amc_visibility_result
    _fields_ = [("num_candidates", C.c_uint64), ("num_observations", C.POINTER(C.c_uint32)),
                ("num_visible_points3D", C.POINTER(C.c_uint32)), ("score", C.POINTER(C.c_uint64)),
                ("max_score", C.c_uint64), ("num_batches", C.c_uint32), ("reserved", C.c_uint32),
                ("host_ms", C.c_double), ("device_ms", C.c_double), ("kernel_ms", C.c_double), ("copy_ms", C.c_double),
                ("alloc_ms", C.c_double)]


class PairAngleOpts(C.Structure):  # amc_pair_angle_opts
    _fields_ = [("percentile", C.c_double)]


class PairAngleProblem(C.Structure):  # amc_pair_angle_problem
    _fields_ = [("num_images", C.c_size_t), ("qvec", C.c_void_p), ("tvec", C.c_void_p),
                ("num_points", C.c_size_t), ("point_xyz", C.c_void_p),
                ("num_pairs", C.c_size_t), ("pair_images", C.c_void_p), ("pair_offsets", C.c_void_p),
                ("shared_points", C.c_void_p)]


class PairAngleResult(C.Structure):  # amc_pair_angle_result
    _fields_ = [("num_pairs", C.c_uint64), ("angle", C.POINTER(C.c_double)), ("num_batches", C.c_uint32),
                ("reserved", C.c_uint32), ("host_ms", C.c_double), ("device_ms", C.c_double), ("kernel_ms", C.c_double),
                ("copy_ms", C.c_double), ("alloc_ms", C.c_double)]


MAPPER_NO_POINT3D = (1 << 64) - 1
MAPPER_MAX_SCORE = 17895696
MAPPER_MAX_PAIR_POINTS = 1 << 20


def _u32_index(who, name, a):
    a = np.array(a, dtype=np.int64).reshape(-1)
    if a.size and (a.min() < 0 or a.max() > 0xffffffff):
        raise ValueError(f"{who}: {name} has a value outside 0 .. 2^32 - 1")
    return a.astype(np.uint32)


def _offsets(who, name, a):
    a = np.array(a, dtype=np.int64).reshape(-1)
    if a.size < 1 or a.min() < 0:
        raise ValueError(f"{who}: {name} needs at least one entry, none negative")
    return a.astype(np.uint64)


def visibility_inputs(image_point_offsets, point2D_point3D, cand_width, cand_height, cand_point_offsets, cand_xy,
                      corr_offsets, corr_image, corr_point2D):
    """The flat problem of amc_image_visibility as contiguous arrays (copies): image_point_offsets (G + 1,) uint64,
    point2D_point3D (T,) uint64 (MAPPER_NO_POINT3D = none), cand_width / cand_height (K,) uint32, cand_point_offsets
    (K + 1,) uint64, cand_xy (N, 2), corr_offsets (N + 1,) uint64, corr_image / corr_point2D (M,) uint32."""
    who = "image_visibility"
    ipoff = _offsets(who, "image_point_offsets", image_point_offsets)
    table = np.array(point2D_point3D, dtype=np.uint64).reshape(-1)
    cw, ch = _u32_index(who, "cand_width", cand_width), _u32_index(who, "cand_height", cand_height)
    cpoff = _offsets(who, "cand_point_offsets", cand_point_offsets)
    xy = np.array(cand_xy, dtype=np.float64).reshape(-1, 2)
    coff = _offsets(who, "corr_offsets", corr_offsets)
    ci, cp = _u32_index(who, "corr_image", corr_image), _u32_index(who, "corr_point2D", corr_point2D)
    if int(ipoff[-1]) != table.size:
        raise ValueError(f"{who}: image_point_offsets ends at {int(ipoff[-1])}, {table.size} table rows")
    if not (cw.size == ch.size == cpoff.size - 1):
        raise ValueError(f"{who}: {cw.size} widths, {ch.size} heights, {cpoff.size} candidate offsets")
    if int(cpoff[-1]) != xy.shape[0] or coff.size != xy.shape[0] + 1:
        raise ValueError(f"{who}: cand_point_offsets ends at {int(cpoff[-1])}, {xy.shape[0]} pixels, {coff.size} correspondence offsets")
    if int(coff[-1]) != ci.size or ci.size != cp.size:
        raise ValueError(f"{who}: corr_offsets ends at {int(coff[-1])}, {ci.size} images, {cp.size} point2D indices")
    return ipoff, table, cw, ch, cpoff, xy, coff, ci, cp


def pair_angle_inputs(qvec, tvec, point_xyz, pair_images, pair_offsets, shared_points):
    """The flat problem of amc_shared_point_angles as contiguous arrays (copies): qvec (I, 4) x y z w, tvec (I, 3),
    point_xyz (P, 3), pair_images (K, 2) uint32, pair_offsets (K + 1,) uint64, shared_points (S,) uint32."""
    who = "shared_point_angles"
    q = np.array(qvec, dtype=np.float64).reshape(-1, 4)
    t = np.array(tvec, dtype=np.float64).reshape(-1, 3)
    X = np.array(point_xyz, dtype=np.float64).reshape(-1, 3)
    pi = np.ascontiguousarray(_u32_index(who, "pair_images", pair_images).reshape(-1, 2))
    poff = _offsets(who, "pair_offsets", pair_offsets)
    sp = _u32_index(who, "shared_points", shared_points)
    if q.shape[0] != t.shape[0]:
        raise ValueError(f"{who}: {q.shape[0]} rotations, {t.shape[0]} translations")
    if poff.size != pi.shape[0] + 1 or int(poff[-1]) != sp.size:
        raise ValueError(f"{who}: {pi.shape[0]} pairs, {poff.size} offsets ending at {int(poff[-1])}, {sp.size} shared points")
    return q, t, X, pi, poff, sp


class PairTriOpts(C.Structure):  # amc_pair_tri_opts (include/amc_initpair.h)
    _fields_ = [("min_tri_angle", C.c_double), ("reserved", C.c_double)]


class PairTriProblem(C.Structure):  # amc_pair_tri_problem
    _fields_ = [("num_cameras", C.c_size_t), ("camera_models", C.c_void_p), ("camera_params", C.c_void_p),
                ("num_images", C.c_size_t), ("image_cameras", C.c_void_p), ("qvec", C.c_void_p), ("tvec", C.c_void_p),
                ("num_pairs", C.c_size_t), ("pair_images", C.c_void_p), ("pair_offsets", C.c_void_p),
                ("corr_xy1", C.c_void_p), ("corr_xy2", C.c_void_p)]


class PairTriResult(C.Structure):  # amc_pair_tri_result
    _fields_ = [("num_pairs", C.c_uint64), ("num_corrs", C.c_uint64), ("num_accepted", C.c_uint64),
                ("accepted", C.POINTER(C.c_uint8)), ("xyz", C.POINTER(C.c_double)), ("tri_angle", C.POINTER(C.c_double)),
                ("num_batches", C.c_uint32), ("reserved", C.c_uint32),
                ("host_ms", C.c_double), ("device_ms", C.c_double), ("kernel_ms", C.c_double), ("copy_ms", C.c_double),
                ("alloc_ms", C.c_double)]


INITPAIR_MAX_CORRS = 1 << 26
INITPAIR_DEFAULT_MIN_TRI_ANGLE = 0.017453292519943295 * 16.0  # DegToRad(IncrementalMapperOptions.init_min_tri_angle)


def pair_tri_inputs(camera_models, camera_params, image_cameras, qvec, tvec, pair_images, pair_offsets, corr_xy1, corr_xy2):
    """The flat problem of amc_triangulate_pairs as contiguous arrays (copies: the caller's arrays are not touched):
    models (C,) int32, params (C, 12), image_cameras (I,) uint32, qvec (I, 4) x y z w, tvec (I, 3), pair_images (K, 2)
    uint32, pair_offsets (K + 1,) uint64, corr_xy1 / corr_xy2 (M, 2) pixels."""
    who = "triangulate_pairs"
    models = np.array(camera_models, dtype=np.int32).reshape(-1)
    if len(camera_params) != models.size:
        raise ValueError(f"{who}: {models.size} camera models, {len(camera_params)} parameter sets")
    prm = np.zeros((models.size, 12), np.float64)
    for i, p in enumerate(camera_params):
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        if p.size > 12:
            raise ValueError(f"{who}: camera {i} has {p.size} parameters (at most 12)")
        prm[i, :p.size] = p
    icam = _u32_index(who, "image_cameras", image_cameras)
    q = np.array(qvec, dtype=np.float64).reshape(-1, 4)
    t = np.array(tvec, dtype=np.float64).reshape(-1, 3)
    pi = np.ascontiguousarray(_u32_index(who, "pair_images", pair_images).reshape(-1, 2))
    poff = _offsets(who, "pair_offsets", pair_offsets)
    xy1 = np.array(corr_xy1, dtype=np.float64).reshape(-1, 2)
    xy2 = np.array(corr_xy2, dtype=np.float64).reshape(-1, 2)
    if q.shape[0] != icam.size or t.shape[0] != icam.size:
        raise ValueError(f"{who}: {icam.size} images by image_cameras, {q.shape[0]} rotations, {t.shape[0]} translations")
    if poff.size != pi.shape[0] + 1 or int(poff[-1]) != xy1.shape[0] or xy1.shape[0] != xy2.shape[0]:
        raise ValueError(f"{who}: {pi.shape[0]} pairs, {poff.size} offsets ending at {int(poff[-1])}, {xy1.shape[0]} and "
                         f"{xy2.shape[0]} pixels")
    return models, prm, icam, q, t, pi, poff, xy1, xy2


class PatchMatchOpts(C.Structure):  # amc_patch_match_opts (include/amc_patchmatch.h)
    _fields_ = [("window_radius", C.c_int32), ("window_step", C.c_int32), ("num_samples", C.c_int32),
                ("num_iterations", C.c_int32), ("geom_consistency", C.c_int32), ("filter", C.c_int32),
                ("filter_min_num_consistent", C.c_int32), ("want_costs", C.c_int32), ("seed", C.c_uint32),
                ("reserved", C.c_uint32), ("sigma_spatial", C.c_double), ("sigma_color", C.c_double),
                ("ncc_sigma", C.c_double), ("min_triangulation_angle", C.c_double), ("incident_angle_sigma", C.c_double),
                ("geom_consistency_regularizer", C.c_double), ("geom_consistency_max_cost", C.c_double),
                ("filter_min_ncc", C.c_double), ("filter_min_triangulation_angle", C.c_double),
                ("filter_geom_consistency_max_cost", C.c_double)]


class PatchMatchProblem(C.Structure):  # amc_patch_match_problem
    _fields_ = [("num_images", C.c_size_t), ("pixels", C.c_void_p), ("pixel_offsets", C.c_void_p), ("widths", C.c_void_p),
                ("heights", C.c_void_p), ("K", C.c_void_p), ("R", C.c_void_p), ("t", C.c_void_p),
                ("num_problems", C.c_size_t), ("ref_images", C.c_void_p), ("src_offsets", C.c_void_p),
                ("src_images", C.c_void_p), ("depth_ranges", C.c_void_p), ("in_depth", C.c_void_p),
                ("in_normal", C.c_void_p), ("in_map_offsets", C.c_void_p)]


class PatchMatchResult(C.Structure):  # amc_patch_match_result
    _fields_ = [("num_problems", C.c_uint64), ("num_pixels", C.c_uint64), ("num_costs", C.c_uint64),
                ("map_offsets", C.POINTER(C.c_uint64)), ("cost_offsets", C.POINTER(C.c_uint64)),
                ("depth", C.POINTER(C.c_float)), ("normal", C.POINTER(C.c_float)),
                ("num_consistent", C.POINTER(C.c_uint8)), ("costs", C.POINTER(C.c_float)),
                ("num_batches", C.c_uint32), ("num_launches", C.c_uint32),
                ("host_ms", C.c_double), ("device_ms", C.c_double), ("kernel_ms", C.c_double), ("copy_ms", C.c_double),
                ("alloc_ms", C.c_double)]


PATCHMATCH_MAX_SOURCES = 32
PATCHMATCH_NO_MAP = 0xFFFFFFFFFFFFFFFF
PATCHMATCH_DEFAULTS = dict(
    window_radius=5, window_step=1, num_samples=15, num_iterations=5, geom_consistency=0, filter=0,
    filter_min_num_consistent=2, want_costs=0, seed=0, sigma_spatial=-1.0, sigma_color=0.2, ncc_sigma=0.6,
    min_triangulation_angle=1.0, incident_angle_sigma=0.9, geom_consistency_regularizer=0.3,
    geom_consistency_max_cost=3.0, filter_min_ncc=0.1, filter_min_triangulation_angle=3.0,
    filter_geom_consistency_max_cost=1.0)


def patch_match_options(**kw) -> PatchMatchOpts:
    """amc_patch_match_opts with the library's defaults (PATCHMATCH_DEFAULTS) and the given fields."""
    unknown = set(kw) - set(PATCHMATCH_DEFAULTS)
    if unknown:
        raise ValueError(f"patch_match: unknown option {sorted(unknown)[0]!r}")
    o = PatchMatchOpts()
    for k, v in {**PATCHMATCH_DEFAULTS, **kw}.items():
        setattr(o, k, type(PATCHMATCH_DEFAULTS[k])(v))
    return o


def patch_match_inputs(images, K, R, t, ref_images, src_offsets, src_images, depth_ranges, in_depth=None, in_normal=None):
    """The flat problem of amc_patch_match as contiguous arrays (copies: the caller's arrays are not touched).  images: a
    list of H x W uint8 arrays; K (I, 4) fx fy cx cy; R (I, 3, 3) and t (I, 3) cam_from_world; ref_images (P,);
    src_offsets (P + 1,) CSR over src_images; depth_ranges (P, 2).  in_depth / in_normal: per image an H x W and a
    3 x H x W float32 array or None, or None for no maps at all.  Returns (problem, keep): the PatchMatchProblem and the
    arrays it points into."""
    who = "patch_match"
    imgs = [np.ascontiguousarray(a, dtype=np.uint8) for a in images]
    for i, a in enumerate(imgs):
        if a.ndim != 2 or a.size == 0:
            raise ValueError(f"{who}: image {i} is not a non-empty H x W grey image")
    n = len(imgs)
    sizes = np.array([a.size for a in imgs], dtype=np.uint64)
    poff = np.zeros(n + 1, np.uint64)
    poff[1:] = np.cumsum(sizes)
    pixels = np.concatenate([a.reshape(-1) for a in imgs]) if n else np.zeros(1, np.uint8)
    w = np.array([a.shape[1] for a in imgs], dtype=np.int32)
    h = np.array([a.shape[0] for a in imgs], dtype=np.int32)
    Kf = np.array(K, dtype=np.float64).reshape(-1, 4)
    Rf = np.array(R, dtype=np.float64).reshape(-1, 9)
    tf = np.array(t, dtype=np.float64).reshape(-1, 3)
    if not (Kf.shape[0] == Rf.shape[0] == tf.shape[0] == n):
        raise ValueError(f"{who}: {n} images, {Kf.shape[0]} K, {Rf.shape[0]} R, {tf.shape[0]} t")
    ref = _u32_index(who, "ref_images", ref_images)
    soff = _offsets(who, "src_offsets", src_offsets)
    src = _u32_index(who, "src_images", src_images)
    rng = np.array(depth_ranges, dtype=np.float64).reshape(-1, 2)
    if soff.size != ref.size + 1 or int(soff[-1]) != src.size or rng.shape[0] != ref.size:
        raise ValueError(f"{who}: {ref.size} problems, {soff.size} offsets ending at {int(soff[-1])}, {src.size} sources, "
                         f"{rng.shape[0]} depth ranges")
    keep = [pixels, poff, w, h, Kf, Rf, tf, ref, soff, src, rng]
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    pd = pn = pm = None
    if (in_depth is None) != (in_normal is None):
        raise ValueError(f"{who}: in_depth and in_normal are given together")
    if in_depth is not None:
        if len(in_depth) != n or len(in_normal) != n:
            raise ValueError(f"{who}: {n} images, {len(in_depth)} depth maps, {len(in_normal)} normal maps")
        moff = np.full(n, PATCHMATCH_NO_MAP, np.uint64)
        ds, ns, at = [], [], 0
        for i in range(n):
            if in_depth[i] is None:
                continue
            dm = np.ascontiguousarray(in_depth[i], dtype=np.float32)
            nm = np.ascontiguousarray(in_normal[i], dtype=np.float32)
            if dm.shape != imgs[i].shape or nm.shape != (3,) + imgs[i].shape:
                raise ValueError(f"{who}: image {i} is {imgs[i].shape}, its depth map {dm.shape}, its normal map {nm.shape}")
            moff[i] = at
            ds.append(dm.reshape(-1))
            # the call addresses the normal maps at three times the depth maps' offsets
            ns.append(nm.reshape(-1))
            at += dm.size
        dflat = np.concatenate(ds) if ds else np.zeros(1, np.float32)
        nflat = np.concatenate(ns) if ns else np.zeros(3, np.float32)
        keep += [dflat, nflat, moff]
        pd, pn, pm = ptr(dflat), ptr(nflat), ptr(moff)
    pb = PatchMatchProblem(n, ptr(pixels), ptr(poff), ptr(w), ptr(h), ptr(Kf), ptr(Rf), ptr(tf), ref.size, ptr(ref), ptr(soff),
                           ptr(src), ptr(rng), pd, pn, pm)
    return pb, keep


def patch_match_unpack(keep, num_problems, map_offsets, cost_offsets, depth, normal, num_consistent, costs):
    """The per-problem arrays of a patch match result (copies) from its flat ones; `keep` as patch_match_inputs returns it."""
    w, h, ref, soff = keep[2], keep[3], keep[7], keep[8]
    out = {"depth": [], "normal": [], "num_consistent": [], "costs": [] if costs is not None else None}
    for p in range(int(num_problems)):
        H, W, S = int(h[ref[p]]), int(w[ref[p]]), int(soff[p + 1] - soff[p])
        m, c = int(map_offsets[p]), int(cost_offsets[p])
        arr = lambda ptr, at, k: np.ctypeslib.as_array(ptr, (at + k,))[at:].copy()  # noqa: E731
        out["depth"].append(arr(depth, m, H * W).reshape(H, W))
        out["normal"].append(arr(normal, 3 * m, 3 * H * W).reshape(3, H, W))
        out["num_consistent"].append(arr(num_consistent, m, H * W).reshape(H, W))
        if costs is not None:
            out["costs"].append(arr(costs, c, S * H * W).reshape(S, H, W))
    return out


class FusionOpts(C.Structure):  # amc_fusion_opts (include/amc_fusion.h)
    _fields_ = [("min_num_pixels", C.c_int32), ("max_num_pixels", C.c_int32), ("max_traversal_depth", C.c_int32),
                ("reserved", C.c_int32), ("max_reproj_error", C.c_double), ("max_depth_error", C.c_double),
                ("max_normal_error", C.c_double), ("bounding_box", C.c_double * 6)]


class FusionProblem(C.Structure):  # amc_fusion_problem
    _fields_ = [("num_images", C.c_size_t), ("rgb", C.c_void_p), ("rgb_offsets", C.c_void_p), ("widths", C.c_void_p),
                ("heights", C.c_void_p), ("K", C.c_void_p), ("R", C.c_void_p), ("t", C.c_void_p), ("depth", C.c_void_p),
                ("normal", C.c_void_p), ("map_offsets", C.c_void_p), ("nb_offsets", C.c_void_p), ("nb_images", C.c_void_p)]


class FusionResult(C.Structure):  # amc_fusion_result
    _fields_ = [("num_points", C.c_uint64), ("xyz", C.POINTER(C.c_float)), ("normal", C.POINTER(C.c_float)),
                ("color", C.POINTER(C.c_uint8)), ("seed_image", C.POINTER(C.c_uint32)), ("seed_pixel", C.POINTER(C.c_uint32)),
                ("num_fused", C.POINTER(C.c_uint32)), ("vis_offsets", C.POINTER(C.c_uint64)),
                ("vis_images", C.POINTER(C.c_uint32)), ("num_seeds", C.c_uint64), ("num_truncated", C.c_uint64),
                ("num_batches", C.c_uint32), ("num_launches", C.c_uint32),
                ("host_ms", C.c_double), ("device_ms", C.c_double), ("kernel_ms", C.c_double), ("copy_ms", C.c_double),
                ("alloc_ms", C.c_double)]


FUSION_MAX_NEIGHBOURS = 64
FUSION_MAX_TRAVERSAL_DEPTH = 128
FUSION_MAX_CLUSTER = 256
FUSION_NO_MAP = 0xFFFFFFFFFFFFFFFF
FLOAT32_MAX = 3.4028234663852886e38
FUSION_DEFAULTS = dict(
    min_num_pixels=5, max_num_pixels=10000, max_traversal_depth=100, max_reproj_error=2.0, max_depth_error=0.01,
    max_normal_error=10.0, bounding_box=((-FLOAT32_MAX,) * 3, (FLOAT32_MAX,) * 3))


def fusion_options(**kw) -> FusionOpts:
    """amc_fusion_opts with the library's defaults (FUSION_DEFAULTS) and the given fields; bounding_box is a pair of
    3-vectors (min, max)."""
    unknown = set(kw) - set(FUSION_DEFAULTS)
    if unknown:
        raise ValueError(f"fuse_depth_maps: unknown option {sorted(unknown)[0]!r}")
    o = FusionOpts()
    for k, v in {**FUSION_DEFAULTS, **kw}.items():
        if k == "bounding_box":
            box = np.array(v, dtype=np.float64).reshape(-1)
            if box.size != 6:
                raise ValueError("fuse_depth_maps: bounding_box is not a pair of 3-vectors")
            o.bounding_box = (C.c_double * 6)(*box)
        else:
            setattr(o, k, type(FUSION_DEFAULTS[k])(v))
    return o


def fusion_inputs(images, K, R, t, depth_maps, normal_maps, neighbours):
    """The flat problem of amc_fuse_depth_maps as contiguous arrays (copies: the caller's arrays are not touched).
    images: a list of H x W x 3 uint8 arrays in fusion order; K (I, 4) fx fy cx cy; R (I, 3, 3) and t (I, 3)
    cam_from_world; depth_maps / normal_maps: per image an H x W and a 3 x H x W float32 array, or None for an image
    without maps; neighbours: per image the ordered list of image indices.  Returns (problem, keep)."""
    who = "fuse_depth_maps"
    imgs = [np.ascontiguousarray(a, dtype=np.uint8) for a in images]
    for i, a in enumerate(imgs):
        if a.ndim != 3 or a.shape[2] != 3 or a.size == 0:
            raise ValueError(f"{who}: image {i} is not a non-empty H x W x 3 image")
    n = len(imgs)
    roff = np.zeros(n + 1, np.uint64)
    roff[1:] = np.cumsum([a.size for a in imgs], dtype=np.uint64)
    rgb = np.concatenate([a.reshape(-1) for a in imgs]) if n else np.zeros(1, np.uint8)
    w = np.array([a.shape[1] for a in imgs], dtype=np.int32)
    h = np.array([a.shape[0] for a in imgs], dtype=np.int32)
    Kf = np.array(K, dtype=np.float64).reshape(-1, 4)
    Rf = np.array(R, dtype=np.float64).reshape(-1, 9)
    tf = np.array(t, dtype=np.float64).reshape(-1, 3)
    if not (Kf.shape[0] == Rf.shape[0] == tf.shape[0] == n):
        raise ValueError(f"{who}: {n} images, {Kf.shape[0]} K, {Rf.shape[0]} R, {tf.shape[0]} t")
    if len(depth_maps) != n or len(normal_maps) != n or len(neighbours) != n:
        raise ValueError(f"{who}: {n} images, {len(depth_maps)} depth maps, {len(normal_maps)} normal maps, "
                         f"{len(neighbours)} neighbour lists")
    moff = np.full(max(n, 1), FUSION_NO_MAP, np.uint64)
    ds, ns, at = [], [], 0
    for i in range(n):
        if (depth_maps[i] is None) != (normal_maps[i] is None):
            raise ValueError(f"{who}: image {i} has one map of the two")
        if depth_maps[i] is None:
            continue
        dm = np.ascontiguousarray(depth_maps[i], dtype=np.float32)
        nm = np.ascontiguousarray(normal_maps[i], dtype=np.float32)
        if dm.shape != imgs[i].shape[:2] or nm.shape != (3,) + imgs[i].shape[:2]:
            raise ValueError(f"{who}: image {i} is {imgs[i].shape[:2]}, its depth map {dm.shape}, its normal map {nm.shape}")
        moff[i] = at
        ds.append(dm.reshape(-1))
        ns.append(nm.reshape(-1))  # the call addresses the normal maps at three times the depth maps' offsets
        at += dm.size
    dflat = np.concatenate(ds) if ds else np.zeros(1, np.float32)
    nflat = np.concatenate(ns) if ns else np.zeros(3, np.float32)
    noff = np.zeros(n + 1, np.uint64)
    lists = []
    for i, lst in enumerate(neighbours):
        lst = _u32_index(who, f"neighbours[{i}]", lst)
        if lst.size > FUSION_MAX_NEIGHBOURS:
            raise ValueError(f"{who}: image {i} has {lst.size} neighbours, more than {FUSION_MAX_NEIGHBOURS} "
                             "(AMC_FUSION_MAX_NEIGHBOURS)")
        lists.append(lst)
        noff[i + 1] = noff[i] + np.uint64(lst.size)
    nb = np.concatenate(lists + [np.zeros(1, np.uint32)]).astype(np.uint32)
    keep = [rgb, roff, w, h, Kf, Rf, tf, dflat, nflat, moff, noff, nb]
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    pb = FusionProblem(n, ptr(rgb), ptr(roff), ptr(w), ptr(h), ptr(Kf), ptr(Rf), ptr(tf), ptr(dflat), ptr(nflat), ptr(moff),
                       ptr(noff), ptr(nb))
    return pb, keep


def fusion_unpack(num_points, xyz, normal, color, seed_image, seed_pixel, num_fused, vis_offsets, vis_images):
    """The arrays of a fusion result (copies) from its flat ones"""
    n = int(num_points)
    arr = lambda p, k: np.ctypeslib.as_array(p, (max(k, 1),))[:k].copy()  # noqa: E731
    voff = arr(vis_offsets, n + 1)
    return {"num_points": n, "xyz": arr(xyz, 3 * n).reshape(n, 3), "normal": arr(normal, 3 * n).reshape(n, 3),
            "color": arr(color, 3 * n).reshape(n, 3), "seed_image": arr(seed_image, n), "seed_pixel": arr(seed_pixel, n),
            "num_fused": arr(num_fused, n), "vis_offsets": voff, "vis_images": arr(vis_images, int(voff[-1]))}


RETRI_NONE, RETRI_CONTINUE_1TO2, RETRI_CONTINUE_2TO1, RETRI_CREATED = 0, 1, 2, 3
RETRI_MAX_CORRS = 1 << 24


def retri_inputs(camera_models, camera_params, image_cameras, qvec, tvec, obs_image, obs_xy, obs_point, point_xyz,
                 pair_images, pair_offsets, corr_obs, round_offsets, corr_two_view=None):
    """The flat problem of amc_retriangulate_pairs as contiguous arrays (copies: the caller's arrays are not touched):
    models (C,) int32, params (C, 12), image_cameras (I,) uint32, qvec (I, 4) x y z w, tvec (I, 3), obs_image (N,)
    uint32, obs_xy (N, 2), obs_point (N,) int32, point_xyz (P, 3), pair_images (K, 2) uint32, pair_offsets (K + 1,)
    uint64, corr_obs (M, 2) uint32, round_offsets (R + 1,) uint64, corr_two_view (M,) uint8 or None."""
    who = "retriangulate_pairs"
    models = np.array(camera_models, dtype=np.int32).reshape(-1)
    if len(camera_params) != models.size:
        raise ValueError(f"{who}: {models.size} camera models, {len(camera_params)} parameter sets")
    prm = np.zeros((models.size, 12), np.float64)
    for i, p in enumerate(camera_params):
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        if p.size > 12:
            raise ValueError(f"{who}: camera {i} has {p.size} parameters (at most 12)")
        prm[i, :p.size] = p
    icam = np.array(image_cameras, dtype=np.int64).reshape(-1)
    q = np.array(qvec, dtype=np.float64).reshape(-1, 4)
    t = np.array(tvec, dtype=np.float64).reshape(-1, 3)
    oi = np.array(obs_image, dtype=np.int64).reshape(-1)
    xy = np.array(obs_xy, dtype=np.float64).reshape(-1, 2)
    op = np.array(obs_point, dtype=np.int64).reshape(-1)
    X = np.array(point_xyz, dtype=np.float64).reshape(-1, 3)
    pi = np.array(pair_images, dtype=np.int64).reshape(-1, 2)
    poff = np.array(pair_offsets, dtype=np.int64).reshape(-1)
    co = np.array(corr_obs, dtype=np.int64).reshape(-1, 2)
    roff = np.array(round_offsets, dtype=np.int64).reshape(-1)
    if q.shape[0] != icam.size or t.shape[0] != icam.size or not (xy.shape[0] == op.size == oi.size):
        raise ValueError(f"{who}: {icam.size} images by image_cameras, {q.shape[0]} rotations, {t.shape[0]} translations; "
                         f"{oi.size} observations by obs_image, {xy.shape[0]} pixels, {op.size} point indices")
    if poff.size != pi.shape[0] + 1 or poff.min() < 0 or int(poff[-1]) != co.shape[0]:
        raise ValueError(f"{who}: {pi.shape[0]} pairs, {poff.size} pair offsets ending at {int(poff[-1]) if poff.size else None}, "
                         f"{co.shape[0]} correspondences")
    if roff.size < 1 or roff.min() < 0:
        raise ValueError(f"{who}: round_offsets needs at least one non-negative entry")
    for name, a in (("image_cameras", icam), ("obs_image", oi), ("pair_images", pi), ("corr_obs", co)):
        if a.size and (a.min() < 0 or a.max() > 0xffffffff):
            raise ValueError(f"{who}: {name} has an index outside 0 .. 2^32 - 1")
    if op.size and (op.min() < -(1 << 31) or op.max() >= (1 << 31)):
        raise ValueError(f"{who}: obs_point has an index outside the int32 range")
    two = None
    if corr_two_view is not None:
        two = np.ascontiguousarray(np.asarray(corr_two_view).reshape(-1) != 0, dtype=np.uint8)
        if two.size != co.shape[0]:
            raise ValueError(f"{who}: {co.shape[0]} correspondences, {two.size} two-view flags")
    return (models, prm, icam.astype(np.uint32), q, t, oi.astype(np.uint32), xy, op.astype(np.int32), X,
            np.ascontiguousarray(pi.astype(np.uint32)), poff.astype(np.uint64), np.ascontiguousarray(co.astype(np.uint32)),
            roff.astype(np.uint64), two)


class CompleteOpts(C.Structure):  # amc_complete_opts (include/amc_tracks.h)
    _fields_ = [("complete_max_reproj_error", C.c_double), ("reserved", C.c_double)]


class CompleteProblem(C.Structure):  # amc_complete_problem
    _fields_ = [("num_cameras", C.c_size_t), ("camera_models", C.c_void_p), ("camera_params", C.c_void_p),
                ("num_images", C.c_size_t), ("image_cameras", C.c_void_p), ("qvec", C.c_void_p), ("tvec", C.c_void_p),
                ("num_items", C.c_size_t), ("item_xyz", C.c_void_p), ("item_offsets", C.c_void_p),
                ("cand_image", C.c_void_p), ("cand_xy", C.c_void_p)]


class CompleteResult(C.Structure):  # amc_complete_result
    _fields_ = [("num_items", C.c_uint64), ("num_candidates", C.c_uint64), ("num_passed", C.c_uint64),
                ("cand_sq_error", C.POINTER(C.c_double)), ("cand_pass", C.POINTER(C.c_uint8)),
                ("num_batches", C.c_uint32), ("reserved", C.c_uint32), ("host_ms", C.c_double),
                ("device_ms", C.c_double), ("kernel_ms", C.c_double), ("copy_ms", C.c_double),
                ("alloc_ms", C.c_double)]


def complete_inputs(camera_models, camera_params, image_cameras, qvec, tvec, item_xyz, item_offsets, cand_image, cand_xy):
    """The flat problem of amc_complete_tracks as contiguous arrays (copies: the caller's arrays are not touched):
    models (C,) int32, params (C, 12), image_cameras (I,) uint32, qvec (I, 4) x y z w, tvec (I, 3), item_xyz (T, 3),
    item_offsets (T + 1,) uint64, cand_image (N,) uint32, cand_xy (N, 2)."""
    who = "complete_tracks"
    models = np.array(camera_models, dtype=np.int32).reshape(-1)
    if len(camera_params) != models.size:
        raise ValueError(f"{who}: {models.size} camera models, {len(camera_params)} parameter sets")
    prm = np.zeros((models.size, 12), np.float64)
    for i, p in enumerate(camera_params):
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        if p.size > 12:
            raise ValueError(f"{who}: camera {i} has {p.size} parameters (at most 12)")
        prm[i, :p.size] = p
    icam = np.array(image_cameras, dtype=np.int64).reshape(-1)
    q = np.array(qvec, dtype=np.float64).reshape(-1, 4)
    t = np.array(tvec, dtype=np.float64).reshape(-1, 3)
    X = np.array(item_xyz, dtype=np.float64).reshape(-1, 3)
    off = np.array(item_offsets, dtype=np.int64).reshape(-1)
    ci = np.array(cand_image, dtype=np.int64).reshape(-1)
    xy = np.array(cand_xy, dtype=np.float64).reshape(-1, 2)
    if q.shape[0] != icam.size or t.shape[0] != icam.size or off.size != X.shape[0] + 1 or xy.shape[0] != ci.size:
        raise ValueError(f"{who}: {icam.size} images by image_cameras, {q.shape[0]} rotations, {t.shape[0]} translations; "
                         f"{X.shape[0]} items, {off.size} offsets; {ci.size} candidates by cand_image, {xy.shape[0]} pixels")
    if off.min() < 0 or int(off[-1]) != ci.size:
        raise ValueError(f"{who}: item_offsets ends at {int(off[-1])}, {ci.size} candidates")
    for name, a in (("image_cameras", icam), ("cand_image", ci)):
        if a.size and (a.min() < 0 or a.max() > 0xffffffff):
            raise ValueError(f"{who}: {name} has an index outside 0 .. 2^32 - 1")
    return models, prm, icam.astype(np.uint32), q, t, X, off.astype(np.uint64), ci.astype(np.uint32), xy


class MergeOpts(C.Structure):  # amc_merge_opts (include/amc_tracks.h)
    _fields_ = [("merge_max_reproj_error", C.c_double), ("reserved", C.c_double)]


class MergeProblem(C.Structure):  # amc_merge_problem
    _fields_ = [("num_cameras", C.c_size_t), ("camera_models", C.c_void_p), ("camera_params", C.c_void_p),
                ("num_images", C.c_size_t), ("image_cameras", C.c_void_p), ("qvec", C.c_void_p), ("tvec", C.c_void_p),
                ("num_components", C.c_size_t), ("comp_point_offsets", C.c_void_p), ("comp_root_offsets", C.c_void_p),
                ("roots", C.c_void_p), ("point_xyz", C.c_void_p), ("point_obs_offsets", C.c_void_p),
                ("obs_image", C.c_void_p), ("obs_xy", C.c_void_p), ("obs_corr_offsets", C.c_void_p),
                ("corr_obs", C.c_void_p)]


class MergeResult(C.Structure):  # amc_merge_result
    _fields_ = [("num_components", C.c_uint64), ("num_points", C.c_uint64), ("num_observations", C.c_uint64),
                ("num_roots", C.c_uint64), ("num_merges", C.c_uint64), ("num_pairs_tried", C.c_uint64),
                ("root_return", C.POINTER(C.c_uint32)), ("root_merge_offsets", C.POINTER(C.c_uint64)),
                ("merge_current", C.POINTER(C.c_uint32)), ("merge_other", C.POINTER(C.c_uint32)),
                ("merge_xyz", C.POINTER(C.c_double)), ("num_batches", C.c_uint32), ("reserved", C.c_uint32),
                ("host_ms", C.c_double), ("device_ms", C.c_double), ("kernel_ms", C.c_double), ("copy_ms", C.c_double),
                ("alloc_ms", C.c_double)]


def merge_inputs(camera_models, camera_params, image_cameras, qvec, tvec, comp_point_offsets, comp_root_offsets, roots,
                 point_xyz, point_obs_offsets, obs_image, obs_xy, obs_corr_offsets, corr_obs):
    """The flat problem of amc_merge_tracks as contiguous arrays (copies: the caller's arrays are not touched): models
    (C,) int32, params (C, 12), image_cameras (I,) uint32, qvec (I, 4) x y z w, tvec (I, 3), comp_point_offsets and
    comp_root_offsets (K + 1,) uint64, roots (R,) uint32, point_xyz (P, 3), point_obs_offsets (P + 1,) uint64, obs_image
    (N,) uint32, obs_xy (N, 2), obs_corr_offsets (N + 1,) uint64, corr_obs (M,) uint32."""
    who = "merge_tracks"
    models = np.array(camera_models, dtype=np.int32).reshape(-1)
    if len(camera_params) != models.size:
        raise ValueError(f"{who}: {models.size} camera models, {len(camera_params)} parameter sets")
    prm = np.zeros((models.size, 12), np.float64)
    for i, p in enumerate(camera_params):
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        if p.size > 12:
            raise ValueError(f"{who}: camera {i} has {p.size} parameters (at most 12)")
        prm[i, :p.size] = p
    icam = np.array(image_cameras, dtype=np.int64).reshape(-1)
    q = np.array(qvec, dtype=np.float64).reshape(-1, 4)
    t = np.array(tvec, dtype=np.float64).reshape(-1, 3)
    cpo = np.array(comp_point_offsets, dtype=np.int64).reshape(-1)
    cro = np.array(comp_root_offsets, dtype=np.int64).reshape(-1)
    rt = np.array(roots, dtype=np.int64).reshape(-1)
    X = np.array(point_xyz, dtype=np.float64).reshape(-1, 3)
    poo = np.array(point_obs_offsets, dtype=np.int64).reshape(-1)
    oi = np.array(obs_image, dtype=np.int64).reshape(-1)
    xy = np.array(obs_xy, dtype=np.float64).reshape(-1, 2)
    oco = np.array(obs_corr_offsets, dtype=np.int64).reshape(-1)
    co = np.array(corr_obs, dtype=np.int64).reshape(-1)
    if (q.shape[0] != icam.size or t.shape[0] != icam.size or cpo.size < 1 or cro.size != cpo.size or poo.size != X.shape[0] + 1
            or xy.shape[0] != oi.size or oco.size != oi.size + 1):
        raise ValueError(f"{who}: {icam.size} images by image_cameras, {q.shape[0]} rotations, {t.shape[0]} translations; "
                         f"{cpo.size} and {cro.size} component offsets; {X.shape[0]} points, {poo.size} offsets; {oi.size} "
                         f"observations by obs_image, {xy.shape[0]} pixels, {oco.size} offsets")
    for name, off, n in (("comp_point_offsets", cpo, X.shape[0]), ("comp_root_offsets", cro, rt.size),
                         ("point_obs_offsets", poo, oi.size), ("obs_corr_offsets", oco, co.size)):
        if off.min() < 0 or int(off[-1]) != n:
            raise ValueError(f"{who}: {name} ends at {int(off[-1])}, {n} elements")
    for name, a in (("image_cameras", icam), ("roots", rt), ("obs_image", oi), ("corr_obs", co)):
        if a.size and (a.min() < 0 or a.max() > 0xffffffff):
            raise ValueError(f"{who}: {name} has an index outside 0 .. 2^32 - 1")
    u32, u64 = np.uint32, np.uint64
    return (models, prm, icam.astype(u32), q, t, cpo.astype(u64), cro.astype(u64), rt.astype(u32), X, poo.astype(u64),
            oi.astype(u32), xy, oco.astype(u64), co.astype(u32))


class RigPoseResult(C.Structure):  # amc_rigpose_result (include/amc_rigpose.h)
    _fields_ = [("nqueries", C.c_size_t), ("ncorr", C.c_size_t), ("success", C.POINTER(C.c_uint8)),
                ("qvec", C.POINTER(C.c_double)), ("tvec", C.POINTER(C.c_double)),
                ("num_inliers", C.POINTER(C.c_uint32)), ("num_all_inliers", C.POINTER(C.c_uint32)),
                ("num_trials", C.POINTER(C.c_uint64)), ("covariance", C.POINTER(C.c_double)),
                ("inlier_mask", C.POINTER(C.c_uint8)), ("device_ms", C.c_double), ("kernel_ms", C.c_double),
                ("num_batches", C.c_uint32), ("_priv", C.c_void_p)]


def rigpose_options(estimation=None, refinement=None):
    """amc_ransac_opts at pycolmap's RANSACOptions() defaults and amc_abspose_refine_opts at its own, with the given
    fields replaced; an unknown field raises ValueError."""
    eo = RansacOpts()
    for k, v in dict(max_error=4.0, min_inlier_ratio=0.01, confidence=0.9999, dyn_num_trials_multiplier=3.0,
                     min_num_trials=1000, max_num_trials=100000).items():
        setattr(eo, k, v)
    for k, v in (estimation or {}).items():
        if k not in dict(RansacOpts._fields_):
            raise ValueError(f"unknown rig pose RANSAC option {k!r}")
        setattr(eo, k, type(getattr(eo, k))(v))
    return eo, abspose_options(None, refinement)[1]


def rigpose_inputs(offsets, camera_offsets, camera_models, camera_params, cams_from_rig, camera_idxs, points2D,
                   points3D):
    """The CSR batch of amc_estimate_rig_absolute_poses as contiguous arrays: offsets (Q + 1,) and camera_offsets
    (Q + 1,) uint64, models (C,) int32, params (C, 12), cams_from_rig (C, 7) x y z w tx ty tz, camera_idxs (N,) int32
    (each into its query's own cameras), points2D (N, 2), points3D (N, 3)."""
    off = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    coff = np.ascontiguousarray(camera_offsets, dtype=np.uint64).reshape(-1)
    if off.size < 1 or coff.size != off.size:
        raise ValueError("rig poses: offsets and camera_offsets need nqueries + 1 entries each")
    n, nc = int(off[-1]), int(coff[-1])
    models = np.ascontiguousarray(camera_models, dtype=np.int32).reshape(-1)
    rigs = np.ascontiguousarray(cams_from_rig, dtype=np.float64).reshape(-1, 7)
    if models.size != nc or len(camera_params) != nc or rigs.shape[0] != nc:
        raise ValueError(f"rig poses: {nc} cameras by camera_offsets, {models.size} camera models, "
                         f"{len(camera_params)} parameter sets, {rigs.shape[0]} cams_from_rig")
    prm = np.zeros((nc, 12), np.float64)
    for i, p in enumerate(camera_params):
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        if p.size > 12:
            raise ValueError(f"rig poses: camera {i} has {p.size} parameters (at most 12)")
        prm[i, :p.size] = p
    idx = np.ascontiguousarray(camera_idxs, dtype=np.int32).reshape(-1)
    p2 = np.ascontiguousarray(points2D, dtype=np.float64).reshape(-1, 2)
    p3 = np.ascontiguousarray(points3D, dtype=np.float64).reshape(-1, 3)
    if p2.shape[0] != n or p3.shape[0] != n or idx.size != n:
        raise ValueError(f"rig poses: {n} correspondences by offsets, {p2.shape[0]} points2D, {p3.shape[0]} points3D, "
                         f"{idx.size} camera_idxs")
    return off, coff, models, prm, rigs, idx, p2, p3


class TriOpts(C.Structure):  # amc_tri_opts (include/amc_tri.h)
    _fields_ = [("min_tri_angle", C.c_double), ("max_error", C.c_double), ("min_inlier_ratio", C.c_double),
                ("confidence", C.c_double), ("dyn_num_trials_multiplier", C.c_double),
                ("min_num_trials", C.c_int64), ("max_num_trials", C.c_int64)]


class TriResult(C.Structure):
    _fields_ = [("ntracks", C.c_size_t), ("nobs", C.c_size_t), ("xyz", C.POINTER(C.c_double)),
                ("success", C.POINTER(C.c_uint8)), ("num_inliers", C.POINTER(C.c_uint32)),
                ("num_trials", C.POINTER(C.c_uint64)), ("inlier_mask", C.POINTER(C.c_uint8)),
                ("device_ms", C.c_double), ("kernel_ms", C.c_double), ("num_batches", C.c_uint32),
                ("_priv", C.c_void_p)]


SIFT_NORMALIZATIONS = {"L1_ROOT": 0, "L2": 1}
SIFT_STAGES = ("scale_space", "detection", "orientation", "descriptors")


class UndistortOpts(C.Structure):  # amc_undistort_opts (include/amc_undistort.h)
    _fields_ = [("blank_pixels", C.c_double), ("min_scale", C.c_double), ("max_scale", C.c_double),
                ("max_image_size", C.c_int32), ("_pad", C.c_int32), ("roi_min_x", C.c_double), ("roi_min_y", C.c_double),
                ("roi_max_x", C.c_double), ("roi_max_y", C.c_double)]


class UndistortCam(C.Structure):  # amc_undistort_cam
    _fields_ = [("model", C.c_int32), ("_pad", C.c_int32), ("width", C.c_uint64), ("height", C.c_uint64),
                ("params", C.c_double * 12)]


class UndistortImage(C.Structure):  # amc_undistort_image
    _fields_ = [("src", C.c_void_p), ("src_stride", C.c_uint64), ("channels", C.c_int32), ("_pad", C.c_int32),
                ("src_camera", UndistortCam), ("dst_camera", UndistortCam), ("dst", C.c_void_p)]


class UndistortResult(C.Structure):  # amc_undistort_result
    _fields_ = [("device_ms", C.c_double), ("kernel_ms", C.c_double), ("num_batches", C.c_uint32),
                ("num_resized", C.c_uint32)]


CAMERA_MODEL_IDS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4, "OPENCV_FISHEYE": 5,
                    "FULL_OPENCV": 6, "FOV": 7, "SIMPLE_RADIAL_FISHEYE": 8, "RADIAL_FISHEYE": 9, "THIN_PRISM_FISHEYE": 10}
CAMERA_NUM_PARAMS = [3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12]


def _undistort_cam(camera) -> UndistortCam:
    """(model name or id, width, height, params) -> amc_undistort_cam; the parameter count is checked here (the C
    struct has room for 12 and cannot tell)."""
    model, width, height, params = camera
    mid = CAMERA_MODEL_IDS[model] if isinstance(model, str) else int(model)
    p = [float(v) for v in params]
    if 0 <= mid < len(CAMERA_NUM_PARAMS) and len(p) != CAMERA_NUM_PARAMS[mid]:
        raise ValueError(f"camera model {model} takes {CAMERA_NUM_PARAMS[mid]} parameters, got {len(p)}")
    c = UndistortCam()
    c.model, c.width, c.height = mid, int(width), int(height)
    for i, v in enumerate(p[:12]):
        c.params[i] = v
    return c


def _undistort_cam_tuple(c: UndistortCam):
    n = CAMERA_NUM_PARAMS[c.model]
    return (c.model, int(c.width), int(c.height), np.array(c.params[:n], dtype=np.float64))


def undistort_options(**kw) -> UndistortOpts:
    """UndistortCameraOptions() with keyword overrides."""
    o = UndistortOpts()
    load().amc_undistort_opts_default(C.byref(o))
    for k, v in kw.items():
        if k.startswith("_") or k not in dict(UndistortOpts._fields_):
            raise ValueError(f"undistort options: unknown option {k!r}")
        setattr(o, k, v)
    return o


def undistort_camera(camera, **opts):
    """amc_undistort_camera (a host computation, no device): camera = (model, width, height, params) ->
    (1 = PINHOLE, width, height, params (4,) float64)."""
    out = UndistortCam()
    _check(load().amc_undistort_camera(C.byref(undistort_options(**opts)), C.byref(_undistort_cam(camera)), C.byref(out)))
    return _undistort_cam_tuple(out)


def undistort_points(camera, undistorted, points) -> np.ndarray:
    """amc_undistort_points (host): undistorted.ImgFromCam(camera.CamFromImg(xy)) of N x 2 points."""
    xy = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    out = np.empty_like(xy)
    _check(load().amc_undistort_points(C.byref(_undistort_cam(camera)), C.byref(_undistort_cam(undistorted)), xy.shape[0],
                                       xy.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


class RansacOpts(C.Structure):
    _fields_ = [("max_error", C.c_double), ("min_inlier_ratio", C.c_double),
                ("confidence", C.c_double), ("dyn_num_trials_multiplier", C.c_double),
                ("min_num_trials", C.c_int64), ("max_num_trials", C.c_int64)]


class TvgOpts(C.Structure):
    _fields_ = [("min_num_inliers", C.c_int32), ("detect_watermark", C.c_int32),
                ("multiple_ignore_watermark", C.c_int32), ("force_H_use", C.c_int32),
                ("compute_relative_pose", C.c_int32), ("multiple_models", C.c_int32),
                ("min_E_F_inlier_ratio", C.c_double), ("max_H_inlier_ratio", C.c_double),
                ("watermark_min_inlier_ratio", C.c_double), ("watermark_border_size", C.c_double),
                ("ransac", RansacOpts)]


class Tvg(C.Structure):
    _fields_ = [("config", C.c_int32), ("num_inliers", C.c_int32), ("E", C.c_double * 9),
                ("F", C.c_double * 9), ("H", C.c_double * 9), ("num_trials", C.c_int64 * 4),
                ("model_inliers", C.c_int64 * 3)]


class Pose(C.Structure):
    _fields_ = [("ok", C.c_int32), ("config", C.c_int32), ("qvec", C.c_double * 4), ("tvec", C.c_double * 3),
                ("R", C.c_double * 9), ("tri_angle", C.c_double), ("num_points3D", C.c_uint32),
                ("pad_", C.c_uint32)]


class VerifyResult(C.Structure):
    _fields_ = [("npairs", C.c_size_t), ("tvg", C.POINTER(Tvg)), ("inlier_mask", C.POINTER(C.c_uint8)),
                ("device_ms", C.c_double), ("kernel_ms", C.c_double), ("kernel_launches", C.c_uint32),
                ("pose", C.POINTER(Pose)), ("pose_kernel_ms", C.c_double), ("work", C.c_uint64 * 12),
                ("_priv", C.c_void_p)]


class RansacReport(C.Structure):
    _fields_ = [("success", C.c_int32), ("num_inliers", C.c_int32), ("num_trials", C.c_int64),
                ("model", C.c_double * 9)]


class RansacResult(C.Structure):
    _fields_ = [("npairs", C.c_size_t), ("reports", C.POINTER(RansacReport)),
                ("inlier_mask", C.POINTER(C.c_uint8)), ("device_ms", C.c_double), ("_priv", C.c_void_p)]


RANSAC_DTYPE = np.dtype([("success", np.int32), ("num_inliers", np.int32), ("num_trials", np.int64),
                         ("model", np.float64, (3, 3))])
POSE_DTYPE = np.dtype([("ok", np.int32), ("config", np.int32), ("qvec", np.float64, (4,)),
                       ("tvec", np.float64, (3,)), ("R", np.float64, (3, 3)), ("tri_angle", np.float64),
                       ("num_points3D", np.uint32), ("pad_", np.uint32)])
TVG_DTYPE = np.dtype([("config", np.int32), ("num_inliers", np.int32), ("E", np.float64, (3, 3)),
                      ("F", np.float64, (3, 3)), ("H", np.float64, (3, 3)),
                      ("num_trials", np.int64, (4,)), ("model_inliers", np.int64, (3,))])
CAMERA_MODELS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4, "OPENCV_FISHEYE": 5,
                 "FULL_OPENCV": 6, "FOV": 7, "SIMPLE_RADIAL_FISHEYE": 8, "RADIAL_FISHEYE": 9,
                 "THIN_PRISM_FISHEYE": 10}
CONFIG_NAMES = ["UNDEFINED", "DEGENERATE", "CALIBRATED", "UNCALIBRATED", "PLANAR", "PANORAMIC",
                "PLANAR_OR_PANORAMIC", "WATERMARK", "MULTIPLE"]

_lib = None


def load() -> C.CDLL:
    """Load libamc.so (raises if it has not been built: there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    import os
    path = Path(os.environ.get("AMC_LIB_PATH", LIB_PATH))  # override: A/B benchmarking of kernel builds
    if not path.exists():
        raise ImportError(
            f"{path} not found — run `python -m pycolmap_amd.build` (hipcc, gfx950). "
            "pycolmap_amd has no CPU fallback.")
    lib = C.CDLL(str(path))
    lib.amc_last_error.restype = C.c_char_p
    lib.amc_abi_version.restype = C.c_int
    lib.amc_device_count.restype = C.c_int
    lib.amc_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.amc_ctx_destroy.argtypes = [C.c_void_p]
    lib.amc_ctx_destroy.restype = None
    lib.amc_ctx_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.amc_ctx_trim.argtypes = [C.c_void_p]
    lib.amc_ctx_trim.restype = C.c_int
    lib.amc_ctx_resident_matches.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.amc_ctx_resident_matches.restype = C.c_int
    lib.amc_upload_matches.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    lib.amc_upload_matches.restype = C.c_int
    if hasattr(lib, "amc_ctx_last_timeline"):
        lib.amc_ctx_last_timeline.argtypes = [C.c_void_p, C.c_void_p]
    lib.amc_ctx_reserve_slots.argtypes = [C.c_void_p, C.c_uint32]
    lib.amc_ctx_grow_slots.argtypes = [C.c_void_p, C.c_uint32]
    lib.amc_upload_descriptors.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    lib.amc_upload_descriptors_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    lib.amc_match_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                    C.POINTER(MatchOpts), C.POINTER(MatchResult)]
    lib.amc_match_result_free.argtypes = [C.POINTER(MatchResult)]
    lib.amc_match_result_free.restype = None
    lib.amc_match_opts_default.argtypes = [C.POINTER(MatchOpts)]
    if hasattr(lib, "amc_sift_extract"):  # (an older library under AMC_LIB_PATH, for A/B runs, has no extractor)
        lib.amc_sift_opts_default.argtypes = [C.POINTER(SiftOpts)]
        lib.amc_sift_opts_default.restype = None
        lib.amc_sift_extract.argtypes = [C.c_void_p, C.POINTER(SiftImage), C.c_size_t, C.POINTER(SiftOpts),
                                         C.POINTER(SiftResult)]
        lib.amc_sift_extract.restype = C.c_int
        lib.amc_sift_result_free.argtypes = [C.POINTER(SiftResult)]
        lib.amc_sift_result_free.restype = None
    lib.amc_match_opts_default.restype = None
    if hasattr(lib, "amc_estimate_absolute_poses"):
        lib.amc_estimate_absolute_poses.argtypes = ([C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 4 +
                                                    [C.POINTER(AbsPoseOpts), C.POINTER(AbsPoseRefineOpts), C.c_int,
                                                     C.POINTER(AbsPoseResult)])
        lib.amc_estimate_absolute_poses.restype = C.c_int
        lib.amc_refine_absolute_poses.argtypes = ([C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 7 +
                                                  [C.POINTER(AbsPoseRefineOpts), C.c_int, C.POINTER(AbsPoseResult)])
        lib.amc_refine_absolute_poses.restype = C.c_int
        lib.amc_abspose_result_free.argtypes = [C.POINTER(AbsPoseResult)]
        lib.amc_abspose_result_free.restype = None
    if hasattr(lib, "amc_refine_poses_and_cameras"):  # (absent from a library built from an older revision)
        lib.amc_estimate_poses_and_cameras.argtypes = ([C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 4 +
                                                       [C.POINTER(AbsPoseOpts), C.POINTER(AbsPoseRefineOpts), C.c_int,
                                                        C.POINTER(AbsRefineResult)])
        lib.amc_estimate_poses_and_cameras.restype = C.c_int
        lib.amc_refine_poses_and_cameras.argtypes = ([C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 7 +
                                                     [C.POINTER(AbsPoseRefineOpts), C.c_int,
                                                      C.POINTER(AbsRefineResult)])
        lib.amc_refine_poses_and_cameras.restype = C.c_int
        lib.amc_absrefine_result_free.argtypes = [C.POINTER(AbsRefineResult)]
        lib.amc_absrefine_result_free.restype = None
    if hasattr(lib, "amc_estimate_rig_absolute_poses"):
        lib.amc_estimate_rig_absolute_poses.argtypes = ([C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 7 +
                                                        [C.POINTER(RansacOpts), C.POINTER(AbsPoseRefineOpts), C.c_int,
                                                         C.POINTER(RigPoseResult)])
        lib.amc_estimate_rig_absolute_poses.restype = C.c_int
        lib.amc_rigpose_result_free.argtypes = [C.POINTER(RigPoseResult)]
        lib.amc_rigpose_result_free.restype = None
    if hasattr(lib, "amc_bundle_adjust"):  # (absent from a library built from an older revision)
        lib.amc_ba_opts_default.argtypes = [C.POINTER(BaOpts)]
        lib.amc_ba_opts_default.restype = None
        lib.amc_bundle_adjust.argtypes = [C.c_void_p, C.POINTER(BaProblem), C.POINTER(BaOpts), C.POINTER(BaResult)]
        lib.amc_bundle_adjust.restype = C.c_int
    if hasattr(lib, "amc_ba_covariance"):
        lib.amc_bacov_opts_default.argtypes = [C.POINTER(BacovOpts)]
        lib.amc_bacov_opts_default.restype = None
        lib.amc_ba_covariance.argtypes = [C.c_void_p, C.POINTER(BaProblem), C.c_void_p, C.POINTER(BacovOpts),
                                          C.POINTER(BacovResult)]
        lib.amc_ba_covariance.restype = C.c_int
        lib.amc_bacov_result_free.argtypes = [C.POINTER(BacovResult)]
        lib.amc_bacov_result_free.restype = None
    if hasattr(lib, "amc_bundle_adjust_masked"):
        lib.amc_bundle_adjust_masked.argtypes = [C.c_void_p, C.POINTER(BaProblem), C.c_void_p, C.POINTER(BaOpts),
                                                 C.POINTER(BaResult)]
        lib.amc_bundle_adjust_masked.restype = C.c_int
    if hasattr(lib, "amc_filter_points3d"):  # (absent from a library built from an older revision)
        lib.amc_filter_opts_default.argtypes = [C.POINTER(FilterOpts)]
        lib.amc_filter_opts_default.restype = None
        lib.amc_filter_points3d.argtypes = [C.c_void_p, C.POINTER(FilterProblem), C.POINTER(FilterOpts),
                                            C.POINTER(FilterResult)]
        lib.amc_filter_points3d.restype = C.c_int
        lib.amc_filter_result_free.argtypes = [C.POINTER(FilterResult)]
        lib.amc_filter_result_free.restype = None
    if hasattr(lib, "amc_triangulate_observations"):  # (absent from a library built from an older revision)
        lib.amc_triobs_opts_default.argtypes = [C.POINTER(TriobsOpts)]
        lib.amc_triobs_opts_default.restype = None
        lib.amc_triangulate_observations.argtypes = [C.c_void_p, C.POINTER(TriobsProblem), C.POINTER(TriobsOpts),
                                                     C.POINTER(TriobsResult)]
        lib.amc_triangulate_observations.restype = C.c_int
        lib.amc_triobs_result_free.argtypes = [C.POINTER(TriobsResult)]
        lib.amc_triobs_result_free.restype = None
    if hasattr(lib, "amc_complete_tracks"):  # (absent from a library built from an older revision)
        lib.amc_complete_opts_default.argtypes = [C.POINTER(CompleteOpts)]
        lib.amc_complete_opts_default.restype = None
        lib.amc_complete_tracks.argtypes = [C.c_void_p, C.POINTER(CompleteProblem), C.POINTER(CompleteOpts),
                                            C.POINTER(CompleteResult)]
        lib.amc_complete_tracks.restype = C.c_int
        lib.amc_complete_result_free.argtypes = [C.POINTER(CompleteResult)]
        lib.amc_complete_result_free.restype = None
    if hasattr(lib, "amc_merge_tracks"):  # (absent from a library built from an older revision)
        lib.amc_merge_opts_default.argtypes = [C.POINTER(MergeOpts)]
        lib.amc_merge_opts_default.restype = None
        lib.amc_merge_tracks.argtypes = [C.c_void_p, C.POINTER(MergeProblem), C.POINTER(MergeOpts), C.POINTER(MergeResult)]
        lib.amc_merge_tracks.restype = C.c_int
        lib.amc_merge_result_free.argtypes = [C.POINTER(MergeResult)]
        lib.amc_merge_result_free.restype = None
    if hasattr(lib, "amc_retriangulate_pairs"):  # (absent from a library built from an older revision)
        lib.amc_retri_opts_default.argtypes = [C.POINTER(RetriOpts)]
        lib.amc_retri_opts_default.restype = None
        lib.amc_retriangulate_pairs.argtypes = [C.c_void_p, C.POINTER(RetriProblem), C.POINTER(RetriOpts), C.POINTER(RetriResult)]
        lib.amc_retriangulate_pairs.restype = C.c_int
        lib.amc_retri_result_free.argtypes = [C.POINTER(RetriResult)]
        lib.amc_retri_result_free.restype = None
    if hasattr(lib, "amc_image_visibility"):  # (absent from a library built from an older revision)
        lib.amc_image_visibility.argtypes = [C.c_void_p, C.POINTER(VisibilityProblem), C.POINTER(VisibilityResult)]
        lib.amc_image_visibility.restype = C.c_int
        lib.amc_visibility_result_free.argtypes = [C.POINTER(VisibilityResult)]
        lib.amc_visibility_result_free.restype = None
        lib.amc_pair_angle_opts_default.argtypes = [C.POINTER(PairAngleOpts)]
        lib.amc_pair_angle_opts_default.restype = None
        lib.amc_shared_point_angles.argtypes = [C.c_void_p, C.POINTER(PairAngleProblem), C.POINTER(PairAngleOpts),
                                                C.POINTER(PairAngleResult)]
        lib.amc_shared_point_angles.restype = C.c_int
        lib.amc_pair_angle_result_free.argtypes = [C.POINTER(PairAngleResult)]
        lib.amc_pair_angle_result_free.restype = None
    if hasattr(lib, "amc_patch_match"):  # (absent from a library built from an older revision)
        lib.amc_patch_match_opts_default.argtypes = [C.POINTER(PatchMatchOpts)]
        lib.amc_patch_match_opts_default.restype = None
        lib.amc_patch_match.argtypes = [C.c_void_p, C.POINTER(PatchMatchOpts), C.POINTER(PatchMatchProblem), C.POINTER(PatchMatchResult)]
        lib.amc_patch_match.restype = C.c_int
        lib.amc_patch_match_result_free.argtypes = [C.POINTER(PatchMatchResult)]
        lib.amc_patch_match_result_free.restype = None
    if hasattr(lib, "amc_fuse_depth_maps"):  # (absent from a library built from an older revision)
        lib.amc_fusion_opts_default.argtypes = [C.POINTER(FusionOpts)]
        lib.amc_fusion_opts_default.restype = None
        lib.amc_fuse_depth_maps.argtypes = [C.c_void_p, C.POINTER(FusionOpts), C.POINTER(FusionProblem), C.POINTER(FusionResult)]
        lib.amc_fuse_depth_maps.restype = C.c_int
        lib.amc_fusion_result_free.argtypes = [C.POINTER(FusionResult)]
        lib.amc_fusion_result_free.restype = None
    if hasattr(lib, "amc_triangulate_pairs"):  # (absent from a library built from an older revision)
        lib.amc_pair_tri_opts_default.argtypes = [C.POINTER(PairTriOpts)]
        lib.amc_pair_tri_opts_default.restype = None
        lib.amc_triangulate_pairs.argtypes = [C.c_void_p, C.POINTER(PairTriProblem), C.POINTER(PairTriOpts), C.POINTER(PairTriResult)]
        lib.amc_triangulate_pairs.restype = C.c_int
        lib.amc_pair_tri_result_free.argtypes = [C.POINTER(PairTriResult)]
        lib.amc_pair_tri_result_free.restype = None
    if hasattr(lib, "amc_triangulate_tracks"):  # (absent from a library built from an older revision)
        lib.amc_tri_opts_default.argtypes = [C.POINTER(TriOpts)]
        lib.amc_tri_opts_default.restype = None
        lib.amc_triangulate_tracks.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                               C.c_void_p, C.POINTER(TriOpts), C.POINTER(TriResult)]
        lib.amc_triangulate_tracks.restype = C.c_int
        lib.amc_tri_result_free.argtypes = [C.POINTER(TriResult)]
        lib.amc_tri_result_free.restype = None
    if hasattr(lib, "amc_undistort_images"):  # (absent from a library built from an older revision)
        lib.amc_undistort_opts_default.argtypes = [C.POINTER(UndistortOpts)]
        lib.amc_undistort_opts_default.restype = None
        lib.amc_undistort_camera.argtypes = [C.POINTER(UndistortOpts), C.POINTER(UndistortCam), C.POINTER(UndistortCam)]
        lib.amc_undistort_camera.restype = C.c_int
        lib.amc_undistort_points.argtypes = [C.POINTER(UndistortCam), C.POINTER(UndistortCam), C.c_size_t, C.c_void_p,
                                             C.c_void_p]
        lib.amc_undistort_points.restype = C.c_int
        lib.amc_undistort_images.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(UndistortResult)]
        lib.amc_undistort_images.restype = C.c_int
    lib.amc_get_acos_lut.argtypes = [C.c_void_p, C.c_void_p]
    lib.amc_tvg_opts_default.argtypes = [C.POINTER(TvgOpts)]
    lib.amc_tvg_opts_default.restype = None
    lib.amc_upload_keypoints.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
    lib.amc_upload_camera.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.c_uint64, C.c_uint64,
                                      C.c_void_p, C.c_int32, C.c_int32]
    lib.amc_verify_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_void_p, C.POINTER(TvgOpts), C.c_uint32, C.POINTER(VerifyResult)]
    lib.amc_verify_result_free.argtypes = [C.POINTER(VerifyResult)]
    lib.amc_verify_result_free.restype = None
    lib.amc_match_guided_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_double,
                                           C.POINTER(MatchOpts), C.POINTER(MatchResult)]
    lib.amc_upload_points_f64.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    lib.amc_ransac_pairs.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_void_p, C.POINTER(RansacOpts), C.c_uint32, C.POINTER(RansacResult)]
    lib.amc_ransac_result_free.argtypes = [C.POINTER(RansacResult)]
    lib.amc_ransac_result_free.restype = None
    lib.amc_cam_from_img.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
    if hasattr(lib, "amc_img_from_cam"):   # (absent from a library built from an older revision: tools/ab_prev_lib.sh)
        lib.amc_img_from_cam.argtypes = lib.amc_cam_from_img.argtypes
    lib.amc_squared_sampson_error.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                              C.c_void_p]
    lib.amc_pose_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]
    if hasattr(lib, "amc_homography_decomposition"):
        lib.amc_homography_decomposition.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_size_t] + [C.c_void_p] * 5
    if hasattr(lib, "amc_comm_create"):
        lib.amc_comm_unique_id.argtypes = [C.c_void_p]
        lib.amc_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        lib.amc_comm_destroy.argtypes = [C.c_void_p]
        lib.amc_comm_destroy.restype = None
        lib.amc_allgather_match_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                   C.c_int, C.POINTER(GatheredTables)]
        lib.amc_gathered_tables_free.argtypes = [C.POINTER(GatheredTables)]
        lib.amc_gathered_tables_free.restype = None
    if hasattr(lib, "amc_allgather_pair_records"):
        lib.amc_allgather_pair_records.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                   C.c_int, C.POINTER(GatheredRecords)]
        lib.amc_gathered_records_free.argtypes = [C.POINTER(GatheredRecords)]
        lib.amc_gathered_records_free.restype = None
        lib.amc_allgather_inlier_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int,
                                                    C.POINTER(GatheredTables)]
    _lib = lib
    return lib


def _check(rc: int) -> None:
    if rc != AMC_OK:
        raise AmcError(rc, load().amc_last_error().decode(errors="replace"))


def tvg_options(**kw) -> TvgOpts:
    """TwoViewGeometryOptions with COLMAP's C++ defaults; keyword overrides; `ransac` may be a
    dict of RANSACOptions fields."""
    o = TvgOpts()
    load().amc_tvg_opts_default(C.byref(o))
    for k, v in kw.items():
        if k == "ransac":
            for rk, rv in v.items():
                assert hasattr(o.ransac, rk), rk
                setattr(o.ransac, rk, rv)
        else:
            assert hasattr(o, k), k
            setattr(o, k, v)
    return o


def device_count() -> int:
    n = load().amc_device_count()
    if n < 0:
        _check(n)
    return n


def comm_unique_id() -> bytes:
    """amc_comm_unique_id (ncclGetUniqueId): one rank calls it, every rank passes the bytes to Context.comm_create."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(load().amc_comm_unique_id(buf))
    return buf.raw


class Comm:
    """One amc_comm: this context's rank in the RCCL communicator of the exchange step (include/amc.h)."""

    def __init__(self, ctx: "Context", world_size: int, rank: int, unique_id: bytes):
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError(f"unique_id must be {COMM_ID_BYTES} bytes")
        self._lib, self._ctx = ctx._lib, ctx
        self.world_size, self.rank = int(world_size), int(rank)
        h = C.c_void_p()
        _check(self._lib.amc_comm_create(ctx._h, int(world_size), int(rank), unique_id, C.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None) and getattr(self._ctx, "_h", None):
            self._lib.amc_comm_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _tables_out(self, res, download):
        try:
            g_off = np.ctypeslib.as_array(res.offsets, shape=(int(res.npairs) + 1,)).copy()
            total = int(res.num_matches)
            g_m = None
            if download:
                g_m = (np.ctypeslib.as_array(res.matches, shape=(total, 2)).copy() if total
                       else np.zeros((0, 2), dtype=np.uint32))
            stats = {k: float(getattr(res, k)) for k in ("sizes_ms", "meta_ms", "rows_ms", "reorder_ms", "download_ms", "total_ms")}
            stats.update(num_matches=total, rows_sent=int(res.rows_sent), rows_received=int(res.rows_received),
                         world_size=int(res.world_size), rank=int(res.rank), device_ptr=int(res.matches_device or 0),
                         gather_path="C ABI: ncclAllGather (sizes) + grouped ncclSend/ncclRecv (records, rows) from device memory")
        finally:
            self._lib.amc_gathered_tables_free(C.byref(res))
        return g_off, g_m, stats

    def allgather_match_tables(self, pair_index, offsets, matches=None, download: bool = True):
        """amc_allgather_match_tables (collective).  pair_index: global positions of this rank's pairs, or None (the
        ranks' lists are appended in rank order); offsets: this rank's CSR; matches: this rank's rows on the host, or
        None = the context's device-resident table of the last match call.  Returns (global offsets uint64, global
        matches [M, 2] uint32 or None when download is False, stats dict incl. the device pointer of the table).

        Arguments this wrapper itself finds wrong (shapes, a `matches` array that does not hold offsets[-1] rows - the C
        entry point takes no length and would read past it) do NOT raise here, before the collective: the other ranks
        would wait for this one for ever.  The rank enters the exchange with offsets the library rejects ([1, 0]:
        "offsets[0] != 0"), so that every rank raises together; the local reason is appended to this rank's message."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        n = off.size - 1
        idx = None if pair_index is None else np.ascontiguousarray(pair_index, dtype=np.uint64)
        m = None if matches is None else np.ascontiguousarray(matches, dtype=np.uint32).reshape(-1, 2)
        local = None
        if n < 0:
            local = "offsets must have npairs + 1 entries"
        elif idx is not None and idx.shape != (n,):
            local = "one global position per local pair"
        elif m is not None and m.shape[0] != int(off[-1]) - int(off[0]):
            local = "offsets and matches disagree (%d rows for offsets[-1] = %d)" % (m.shape[0], int(off[-1]))
        if local is not None:   # poisoned entry: a one-pair CSR the library refuses collectively
            off, n, idx, m = np.array([1, 0], dtype=np.uint64), 1, None, np.zeros((1, 2), dtype=np.uint32)
        res = GatheredTables()
        rc = self._lib.amc_allgather_match_tables(
            self._ctx._h, self._h, None if idx is None else idx.ctypes.data_as(C.c_void_p), n,
            off.ctypes.data_as(C.c_void_p), None if m is None else m.ctypes.data_as(C.c_void_p), 1 if download else 0,
            C.byref(res))
        if local is not None:
            raise AmcError(rc if rc != AMC_OK else AMC_E_INVALID, "amc_allgather_match_tables: " + local)
        _check(rc)
        return self._tables_out(res, download)

    def allgather_pair_records(self, pair_index, records=None, download: bool = True, dtype=None):
        """amc_allgather_pair_records (collective): one fixed-size record per pair of every rank, in the global pair
        order.  records: a 1-D structured / plain array with one element per local pair (itemsize a multiple of 8), or
        None = the amc_tvg records of this context's last verification call, read in device memory (then pair_index
        must have that call's number of pairs and the result has TVG_DTYPE).  Returns (records of all pairs or None when
        download is False, stats)."""
        idx = None if pair_index is None else np.ascontiguousarray(pair_index, dtype=np.uint64).reshape(-1)
        rec = None if records is None else np.ascontiguousarray(records).reshape(-1)
        rdt = TVG_DTYPE if rec is None else rec.dtype
        if dtype is not None:
            rdt = np.dtype(dtype)
        n = len(rec) if rec is not None else (len(idx) if idx is not None else 0)
        width = rdt.itemsize
        if rec is not None and idx is not None and len(idx) != n:   # (collective error, as above: a record size the library refuses)
            width, bad = 4, "one global position per local record"
        else:
            bad = None
        res = GatheredRecords()
        rc = self._lib.amc_allgather_pair_records(
            self._ctx._h, self._h, None if idx is None else idx.ctypes.data_as(C.c_void_p), n,
            None if rec is None else rec.ctypes.data_as(C.c_void_p), width, 1 if download else 0, C.byref(res))
        if bad is not None:
            raise AmcError(rc if rc != AMC_OK else AMC_E_INVALID, "amc_allgather_pair_records: " + bad)
        _check(rc)
        try:
            total = int(res.npairs)
            out = None
            if download:
                out = (np.frombuffer(C.string_at(res.records, total * width), dtype=rdt).copy() if total
                       else np.zeros(0, dtype=rdt))
            stats = dict(npairs=total, record_bytes=int(res.record_bytes), bytes_sent=int(res.bytes_sent),
                         bytes_received=int(res.bytes_received), world_size=int(res.world_size), rank=int(res.rank),
                         total_ms=float(res.total_ms), device_ptr=int(res.records_device or 0))
        finally:
            self._lib.amc_gathered_records_free(C.byref(res))
        return out, stats

    def allgather_inlier_tables(self, pair_index, npairs_local: int | None = None, download: bool = True):
        """amc_allgather_inlier_tables (collective): the inlier matches of this context's last verification call
        (compacted on the device from the match table and the masks), of every rank, in the global pair order - the
        `two_view_geometries.data` blobs.  Returns what allgather_match_tables returns."""
        idx = None if pair_index is None else np.ascontiguousarray(pair_index, dtype=np.uint64).reshape(-1)
        n = len(idx) if idx is not None else int(npairs_local or 0)
        res = GatheredTables()
        _check(self._lib.amc_allgather_inlier_tables(self._ctx._h, self._h, None if idx is None else idx.ctypes.data_as(C.c_void_p),
                                                     n, 1 if download else 0, C.byref(res)))
        return self._tables_out(res, download)


class Context:
    """One amc_ctx (one GPU). Owns device copies of every uploaded image."""

    def comm_create(self, world_size: int, rank: int, unique_id: bytes) -> Comm:
        """amc_comm_create (collective over the ranks that share `unique_id`)."""
        import weakref
        comm = Comm(self, world_size, rank, unique_id)
        self.__dict__.setdefault("_comms", []).append(weakref.ref(comm))   # closed with the context, before it
        return comm

    def __init__(self, device_id: int = 0):
        self._lib = load()
        h = C.c_void_p()
        _check(self._lib.amc_ctx_create(device_id, C.byref(h)))
        self._h = h
        self.device_id = device_id
        # Bumped by everything that may free or overwrite the resident match table (a match call of any kind, trim,
        # close).  A holder of resident_matches_tensor() - memory the library owns - records it when it takes the view
        # and checks it (resident_view_valid) before / after it hands the view to anything asynchronous.
        self.resident_generation = 0

    def close(self) -> None:
        self.resident_generation = getattr(self, "resident_generation", 0) + 1
        for ref in self.__dict__.pop("_comms", []):
            comm = ref()
            if comm is not None:
                comm.close()
        if getattr(self, "_h", None):
            self._lib.amc_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_stream(self, hip_stream: int | None) -> None:
        _check(self._lib.amc_ctx_set_stream(self._h, C.c_void_p(hip_stream or 0)))

    def last_timeline(self) -> dict:
        """amc_ctx_last_timeline: the host-side timeline of the last match_verify_pairs call (ms since its entry)."""
        buf = (C.c_double * 8)()
        _check(self._lib.amc_ctx_last_timeline(self._h, buf))
        return dict(verify_setup_done=buf[0], match_returned=buf[1], verify_launched=buf[2], verify_results_on_host=buf[3],
                    call_returned=buf[4], batch_handover_host_ms_hidden=buf[5])

    def resident_matches(self):
        """(device pointer, number of matches) of the last match call's table in device memory (amc_ctx_resident_matches):
        CSR order of that call's result, valid until the next match call / trim / close."""
        ptr, n = C.c_void_p(), C.c_uint64()
        _check(self._lib.amc_ctx_resident_matches(self._h, C.byref(ptr), C.byref(n)))
        return int(ptr.value or 0), int(n.value)

    def upload_matches(self, matches) -> int:
        """Match rows (uint32 [n, 2], the CSR order of the pair list they belong to) into the resident match table
        (amc_upload_matches): verify_pairs(..., matches=None) reads them there - once, or again with other options -
        instead of taking them over PCIe in every call.  Returns the number of rows."""
        m = np.ascontiguousarray(matches, dtype=np.uint32).reshape(-1, 2)
        self.resident_generation += 1
        _check(self._lib.amc_upload_matches(self._h, m.ctypes.data_as(C.c_void_p), C.c_uint64(m.shape[0])))
        return int(m.shape[0])

    def resident_view_valid(self, generation: int) -> bool:
        """True while a view taken at `generation` (= self.resident_generation at that time) still points at live memory."""
        return generation == self.resident_generation and bool(getattr(self, "_h", None))

    def resident_matches_tensor(self, device_index: int = 0, copy: bool = False):
        """The same table as a torch int32 [n, 2] tensor.  copy=False: it ALIASES the library's device memory (no copy) -
        what the exchange step hands to RCCL - and dies with the next match call / trim / close of this context: note
        `self.resident_generation` when taking it and check `resident_view_valid()` before relying on it (bench.py and
        tools/dist_smoke.py do, around their collectives).  copy=True: a private clone, valid for as long as it is held."""
        import torch
        ptr, n = self.resident_matches()
        if n == 0:
            return torch.zeros((0, 2), dtype=torch.int32, device=torch.device("cuda", device_index))
        if copy:
            return self.resident_matches_tensor(device_index, copy=False).clone()

        class _View:   # numpy-style CUDA array interface over the raw pointer (uint32 bit patterns viewed as int32)
            __cuda_array_interface__ = {"shape": (n, 2), "typestr": "<i4", "data": (ptr, False), "version": 3, "strides": None}
        return torch.as_tensor(_View(), device=torch.device("cuda", device_index))

    def trim(self) -> None:
        """Release per-call scratch, staging buffers and idle result buffers (amc_ctx_trim); uploaded images stay."""
        self.resident_generation += 1
        _check(self._lib.amc_ctx_trim(self._h))

    def reserve_slots(self, n: int) -> None:
        _check(self._lib.amc_ctx_reserve_slots(self._h, n))

    def grow_slots(self, n: int) -> None:
        """Append empty slots up to n, keeping every uploaded image."""
        _check(self._lib.amc_ctx_grow_slots(self._h, n))

    def upload_descriptors(self, slot: int, desc: np.ndarray) -> None:
        d = np.ascontiguousarray(desc, dtype=np.uint8)
        if d.size and (d.ndim != 2 or d.shape[1] != 128):
            raise ValueError(f"descriptors must be N x 128 uint8, got {d.shape}")
        rows = d.shape[0] if d.ndim == 2 else 0
        _check(self._lib.amc_upload_descriptors(self._h, slot, d.ctypes.data_as(C.c_void_p), rows))

    def upload_descriptors_device(self, slot: int, dev_ptr: int, rows: int) -> None:
        _check(self._lib.amc_upload_descriptors_device(self._h, slot, C.c_void_p(dev_ptr), rows))

    def sift_extract(self, images, **opts):
        """amc_sift_extract on a batch of 2-D uint8 images (or one).  Keyword options are amc_sift_opts fields
        (normalization: "L1_ROOT" / "L2" or 0 / 1); the rest keep amc_sift_opts_default.  Returns (list of
        (N x 4 float32 keypoints (x, y, scale, orientation), N x 128 uint8 descriptors) per image, stats dict)."""
        single = isinstance(images, np.ndarray)
        imgs = [im if isinstance(im, np.ndarray) and im.ndim == 2 and im.strides[1] == 1 and im.strides[0] >= im.shape[1]
                else np.ascontiguousarray(im) for im in ([images] if single else images)]
        for im in imgs:
            if im.dtype != np.uint8 or im.ndim != 2:
                raise ValueError(f"sift_extract: images must be 2-D uint8, got {im.dtype} {im.shape}")
        o = SiftOpts()
        self._lib.amc_sift_opts_default(C.byref(o))
        for k, v in opts.items():
            if k == "normalization" and isinstance(v, str):
                v = SIFT_NORMALIZATIONS[v]
            if k not in dict(SiftOpts._fields_):
                raise ValueError(f"sift_extract: unknown option {k!r}")
            setattr(o, k, type(getattr(o, k))(v) if not isinstance(v, bool) else int(v))
        arr = (SiftImage * max(1, len(imgs)))()
        for i, im in enumerate(imgs):
            arr[i] = SiftImage(im.ctypes.data, im.shape[1], im.shape[0], im.strides[0])
        res = SiftResult()
        _check(self._lib.amc_sift_extract(self._h, arr, len(imgs), C.byref(o), C.byref(res)))
        try:
            off = np.ctypeslib.as_array(res.offsets, (len(imgs) + 1,)).copy()
            n = int(off[-1])
            kp = np.ctypeslib.as_array(res.keypoints, (max(n, 1), 4))[:n].copy()
            desc = np.ctypeslib.as_array(res.descriptors, (max(n, 1), 128))[:n].copy()
            stats = {"device_ms": res.device_ms, "stage_ms": dict(zip(SIFT_STAGES, list(res.stage_ms)))}
        finally:
            self._lib.amc_sift_result_free(C.byref(res))
        out = [(kp[off[i]:off[i + 1]], desc[off[i]:off[i + 1]]) for i in range(len(imgs))]
        return (out[0] if single else out), stats

    def estimate_absolute_poses(self, offsets, camera_models, camera_params, points2D, points3D, estimation=None,
                                refinement=None, return_covariance=False):
        """amc_estimate_absolute_poses: one LO-RANSAC per focal-length factor and one refinement per query (DESIGN.md
        section 12).  offsets: (Q + 1,) CSR over the correspondences; camera_models: (Q,) COLMAP model ids;
        camera_params: Q parameter vectors; points2D: (N, 2) pixels; points3D: (N, 3).  estimation / refinement: dicts
        of amc_abspose_opts / amc_abspose_refine_opts fields (the rest keep their defaults).  Returns a dict: success
        (Q,) bool, qvec (Q, 4) x y z w, tvec (Q, 3), num_inliers, num_trials, focal_factor, inlier_mask (N,) bool,
        covariance (Q, 6, 6) when asked, device_ms, kernel_ms, num_batches."""
        off, models, prm, p2, p3 = abspose_inputs(offsets, camera_models, camera_params, points2D, points3D)
        eo, ro = abspose_options(estimation, refinement)
        res = AbsPoseResult()
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        _check(self._lib.amc_estimate_absolute_poses(self._h, ptr(off), off.size - 1, ptr(models), ptr(prm), ptr(p2),
                                                      ptr(p3), C.byref(eo), C.byref(ro), int(bool(return_covariance)),
                                                      C.byref(res)))
        return self._abspose_out(res, off.size - 1, int(off[-1]), return_covariance)

    def refine_absolute_poses(self, offsets, camera_models, camera_params, points2D, points3D, qvec, tvec, inlier_mask,
                              refinement=None, return_covariance=False):
        """amc_refine_absolute_poses: RefineAbsolutePose per query from the poses qvec (Q, 4) x y z w, tvec (Q, 3) over
        the correspondences inlier_mask (N,) marks; the rest as estimate_absolute_poses, same result dict."""
        off, models, prm, p2, p3 = abspose_inputs(offsets, camera_models, camera_params, points2D, points3D)
        nq, n = off.size - 1, int(off[-1])
        q = np.ascontiguousarray(qvec, dtype=np.float64).reshape(-1, 4)
        t = np.ascontiguousarray(tvec, dtype=np.float64).reshape(-1, 3)
        m = np.ascontiguousarray(inlier_mask, dtype=bool).reshape(-1).astype(np.uint8)
        if q.shape[0] != nq or t.shape[0] != nq or m.size != n:
            raise ValueError(f"refine_absolute_poses: {nq} queries and {n} correspondences by offsets, {q.shape[0]} "
                             f"rotations, {t.shape[0]} translations, {m.size} mask entries")
        _, ro = abspose_options(None, refinement)
        res = AbsPoseResult()
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        _check(self._lib.amc_refine_absolute_poses(self._h, ptr(off), nq, ptr(models), ptr(prm), ptr(p2), ptr(p3),
                                                    ptr(q), ptr(t), ptr(m), C.byref(ro), int(bool(return_covariance)),
                                                    C.byref(res)))
        return self._abspose_out(res, nq, n, return_covariance)

    def _abspose_out(self, res, nq, n, cov):
        try:
            a = lambda p, shape: np.ctypeslib.as_array(p, (max(shape[0], 1),) + shape[1:])[:shape[0]].copy()  # noqa: E731
            out = {"success": a(res.success, (nq,)).astype(bool), "qvec": a(res.qvec, (nq, 4)),
                   "tvec": a(res.tvec, (nq, 3)), "num_inliers": a(res.num_inliers, (nq,)),
                   "num_trials": a(res.num_trials, (nq,)), "focal_factor": a(res.focal_factor, (nq,)),
                   "inlier_mask": a(res.inlier_mask, (n,)).astype(bool), "device_ms": res.device_ms,
                   "kernel_ms": res.kernel_ms, "num_batches": int(res.num_batches)}
            if cov:
                out["covariance"] = a(res.covariance, (nq, 36)).reshape(nq, 6, 6)
        finally:
            self._lib.amc_abspose_result_free(C.byref(res))
        return out

    def estimate_poses_and_cameras(self, offsets, camera_models, camera_params, points2D, points3D, estimation=None,
                                   refinement=None, return_covariance=False):
        """amc_estimate_poses_and_cameras: estimate_absolute_poses' LO-RANSAC per focal-length factor, then one joint
        refinement of the RANSAC's pose and the scaled camera.  refinement's refine_focal_length
        / refine_extra_params are honoured.  Returns estimate_absolute_poses' dict plus camera_params (Q, 12)."""
        off, models, prm, p2, p3 = abspose_inputs(offsets, camera_models, camera_params, points2D, points3D)
        eo, ro = abspose_options(estimation, refinement)
        res = AbsRefineResult()
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        _check(self._lib.amc_estimate_poses_and_cameras(self._h, ptr(off), off.size - 1, ptr(models), ptr(prm),
                                                         ptr(p2), ptr(p3), C.byref(eo), C.byref(ro),
                                                         int(bool(return_covariance)), C.byref(res)))
        return self._absrefine_out(res, off.size - 1, int(off[-1]), return_covariance)

    def refine_poses_and_cameras(self, offsets, camera_models, camera_params, points2D, points3D, qvec, tvec,
                                 inlier_mask, refinement=None, return_covariance=False):
        """amc_refine_poses_and_cameras: refine_absolute_poses with the camera's focal lengths (refine_focal_length) and
        extra parameters (refine_extra_params) refined with the pose; the same dict plus camera_params (Q, 12): the
        refined camera of a successful query, the input of a failed one."""
        off, models, prm, p2, p3 = abspose_inputs(offsets, camera_models, camera_params, points2D, points3D)
        nq, n = off.size - 1, int(off[-1])
        q = np.ascontiguousarray(qvec, dtype=np.float64).reshape(-1, 4)
        t = np.ascontiguousarray(tvec, dtype=np.float64).reshape(-1, 3)
        m = np.ascontiguousarray(inlier_mask, dtype=bool).reshape(-1).astype(np.uint8)
        if q.shape[0] != nq or t.shape[0] != nq or m.size != n:
            raise ValueError(f"refine_poses_and_cameras: {nq} queries and {n} correspondences by offsets, {q.shape[0]} "
                             f"rotations, {t.shape[0]} translations, {m.size} mask entries")
        _, ro = abspose_options(None, refinement)
        res = AbsRefineResult()
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        _check(self._lib.amc_refine_poses_and_cameras(self._h, ptr(off), nq, ptr(models), ptr(prm), ptr(p2), ptr(p3),
                                                       ptr(q), ptr(t), ptr(m), C.byref(ro),
                                                       int(bool(return_covariance)), C.byref(res)))
        return self._absrefine_out(res, nq, n, return_covariance)

    def _absrefine_out(self, res, nq, n, cov):
        try:
            a = lambda p, shape: np.ctypeslib.as_array(p, (max(shape[0], 1),) + shape[1:])[:shape[0]].copy()  # noqa: E731
            out = {"success": a(res.success, (nq,)).astype(bool), "qvec": a(res.qvec, (nq, 4)),
                   "tvec": a(res.tvec, (nq, 3)), "num_inliers": a(res.num_inliers, (nq,)),
                   "num_trials": a(res.num_trials, (nq,)), "focal_factor": a(res.focal_factor, (nq,)),
                   "inlier_mask": a(res.inlier_mask, (n,)).astype(bool),
                   "camera_params": a(res.camera_params, (nq, 12)), "device_ms": res.device_ms,
                   "kernel_ms": res.kernel_ms, "num_batches": int(res.num_batches)}
            if cov:
                out["covariance"] = a(res.covariance, (nq, 36)).reshape(nq, 6, 6)
        finally:
            self._lib.amc_absrefine_result_free(C.byref(res))
        return out

    def bundle_adjust(self, camera_models, camera_params, camera_const, image_cameras, qvec, tvec, pose_const, xyz,
                      obs_image, obs_point, obs_xy, options=None, point_const=None):
        """amc_bundle_adjust: Levenberg-Marquardt over every pose, point and camera at once.
        camera_models (C,), camera_params: C parameter vectors, camera_const (C, <= 12) non-zero = constant;
        image_cameras (I,) camera indices, qvec (I, 4) x y z w, tvec (I, 3), pose_const (I, 6) over the tangent
        (rotation 3, translation 3); xyz (P, 3); obs_image / obs_point (N,), obs_xy (N, 2) pixels.  options: a dict of
        amc_ba_opts fields.  point_const (P,): non-zero = the point is constant (amc_bundle_adjust_masked, 15.12); None
        = amc_bundle_adjust.  The inputs are not modified.  Returns a dict: camera_params (C, 12), qvec, tvec, xyz and
        the statistics of amc_ba_result (termination as a name)."""
        models, prm, cc, icam, q, t, pc, X, oi, op, xy = ba_inputs(camera_models, camera_params, camera_const,
                                                                   image_cameras, qvec, tvec, pose_const, xyz,
                                                                   obs_image, obs_point, obs_xy)
        o = ba_options(options)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        pb = BaProblem(models.size, ptr(models), ptr(prm), ptr(cc), icam.size, ptr(icam), ptr(q), ptr(t), ptr(pc),
                       X.shape[0], ptr(X), oi.size, ptr(oi), ptr(op), ptr(xy))
        res = BaResult()
        if point_const is None:
            _check(self._lib.amc_bundle_adjust(self._h, C.byref(pb), C.byref(o), C.byref(res)))
        else:
            mask = np.ascontiguousarray(np.asarray(point_const).reshape(-1) != 0, dtype=np.uint8)
            if mask.size != X.shape[0]:
                raise ValueError(f"bundle adjustment: {X.shape[0]} points, {mask.size} point_const flags")
            _check(self._lib.amc_bundle_adjust_masked(self._h, C.byref(pb), ptr(mask), C.byref(o), C.byref(res)))
        out = {k: getattr(res, k) for k, _ in BaResult._fields_}
        out["termination"] = BA_TERMINATIONS[res.termination]
        out.update(camera_params=prm, qvec=q, tvec=t, xyz=X)
        return out

    def ba_covariance(self, camera_models, camera_params, camera_const, image_cameras, qvec, tvec, pose_const, xyz,
                      obs_image, obs_point, obs_xy, options=None, point_const=None):
        """amc_ba_covariance: the covariance of the variable columns of bundle_adjust's flat problem at the parameters
        given; the arguments are bundle_adjust's, options a dict of amc_bacov_opts fields.
        Nothing is refined and the inputs are not modified.  Returns a dict: success, failed_column, num_columns,
        min_pivot_ratio, column_owner / column_coord (m,), and on success matrix (m, m) with want_matrix and
        point_present (P,) bool / point_cov (P, 3, 3) with want_points (None otherwise); host_ms, device_ms,
        kernel_ms, copy_ms and phase_ms by BACOV_PHASES."""
        models, prm, cc, icam, q, t, pc, X, oi, op, xy, mask = bacov_inputs(
            camera_models, camera_params, camera_const, image_cameras, qvec, tvec, pose_const, xyz, obs_image,
            obs_point, obs_xy, point_const)
        o = bacov_options(options)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        pb = BaProblem(models.size, ptr(models), ptr(prm), ptr(cc), icam.size, ptr(icam), ptr(q), ptr(t), ptr(pc),
                       X.shape[0], ptr(X), oi.size, ptr(oi), ptr(op), ptr(xy))
        res = BacovResult()
        _check(self._lib.amc_ba_covariance(self._h, C.byref(pb), None if mask is None else ptr(mask), C.byref(o),
                                           C.byref(res)))
        try:
            m, npts = int(res.num_columns), X.shape[0]
            a = lambda p, k: np.ctypeslib.as_array(p, (max(k, 1),))[:k].copy()  # noqa: E731
            out = {"success": bool(res.success), "failed_column": int(res.failed_column), "num_columns": m,
                   "min_pivot_ratio": float(res.min_pivot_ratio), "column_owner": a(res.column_owner, m),
                   "column_coord": a(res.column_coord, m), "matrix": None, "point_present": None, "point_cov": None,
                   "host_ms": res.host_ms, "device_ms": res.device_ms, "kernel_ms": res.kernel_ms,
                   "copy_ms": res.copy_ms, "phase_ms": dict(zip(BACOV_PHASES, res.phase_ms))}
            if res.matrix:
                out["matrix"] = a(res.matrix, m * m).reshape(m, m)
            if res.point_present:
                out["point_present"] = a(res.point_present, npts).astype(bool)
                out["point_cov"] = a(res.point_cov, 9 * npts).reshape(npts, 3, 3)
        finally:
            self._lib.amc_bacov_result_free(C.byref(res))
        return out

    def filter_points3d(self, camera_models, camera_params, image_cameras, qvec, tvec, xyz, track_offsets, obs_image,
                        obs_xy, selected=None, max_reproj_error=4.0, min_tri_angle=1.5, errors_only=False):
        """amc_filter_points3d: COLMAP's FilterPoints3D on a flat model.  camera_models (C,),
        camera_params: C parameter vectors; image_cameras (I,), qvec (I, 4) x y z w, tvec (I, 3); xyz (P, 3);
        track_offsets (P + 1,) CSR over the observations in track order, obs_image (N,), obs_xy (N, 2) pixels;
        selected (P,) non-zero = the point is filtered, None = every point.  errors_only: no thresholds and no
        verdicts, point_error is the mean over the whole track.  The inputs are not modified.  Returns a dict:
        obs_sq_error (N,), obs_deleted (N,) bool, point_verdict (P,) uint8 (FILTER_VERDICTS), point_error (P,),
        num_filtered, num_batches, host_ms, device_ms, kernel_ms, copy_ms, alloc_ms."""
        models, prm, icam, q, t, X, off, oi, xy, sel = filter_inputs(camera_models, camera_params, image_cameras, qvec,
                                                                     tvec, xyz, track_offsets, obs_image, obs_xy,
                                                                     selected)
        o = FilterOpts(float(max_reproj_error), float(min_tri_angle), int(bool(errors_only)), 0)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        pb = FilterProblem(models.size, ptr(models), ptr(prm), icam.size, ptr(icam), ptr(q), ptr(t), X.shape[0], ptr(X),
                           ptr(off), ptr(oi), ptr(xy), None if sel is None else ptr(sel))
        res = FilterResult()
        _check(self._lib.amc_filter_points3d(self._h, C.byref(pb), C.byref(o), C.byref(res)))
        try:
            n, npts = oi.size, X.shape[0]
            a = lambda p, k: np.ctypeslib.as_array(p, (max(k, 1),))[:k].copy()  # noqa: E731
            out = {"obs_sq_error": a(res.obs_sq_error, n), "obs_deleted": a(res.obs_deleted, n).astype(bool),
                   "point_verdict": a(res.point_verdict, npts), "point_error": a(res.point_error, npts),
                   "num_filtered": int(res.num_filtered), "num_batches": int(res.num_batches),
                   "host_ms": res.host_ms, "device_ms": res.device_ms, "kernel_ms": res.kernel_ms,
                   "copy_ms": res.copy_ms, "alloc_ms": res.alloc_ms}
        finally:
            self._lib.amc_filter_result_free(C.byref(res))
        return out

    def triangulate_observations(self, camera_models, camera_params, image_cameras, qvec, tvec, item_offsets, cand_image,
                                 cand_xy, cand_has_point, cand_xyz, no_create_two_view=None, create_max_angle_error=2.0,
                                 continue_max_angle_error=2.0, min_angle=1.5):
        """amc_triangulate_observations: Continue and the Create rounds of COLMAP's TriangulateImage for a batch of
        points2D.  camera_models (C,), camera_params: C parameter vectors; image_cameras (I,),
        qvec (I, 4) x y z w, tvec (I, 3); item_offsets (T + 1,) CSR over the candidates, an item's correspondences in
        Find's order and its reference observation last; cand_image (N,), cand_xy (N, 2) pixels, cand_has_point (N,),
        cand_xyz (N, 3); no_create_two_view (T,) or None.  The angles are in degrees.  The inputs are not modified.
        Returns a dict: continued (T,) int32 item-local candidate or -1, cand_round (N,) uint32, round_offsets (T + 1,),
        round_xyz (R, 3), num_created, num_continued, num_batches, host_ms, device_ms, kernel_ms, copy_ms, alloc_ms."""
        models, prm, icam, q, t, off, ci, xy, has, X, two = triobs_inputs(
            camera_models, camera_params, image_cameras, qvec, tvec, item_offsets, cand_image, cand_xy, cand_has_point,
            cand_xyz, no_create_two_view)
        o = TriobsOpts(float(create_max_angle_error), float(continue_max_angle_error), float(min_angle), 0.0)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        pb = TriobsProblem(models.size, ptr(models), ptr(prm), icam.size, ptr(icam), ptr(q), ptr(t), off.size - 1,
                           ptr(off), ptr(ci), ptr(xy), ptr(has), ptr(X), None if two is None else ptr(two))
        res = TriobsResult()
        _check(self._lib.amc_triangulate_observations(self._h, C.byref(pb), C.byref(o), C.byref(res)))
        try:
            nit, n, nr = off.size - 1, ci.size, int(res.num_created)
            a = lambda p, k: np.ctypeslib.as_array(p, (max(k, 1),))[:k].copy()  # noqa: E731
            out = {"continued": a(res.continued, nit), "cand_round": a(res.cand_round, n),
                   "round_offsets": a(res.round_offsets, nit + 1), "round_xyz": a(res.round_xyz, 3 * nr).reshape(nr, 3),
                   "num_created": nr, "num_continued": int(res.num_continued), "num_batches": int(res.num_batches),
                   "host_ms": res.host_ms, "device_ms": res.device_ms, "kernel_ms": res.kernel_ms,
                   "copy_ms": res.copy_ms, "alloc_ms": res.alloc_ms}
        finally:
            self._lib.amc_triobs_result_free(C.byref(res))
        return out

    def complete_tracks(self, camera_models, camera_params, image_cameras, qvec, tvec, item_xyz, item_offsets, cand_image,
                        cand_xy, complete_max_reproj_error=4.0):
        """amc_complete_tracks: the error test of COLMAP's CompleteTracks for every candidate observation of a batch of
        points.  camera_models (C,), camera_params: C parameter vectors; image_cameras (I,),
        qvec (I, 4) x y z w, tvec (I, 3); item_xyz (T, 3) the points; item_offsets (T + 1,) CSR over the candidates;
        cand_image (N,), cand_xy (N, 2) pixels.  The threshold is in pixels.  The inputs are not modified.  Returns a
        dict: cand_sq_error (N,), cand_pass (N,) bool, num_passed, num_batches, host_ms, device_ms, kernel_ms, copy_ms,
        alloc_ms."""
        models, prm, icam, q, t, X, off, ci, xy = complete_inputs(camera_models, camera_params, image_cameras, qvec, tvec,
                                                                  item_xyz, item_offsets, cand_image, cand_xy)
        o = CompleteOpts(float(complete_max_reproj_error), 0.0)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        pb = CompleteProblem(models.size, ptr(models), ptr(prm), icam.size, ptr(icam), ptr(q), ptr(t), off.size - 1,
                             ptr(X), ptr(off), ptr(ci), ptr(xy))
        res = CompleteResult()
        _check(self._lib.amc_complete_tracks(self._h, C.byref(pb), C.byref(o), C.byref(res)))
        try:
            n = ci.size
            a = lambda p, k: np.ctypeslib.as_array(p, (max(k, 1),))[:k].copy()  # noqa: E731
            out = {"cand_sq_error": a(res.cand_sq_error, n), "cand_pass": a(res.cand_pass, n).astype(bool),
                   "num_passed": int(res.num_passed), "num_batches": int(res.num_batches), "host_ms": res.host_ms,
                   "device_ms": res.device_ms, "kernel_ms": res.kernel_ms, "copy_ms": res.copy_ms,
                   "alloc_ms": res.alloc_ms}
        finally:
            self._lib.amc_complete_result_free(C.byref(res))
        return out

    def merge_tracks(self, camera_models, camera_params, image_cameras, qvec, tvec, comp_point_offsets, comp_root_offsets,
                     roots, point_xyz, point_obs_offsets, obs_image, obs_xy, obs_corr_offsets, corr_obs,
                     merge_max_reproj_error=4.0):
        """amc_merge_tracks: COLMAP's MergeTracks for the roots of a batch of connected components of points (DESIGN.md
        section 18).  The cameras and images as in complete_tracks; comp_point_offsets / comp_root_offsets (K + 1,) CSRs
        over the points / the roots; roots (R,) point indices; point_xyz (P, 3); point_obs_offsets (P + 1,) CSR over
        the observations in track order; obs_image (N,), obs_xy (N, 2) pixels; obs_corr_offsets (N + 1,) CSR over
        corr_obs (M,), the corresponding observations that carry a point.  The threshold is in pixels.  The inputs are
        not modified.  Returns a dict: root_return (R,), root_merge_offsets (R + 1,), merge_current and merge_other
        (S,) component slots, merge_xyz (S, 3), num_merges, num_pairs_tried, num_batches, host_ms, device_ms, kernel_ms,
        copy_ms, alloc_ms."""
        a = merge_inputs(camera_models, camera_params, image_cameras, qvec, tvec, comp_point_offsets, comp_root_offsets,
                         roots, point_xyz, point_obs_offsets, obs_image, obs_xy, obs_corr_offsets, corr_obs)
        models, prm, icam, q, t, cpo, cro, rt, X, poo, oi, xy, oco, co = a
        o = MergeOpts(float(merge_max_reproj_error), 0.0)
        ptr = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
        pb = MergeProblem(models.size, ptr(models), ptr(prm), icam.size, ptr(icam), ptr(q), ptr(t), cpo.size - 1, ptr(cpo),
                          ptr(cro), ptr(rt), ptr(X), ptr(poo), ptr(oi), ptr(xy), ptr(oco), ptr(co))
        res = MergeResult()
        _check(self._lib.amc_merge_tracks(self._h, C.byref(pb), C.byref(o), C.byref(res)))
        try:
            nr, nm = rt.size, int(res.num_merges)
            arr = lambda p, k: np.ctypeslib.as_array(p, (max(k, 1),))[:k].copy()  # noqa: E731
            out = {"root_return": arr(res.root_return, nr), "root_merge_offsets": arr(res.root_merge_offsets, nr + 1),
                   "merge_current": arr(res.merge_current, nm), "merge_other": arr(res.merge_other, nm),
                   "merge_xyz": arr(res.merge_xyz, 3 * nm).reshape(nm, 3), "num_merges": nm,
                   "num_pairs_tried": int(res.num_pairs_tried), "num_batches": int(res.num_batches),
                   "host_ms": res.host_ms, "device_ms": res.device_ms, "kernel_ms": res.kernel_ms,
                   "copy_ms": res.copy_ms, "alloc_ms": res.alloc_ms}
        finally:
            self._lib.amc_merge_result_free(C.byref(res))
        return out

    def retriangulate_pairs(self, camera_models, camera_params, image_cameras, qvec, tvec, obs_image, obs_xy, obs_point,
                            point_xyz, pair_images, pair_offsets, corr_obs, round_offsets, corr_two_view=None,
                            create_max_angle_error=2.0, re_max_angle_error=5.0, min_angle=1.5, re_min_ratio=0.2):
        """amc_retriangulate_pairs: COLMAP's Retriangulate for image pairs coloured into rounds.
        The cameras and images as in triangulate_observations; obs_image (N,), obs_xy (N, 2) pixels, obs_point (N,) the
        index of the point an observation carries or -1; point_xyz (P, 3); pair_images (K, 2); pair_offsets (K + 1,) CSR
        over corr_obs (M, 2), the observation of the pair's first and of its second image; round_offsets (R + 1,) CSR
        over the pairs, the pairs of a round sharing no image; corr_two_view (M,) or None.  The angles are in degrees.
        The inputs are not modified.  Returns a dict: pair_ran (K,) bool, pair_num_tri (K,), corr_action (M,) uint8
        (RETRI_*), created_offsets (K + 1,), created_xyz (S, 3), num_pairs_run, num_continued, num_created,
        num_launches, host_ms, device_ms, kernel_ms, copy_ms, alloc_ms."""
        a = retri_inputs(camera_models, camera_params, image_cameras, qvec, tvec, obs_image, obs_xy, obs_point, point_xyz,
                         pair_images, pair_offsets, corr_obs, round_offsets, corr_two_view)
        models, prm, icam, q, t, oi, xy, op, X, pi, poff, co, roff, two = a
        o = RetriOpts(float(create_max_angle_error), float(re_max_angle_error), float(min_angle), float(re_min_ratio))
        ptr = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
        pb = RetriProblem(models.size, ptr(models), ptr(prm), icam.size, ptr(icam), ptr(q), ptr(t), oi.size, ptr(oi),
                          ptr(xy), ptr(op), X.shape[0], ptr(X), pi.shape[0], ptr(pi), ptr(poff), ptr(co),
                          None if two is None else ptr(two), roff.size - 1, ptr(roff))
        res = RetriResult()
        _check(self._lib.amc_retriangulate_pairs(self._h, C.byref(pb), C.byref(o), C.byref(res)))
        try:
            npairs, nc, made = pi.shape[0], co.shape[0], int(res.num_created)
            arr = lambda p, k: np.ctypeslib.as_array(p, (max(k, 1),))[:k].copy()  # noqa: E731
            out = {"pair_ran": arr(res.pair_ran, npairs).astype(bool), "pair_num_tri": arr(res.pair_num_tri, npairs),
                   "corr_action": arr(res.corr_action, nc), "created_offsets": arr(res.created_offsets, npairs + 1),
                   "created_xyz": arr(res.created_xyz, 3 * made).reshape(made, 3), "num_pairs_run": int(res.num_pairs_run),
                   "num_continued": int(res.num_continued), "num_created": made, "num_launches": int(res.num_launches),
                   "host_ms": res.host_ms, "device_ms": res.device_ms, "kernel_ms": res.kernel_ms,
                   "copy_ms": res.copy_ms, "alloc_ms": res.alloc_ms}
        finally:
            self._lib.amc_retri_result_free(C.byref(res))
        return out

    def image_visibility(self, image_point_offsets, point2D_point3D, cand_width, cand_height, cand_point_offsets, cand_xy,
                         corr_offsets, corr_image, corr_point2D):
        """amc_image_visibility: for a batch of candidate images, what COLMAP's Image keeps incrementally (DESIGN.md
        section 20).  image_point_offsets (G + 1,) CSR over point2D_point3D (T,), the point3D id of every point2D of
        every graph image or MAPPER_NO_POINT3D; cand_width / cand_height (K,); cand_point_offsets (K + 1,) CSR over
        cand_xy (N, 2) pixels; corr_offsets (N + 1,) CSR over corr_image / corr_point2D (M,), graph image index and
        point2D index.  The inputs are not modified.  Returns a dict: num_observations, num_visible_points3D (K,)
        uint32, score (K,) uint64, max_score, num_batches, host_ms, device_ms, kernel_ms, copy_ms, alloc_ms."""
        ipoff, table, cw, ch, cpoff, xy, coff, ci, cp = visibility_inputs(
            image_point_offsets, point2D_point3D, cand_width, cand_height, cand_point_offsets, cand_xy, corr_offsets,
            corr_image, corr_point2D)
        ptr = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
        pb = VisibilityProblem(ipoff.size - 1, ptr(ipoff), ptr(table), cw.size, ptr(cw), ptr(ch), ptr(cpoff), ptr(xy),
                               ptr(coff), ptr(ci), ptr(cp))
        res = VisibilityResult()
        _check(self._lib.amc_image_visibility(self._h, C.byref(pb), C.byref(res)))
        try:
            k = cw.size
            arr = lambda p, n: np.ctypeslib.as_array(p, (max(n, 1),))[:n].copy()  # noqa: E731
            out = {"num_observations": arr(res.num_observations, k), "num_visible_points3D": arr(res.num_visible_points3D, k),
                   "score": arr(res.score, k), "max_score": int(res.max_score), "num_batches": int(res.num_batches),
                   "host_ms": res.host_ms, "device_ms": res.device_ms, "kernel_ms": res.kernel_ms,
                   "copy_ms": res.copy_ms, "alloc_ms": res.alloc_ms}
        finally:
            self._lib.amc_visibility_result_free(C.byref(res))
        return out

    def shared_point_angles(self, qvec, tvec, point_xyz, pair_images, pair_offsets, shared_points, percentile=75.0):
        """amc_shared_point_angles: per image pair the percentile of the triangulation angles at the points the two
        images share.  qvec (I, 4) x y z w, tvec (I, 3); point_xyz (P, 3); pair_images (K, 2);
        pair_offsets (K + 1,) CSR over shared_points (S,), point indices, every pair holding 1 .. MAPPER_MAX_PAIR_POINTS.
        The inputs are not modified.  Returns a dict: angle (K,) radians, num_batches, host_ms, device_ms, kernel_ms,
        copy_ms, alloc_ms."""
        q, t, X, pi, poff, sp = pair_angle_inputs(qvec, tvec, point_xyz, pair_images, pair_offsets, shared_points)
        ptr = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
        o = PairAngleOpts(float(percentile))
        pb = PairAngleProblem(q.shape[0], ptr(q), ptr(t), X.shape[0], ptr(X), pi.shape[0], ptr(pi), ptr(poff), ptr(sp))
        res = PairAngleResult()
        _check(self._lib.amc_shared_point_angles(self._h, C.byref(pb), C.byref(o), C.byref(res)))
        try:
            k = pi.shape[0]
            out = {"angle": np.ctypeslib.as_array(res.angle, (max(k, 1),))[:k].copy(), "num_batches": int(res.num_batches),
                   "host_ms": res.host_ms, "device_ms": res.device_ms, "kernel_ms": res.kernel_ms,
                   "copy_ms": res.copy_ms, "alloc_ms": res.alloc_ms}
        finally:
            self._lib.amc_pair_angle_result_free(C.byref(res))
        return out

    def triangulate_pairs(self, camera_models, camera_params, image_cameras, qvec, tvec, pair_images, pair_offsets, corr_xy1,
                          corr_xy2, min_tri_angle=INITPAIR_DEFAULT_MIN_TRI_ANGLE):
        """amc_triangulate_pairs: the two-view triangulation of every correspondence of a batch of image pairs, as
        COLMAP's RegisterInitialImagePair does it.  The cameras and images as in
        triangulate_observations; pair_images (K, 2); pair_offsets (K + 1,) CSR over corr_xy1 / corr_xy2 (M, 2), the
        pixels in the pair's first and second image.  min_tri_angle is in radians.  The inputs are not modified.
        Returns a dict: accepted (M,) bool, xyz (M, 3), tri_angle (M,) radians, num_accepted, num_batches, host_ms,
        device_ms, kernel_ms, copy_ms, alloc_ms."""
        models, prm, icam, q, t, pi, poff, xy1, xy2 = pair_tri_inputs(camera_models, camera_params, image_cameras, qvec, tvec,
                                                                      pair_images, pair_offsets, corr_xy1, corr_xy2)
        ptr = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
        o = PairTriOpts(float(min_tri_angle), 0.0)
        pb = PairTriProblem(models.size, ptr(models), ptr(prm), icam.size, ptr(icam), ptr(q), ptr(t), pi.shape[0], ptr(pi),
                            ptr(poff), ptr(xy1), ptr(xy2))
        res = PairTriResult()
        _check(self._lib.amc_triangulate_pairs(self._h, C.byref(pb), C.byref(o), C.byref(res)))
        try:
            n = xy1.shape[0]
            arr = lambda p, k: np.ctypeslib.as_array(p, (max(k, 1),))[:k].copy()  # noqa: E731
            out = {"accepted": arr(res.accepted, n).astype(bool), "xyz": arr(res.xyz, 3 * n).reshape(n, 3),
                   "tri_angle": arr(res.tri_angle, n), "num_accepted": int(res.num_accepted),
                   "num_batches": int(res.num_batches), "host_ms": res.host_ms, "device_ms": res.device_ms,
                   "kernel_ms": res.kernel_ms, "copy_ms": res.copy_ms, "alloc_ms": res.alloc_ms}
        finally:
            self._lib.amc_pair_tri_result_free(C.byref(res))
        return out

    def patch_match(self, images, K, R, t, ref_images, src_offsets, src_images, depth_ranges, in_depth=None, in_normal=None,
                    **options):
        """amc_patch_match: one pass of PatchMatch stereo over a list of problems.  The arrays as
        in patch_match_inputs; the options are the fields of amc_patch_match_opts (PATCHMATCH_DEFAULTS).  The inputs are
        not modified.  Returns a dict: depth, normal, num_consistent and (with want_costs) costs, each a list with one
        array per problem (H x W float32, 3 x H x W float32, H x W uint8, S x H x W float32), num_batches, num_launches,
        host_ms, device_ms, kernel_ms, copy_ms, alloc_ms."""
        o = patch_match_options(**options)
        pb, keep = patch_match_inputs(images, K, R, t, ref_images, src_offsets, src_images, depth_ranges, in_depth, in_normal)
        res = PatchMatchResult()
        _check(self._lib.amc_patch_match(self._h, C.byref(o), C.byref(pb), C.byref(res)))
        try:
            out = patch_match_unpack(keep, res.num_problems, res.map_offsets, res.cost_offsets, res.depth, res.normal,
                                     res.num_consistent, res.costs if o.want_costs else None)
            out.update({"num_batches": int(res.num_batches), "num_launches": int(res.num_launches), "host_ms": res.host_ms,
                        "device_ms": res.device_ms, "kernel_ms": res.kernel_ms, "copy_ms": res.copy_ms,
                        "alloc_ms": res.alloc_ms})
        finally:
            self._lib.amc_patch_match_result_free(C.byref(res))
        return out

    def fuse_depth_maps(self, images, K, R, t, depth_maps, normal_maps, neighbours, **options):
        """amc_fuse_depth_maps: the maps of an ordered list of images fused into points.  The
        arrays as in fusion_inputs; the options are the fields of amc_fusion_opts (FUSION_DEFAULTS).  The inputs are not
        modified.  Returns a dict: num_points, xyz (P, 3) float32, normal (P, 3) float32, color (P, 3) uint8, seed_image,
        seed_pixel, num_fused (P,) uint32, vis_offsets (P + 1,) uint64, vis_images uint32, num_seeds, num_truncated,
        num_batches, num_launches, host_ms, device_ms, kernel_ms, copy_ms, alloc_ms."""
        o = fusion_options(**options)
        pb, keep = fusion_inputs(images, K, R, t, depth_maps, normal_maps, neighbours)
        res = FusionResult()
        _check(self._lib.amc_fuse_depth_maps(self._h, C.byref(o), C.byref(pb), C.byref(res)))
        try:
            out = fusion_unpack(res.num_points, res.xyz, res.normal, res.color, res.seed_image, res.seed_pixel,
                                res.num_fused, res.vis_offsets, res.vis_images)
            out.update({"num_seeds": int(res.num_seeds), "num_truncated": int(res.num_truncated),
                        "num_batches": int(res.num_batches), "num_launches": int(res.num_launches), "host_ms": res.host_ms,
                        "device_ms": res.device_ms, "kernel_ms": res.kernel_ms, "copy_ms": res.copy_ms,
                        "alloc_ms": res.alloc_ms})
        finally:
            self._lib.amc_fusion_result_free(C.byref(res))
        return out

    def estimate_rig_absolute_poses(self, offsets, camera_offsets, camera_models, camera_params, cams_from_rig,
                                    camera_idxs, points2D, points3D, estimation=None, refinement=None,
                                    return_covariance=False):
        """amc_estimate_rig_absolute_poses: one RANSAC of the generalised P3P and one refinement of rig_from_world per
        query.  offsets / camera_offsets: (Q + 1,) CSR over the correspondences / the cameras;
        camera_models, camera_params, cams_from_rig (x y z w tx ty tz): one entry per camera; camera_idxs: (N,) indices
        into the query's own cameras; points2D: (N, 2) pixels; points3D: (N, 3).  estimation / refinement: dicts of
        amc_ransac_opts / amc_abspose_refine_opts fields.  Returns a dict: success (Q,) bool, qvec (Q, 4) x y z w,
        tvec (Q, 3), num_inliers (distinct 3D points), num_all_inliers, num_trials, inlier_mask (N,) bool, covariance
        (Q, 6, 6) when asked, device_ms, kernel_ms, num_batches."""
        off, coff, models, prm, rigs, idx, p2, p3 = rigpose_inputs(offsets, camera_offsets, camera_models,
                                                                   camera_params, cams_from_rig, camera_idxs,
                                                                   points2D, points3D)
        eo, ro = rigpose_options(estimation, refinement)
        nq, n = off.size - 1, int(off[-1])
        res = RigPoseResult()
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        _check(self._lib.amc_estimate_rig_absolute_poses(self._h, ptr(off), nq, ptr(coff), ptr(models), ptr(prm),
                                                          ptr(rigs), ptr(idx), ptr(p2), ptr(p3), C.byref(eo),
                                                          C.byref(ro), int(bool(return_covariance)), C.byref(res)))
        try:
            a = lambda p, shape: np.ctypeslib.as_array(p, (max(shape[0], 1),) + shape[1:])[:shape[0]].copy()  # noqa: E731
            out = {"success": a(res.success, (nq,)).astype(bool), "qvec": a(res.qvec, (nq, 4)),
                   "tvec": a(res.tvec, (nq, 3)), "num_inliers": a(res.num_inliers, (nq,)),
                   "num_all_inliers": a(res.num_all_inliers, (nq,)), "num_trials": a(res.num_trials, (nq,)),
                   "inlier_mask": a(res.inlier_mask, (n,)).astype(bool), "device_ms": res.device_ms,
                   "kernel_ms": res.kernel_ms, "num_batches": int(res.num_batches)}
            if return_covariance:
                out["covariance"] = a(res.covariance, (nq, 36)).reshape(nq, 6, 6)
        finally:
            self._lib.amc_rigpose_result_free(C.byref(res))
        return out

    def triangulate_tracks(self, poses, track_offsets, obs_pose, obs_xy, **opts):
        """amc_triangulate_tracks: one LO-RANSAC triangulation per track.
        poses: (P, 3, 4) float64 cam_from_world [R | t]; track_offsets: (T + 1,) CSR over the observations;
        obs_pose: (M,) pose index per observation; obs_xy: (M, 2) normalized image coordinates.  Keyword options
        are amc_tri_opts fields (min_tri_angle, max_error, min_inlier_ratio, confidence, dyn_num_trials_multiplier,
        min_num_trials, max_num_trials); the rest keep amc_tri_opts_default.  Returns (xyz (T, 3) float64,
        success (T,) bool, inlier_mask (M,) bool, stats dict with num_inliers, num_trials, device_ms, kernel_ms,
        num_batches)."""
        P = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12)
        off = np.ascontiguousarray(track_offsets, dtype=np.uint64).reshape(-1)
        if off.size < 1:
            raise ValueError("triangulate_tracks: track_offsets needs ntracks + 1 entries")
        nobs = int(off[-1])
        op = np.ascontiguousarray(obs_pose, dtype=np.uint32).reshape(-1)
        xy = np.ascontiguousarray(obs_xy, dtype=np.float64).reshape(-1, 2)
        if op.size != nobs or xy.shape[0] != nobs:
            raise ValueError(f"triangulate_tracks: {nobs} observations by track_offsets, {op.size} pose indices, "
                             f"{xy.shape[0]} points")
        o = TriOpts()
        self._lib.amc_tri_opts_default(C.byref(o))
        for k, v in opts.items():
            if k not in dict(TriOpts._fields_):
                raise ValueError(f"triangulate_tracks: unknown option {k!r}")
            setattr(o, k, type(getattr(o, k))(v))
        nt = off.size - 1
        res = TriResult()
        _check(self._lib.amc_triangulate_tracks(self._h, P.ctypes.data_as(C.c_void_p), P.shape[0],
                                                 off.ctypes.data_as(C.c_void_p), nt, op.ctypes.data_as(C.c_void_p),
                                                 xy.ctypes.data_as(C.c_void_p), C.byref(o), C.byref(res)))
        try:
            xyz = np.ctypeslib.as_array(res.xyz, (max(nt, 1), 3))[:nt].copy()
            ok = np.ctypeslib.as_array(res.success, (max(nt, 1),))[:nt].astype(bool)
            mask = np.ctypeslib.as_array(res.inlier_mask, (max(nobs, 1),))[:nobs].astype(bool)
            stats = {"num_inliers": np.ctypeslib.as_array(res.num_inliers, (max(nt, 1),))[:nt].copy(),
                     "num_trials": np.ctypeslib.as_array(res.num_trials, (max(nt, 1),))[:nt].copy(),
                     "device_ms": res.device_ms, "kernel_ms": res.kernel_ms, "num_batches": int(res.num_batches)}
        finally:
            self._lib.amc_tri_result_free(C.byref(res))
        return xyz, ok, mask, stats

    def undistort_images(self, images, src_cameras, dst_cameras):
        """amc_undistort_images: warp every image from its source camera onto its PINHOLE target.

        images: H x W or H x W x 3 uint8 arrays (the last axis contiguous, rows at any stride); cameras: (model name or
        id, width, height, params) each.  Returns (list of target arrays, stats dict with device_ms, kernel_ms,
        num_batches, num_resized)."""
        n = len(images)
        if len(src_cameras) != n or len(dst_cameras) != n:
            raise ValueError(f"undistort_images: {n} images, {len(src_cameras)} source and {len(dst_cameras)} target cameras")
        arr = (UndistortImage * max(n, 1))()
        keep, outs = [], []
        for i, im in enumerate(images):
            ok = (isinstance(im, np.ndarray) and im.dtype == np.uint8 and im.ndim in (2, 3) and im.size > 0
                  and (im.ndim == 2 or im.shape[2] in (1, 3)))
            if not ok:
                raise ValueError(f"undistort_images: image {i} must be a non-empty H x W or H x W x 3 uint8 array")
            ch = 1 if im.ndim == 2 else im.shape[2]
            packed = im.strides[-1] == 1 and (im.ndim == 2 or im.strides[1] == ch) and im.strides[0] >= im.shape[1] * ch
            a = im if packed else np.ascontiguousarray(im)
            keep.append(a)
            dc = _undistort_cam(dst_cameras[i])
            out = np.empty((int(dc.height), int(dc.width)) + ((ch,) if im.ndim == 3 else ()), dtype=np.uint8)
            outs.append(out)
            arr[i] = UndistortImage(a.ctypes.data, a.strides[0], ch, 0, _undistort_cam(src_cameras[i]), dc,
                                    out.ctypes.data if out.size else None)
        res = UndistortResult()
        _check(self._lib.amc_undistort_images(self._h, n, C.cast(arr, C.c_void_p), C.byref(res)))
        return outs, {"device_ms": res.device_ms, "kernel_ms": res.kernel_ms, "num_batches": int(res.num_batches),
                      "num_resized": int(res.num_resized)}

    def match_pairs(self, slot1, slot2, max_ratio: float = 0.8, max_distance: float = 0.7,
                    cross_check: bool = True, kernel: str = "auto", copy: bool = True):
        """Returns (offsets uint64[npairs+1], matches uint32[M,2], stats dict).  copy=False: the arrays are views of
        the library's pinned result buffer (freed when they are collected) instead of private copies."""
        s1 = np.ascontiguousarray(slot1, dtype=np.uint32)
        s2 = np.ascontiguousarray(slot2, dtype=np.uint32)
        if s1.shape != s2.shape or s1.ndim != 1:
            raise ValueError("slot1/slot2 must be equal-length 1-D arrays")
        opts = MatchOpts(max_ratio, max_distance, 1 if cross_check else 0, KERNELS[kernel])
        res = MatchResult()
        self.resident_generation += 1
        _check(self._lib.amc_match_pairs(self._h, s1.ctypes.data_as(C.c_void_p),
                                         s2.ctypes.data_as(C.c_void_p), s1.size, C.byref(opts),
                                         C.byref(res)))
        if not copy:
            # zero-copy views of the library's pinned result buffer (what a C++ caller reads): the arrays keep the
            # result alive and amc_match_result_free runs when the last of them is collected
            return self._unpack_match(res, _MatchLease(self._lib, res))
        try:
            offsets, matches, stats = self._unpack_match(res)
        finally:
            self._lib.amc_match_result_free(C.byref(res))
        return offsets, matches, stats

    @staticmethod
    def _unpack_match(res, lease=None):
        n = int(res.npairs)

        def view(ptr, count, dtype):   # a buffer over the address: no per-call ctypes array types, no element walk
            nbytes = count * np.dtype(dtype).itemsize
            return np.frombuffer((C.c_char * nbytes).from_address(C.addressof(ptr.contents)), dtype=dtype)

        offsets = view(res.offsets, n + 1, np.uint64)
        total = int(offsets[-1])
        offsets = offsets.copy() if lease is None else _LeasedArray.wrap(offsets, lease)
        if total:
            matches = view(res.matches, 2 * total, np.uint32).reshape(total, 2)
            matches = matches.copy() if lease is None else _LeasedArray.wrap(matches, lease)
        else:
            matches = np.zeros((0, 2), dtype=np.uint32)
        stats = dict(num_distances=int(res.num_distances), pairs_mfma=int(res.pairs_mfma),
                     pairs_dot4=int(res.pairs_dot4), device_ms=float(res.device_ms),
                     match_kernel_ms=float(res.match_kernel_ms),
                     cross_kernel_ms=float(res.cross_kernel_ms),
                     match_kernel_launches=int(res.match_kernel_launches), scan_run=int(res.scan_run))
        return offsets, matches, stats

    @staticmethod
    def _unpack_verify(res, total, labelled=False, lease=None):
        """The result as numpy arrays: copies (one per array), or - with a lease, which then owns the C result -
        views of the library's own buffers.  `labelled`: the mask holds geometry labels (multiple_models) rather
        than 0 / 1."""
        n = int(res.npairs)
        assert C.sizeof(Tvg) == TVG_DTYPE.itemsize

        def take(ptr, count, dtype):
            nbytes = count * np.dtype(dtype).itemsize
            if not nbytes:
                return np.zeros(0, dtype=dtype)
            addr = C.cast(ptr, C.c_void_p).value
            a = np.frombuffer((C.c_char * nbytes).from_address(addr), dtype=dtype)
            return a.copy() if lease is None else _LeasedArray.wrap(a, lease)

        tvg = take(res.tvg, n, TVG_DTYPE)
        labels = take(res.inlier_mask, total, np.uint8)
        mask = labels.astype(bool) if labelled else labels.view(np.bool_)   # 0 / 1 bytes are numpy bools as they are
        # inlier_labels: 1 + index of the geometry a match belongs to (multiple_models), else 0 / 1
        stats = dict(device_ms=float(res.device_ms), kernel_ms=float(res.kernel_ms), inlier_labels=labels,
                     kernel_launches=int(res.kernel_launches), work=[int(x) for x in res.work])
        stats["pose_kernel_ms"] = float(res.pose_kernel_ms)
        if res.pose:  # compute_relative_pose: one amc_pose per pair
            assert C.sizeof(Pose) == POSE_DTYPE.itemsize
            stats["pose"] = take(res.pose, n, POSE_DTYPE)
        return tvg, mask, stats

    def match_verify_pairs(self, slot1, slot2, opts: TvgOpts | None = None, seed: int = 0, max_ratio: float = 0.8,
                           max_distance: float = 0.7, cross_check: bool = True, kernel: str = "auto", copy: bool = True):
        """amc_match_verify_pairs: match every pair, then EstimateTwoViewGeometry on its matches where the matcher
        left them in HBM.  Returns (offsets, matches, match stats, tvg, inlier_mask, verify stats).  copy=False: the
        arrays are views of the library's result buffers (as a C++ caller reads them), each result released when the last
        array viewing it is garbage collected."""
        s1 = np.ascontiguousarray(slot1, dtype=np.uint32)
        s2 = np.ascontiguousarray(slot2, dtype=np.uint32)
        if s1.shape != s2.shape or s1.ndim != 1:
            raise ValueError("slot1/slot2 must be equal-length 1-D arrays")
        mo = MatchOpts(max_ratio, max_distance, 1 if cross_check else 0, KERNELS[kernel])
        o = opts or tvg_options()
        mres, vres = MatchResult(), VerifyResult()
        self.resident_generation += 1
        _check(self._lib.amc_match_verify_pairs(self._h, s1.ctypes.data_as(C.c_void_p), s2.ctypes.data_as(C.c_void_p),
                                                s1.size, C.byref(mo), C.byref(o), seed, C.byref(mres), C.byref(vres)))
        if not copy:
            offsets, matches, mstats = self._unpack_match(mres, _MatchLease(self._lib, mres))
            tvg, mask, vstats = self._unpack_verify(vres, matches.shape[0], bool(o.multiple_models),
                                                    _VerifyLease(self._lib, vres))
            return offsets, matches, mstats, tvg, mask, vstats
        try:
            offsets, matches, mstats = self._unpack_match(mres)
            tvg, mask, vstats = self._unpack_verify(vres, matches.shape[0], bool(o.multiple_models))
        finally:
            self._lib.amc_match_result_free(C.byref(mres))
            self._lib.amc_verify_result_free(C.byref(vres))
        return offsets, matches, mstats, tvg, mask, vstats

    def match_guided_pairs(self, slot1, slot2, tvg, max_error: float, max_ratio: float = 0.8,
                           max_distance: float = 0.7, cross_check: bool = True):
        """FeatureMatcher::MatchGuided per pair: `tvg` is a TVG_DTYPE array (config, F, H used), e.g.
        the output of verify_pairs.  Returns (offsets, matches, stats) like match_pairs."""
        s1 = np.ascontiguousarray(slot1, dtype=np.uint32)
        s2 = np.ascontiguousarray(slot2, dtype=np.uint32)
        g = np.ascontiguousarray(tvg, dtype=TVG_DTYPE)
        if s1.shape != s2.shape or s1.ndim != 1 or g.shape != s1.shape:
            raise ValueError("slot1/slot2/tvg must be equal-length 1-D arrays")
        assert C.sizeof(Tvg) == TVG_DTYPE.itemsize
        opts = MatchOpts(max_ratio, max_distance, 1 if cross_check else 0, KERNEL_AUTO)
        res = MatchResult()
        self.resident_generation += 1
        _check(self._lib.amc_match_guided_pairs(self._h, s1.ctypes.data_as(C.c_void_p),
                                                s2.ctypes.data_as(C.c_void_p), s1.size,
                                                g.ctypes.data_as(C.c_void_p), float(max_error), C.byref(opts),
                                                C.byref(res)))
        try:
            n = int(res.npairs)
            offsets = np.ctypeslib.as_array(res.offsets, shape=(n + 1,)).copy()
            total = int(offsets[-1])
            matches = (np.ctypeslib.as_array(res.matches, shape=(total, 2)).copy() if total
                       else np.zeros((0, 2), dtype=np.uint32))
            stats = dict(num_distances=int(res.num_distances), pairs_dot4=int(res.pairs_dot4),
                         pairs_guided_grid=int(res.pairs_guided_grid),
                         device_ms=float(res.device_ms))
        finally:
            self._lib.amc_match_result_free(C.byref(res))
        return offsets, matches, stats

    def upload_keypoints(self, slot: int, kp: np.ndarray) -> None:
        k = np.ascontiguousarray(kp, dtype=np.float32)
        if k.size and (k.ndim != 2 or k.shape[1] < 2):
            raise ValueError(f"keypoints must be N x (>=2) float32, got {k.shape}")
        rows = k.shape[0] if k.ndim == 2 else 0
        stride = k.shape[1] if k.ndim == 2 and rows else 2
        _check(self._lib.amc_upload_keypoints(self._h, slot, k.ctypes.data_as(C.c_void_p), rows, stride))

    def upload_points_f64(self, slot: int, pts: np.ndarray) -> None:
        """Double-precision image points (N x 2), as pycolmap's estimator bindings take them."""
        k = np.ascontiguousarray(pts, dtype=np.float64)
        if k.size and (k.ndim != 2 or k.shape[1] != 2):
            raise ValueError(f"points must be N x 2 float64, got {k.shape}")
        rows = k.shape[0] if k.ndim == 2 else 0
        _check(self._lib.amc_upload_points_f64(self._h, slot, k.ctypes.data_as(C.c_void_p), rows))

    def ransac_pairs(self, kind, slot1, slot2, match_offsets, matches, ransac: dict | RansacOpts | None = None,
                     seed: int = 0):
        """One LO-RANSAC (kind 'F' | 'H' | 'E') per pair. Returns (reports structured array [npairs],
        inlier_mask bool [total correspondences])."""
        s1 = np.ascontiguousarray(slot1, dtype=np.uint32)
        s2 = np.ascontiguousarray(slot2, dtype=np.uint32)
        off = np.ascontiguousarray(match_offsets, dtype=np.uint64)
        m = np.ascontiguousarray(matches, dtype=np.uint32).reshape(-1, 2)
        if off.shape != (s1.size + 1,) or s1.shape != s2.shape:
            raise ValueError("match_offsets must have npairs + 1 entries")
        if int(off[-1]) != m.shape[0]:
            raise ValueError("match_offsets[-1] must equal the number of matches")
        if isinstance(ransac, RansacOpts):
            ro = ransac
        else:
            ro = tvg_options(ransac=ransac or {}).ransac
        k = RANSAC_KINDS[kind] if isinstance(kind, str) else int(kind)
        res = RansacResult()
        _check(self._lib.amc_ransac_pairs(self._h, k, s1.ctypes.data_as(C.c_void_p), s2.ctypes.data_as(C.c_void_p),
                                          s1.size, off.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p),
                                          C.byref(ro), seed, C.byref(res)))
        try:
            n = int(res.npairs)
            assert C.sizeof(RansacReport) == RANSAC_DTYPE.itemsize
            rep = (np.frombuffer(C.string_at(res.reports, n * C.sizeof(RansacReport)), dtype=RANSAC_DTYPE).copy()
                   if n else np.zeros(0, dtype=RANSAC_DTYPE))
            total = m.shape[0]
            mask = (np.ctypeslib.as_array(res.inlier_mask, shape=(total,)).astype(bool) if total
                    else np.zeros(0, dtype=bool))
        finally:
            self._lib.amc_ransac_result_free(C.byref(res))
        return rep, mask

    def squared_sampson_error(self, points1, points2, E) -> np.ndarray:
        p1 = np.ascontiguousarray(points1, dtype=np.float64).reshape(-1, 2)
        p2 = np.ascontiguousarray(points2, dtype=np.float64).reshape(-1, 2)
        if p1.shape != p2.shape:
            raise ValueError("points1 and points2 must have the same shape")
        e = np.ascontiguousarray(E, dtype=np.float64).reshape(9)
        out = np.empty(p1.shape[0], dtype=np.float64)
        _check(self._lib.amc_squared_sampson_error(self._h, p1.ctypes.data_as(C.c_void_p),
                                                   p2.ctypes.data_as(C.c_void_p), p1.shape[0],
                                                   e.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def homography_decomposition(self, H, K1, K2, points1, points2) -> dict:
        """PoseFromHomographyMatrix: dict(R [3,3], t [3], n [3], points3D [m,3])."""
        p1 = np.ascontiguousarray(points1, dtype=np.float64).reshape(-1, 2)
        p2 = np.ascontiguousarray(points2, dtype=np.float64).reshape(-1, 2)
        if p1.shape != p2.shape:
            raise ValueError("points1 and points2 must have the same shape")
        mats = [np.ascontiguousarray(a, dtype=np.float64).reshape(9) for a in (H, K1, K2)]
        R, t, n = np.empty(9), np.empty(3), np.empty(3)
        X = np.empty((max(1, len(p1)), 3))
        m = C.c_uint64(0)
        v = lambda a: a.ctypes.data_as(C.c_void_p)
        _check(self._lib.amc_homography_decomposition(self._h, v(mats[0]), v(mats[1]), v(mats[2]), v(p1), v(p2), len(p1),
                                                      v(R), v(t), v(n), v(X), C.cast(C.byref(m), C.c_void_p)))
        return dict(R=R.reshape(3, 3), t=t, n=n, points3D=X[:m.value].copy())

    def cam_from_img(self, model: str | int, params, points) -> np.ndarray:
        """Camera::CamFromImg of an N x 2 array of image points."""
        p = np.ascontiguousarray(params, dtype=np.float64)
        xy = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
        mid = CAMERA_MODELS[model] if isinstance(model, str) else int(model)
        out = np.empty_like(xy)
        _check(self._lib.amc_cam_from_img(self._h, mid, p.ctypes.data_as(C.c_void_p), p.size,
                                          xy.ctypes.data_as(C.c_void_p), xy.shape[0], out.ctypes.data_as(C.c_void_p)))
        return out

    def img_from_cam(self, model: str | int, params, points) -> np.ndarray:
        """Camera::ImgFromCam of an N x 2 array of normalised image-plane points."""
        p = np.ascontiguousarray(params, dtype=np.float64)
        uv = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
        mid = CAMERA_MODELS[model] if isinstance(model, str) else int(model)
        out = np.empty_like(uv)
        _check(self._lib.amc_img_from_cam(self._h, mid, p.ctypes.data_as(C.c_void_p), p.size, uv.ctypes.data_as(C.c_void_p),
                                          uv.shape[0], out.ctypes.data_as(C.c_void_p)))
        return out

    def upload_camera(self, slot: int, model: str | int, width: int, height: int, params,
                      has_prior_focal_length: bool = False) -> None:
        p = np.ascontiguousarray(params, dtype=np.float64)
        mid = CAMERA_MODELS[model] if isinstance(model, str) else int(model)
        _check(self._lib.amc_upload_camera(self._h, slot, mid, width, height,
                                           p.ctypes.data_as(C.c_void_p), p.size,
                                           int(has_prior_focal_length)))

    def verify_pairs(self, slot1, slot2, match_offsets, matches, opts: TvgOpts | None = None, seed: int = 0,
                     copy: bool = True):
        """EstimateTwoViewGeometry per pair. Returns (tvg structured array [npairs], inlier_mask
        bool [total matches], stats).  copy=False: the arrays are views of the library's result buffers (as a C++
        caller reads them), released when the last of them is garbage collected.  matches=None: the rows are read from
        the resident match table (upload_matches, or the last match call's) - match_offsets[-1] must be its row count."""
        s1 = np.ascontiguousarray(slot1, dtype=np.uint32)
        s2 = np.ascontiguousarray(slot2, dtype=np.uint32)
        off = np.ascontiguousarray(match_offsets, dtype=np.uint64)
        if off.shape != (s1.size + 1,) or s1.shape != s2.shape:
            raise ValueError("match_offsets must have npairs + 1 entries")
        if matches is None:
            m, nrows = None, int(off[-1]) if off.size else 0
        else:
            m = np.ascontiguousarray(matches, dtype=np.uint32).reshape(-1, 2)
            nrows = m.shape[0]
            if int(off[-1]) != nrows:
                raise ValueError("match_offsets[-1] must equal the number of matches")
        o = opts if opts is not None else tvg_options()
        res = VerifyResult()
        _check(self._lib.amc_verify_pairs(self._h, s1.ctypes.data_as(C.c_void_p), s2.ctypes.data_as(C.c_void_p),
                                          s1.size, off.ctypes.data_as(C.c_void_p),
                                          m.ctypes.data_as(C.c_void_p) if m is not None else None,
                                          C.byref(o), seed, C.byref(res)))
        if not copy:
            return self._unpack_verify(res, nrows, bool(o.multiple_models), _VerifyLease(self._lib, res))
        try:
            tvg, mask, stats = self._unpack_verify(res, nrows, bool(o.multiple_models))
        finally:
            self._lib.amc_verify_result_free(C.byref(res))
        return tvg, mask, stats

    def pose_pairs(self, slot1, slot2, match_offsets, inlier_matches, config, E=None, H=None) -> np.ndarray:
        """EstimateTwoViewGeometryPose for given geometries: config [npairs], E / H [npairs, 3, 3].
        Returns a POSE_DTYPE array [npairs]."""
        s1 = np.ascontiguousarray(slot1, dtype=np.uint32)
        s2 = np.ascontiguousarray(slot2, dtype=np.uint32)
        off = np.ascontiguousarray(match_offsets, dtype=np.uint64)
        m = np.ascontiguousarray(inlier_matches, dtype=np.uint32).reshape(-1, 2)
        if off.shape != (s1.size + 1,) or s1.shape != s2.shape:
            raise ValueError("match_offsets must have npairs + 1 entries")
        if int(off[-1]) != m.shape[0]:
            raise ValueError("match_offsets[-1] must equal the number of matches")
        n = s1.size
        geoms = np.zeros(n, dtype=TVG_DTYPE)
        geoms["config"] = np.asarray(config, dtype=np.int32).reshape(n)
        if E is not None:
            geoms["E"] = np.asarray(E, dtype=np.float64).reshape(n, 3, 3)
        if H is not None:
            geoms["H"] = np.asarray(H, dtype=np.float64).reshape(n, 3, 3)
        out = np.zeros(n, dtype=POSE_DTYPE)
        assert C.sizeof(Pose) == POSE_DTYPE.itemsize and C.sizeof(Tvg) == TVG_DTYPE.itemsize
        _check(self._lib.amc_pose_pairs(self._h, s1.ctypes.data_as(C.c_void_p), s2.ctypes.data_as(C.c_void_p),
                                        C.c_size_t(n), off.ctypes.data_as(C.c_void_p),
                                        m.ctypes.data_as(C.c_void_p), geoms.ctypes.data_as(C.c_void_p),
                                        out.ctypes.data_as(C.c_void_p)))
        return out

    def acos_lut(self) -> np.ndarray:
        out = np.empty(262145, dtype=np.float32)
        _check(self._lib.amc_get_acos_lut(self._h, out.ctypes.data_as(C.c_void_p)))
        return out
