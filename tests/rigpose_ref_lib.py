"""ctypes wrapper of the rig absolute pose CPU reference (tests/rigpose_ref/rigpose_ref.cc, written from DESIGN.md
section 13 without any product header; it includes tests/abspose_ref/abspose_ref.cc for the pieces section 13 shares with
section 12), built on first use into tests/rigpose_ref/_build/ with the flags of tests/abspose_ref_lib.py."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from pycolmap_amd._capi import rigpose_inputs, rigpose_options

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "rigpose_ref" / "rigpose_ref.cc"
DEP = ROOT / "tests" / "abspose_ref" / "abspose_ref.cc"
LIB = ROOT / "tests" / "rigpose_ref" / "_build" / "librigposeref.so"
_lib = None
_p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    LIB.parent.mkdir(parents=True, exist_ok=True)
    if not LIB.exists() or LIB.stat().st_mtime < max(SRC.stat().st_mtime, DEP.stat().st_mtime):
        tmp = LIB.with_name(LIB.name + ".tmp")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-Wall", "-Wno-unknown-pragmas",
                        "-Wno-unused-function", "-shared", "-fPIC", str(SRC), "-o", str(tmp)], check=True)
        tmp.replace(LIB)
    lib = C.CDLL(str(LIB))
    lib.rigpose_ref_gp3p.restype = C.c_int
    lib.rigpose_ref_gp3p.argtypes = [C.c_void_p] * 5
    lib.rigpose_ref_support.restype = None
    lib.rigpose_ref_support.argtypes = [C.c_size_t, C.c_size_t] + [C.c_void_p] * 7 + [C.c_double] + [C.c_void_p] * 2
    lib.rigpose_ref_better.restype = C.c_int
    lib.rigpose_ref_better.argtypes = [C.c_void_p] * 2
    lib.rigpose_ref_residual.restype = None
    lib.rigpose_ref_residual.argtypes = [C.c_int] + [C.c_void_p] * 8
    lib.rigpose_ref_estimate.restype = C.c_int
    lib.rigpose_ref_estimate.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 9 + [C.c_int] + [C.c_void_p] * 8
    lib.rigpose_ref_estimate_trace.restype = C.c_int
    lib.rigpose_ref_estimate_trace.argtypes = lib.rigpose_ref_estimate.argtypes + [C.c_void_p]
    lib.rigpose_ref_point_ids.restype = None
    lib.rigpose_ref_point_ids.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p]
    _lib = lib
    return lib


def _f(a, shape):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(shape)


def gp3p(origins, directions, X):
    """GP3P on three rays (origins (3, 3), unit directions (3, 3), rig frame) and world points (3, 3): the
    rig_from_world models (k, 3, 4) and their depths (k, 3), in root order."""
    c, d, X = _f(origins, (3, 3)), _f(directions, (3, 3)), _f(X, (3, 3))
    models, depths = np.zeros((8, 3, 4)), np.zeros((8, 3))
    n = load().rigpose_ref_gp3p(_p(c), _p(d), _p(X), _p(models), _p(depths))
    return models[:n].copy(), depths[:n].copy()


def _cams(camera_models, camera_params, cams_from_rig):
    models = np.ascontiguousarray(camera_models, dtype=np.int32).reshape(-1)
    prm = np.zeros((models.size, 12))
    for i, p in enumerate(camera_params):
        prm[i, :len(p)] = p
    return models, prm, _f(cams_from_rig, (-1, 7))


def support(camera_models, camera_params, cams_from_rig, camera_idxs, uv, X, model, max_residual):
    """The support of rig_from_world `model` (3, 4) over normalized points uv: (num_inliers, num_unique_inliers,
    residual_sum, mask)."""
    models, prm, rigs = _cams(camera_models, camera_params, cams_from_rig)
    idx = np.ascontiguousarray(camera_idxs, dtype=np.int32).reshape(-1)
    uv, X, P = _f(uv, (-1, 2)), _f(X, (-1, 3)), _f(model, (12,))
    out, mask = np.zeros(3), np.zeros(max(idx.size, 1), np.uint8)
    load().rigpose_ref_support(idx.size, models.size, _p(models), _p(prm), _p(rigs), _p(idx), _p(uv), _p(X), _p(P),
                               float(max_residual), _p(out), _p(mask))
    return int(out[0]), int(out[1]), float(out[2]), mask[:idx.size].astype(bool)


def point_ids(X):
    """The point ids (13.2) of world points X (N, 3): for each the index of the first point equal to it."""
    X = _f(X, (-1, 3))
    ids = np.zeros(max(len(X), 1), np.uint32)
    load().rigpose_ref_point_ids(len(X), _p(X), _p(ids))
    return ids[:len(X)]


def better(a, b) -> bool:
    """Is the support a = (num_inliers, num_unique_inliers, residual_sum) better than b (13.5)."""
    return bool(load().rigpose_ref_better(_p(_f(a, (3,))), _p(_f(b, (3,)))))


def residual(model, params, cam_from_rig, q, t, X, xy):
    """The pixel residual (2,) of one correspondence and its Jacobian (2, 7) by qx qy qz qw tx ty tz (13.7)."""
    prm = np.zeros(12)
    prm[:len(params)] = params
    res, jac = np.zeros(2), np.zeros((2, 7))
    load().rigpose_ref_residual(int(model), _p(prm), _p(_f(cam_from_rig, (7,))), _p(_f(q, (4,))), _p(_f(t, (3,))),
                                _p(_f(X, (3,))), _p(_f(xy, (2,))), _p(res), _p(jac))
    return res, jac


# the exit codes of rigpose_ref_estimate_trace, in the order of abspose_ref.cc's enum Exit; -1 (EXITS[-1]): no refinement
# ran, the RANSAC having failed
EXITS = ("GRADIENT_AT_START", "GRADIENT_AFTER_STEP", "MAX_ITERATIONS", "PARAMETER_TOLERANCE", "FUNCTION_TOLERANCE",
         "INVALID_STEPS", "MIN_RADIUS", "NOT_FINITE_START", "NOTHING_TO_REFINE", "NOT_REFINED")
TRACE_FIELDS = ("iterations", "accepted", "rejected", "invalid", "exit", "rank_failed")


def estimate(offsets, camera_offsets, camera_models, camera_params, cams_from_rig, camera_idxs, points2D, points3D,
             estimation=None, refinement=None, return_covariance=False, trace=False):
    """The reference on a batch, in Context.estimate_rig_absolute_poses' result form (without the timings).  With trace,
    (result, trace): per query what the refinement did, (Q,) int32 arrays by TRACE_FIELDS, `exit` an index into EXITS.
    The product has no such output."""
    off, coff, models, prm, rigs, idx, p2, p3 = rigpose_inputs(offsets, camera_offsets, camera_models, camera_params,
                                                               cams_from_rig, camera_idxs, points2D, points3D)
    eo, ro = rigpose_options(estimation, refinement)
    ok = eo.max_error > 0 and 0 <= eo.min_inlier_ratio <= 1 and 0 <= eo.confidence <= 1 and \
        0 <= eo.min_num_trials <= eo.max_num_trials and ro.gradient_tolerance >= 0 and ro.max_num_iterations >= 0 and \
        ro.loss_function_scale >= 0 and not ro.refine_focal_length and not ro.refine_extra_params
    if not ok:
        raise ValueError("rig pose reference: invalid options")
    for i in range(off.size - 1):
        c = idx[int(off[i]):int(off[i + 1])]
        if c.size and (c.min() < 0 or c.max() >= int(coff[i + 1] - coff[i])):
            raise ValueError("rig pose reference: camera index out of range")
    nq, n = off.size - 1, int(off[-1])
    r = dict(success=np.zeros(nq, np.uint8), qvec=np.zeros((nq, 4)), tvec=np.zeros((nq, 3)),
             num_inliers=np.zeros(nq, np.uint32), num_all_inliers=np.zeros(nq, np.uint32),
             num_trials=np.zeros(nq, np.uint64), covariance=np.zeros((max(nq, 1), 36)),
             inlier_mask=np.zeros(max(n, 1), np.uint8))
    est = np.array([eo.max_error, eo.min_inlier_ratio, eo.confidence, eo.dyn_num_trials_multiplier, eo.min_num_trials,
                    eo.max_num_trials], np.float64)
    ref = np.array([ro.gradient_tolerance, ro.max_num_iterations, ro.loss_function_scale], np.float64)
    rows = np.zeros((max(nq, 1), len(TRACE_FIELDS)), np.int32)
    fn = load().rigpose_ref_estimate_trace if trace else load().rigpose_ref_estimate
    fn(_p(off), nq, _p(coff), _p(models), _p(prm), _p(rigs), _p(idx), _p(p2), _p(p3), _p(est),
       _p(ref), int(bool(return_covariance)), _p(r["success"]), _p(r["qvec"]), _p(r["tvec"]),
       _p(r["num_inliers"]), _p(r["num_all_inliers"]), _p(r["num_trials"]),
       _p(r["covariance"]) if return_covariance else None, _p(r["inlier_mask"]), *([_p(rows)] if trace else []))
    r["success"] = r["success"].astype(bool)
    r["inlier_mask"] = r["inlier_mask"][:n].astype(bool)
    if return_covariance:
        r["covariance"] = r["covariance"][:nq].reshape(nq, 6, 6)
    else:
        del r["covariance"]
    return (r, {k: rows[:nq, i].copy() for i, k in enumerate(TRACE_FIELDS)}) if trace else r
