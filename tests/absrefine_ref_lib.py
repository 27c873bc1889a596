"""ctypes wrapper of the joint pose and camera refinement's CPU reference (tests/absrefine_ref/absrefine_ref.cc, written
from DESIGN.md section 25 on top of the section-12 reference, without any product header), built on first use into
tests/absrefine_ref/_build/ with the flags of tests/abspose_ref_lib.py."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import abspose_ref_lib
from abspose_ref_lib import EXITS, TRACE_FIELDS  # noqa: F401  (the trace has the section-12 reference's form)
from pycolmap_amd._capi import abspose_inputs, abspose_options

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "absrefine_ref" / "absrefine_ref.cc"
DEP = ROOT / "tests" / "abspose_ref" / "abspose_ref.cc"
LIB = ROOT / "tests" / "absrefine_ref" / "_build" / "libabsrefineref.so"
_lib = None
_p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

NUM_FOCAL = {0: 1, 1: 2, 2: 1, 3: 1, 4: 2, 5: 2, 6: 2, 7: 2, 8: 1, 9: 1, 10: 2}
NUM_PARAMS = {0: 3, 1: 4, 2: 4, 3: 5, 4: 8, 5: 8, 6: 12, 7: 5, 8: 4, 9: 5, 10: 12}


def variable_params(model, refine_focal_length, refine_extra_params):
    """25.1: the camera's variable parameter indices, ascending."""
    nf, n = NUM_FOCAL[int(model)], NUM_PARAMS[int(model)]
    return ([*range(nf)] if refine_focal_length else []) + ([*range(nf + 2, n)] if refine_extra_params else [])


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
    lib.absrefine_ref_project.restype = C.c_int
    lib.absrefine_ref_project.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
    lib.absrefine_ref_project_points.restype = None
    lib.absrefine_ref_project_points.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]
    lib.absrefine_ref_refine.restype = C.c_int
    lib.absrefine_ref_refine.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 8 + [C.c_int] + [C.c_void_p] * 6
    _lib = lib
    return lib


def project(model, params, q, t, X, refine_focal_length=False, refine_extra_params=False):
    """One correspondence as the joint refinement evaluates it: the pixel (2,), its derivatives (2, 7 + nv) by
    (qx, qy, qz, qw, tx, ty, tz, variable camera parameters) and the variable parameter indices."""
    prm = np.zeros(12)
    prm[:len(params)] = params
    f = lambda a, n: np.ascontiguousarray(a, dtype=np.float64).reshape(n)  # noqa: E731
    xy, J, idx = np.zeros(2), np.zeros((2, 17)), np.zeros(10, np.int32)
    nv = load().absrefine_ref_project(int(model), _p(prm), int(bool(refine_focal_length)), int(bool(refine_extra_params)),
                                      _p(f(q, 4)), _p(f(t, 3)), _p(f(X, 3)), _p(xy), _p(J), _p(idx))
    return xy, J[:, :7 + nv].copy(), idx[:nv].tolist()


def project_points(model, params, q, t, X):
    """The pixels (N, 2) of the world points X (N, 3) as the refinement evaluates them."""
    prm = np.zeros(12)
    prm[:len(params)] = params
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
    xy = np.zeros((X.shape[0], 2))
    load().absrefine_ref_project_points(int(model), _p(prm), _p(np.ascontiguousarray(q, dtype=np.float64).reshape(4)),
                                        _p(np.ascontiguousarray(t, dtype=np.float64).reshape(3)), _p(X), X.shape[0], _p(xy))
    return xy


def _ref_vec(ro):
    return np.array([ro.gradient_tolerance, ro.max_num_iterations, ro.loss_function_scale,
                     1.0 if ro.refine_focal_length else 0.0, 1.0 if ro.refine_extra_params else 0.0], np.float64)


def _check_opts(ro):
    if not (ro.gradient_tolerance >= 0 and ro.max_num_iterations >= 0 and ro.loss_function_scale >= 0):
        raise ValueError("absrefine reference: invalid options")


def refine(offsets, camera_models, camera_params, points2D, points3D, qvec, tvec, inlier_mask, refinement=None,
           return_covariance=False, trace=False):
    """The reference's joint refinement, in Context.refine_poses_and_cameras' result form (without the timings).  With
    trace, (result, trace) as abspose_ref_lib.refine."""
    off, models, prm, p2, p3 = abspose_inputs(offsets, camera_models, camera_params, points2D, points3D)
    _, ro = abspose_options(None, refinement)
    _check_opts(ro)
    nq, n = off.size - 1, int(off[-1])
    q = np.ascontiguousarray(qvec, dtype=np.float64).reshape(-1, 4)
    t = np.ascontiguousarray(tvec, dtype=np.float64).reshape(-1, 3)
    m = np.ascontiguousarray(inlier_mask, dtype=bool).reshape(-1).astype(np.uint8)
    assert q.shape[0] == nq and t.shape[0] == nq and m.size == n
    r = dict(success=np.zeros(nq, np.uint8), qvec=np.zeros((nq, 4)), tvec=np.zeros((nq, 3)),
             camera_params=np.zeros((max(nq, 1), 12)), covariance=np.zeros((max(nq, 1), 36)))
    rows = np.zeros((max(nq, 1), len(TRACE_FIELDS)), np.int32)
    rc = load().absrefine_ref_refine(_p(off), nq, _p(models), _p(prm), _p(p2), _p(p3), _p(q), _p(t), _p(m),
                                     _p(_ref_vec(ro)), int(bool(return_covariance)), _p(r["success"]), _p(r["qvec"]),
                                     _p(r["tvec"]), _p(r["camera_params"]),
                                     _p(r["covariance"]) if return_covariance else None, _p(rows) if trace else None)
    if rc != 0:
        raise ValueError("absrefine_ref_refine: invalid input")
    r["success"] = r["success"].astype(bool)
    r["camera_params"] = r["camera_params"][:nq]
    r["num_inliers"] = np.array([int(m[int(off[i]):int(off[i + 1])].sum()) for i in range(nq)], np.uint32)
    r["num_trials"] = np.zeros(nq, np.uint64)
    r["focal_factor"] = np.ones(nq)
    r["inlier_mask"] = m.astype(bool)
    if return_covariance:
        r["covariance"] = r["covariance"][:nq].reshape(nq, 6, 6)
    else:
        del r["covariance"]
    return (r, {k: rows[:nq, i].copy() for i, k in enumerate(TRACE_FIELDS)}) if trace else r


def estimate(offsets, camera_models, camera_params, points2D, points3D, estimation=None, refinement=None,
             return_covariance=False):
    """25.3: the section-12 reference's RANSAC per focal factor (its refinement without iterations returns the
    RANSAC's pose), then the joint refinement over the RANSAC's inliers with the camera scaled by the chosen factor."""
    off, models, prm, p2, p3 = abspose_inputs(offsets, camera_models, camera_params, points2D, points3D)
    _, ro = abspose_options(None, refinement)
    _check_opts(ro)
    r0 = dict(gradient_tolerance=ro.gradient_tolerance, max_num_iterations=0, loss_function_scale=ro.loss_function_scale)
    est = abspose_ref_lib.estimate(off, models, prm, p2, p3, estimation, r0)
    nq = off.size - 1
    scaled = prm.copy()
    for i in range(nq):
        scaled[i, NUM_PARAMS[int(models[i])]:] = 0.0
        f = est["focal_factor"][i]
        scaled[i, :NUM_FOCAL[int(models[i])]] *= f if f != 0.0 else 1.0
    mask = est["inlier_mask"].copy()
    for i in range(nq):
        if not est["success"][i]:
            mask[int(off[i]):int(off[i + 1])] = False
    r = refine(off, models, scaled, p2, p3, est["qvec"], est["tvec"], mask, refinement, return_covariance)
    r["success"] = r["success"] & est["success"]
    if return_covariance:
        r["covariance"][~est["success"]] = 0.0
    for k in ("num_inliers", "num_trials", "focal_factor", "inlier_mask"):
        r[k] = est[k]
    return r
