"""ctypes wrapper of the absolute pose CPU reference (tests/abspose_ref/abspose_ref.cc, written from DESIGN.md section 12
without any product header), built on first use into tests/abspose_ref/_build/ with g++ -O2 -ffp-contract=off
-fno-fast-math (the flags of tests/tri_ref_lib.py)."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from pycolmap_amd._capi import abspose_inputs, abspose_options

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "abspose_ref" / "abspose_ref.cc"
LIB = ROOT / "tests" / "abspose_ref" / "_build" / "libabsposeref.so"
_lib = None
_p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    LIB.parent.mkdir(parents=True, exist_ok=True)
    if not LIB.exists() or LIB.stat().st_mtime < SRC.stat().st_mtime:
        tmp = LIB.with_name(LIB.name + ".tmp")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-Wall", "-Wno-unknown-pragmas",
                        "-shared", "-fPIC", str(SRC), "-o", str(tmp)], check=True)
        tmp.replace(LIB)
    lib = C.CDLL(str(LIB))
    for fn in ("atan", "sin", "cos", "log"):
        f = getattr(lib, f"abspose_ref_{fn}")
        f.restype = C.c_double
        f.argtypes = [C.c_double]
    lib.abspose_ref_project.restype = None
    lib.abspose_ref_project.argtypes = [C.c_int] + [C.c_void_p] * 6
    lib.abspose_ref_p3p.restype = C.c_int
    lib.abspose_ref_p3p.argtypes = [C.c_void_p] * 3
    lib.abspose_ref_epnp.restype = C.c_int
    lib.abspose_ref_epnp.argtypes = [C.c_uint32] + [C.c_void_p] * 3
    lib.abspose_ref_focal_factors.restype = C.c_size_t
    lib.abspose_ref_focal_factors.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_size_t]
    lib.abspose_ref_estimate.restype = C.c_int
    lib.abspose_ref_estimate.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 8
    lib.abspose_ref_refine.restype = C.c_int
    lib.abspose_ref_refine.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 8 + [C.c_int] + [C.c_void_p] * 4
    lib.abspose_ref_refine_trace.restype = C.c_int
    lib.abspose_ref_refine_trace.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 8 + [C.c_int] + [C.c_void_p] * 5
    _lib = lib
    return lib


def scalar(fn: str, x: float) -> float:
    return getattr(load(), f"abspose_ref_{fn}")(float(x))


def project(model, params, q, t, X):
    """One correspondence as the refinement evaluates it (12.7): the pixel (2,) and its derivatives (2, 7) by
    (qx, qy, qz, qw, tx, ty, tz)."""
    prm = np.zeros(12)
    prm[:len(params)] = params
    f = lambda a, n: np.ascontiguousarray(a, dtype=np.float64).reshape(n)  # noqa: E731
    xy, J = np.zeros(2), np.zeros((2, 7))
    load().abspose_ref_project(int(model), _p(prm), _p(f(q, 4)), _p(f(t, 3)), _p(f(X, 3)), _p(xy), _p(J))
    return xy, J


def p3p(uv, X):
    """P3P on three normalized points (3, 2) and world points (3, 3): list of (3, 4) models."""
    uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(3, 2)
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(3, 3)
    out = np.zeros((4, 3, 4))
    n = load().abspose_ref_p3p(_p(uv), _p(X), _p(out))
    return [out[i] for i in range(n)]


def epnp(uv, X):
    uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((3, 4))
    ok = load().abspose_ref_epnp(uv.shape[0], _p(uv), _p(X), _p(out))
    return out if ok else None


def focal_factors(**estimation):
    eo, _ = abspose_options(estimation, None)
    buf = np.zeros(4096)
    n = load().abspose_ref_focal_factors(eo.estimate_focal_length, eo.num_focal_length_samples,
                                         eo.min_focal_length_ratio, eo.max_focal_length_ratio, _p(buf), buf.size)
    return buf[:n].copy()


def estimate(offsets, camera_models, camera_params, points2D, points3D, estimation=None, refinement=None,
             return_covariance=False):
    """The reference on a batch, in Context.estimate_absolute_poses' result form (without the timings)."""
    off, models, prm, p2, p3 = abspose_inputs(offsets, camera_models, camera_params, points2D, points3D)
    eo, ro = abspose_options(estimation, refinement)
    nq, n = off.size - 1, int(off[-1])
    r = dict(success=np.zeros(nq, np.uint8), qvec=np.zeros((nq, 4)), tvec=np.zeros((nq, 3)),
             num_inliers=np.zeros(nq, np.uint32), num_trials=np.zeros(nq, np.uint64), focal_factor=np.zeros(nq),
             covariance=np.zeros((max(nq, 1), 36)), inlier_mask=np.zeros(max(n, 1), np.uint8))
    _check_opts(eo, ro)
    rc = load().abspose_ref_estimate(_p(off), nq, _p(models), _p(prm), _p(p2), _p(p3), _p(_est_vec(eo)),
                                     _p(_ref_vec(ro)), int(bool(return_covariance)), _p(r["success"]), _p(r["qvec"]), _p(r["tvec"]),
                                     _p(r["num_inliers"]), _p(r["num_trials"]), _p(r["focal_factor"]),
                                     _p(r["covariance"]) if return_covariance else None, _p(r["inlier_mask"]))
    if rc != 0:
        raise ValueError("abspose_ref_estimate: invalid options")
    return _finish(r, nq, n, return_covariance)


# the exit codes of abspose_ref_refine_trace, in the order of abspose_ref.cc's enum Exit
EXITS = ("GRADIENT_AT_START", "GRADIENT_AFTER_STEP", "MAX_ITERATIONS", "PARAMETER_TOLERANCE", "FUNCTION_TOLERANCE",
         "INVALID_STEPS", "MIN_RADIUS", "NOT_FINITE_START", "NOTHING_TO_REFINE")
TRACE_FIELDS = ("iterations", "accepted", "rejected", "invalid", "exit", "rank_failed")


def refine(offsets, camera_models, camera_params, points2D, points3D, qvec, tvec, inlier_mask, refinement=None,
           return_covariance=False, trace=False):
    """The reference's refinement alone.  With trace, (result, trace): per query what the solver did, (Q,) int32 arrays
    by TRACE_FIELDS, `exit` an index into EXITS.  The product has no such output."""
    off, models, prm, p2, p3 = abspose_inputs(offsets, camera_models, camera_params, points2D, points3D)
    _, ro = abspose_options(None, refinement)
    nq, n = off.size - 1, int(off[-1])
    q = np.ascontiguousarray(qvec, dtype=np.float64).reshape(-1, 4)
    t = np.ascontiguousarray(tvec, dtype=np.float64).reshape(-1, 3)
    m = np.ascontiguousarray(inlier_mask, dtype=bool).reshape(-1).astype(np.uint8)
    r = dict(success=np.zeros(nq, np.uint8), qvec=np.zeros((nq, 4)), tvec=np.zeros((nq, 3)),
             covariance=np.zeros((max(nq, 1), 36)))
    _check_opts(None, ro)
    args = (_p(off), nq, _p(models), _p(prm), _p(p2), _p(p3), _p(q), _p(t), _p(m), _p(_ref_vec(ro)),
            int(bool(return_covariance)), _p(r["success"]), _p(r["qvec"]), _p(r["tvec"]),
            _p(r["covariance"]) if return_covariance else None)
    rows = np.zeros((max(nq, 1), len(TRACE_FIELDS)), np.int32)
    rc = load().abspose_ref_refine_trace(*args, _p(rows)) if trace else load().abspose_ref_refine(*args)
    if rc != 0:
        raise ValueError("abspose_ref_refine: invalid options")
    r["num_inliers"] = np.array([int(m[int(off[i]):int(off[i + 1])].sum()) for i in range(nq)], np.uint32)
    r["num_trials"] = np.zeros(nq, np.uint64)
    r["focal_factor"] = np.ones(nq)
    r["inlier_mask"] = m
    r = _finish(r, nq, n, return_covariance)
    return (r, {k: rows[:nq, i].copy() for i, k in enumerate(TRACE_FIELDS)}) if trace else r


def _est_vec(eo):
    return np.array([eo.estimate_focal_length, eo.num_focal_length_samples, eo.min_focal_length_ratio,
                     eo.max_focal_length_ratio, eo.max_error, eo.min_inlier_ratio, eo.confidence,
                     eo.dyn_num_trials_multiplier, eo.min_num_trials, eo.max_num_trials], np.float64)


def _ref_vec(ro):
    return np.array([ro.gradient_tolerance, ro.max_num_iterations, ro.loss_function_scale], np.float64)


def _check_opts(eo, ro):
    """AbsolutePoseEstimationOptions::Check / AbsolutePoseRefinementOptions::Check and the out-of-scope options"""
    ok = ro.gradient_tolerance >= 0 and ro.max_num_iterations >= 0 and ro.loss_function_scale >= 0 and \
        not ro.refine_focal_length and not ro.refine_extra_params
    if eo is not None:
        ok = ok and eo.num_focal_length_samples > 0 and 0 < eo.min_focal_length_ratio < eo.max_focal_length_ratio \
            and eo.max_error > 0 and 0 <= eo.min_inlier_ratio <= 1 and 0 <= eo.confidence <= 1 \
            and 0 <= eo.min_num_trials <= eo.max_num_trials
    if not ok:
        raise ValueError("absolute pose reference: invalid options")


def _finish(r, nq, n, cov):
    r["success"] = r["success"].astype(bool)
    r["inlier_mask"] = r["inlier_mask"][:n].astype(bool)
    if cov:
        r["covariance"] = r["covariance"][:nq].reshape(nq, 6, 6)
    else:
        del r["covariance"]
    return r
