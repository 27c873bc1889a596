"""ctypes wrapper of the bundle adjustment CPU reference (tests/ba_ref/ba_ref.cc, written from DESIGN.md section 15
without any product header; it includes tests/abspose_ref/abspose_ref.cc for the pieces section 15 shares with section
12), built on first use into tests/ba_ref/_build/ with the flags of tests/abspose_ref_lib.py."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

# The reference's own constants and input packing (nothing of the product is imported here): DESIGN.md 15.6's PCG
# bound, 15.5's termination names in the order of the reference's codes, and COLMAP's option defaults.
PCG_TOLERANCE = 1e-8
TERMINATIONS = ("FUNCTION_TOLERANCE", "PARAMETER_TOLERANCE", "GRADIENT_TOLERANCE", "MAX_ITERATIONS", "MIN_RADIUS",
                "INVALID_STEPS", "NOTHING_TO_REFINE")
LOSSES = {"TRIVIAL": 0, "SOFT_L1": 1, "CAUCHY": 2}
DEFAULTS = dict(loss_function_type=0, loss_function_scale=1.0, max_num_iterations=100, max_linear_solver_iterations=200,
                max_num_consecutive_invalid_steps=10, function_tolerance=0.0, gradient_tolerance=0.0,
                parameter_tolerance=0.0)

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "ba_ref" / "ba_ref.cc"
DEP = ROOT / "tests" / "abspose_ref" / "abspose_ref.cc"
LIB = ROOT / "tests" / "ba_ref" / "_build" / "libbaref.so"
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
    lib.ba_ref_observation.restype = C.c_double
    lib.ba_ref_observation.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_double, C.c_int] + [C.c_void_p] * 4
    lib.ba_ref_sum64.restype = C.c_double
    lib.ba_ref_sum64.argtypes = [C.c_size_t, C.c_void_p]
    lib.ba_ref_spd_inverse.restype = None
    lib.ba_ref_spd_inverse.argtypes = [C.c_void_p, C.c_int]
    lib.ba_ref_solve.restype = C.c_int
    lib.ba_ref_solve.argtypes = ([C.c_size_t] + [C.c_void_p] * 3 + [C.c_size_t] + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p,
                                 C.c_size_t] + [C.c_void_p] * 5)
    _lib = lib
    return lib


def _f(a, shape):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(shape)


def observation(model, params, q, t, X, xy, loss=0, loss_scale=1.0, jac=True):
    """One observation (15.3, 15.4): (cost term, corrected residual (2,), J by the pose tangent (2, 6), by the camera's 12
    parameter slots (2, 12), by the point (2, 3))."""
    prm = np.zeros(12)
    prm[:len(params)] = params
    r, Jp, Jc, Jx = np.zeros(2), np.zeros((2, 6)), np.zeros((2, 12)), np.zeros((2, 3))
    cost = load().ba_ref_observation(int(model), _p(prm), _p(_f(q, (4,))), _p(_f(t, (3,))), _p(_f(X, (3,))),
                                     _p(_f(xy, (2,))), int(loss), float(loss_scale), int(bool(jac)), _p(r), _p(Jp),
                                     _p(Jc), _p(Jx))
    return cost, r, Jp, Jc, Jx


def sum64(values) -> float:
    """The 15.7 order on a vector: lane l adds entries l, l + 64, ... from 0.0; xor butterfly 32 .. 1."""
    v = _f(values, (-1,))
    return float(load().ba_ref_sum64(v.size, _p(v)))


def spd_inverse(A):
    A = _f(A, (-1,)).copy()
    n = int(round(np.sqrt(A.size)))
    load().ba_ref_spd_inverse(_p(A), n)
    return A.reshape(n, n)


def bundle_adjust(camera_models, camera_params, camera_const, image_cameras, qvec, tvec, pose_const, xyz, obs_image,
                  obs_point, obs_xy, options=None):
    """The reference on a flat problem, in Context.bundle_adjust's result form (without the timings)."""
    models = np.array(camera_models, dtype=np.int32).reshape(-1)
    prm = np.zeros((models.size, 12))
    cc = np.ones((models.size, 12), np.uint8)
    for c in range(models.size):
        p = np.asarray(camera_params[c], np.float64).reshape(-1)
        prm[c, :p.size] = p
        mask = np.asarray(camera_const[c]).reshape(-1)[:12]
        cc[c, :mask.size] = mask != 0
    icam = np.array(image_cameras, dtype=np.uint32).reshape(-1)
    q, t = _f(qvec, (-1, 4)).copy(), _f(tvec, (-1, 3)).copy()
    pc = np.ascontiguousarray(np.asarray(pose_const).reshape(-1, 6) != 0, dtype=np.uint8)
    X = _f(xyz, (-1, 3)).copy()
    oi = np.array(obs_image, dtype=np.uint32).reshape(-1)
    op = np.array(obs_point, dtype=np.uint32).reshape(-1)
    xy = _f(obs_xy, (-1, 2))
    if not (q.shape[0] == t.shape[0] == pc.shape[0] == icam.size and oi.size == op.size == xy.shape[0]):
        raise ValueError("bundle adjustment reference: array lengths disagree")
    o = dict(DEFAULTS)
    for k, v in (options or {}).items():
        if k not in o:
            raise ValueError(f"bundle adjustment reference: unknown option {k!r}")
        o[k] = LOSSES[v.upper()] if k == "loss_function_type" and isinstance(v, str) else v
    ok = 0 <= o["loss_function_type"] <= 2 and o["loss_function_scale"] > 0 and o["max_num_iterations"] >= 0 and \
        o["max_linear_solver_iterations"] >= 1 and o["max_num_consecutive_invalid_steps"] >= 1 and \
        o["function_tolerance"] >= 0 and o["gradient_tolerance"] >= 0 and o["parameter_tolerance"] >= 0
    if not ok:
        raise ValueError("bundle adjustment reference: invalid options")
    opts = np.array([o["loss_function_type"], o["loss_function_scale"], o["max_num_iterations"],
                     o["max_linear_solver_iterations"], o["max_num_consecutive_invalid_steps"], o["function_tolerance"],
                     o["gradient_tolerance"], o["parameter_tolerance"], PCG_TOLERANCE], np.float64)
    stats = np.zeros(12)
    rc = load().ba_ref_solve(models.size, _p(models), _p(prm), _p(cc), icam.size, _p(icam), _p(q), _p(t), _p(pc),
                             X.shape[0], _p(X), oi.size, _p(oi), _p(op), _p(xy), _p(opts), _p(stats))
    if rc != 0:
        raise ValueError("bundle adjustment reference: invalid input")
    return dict(num_images=icam.size, num_points=X.shape[0], num_observations=oi.size,
                num_variable_parameters=int(stats[0]), initial_cost=float(stats[1]), final_cost=float(stats[2]),
                num_successful_steps=int(stats[3]), num_unsuccessful_steps=int(stats[4]),
                num_pcg_iterations=int(stats[5]), num_pcg_stops_residual=int(stats[6]), num_pcg_stops_cap=int(stats[7]),
                termination=TERMINATIONS[int(stats[8])], camera_params=prm, qvec=q, tvec=t, xyz=X)
