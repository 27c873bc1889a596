"""ctypes wrapper of the CPU reference of bundle adjustment with constant points (tests/ba_config_ref/ba_config_ref.cc,
written from DESIGN.md 15.12 without any product header; it includes tests/ba_ref/ba_ref.cc for what the addendum leaves
as it is), built on first use into tests/ba_config_ref/_build/ with the flags of tests/ba_ref_lib.py."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import ba_ref_lib
from ba_ref_lib import DEFAULTS, LOSSES, PCG_TOLERANCE, TERMINATIONS, _f, _p

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "ba_config_ref" / "ba_config_ref.cc"
DEPS = [ba_ref_lib.SRC, ba_ref_lib.DEP]
LIB = ROOT / "tests" / "ba_config_ref" / "_build" / "libbaconfigref.so"
_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    LIB.parent.mkdir(parents=True, exist_ok=True)
    if not LIB.exists() or LIB.stat().st_mtime < max(p.stat().st_mtime for p in [SRC] + DEPS):
        tmp = LIB.with_name(LIB.name + ".tmp")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-Wall", "-Wno-unknown-pragmas",
                        "-Wno-unused-function", "-shared", "-fPIC", str(SRC), "-o", str(tmp)], check=True)
        tmp.replace(LIB)
    lib = C.CDLL(str(LIB))
    lib.ba_config_ref_solve.restype = C.c_int
    lib.ba_config_ref_solve.argtypes = ([C.c_size_t] + [C.c_void_p] * 3 + [C.c_size_t] + [C.c_void_p] * 4 +
                                        [C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 5)
    _lib = lib
    return lib


def bundle_adjust(camera_models, camera_params, camera_const, image_cameras, qvec, tvec, pose_const, xyz, obs_image,
                  obs_point, obs_xy, options=None, point_const=None):
    """The reference on a flat problem with a point mask (None = no constant point), in Context.bundle_adjust's result
    form (without the timings)."""
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
    pm = None
    if point_const is not None:
        pm = np.ascontiguousarray(np.asarray(point_const).reshape(-1) != 0, dtype=np.uint8)
        if pm.size != X.shape[0]:
            raise ValueError("bundle adjustment reference: point_const length")
    o = dict(DEFAULTS)
    for k, v in (options or {}).items():
        if k not in o:
            raise ValueError(f"bundle adjustment reference: unknown option {k!r}")
        o[k] = LOSSES[v.upper()] if k == "loss_function_type" and isinstance(v, str) else v
    opts = np.array([o["loss_function_type"], o["loss_function_scale"], o["max_num_iterations"],
                     o["max_linear_solver_iterations"], o["max_num_consecutive_invalid_steps"], o["function_tolerance"],
                     o["gradient_tolerance"], o["parameter_tolerance"], PCG_TOLERANCE], np.float64)
    stats = np.zeros(12)
    rc = load().ba_config_ref_solve(models.size, _p(models), _p(prm), _p(cc), icam.size, _p(icam), _p(q), _p(t), _p(pc),
                                    X.shape[0], _p(X), None if pm is None else _p(pm), oi.size, _p(oi), _p(op), _p(xy),
                                    _p(opts), _p(stats))
    if rc != 0:
        raise ValueError("bundle adjustment reference: invalid input")
    return dict(num_images=icam.size, num_points=X.shape[0], num_observations=oi.size,
                num_variable_parameters=int(stats[0]), initial_cost=float(stats[1]), final_cost=float(stats[2]),
                num_successful_steps=int(stats[3]), num_unsuccessful_steps=int(stats[4]),
                num_pcg_iterations=int(stats[5]), num_pcg_stops_residual=int(stats[6]), num_pcg_stops_cap=int(stats[7]),
                termination=TERMINATIONS[int(stats[8])], camera_params=prm, qvec=q, tvec=t, xyz=X)
