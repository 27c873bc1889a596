"""ctypes wrapper of the bundle-adjustment covariance CPU reference (tests/bacov_ref/bacov_ref.cc, written from DESIGN.md
section 24 without any product header; it includes tests/ba_ref/ba_ref.cc for the pieces section 24 takes from section
15), built on first use into tests/bacov_ref/_build/ with the flags of tests/ba_ref_lib.py."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

# the reference's own constants (nothing of the product is imported here)
LOSSES = {"TRIVIAL": 0, "SOFT_L1": 1, "CAUCHY": 2}
DEFAULTS = dict(loss_function_type=0, loss_function_scale=1.0, damping=1e-8)
MAX_COLUMNS = 8192

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "bacov_ref" / "bacov_ref.cc"
DEPS = [ROOT / "tests" / "ba_ref" / "ba_ref.cc", ROOT / "tests" / "abspose_ref" / "abspose_ref.cc"]
LIB = ROOT / "tests" / "bacov_ref" / "_build" / "libbacovref.so"
_lib = None
_p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    LIB.parent.mkdir(parents=True, exist_ok=True)
    if not LIB.exists() or LIB.stat().st_mtime < max(f.stat().st_mtime for f in [SRC] + DEPS):
        tmp = LIB.with_name(LIB.name + ".tmp")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-Wall", "-Wno-unknown-pragmas",
                        "-Wno-unused-function", "-shared", "-fPIC", str(SRC), "-o", str(tmp)], check=True)
        tmp.replace(LIB)
    lib = C.CDLL(str(LIB))
    lib.bacov_ref_num_columns.restype = C.c_long
    lib.bacov_ref_num_columns.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.bacov_ref_run.restype = C.c_int
    lib.bacov_ref_run.argtypes = ([C.c_size_t] + [C.c_void_p] * 3 + [C.c_size_t] + [C.c_void_p] * 4 + [C.c_size_t] +
                                  [C.c_void_p] * 2 + [C.c_size_t] + [C.c_void_p] * 10)
    _lib = lib
    return lib


def _f(a, shape):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(shape)


def ba_covariance(camera_models, camera_params, camera_const, image_cameras, qvec, tvec, pose_const, xyz, obs_image,
                  obs_point, obs_xy, options=None, point_const=None):
    """The reference on a flat problem, in Context.ba_covariance's result form (without the timings and the want_*
    switches: matrix and point blocks are always there on success)."""
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
    pm = None if point_const is None else np.ascontiguousarray(np.asarray(point_const).reshape(-1) != 0, dtype=np.uint8)
    if not (q.shape[0] == t.shape[0] == pc.shape[0] == icam.size and oi.size == op.size == xy.shape[0]) or \
            (pm is not None and pm.size != X.shape[0]):
        raise ValueError("covariance reference: array lengths disagree")
    o = dict(DEFAULTS)
    for k, v in (options or {}).items():
        if k in ("want_points", "want_matrix"):
            continue
        if k not in o:
            raise ValueError(f"covariance reference: unknown option {k!r}")
        o[k] = LOSSES[v.upper()] if k == "loss_function_type" and isinstance(v, str) else v
    lib = load()
    m = int(lib.bacov_ref_num_columns(models.size, _p(models), _p(cc), icam.size, _p(pc)))
    if m < 0 or m > MAX_COLUMNS:
        raise ValueError("covariance reference: invalid input")
    opts = np.array([o["loss_function_type"], o["loss_function_scale"], o["damping"]], np.float64)
    info = np.zeros(4)
    owner, coord = np.zeros(max(m, 1), np.uint32), np.zeros(max(m, 1), np.uint32)
    matrix = np.zeros((m, m)) if m else np.zeros((0, 0))
    mbuf = matrix if m else np.zeros(1)
    present, pcov = np.zeros(max(X.shape[0], 1), np.uint8), np.zeros((max(X.shape[0], 1), 3, 3))
    rc = lib.bacov_ref_run(models.size, _p(models), _p(prm), _p(cc), icam.size, _p(icam), _p(q), _p(t), _p(pc),
                           X.shape[0], _p(X), _p(pm), oi.size, _p(oi), _p(op), _p(xy), _p(opts), _p(info), _p(owner),
                           _p(coord), _p(mbuf), _p(present), _p(pcov))
    if rc != 0:
        raise ValueError("covariance reference: invalid input")
    ok = bool(info[0])
    return dict(success=ok, failed_column=int(info[3]), num_columns=m, min_pivot_ratio=float(info[2]),
                column_owner=owner[:m].copy(), column_coord=coord[:m].copy(), matrix=matrix if ok else None,
                point_present=present[:X.shape[0]].astype(bool) if ok else None,
                point_cov=pcov[:X.shape[0]].copy() if ok else None)
