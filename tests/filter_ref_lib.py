"""ctypes wrapper of the point filter's CPU reference (tests/filter_ref/filter_ref.cc, written from DESIGN.md section 16
without any product header; it includes tests/ba_ref/ba_ref.cc for the pieces section 16 shares with section 15), built
on first use into tests/filter_ref/_build/ with the flags of tests/ba_ref_lib.py."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

VERDICTS = ("KEPT", "NOT_SELECTED", "SHORT_TRACK", "REPROJECTION", "ANGLE")
KEPT, NOT_SELECTED, SHORT_TRACK, REPROJECTION, ANGLE = range(5)

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "filter_ref" / "filter_ref.cc"
DEPS = [ROOT / "tests" / "ba_ref" / "ba_ref.cc", ROOT / "tests" / "abspose_ref" / "abspose_ref.cc"]
LIB = ROOT / "tests" / "filter_ref" / "_build" / "libfilterref.so"
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
    lib.filter_ref_sq_error.restype = C.c_double
    lib.filter_ref_sq_error.argtypes = [C.c_int] + [C.c_void_p] * 5
    lib.filter_ref_angle.restype = C.c_double
    lib.filter_ref_angle.argtypes = [C.c_void_p] * 3
    lib.filter_ref_centre.restype = None
    lib.filter_ref_centre.argtypes = [C.c_void_p] * 3
    lib.filter_ref_filter.restype = C.c_int
    lib.filter_ref_filter.argtypes = ([C.c_size_t] + [C.c_void_p] * 2 + [C.c_size_t] + [C.c_void_p] * 3 + [C.c_size_t] +
                                      [C.c_void_p] * 5 + [C.c_double, C.c_double, C.c_int] + [C.c_void_p] * 5)
    _lib = lib
    return lib


def _f(a, shape):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(shape)


def sq_error(model, params, q, t, X, xy) -> float:
    prm = np.zeros(12)
    prm[:len(params)] = params
    return float(load().filter_ref_sq_error(int(model), _p(prm), _p(_f(q, (4,))), _p(_f(t, (3,))), _p(_f(X, (3,))),
                                            _p(_f(xy, (2,)))))


def angle(c1, c2, X) -> float:
    return float(load().filter_ref_angle(_p(_f(c1, (3,))), _p(_f(c2, (3,))), _p(_f(X, (3,)))))


def centre(q, t):
    C3 = np.zeros(3)
    load().filter_ref_centre(_p(_f(q, (4,))), _p(_f(t, (3,))), _p(C3))
    return C3


def filter_points3d(camera_models, camera_params, image_cameras, qvec, tvec, xyz, track_offsets, obs_image, obs_xy,
                    selected=None, max_reproj_error=4.0, min_tri_angle=1.5, errors_only=False):
    """The reference on a flat problem, in Context.filter_points3d's result form (without the timings and batches)."""
    models = np.array(camera_models, dtype=np.int32).reshape(-1)
    prm = np.zeros((models.size, 12))
    for c in range(models.size):
        p = np.asarray(camera_params[c], np.float64).reshape(-1)
        prm[c, :p.size] = p
    icam = np.array(image_cameras, dtype=np.uint32).reshape(-1)
    q, t, X = _f(qvec, (-1, 4)), _f(tvec, (-1, 3)), _f(xyz, (-1, 3))
    off = np.array(track_offsets, dtype=np.uint64).reshape(-1)
    oi = np.array(obs_image, dtype=np.uint32).reshape(-1)
    xy = _f(obs_xy, (-1, 2))
    if not (q.shape[0] == t.shape[0] == icam.size and off.size == X.shape[0] + 1 and oi.size == xy.shape[0] == int(off[-1])):
        raise ValueError("point filter reference: array lengths disagree")
    sel = None if selected is None else np.ascontiguousarray(np.asarray(selected).reshape(-1) != 0, dtype=np.uint8)
    n, npts = oi.size, X.shape[0]
    e2, dele = np.zeros(max(n, 1)), np.zeros(max(n, 1), np.uint8)
    verdict, perr = np.zeros(max(npts, 1), np.uint8), np.zeros(max(npts, 1))
    count = np.zeros(1, np.uint64)
    rc = load().filter_ref_filter(models.size, _p(models), _p(prm), icam.size, _p(icam), _p(q), _p(t), npts, _p(X), _p(off),
                                  _p(oi), _p(xy), _p(sel), float(max_reproj_error), float(min_tri_angle),
                                  int(bool(errors_only)), _p(e2), _p(dele), _p(verdict), _p(perr), _p(count))
    if rc != 0:
        raise ValueError("point filter reference: invalid input")
    return dict(obs_sq_error=e2[:n], obs_deleted=dele[:n].astype(bool), point_verdict=verdict[:npts],
                point_error=perr[:npts], num_filtered=int(count[0]))
