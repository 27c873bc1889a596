"""ctypes wrapper of the undistortion CPU reference (tests/undistort_ref/undistort_ref.cc), built on first use into
tests/undistort_ref/_build/ with g++ -O2 -ffp-contract=off -fno-fast-math (the flags of tests/shim)."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "undistort_ref" / "undistort_ref.cc"
LIB = ROOT / "tests" / "undistort_ref" / "_build" / "libundistortref.so"
_lib = None

MODEL_IDS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4, "OPENCV_FISHEYE": 5,
             "FULL_OPENCV": 6, "FOV": 7, "SIMPLE_RADIAL_FISHEYE": 8, "RADIAL_FISHEYE": 9, "THIN_PRISM_FISHEYE": 10}
# UndistortCameraOptions(), in the order undistort_ref_camera reads them
DEFAULTS = dict(blank_pixels=0.0, min_scale=0.2, max_scale=2.0, max_image_size=-1, roi_min_x=0.0, roi_min_y=0.0,
                roi_max_x=1.0, roi_max_y=1.0)


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    LIB.parent.mkdir(parents=True, exist_ok=True)
    if not LIB.exists() or LIB.stat().st_mtime < SRC.stat().st_mtime:
        tmp = LIB.with_name(LIB.name + ".tmp")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-Wall", "-shared", "-fPIC",
                        str(SRC), "-o", str(tmp)], check=True)
        tmp.replace(LIB)
    lib = C.CDLL(str(LIB))
    lib.undistort_ref_atan.restype = C.c_double
    lib.undistort_ref_atan.argtypes = [C.c_double]
    lib.undistort_ref_camera.restype = C.c_int
    lib.undistort_ref_camera.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.undistort_ref_points.restype = None
    lib.undistort_ref_points.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.undistort_ref_resize.restype = None
    lib.undistort_ref_resize.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]
    lib.undistort_ref_warp.restype = None
    lib.undistort_ref_warp.argtypes = ([C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_int, C.c_int] + [C.c_void_p] * 3)
    _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _model_id(model) -> int:
    return MODEL_IDS[model] if isinstance(model, str) else int(model)


def _params12(params) -> np.ndarray:
    p = np.zeros(12, np.float64)
    q = np.asarray(params, dtype=np.float64).reshape(-1)
    p[:q.size] = q
    return p


def undistort_camera(camera, **opts):
    """The reference's UndistortCamera: (model, width, height, params) -> (1, width, height, params (4,))."""
    o = dict(DEFAULTS)
    for k, v in opts.items():
        if k not in o:
            raise ValueError(f"unknown option {k!r}")
        o[k] = v
    model, width, height, params = camera
    ov = np.array([float(o[k]) for k in DEFAULTS], np.float64)
    out = np.zeros(6, np.float64)
    if load().undistort_ref_camera(_ptr(ov), _model_id(model), int(width), int(height), _ptr(_params12(params)), _ptr(out)):
        raise ValueError("undistort_ref_camera: invalid options or camera")
    return (1, int(out[0]), int(out[1]), out[2:6].copy())


def undistort_points(camera, undistorted, points) -> np.ndarray:
    xy = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    out = np.empty_like(xy)
    pin = np.ascontiguousarray(undistorted[3], dtype=np.float64)
    load().undistort_ref_points(_model_id(camera[0]), _ptr(_params12(camera[3])), _ptr(pin), xy.shape[0], _ptr(xy), _ptr(out))
    return out


def resize(img: np.ndarray, dw: int, dh: int) -> np.ndarray:
    a = np.ascontiguousarray(img, dtype=np.uint8)
    ch = 1 if a.ndim == 2 else a.shape[2]
    out = np.zeros((dh, dw) + ((ch,) if a.ndim == 3 else ()), np.uint8)
    load().undistort_ref_resize(_ptr(a), a.shape[1], a.shape[0], ch, dw, dh, _ptr(out))
    return out


def warp(img: np.ndarray, src_camera, dst_camera, details: bool = False):
    """The reference's warp of one image (with the pre-pass when the target has fewer pixels).  details: also the
    values before rounding (-1 outside) and the source coordinates, both of the target's shape."""
    a = np.ascontiguousarray(img, dtype=np.uint8)
    ch = 1 if a.ndim == 2 else a.shape[2]
    dw, dh = int(dst_camera[1]), int(dst_camera[2])
    pin = np.ascontiguousarray(dst_camera[3], dtype=np.float64)
    out = np.zeros((dh, dw) + ((ch,) if a.ndim == 3 else ()), np.uint8)
    vals = np.zeros((dh, dw, ch), np.float64) if details else None
    coords = np.zeros((dh, dw, 2), np.float64) if details else None
    load().undistort_ref_warp(_ptr(a), a.strides[0], a.shape[1], a.shape[0], ch, _model_id(src_camera[0]),
                              _ptr(_params12(src_camera[3])), _ptr(pin), dw, dh, _ptr(out),
                              _ptr(vals) if details else None, _ptr(coords) if details else None)
    return (out, vals, coords) if details else out
