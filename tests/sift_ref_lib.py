"""ctypes wrapper of the SIFT CPU reference (tests/sift_ref/sift_ref.cc), built on first use into
tests/sift_ref/_build/ with g++ -O2 -ffp-contract=off -fno-fast-math (the flags of tests/shim)."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "sift_ref" / "sift_ref.cc"
LIB = ROOT / "tests" / "sift_ref" / "_build" / "libsiftref.so"
_lib = None

# SiftExtractionOptions() defaults (COLMAP 3.9.1), the fields the extractor reads
DEFAULTS = dict(first_octave=-1, num_octaves=4, octave_resolution=3, peak_threshold=0.02 / 3, edge_threshold=10.0,
                max_num_orientations=2, upright=False, normalization=0, max_num_features=8192)


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    LIB.parent.mkdir(parents=True, exist_ok=True)
    if not LIB.exists() or LIB.stat().st_mtime < SRC.stat().st_mtime:
        tmp = LIB.with_name(LIB.name + ".tmp")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-Wall", "-Wdouble-promotion",
                        "-shared", "-fPIC", str(SRC), "-o", str(tmp)], check=True)
        tmp.replace(LIB)
    lib = C.CDLL(str(LIB))
    lib.sift_ref_atan2.restype = C.c_float
    lib.sift_ref_atan2.argtypes = [C.c_float, C.c_float]
    lib.sift_ref_expn.restype = C.c_float
    lib.sift_ref_expn.argtypes = [C.c_float]
    lib.sift_ref_pow2.restype = C.c_float
    lib.sift_ref_pow2.argtypes = [C.c_float]
    lib.sift_ref_sincos.restype = None
    lib.sift_ref_sincos.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.sift_ref_finish_descriptor.restype = None
    lib.sift_ref_finish_descriptor.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.sift_ref_extract.restype = C.c_long
    lib.sift_ref_extract.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_int, C.c_int, C.c_int, C.c_double,
                                     C.c_double, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.sift_ref_fetch.restype = None
    lib.sift_ref_fetch.argtypes = [C.c_void_p, C.c_void_p]
    _lib = lib
    return lib


def extract(image: np.ndarray, **opts):
    """(N x 4 float32 keypoints (x, y, scale, orientation), N x 128 uint8 descriptors) of a 2-D uint8 image."""
    o = dict(DEFAULTS)
    o.update(opts)
    img = np.ascontiguousarray(image, dtype=np.uint8)
    lib = load()
    n = lib.sift_ref_extract(img.ctypes.data_as(C.c_void_p), img.shape[1], img.shape[0], img.shape[1],
                             int(o["first_octave"]), int(o["num_octaves"]), int(o["octave_resolution"]),
                             float(o["peak_threshold"]), float(o["edge_threshold"]), int(o["max_num_orientations"]),
                             int(bool(o["upright"])), int(o["normalization"]), int(o["max_num_features"]))
    if n < 0:
        raise ValueError("sift_ref_extract: invalid arguments")
    kp = np.zeros((n, 4), dtype=np.float32)
    desc = np.zeros((n, 128), dtype=np.uint8)
    lib.sift_ref_fetch(kp.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p))
    return kp, desc


def atan2(y: float, x: float) -> float:
    return load().sift_ref_atan2(y, x)


def expn(x: float) -> float:
    return load().sift_ref_expn(x)


def pow2(t: float) -> float:
    return load().sift_ref_pow2(t)


def sincos(th: float) -> tuple[float, float]:
    s, c = C.c_float(), C.c_float()
    load().sift_ref_sincos(th, C.byref(s), C.byref(c))
    return s.value, c.value


def finish_descriptor(hist: np.ndarray, normalization: int = 0) -> np.ndarray:
    """The bytes of a 128-bin histogram in VLFeat's bin order (t + 8 x + 32 y): the reference's normalisations,
    reorder and byte conversion."""
    h = np.ascontiguousarray(hist, dtype=np.float32)
    out = np.zeros(128, np.uint8)
    load().sift_ref_finish_descriptor(h.ctypes.data_as(C.c_void_p), int(normalization), out.ctypes.data_as(C.c_void_p))
    return out
