"""ctypes wrapper of the triangulation CPU reference (tests/tri_ref/tri_ref.cc), built on first use into
tests/tri_ref/_build/ with g++ -O2 -ffp-contract=off -fno-fast-math (the flags of tests/shim)."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "tri_ref" / "tri_ref.cc"
LIB = ROOT / "tests" / "tri_ref" / "_build" / "libtriref.so"
_lib = None

# EstimateTriangulationOptions() with pycolmap's RANSACOptions()
DEFAULTS = dict(min_tri_angle=0.0, max_error=4.0, min_inlier_ratio=0.01, confidence=0.9999,
                dyn_num_trials_multiplier=3.0, min_num_trials=1000, max_num_trials=100000)


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
    lib.tri_ref_acos.restype = C.c_double
    lib.tri_ref_acos.argtypes = [C.c_double]
    lib.tri_ref_angle.restype = C.c_double
    lib.tri_ref_angle.argtypes = [C.c_void_p] * 3
    lib.tri_ref_triangulate.restype = C.c_int
    lib.tri_ref_triangulate.argtypes = ([C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p] +
                                        [C.c_double] * 5 + [C.c_int64] * 2 + [C.c_void_p] * 5)
    lib.tri_ref_triangulate_trace.restype = C.c_int
    lib.tri_ref_triangulate_trace.argtypes = lib.tri_ref_triangulate.argtypes + [C.c_void_p] * 3
    _lib = lib
    return lib


# tri_ref_triangulate_trace's integers per track, in struct Trace's order (tests/tri_ref/tri_ref.cc)
TRACE_FIELDS = ("dyn_row", "abort_trial", "depth_rejects", "angle_rejects", "lo_rounds", "lo_max_iters", "lo_max_growing",
                "lo_iters", "lo_replaced", "lo_refused", "nan")


def triangulate(poses, track_offsets, obs_pose, obs_xy, **opts):
    """The reference on a batch, in Context.triangulate_tracks' form: (xyz (T, 3), success (T,) bool,
    inlier_mask (M,) bool, {"num_inliers", "num_trials"})."""
    return _run(False, poses, track_offsets, obs_pose, obs_xy, opts)


def triangulate_trace(poses, track_offsets, obs_pose, obs_xy, **opts):
    """triangulate(), and a fifth element: what each track's RANSAC went through, a dict of (T,) int64 arrays named by
    TRACE_FIELDS (abort_trial is -1 where abort was never set), "angle" (T,) - the triangulation angle that admitted the
    final model, or without a model the last one that refused one - and "residuals" (M,), the final model's (NaN in a
    track without a model)."""
    return _run(True, poses, track_offsets, obs_pose, obs_xy, opts)


def _run(trace, poses, track_offsets, obs_pose, obs_xy, opts):
    o = dict(DEFAULTS)
    for k, v in opts.items():
        if k not in o:
            raise ValueError(f"unknown option {k!r}")
        o[k] = v
    P = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12)
    off = np.ascontiguousarray(track_offsets, dtype=np.uint64).reshape(-1)
    op = np.ascontiguousarray(obs_pose, dtype=np.uint32).reshape(-1)
    xy = np.ascontiguousarray(obs_xy, dtype=np.float64).reshape(-1, 2)
    nt, m = off.size - 1, int(off[-1])
    xyz = np.zeros((nt, 3), np.float64)
    ok = np.zeros(nt, np.uint8)
    ninl = np.zeros(nt, np.uint32)
    ntr = np.zeros(nt, np.uint64)
    mask = np.zeros(max(m, 1), np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    args = [ptr(P), P.shape[0], ptr(off), nt, ptr(op), ptr(xy), float(o["min_tri_angle"]), float(o["max_error"]),
            float(o["min_inlier_ratio"]), float(o["confidence"]), float(o["dyn_num_trials_multiplier"]),
            int(o["min_num_trials"]), int(o["max_num_trials"]), ptr(xyz), ptr(ok), ptr(ninl), ptr(ntr), ptr(mask)]
    if trace:
        ti = np.zeros((max(nt, 1), len(TRACE_FIELDS)), np.int64)
        ta = np.zeros(max(nt, 1), np.float64)
        tres = np.zeros(max(m, 1), np.float64)
        rc = load().tri_ref_triangulate_trace(*args, ptr(ti), ptr(ta), ptr(tres))
    else:
        rc = load().tri_ref_triangulate(*args)
    if rc != 0:
        raise ValueError("tri_ref_triangulate: invalid input")
    out = (xyz, ok.astype(bool), mask[:m].astype(bool), {"num_inliers": ninl, "num_trials": ntr})
    if trace:
        tr = {k: ti[:nt, i].copy() for i, k in enumerate(TRACE_FIELDS)}
        tr["angle"] = ta[:nt]
        tr["residuals"] = tres[:m]
        out += (tr,)
    return out


def acos(x: float) -> float:
    return load().tri_ref_acos(x)


def angle(c1, c2, X) -> float:
    a = [np.ascontiguousarray(v, dtype=np.float64) for v in (c1, c2, X)]
    return load().tri_ref_angle(*(v.ctypes.data_as(C.c_void_p) for v in a))
