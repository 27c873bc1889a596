"""ctypes wrapper of the CPU reference of the two-view triangulation of image pairs (tests/initpair_ref/initpair_ref.cc,
written from DESIGN.md section 21 without any product header; it includes tests/tri_ref/tri_ref.cc for section 11's
numerics), built on first use into tests/initpair_ref/_build/ with the flags of tests/ba_ref_lib.py.  Pixels are lifted
to the normalised image plane here, with the oracle's Camera::CamFromImg (tests/triangulator_ref_lib.lift).  Also the
reference of the scene normalisation of section 21.3, in numpy."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "initpair_ref" / "initpair_ref.cc"
DEPS = [ROOT / "tests" / "tri_ref" / "tri_ref.cc"]
LIB = ROOT / "tests" / "initpair_ref" / "_build" / "libinitpairref.so"
DEFAULT_MIN_TRI_ANGLE = 0.017453292519943295 * 16.0
_lib = None
_p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
_f = lambda a, shape: np.ascontiguousarray(a, dtype=np.float64).reshape(shape)  # noqa: E731


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
    V, Z, D = C.c_void_p, C.c_size_t, C.c_double
    lib.initpair_ref_triangulate.restype = C.c_int
    lib.initpair_ref_triangulate.argtypes = [Z, V, V, Z, V, V, V, V, D, V, V, V, V]
    _lib = lib
    return lib


def lift_pairs(camera_models, camera_params, image_cameras, pair_images, pair_offsets, corr_xy1, corr_xy2):
    """Camera::CamFromImg of every correspondence's two pixels, through the camera of its pair's image"""
    import triangulator_ref_lib
    pi = np.asarray(pair_images, np.int64).reshape(-1, 2)
    off = np.asarray(pair_offsets, np.int64).reshape(-1)
    out = [_f(corr_xy1, (-1, 2)).copy(), _f(corr_xy2, (-1, 2)).copy()]
    for p in range(len(pi)):
        for side in (0, 1):
            c = int(np.asarray(image_cameras).reshape(-1)[pi[p, side]])
            s = slice(int(off[p]), int(off[p + 1]))
            out[side][s] = triangulator_ref_lib.lift(int(np.asarray(camera_models).reshape(-1)[c]), np.asarray(camera_params[c], np.float64).reshape(-1),
                                                     out[side][s])
    return out


def triangulate_pairs(camera_models, camera_params, image_cameras, qvec, tvec, pair_images, pair_offsets, corr_xy1, corr_xy2,
                      min_tri_angle=DEFAULT_MIN_TRI_ANGLE, depths=False):
    """The reference on the flat problem of Context.triangulate_pairs, in its result form (without timings); depths=True
    adds the two depths of every correspondence as `depths` (M, 2)."""
    q, t = _f(qvec, (-1, 4)), _f(tvec, (-1, 3))
    pi = np.ascontiguousarray(np.asarray(pair_images).reshape(-1, 2), dtype=np.uint32)
    off = np.ascontiguousarray(np.asarray(pair_offsets).reshape(-1), dtype=np.uint64)
    xy1, xy2 = _f(corr_xy1, (-1, 2)), _f(corr_xy2, (-1, 2))
    n = len(xy1)
    if not (len(q) == len(t) == len(np.asarray(image_cameras).reshape(-1)) and off.size == len(pi) + 1 and int(off[-1]) == n == len(xy2)):
        raise ValueError("initial pair reference: array lengths disagree")
    n1, n2 = lift_pairs(camera_models, camera_params, image_cameras, pi, off, xy1, xy2)
    acc, xyz, ang = np.zeros(max(n, 1), np.uint8), np.zeros((max(n, 1), 3)), np.zeros(max(n, 1))
    dep = np.zeros((max(n, 1), 2)) if depths else None
    if load().initpair_ref_triangulate(len(q), _p(q), _p(t), len(pi), _p(pi), _p(off), _p(n1), _p(n2), float(min_tri_angle), _p(acc),
                                       _p(xyz), _p(ang), _p(dep)) != 0:
        raise ValueError("initial pair reference: invalid input")
    res = dict(accepted=acc[:n].astype(bool), xyz=xyz[:n], tri_angle=ang[:n], num_accepted=int(acc[:n].sum()))
    if depths:
        res["depths"] = dep[:n]
    return res


# ---- 21.3: Normalize(extent = 10, p0 = 0.1, p1 = 0.9, use_images = true) ---------------------------------------------------
def rotation_matrix(q_xyzw):
    """11.1's matrix of a quaternion x y z w"""
    x, y, z, w = (float(v) for v in q_xyzw)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def normalize(poses, points, reg_image_ids, extent=10.0, p0=0.1, p1=0.9):
    """poses {image id: (q x y z w, t)}, points {id: xyz} -> (poses', points', scale, centroid); unchanged below two images"""
    ids = list(reg_image_ids)
    if len(ids) < 2:
        return dict(poses), dict(points), 1.0, np.zeros(3)
    centres = np.array([[-float(sum(rotation_matrix(poses[i][0])[r, c] * poses[i][1][r] for r in range(3))) for c in range(3)] for i in ids])
    coords = np.sort(centres.astype(np.float32), axis=0)
    n = len(ids)
    P0 = int(p0 * (n - 1)) if n > 3 else 0
    P1 = int(p1 * (n - 1)) if n > 3 else n - 1
    lo, hi = coords[P0].astype(np.float64), coords[P1].astype(np.float64)
    mean = np.zeros(3)
    for i in range(P0, P1 + 1):
        mean = mean + coords[i].astype(np.float64)
    mean = mean / float(P1 - P0 + 1)
    d = hi - lo
    old = float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
    scale = 1.0 if old < np.finfo(np.float64).eps else extent / old
    new_poses = {}
    for i, (q, t) in poses.items():
        R = rotation_matrix(q)
        new_poses[i] = (np.array(q, np.float64), np.array([(float(t[r]) + (R[r, 0] * mean[0] + R[r, 1] * mean[1] + R[r, 2] * mean[2])) * scale for r in range(3)]))
    new_points = {p: np.array([scale * float(X[c]) + -(scale * mean[c]) for c in range(3)]) for p, X in points.items()}
    return new_poses, new_points, scale, mean
