"""ctypes wrapper of the CPU reference of track completion and track merging (tests/tracks_ref/tracks_ref.cc, written
from DESIGN.md section 18 without any product header; it includes tests/filter_ref/filter_ref.cc for section 16's squared
reprojection error), built on first use into tests/tracks_ref/_build/ with the flags of tests/ba_ref_lib.py."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from triangulator_ref_lib import NO_POINT, options_array

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "tracks_ref" / "tracks_ref.cc"
DEPS = [ROOT / "tests" / "filter_ref" / "filter_ref.cc", ROOT / "tests" / "ba_ref" / "ba_ref.cc",
        ROOT / "tests" / "abspose_ref" / "abspose_ref.cc"]
LIB = ROOT / "tests" / "tracks_ref" / "_build" / "libtracksref.so"
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
    V, Z, U32, U64, D, I64 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_double, C.c_int64
    sig = {
        "tracksref_scene_new": (V, []),
        "tracksref_scene_free": (None, [V]),
        "tracksref_add_camera": (None, [V, U32, C.c_int, U64, U64, V, C.c_int]),
        "tracksref_add_image": (None, [V, U32, U32, V, V, Z, V, V]),
        "tracksref_add_point": (None, [V, U64, V, V, D, Z, V, V]),
        "tracksref_graph_add_image": (None, [V, U32, Z]),
        "tracksref_graph_add_correspondences": (C.c_int, [V, U32, U32, V, Z]),
        "tracksref_graph_finalize": (None, [V]),
        "tracksref_add_modified": (None, [V, U64]),
        "tracksref_complete": (I64, [V, V, V, Z]),
        "tracksref_merge": (I64, [V, V, V, Z]),
        "tracksref_num_points": (Z, [V]),
        "tracksref_get_points": (None, [V, V, V, V, V, V]),
        "tracksref_get_track": (None, [V, U64, V, V]),
        "tracksref_get_point2D_ids": (None, [V, U32, V]),
        "tracksref_num_modified": (Z, [V]),
        "tracksref_get_modified": (None, [V, V]),
        "tracksref_min_margin": (D, [V]),
        "tracksref_pairs_tried": (U64, [V]),
        "tracksref_flat_complete": (C.c_int, [Z, V, V, Z, V, V, V, Z, V, V, V, V, D, V, V]),
        "tracksref_flat_merge": (C.c_int, [Z, V, V, Z, V, V, V, Z, V, V, V, V, V, V, V, V, V, D, V, V, V, V, V, V]),
    }
    for name, (res, args) in sig.items():
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    _lib = lib
    return lib


def _f(a, shape):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(shape)


def _u(a, dtype):
    return np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=dtype)


def _params12(camera_params, n):
    prm = np.zeros((n, 12))
    for c in range(n):
        p = np.asarray(camera_params[c], np.float64).reshape(-1)
        prm[c, :p.size] = p
    return prm


def complete_tracks(camera_models, camera_params, image_cameras, qvec, tvec, item_xyz, item_offsets, cand_image, cand_xy,
                    complete_max_reproj_error=4.0):
    """The reference on a flat problem, in Context.complete_tracks's result form (without the timings and batches)."""
    models = _u(camera_models, np.int32)
    prm = _params12(camera_params, models.size)
    icam = _u(image_cameras, np.uint32)
    q, t, X = _f(qvec, (-1, 4)), _f(tvec, (-1, 3)), _f(item_xyz, (-1, 3))
    off, ci, xy = _u(item_offsets, np.uint64), _u(cand_image, np.uint32), _f(cand_xy, (-1, 2))
    if not (q.shape[0] == t.shape[0] == icam.size and off.size == X.shape[0] + 1 and ci.size == xy.shape[0] == int(off[-1])):
        raise ValueError("track completion reference: array lengths disagree")
    n = ci.size
    e2, ok = np.zeros(max(n, 1)), np.zeros(max(n, 1), np.uint8)
    rc = load().tracksref_flat_complete(models.size, _p(models), _p(prm), icam.size, _p(icam), _p(q), _p(t), X.shape[0], _p(X),
                                        _p(off), _p(ci), _p(xy), float(complete_max_reproj_error), _p(e2), _p(ok))
    if rc != 0:
        raise ValueError("track completion reference: invalid input")
    return dict(cand_sq_error=e2[:n], cand_pass=ok[:n].astype(bool), num_passed=int(ok[:n].sum()))


def merge_tracks(camera_models, camera_params, image_cameras, qvec, tvec, comp_point_offsets, comp_root_offsets, roots,
                 point_xyz, point_obs_offsets, obs_image, obs_xy, obs_corr_offsets, corr_obs, merge_max_reproj_error=4.0):
    """The reference on a flat problem, in Context.merge_tracks's result form (without the timings and batches;
    num_pairs_tried is the full two-sided cache's count, at most the library's)."""
    models = _u(camera_models, np.int32)
    prm = _params12(camera_params, models.size)
    icam = _u(image_cameras, np.uint32)
    q, t, X = _f(qvec, (-1, 4)), _f(tvec, (-1, 3)), _f(point_xyz, (-1, 3))
    cpo, cro, rt = _u(comp_point_offsets, np.uint64), _u(comp_root_offsets, np.uint64), _u(roots, np.uint32)
    poo, oi, xy = _u(point_obs_offsets, np.uint64), _u(obs_image, np.uint32), _f(obs_xy, (-1, 2))
    oco, co = _u(obs_corr_offsets, np.uint64), _u(corr_obs, np.uint32)
    if not (q.shape[0] == t.shape[0] == icam.size and cpo.size == cro.size >= 1 and int(cpo[-1]) == X.shape[0] == poo.size - 1
            and int(cro[-1]) == rt.size and int(poo[-1]) == oi.size == xy.shape[0] == oco.size - 1 and int(oco[-1]) == co.size):
        raise ValueError("track merging reference: array lengths disagree")
    npts, nr = X.shape[0], rt.size
    ret, nm = np.zeros(max(nr, 1), np.uint32), np.zeros(max(nr, 1), np.uint32)
    lc, lo, lx = np.zeros(max(npts, 1), np.uint32), np.zeros(max(npts, 1), np.uint32), np.zeros((max(npts, 1), 3))
    tried = np.zeros(1, np.uint64)
    rc = load().tracksref_flat_merge(models.size, _p(models), _p(prm), icam.size, _p(icam), _p(q), _p(t), cpo.size - 1, _p(cpo),
                                     _p(cro), _p(rt), _p(X), _p(poo), _p(oi), _p(xy), _p(oco), _p(co),
                                     float(merge_max_reproj_error), _p(ret), _p(nm), _p(lc), _p(lo), _p(lx), _p(tried))
    if rc != 0:
        raise ValueError("track merging reference: invalid input")
    ret, nm = ret[:nr], nm[:nr]
    moff = np.concatenate([[0], np.cumsum(nm)]).astype(np.uint64)
    cur, oth, mxyz = [], [], []
    for c in range(cpo.size - 1):
        n = int(nm[int(cro[c]):int(cro[c + 1])].sum())
        p0 = int(cpo[c])
        cur.append(lc[p0:p0 + n])
        oth.append(lo[p0:p0 + n])
        mxyz.append(lx[p0:p0 + n])
    cat = lambda v, shape, dt: (np.concatenate(v) if v else np.zeros(0, dt)).reshape(shape).astype(dt)  # noqa: E731
    return dict(root_return=ret, root_merge_offsets=moff, merge_current=cat(cur, (-1,), np.uint32),
                merge_other=cat(oth, (-1,), np.uint32), merge_xyz=cat(mxyz, (-1, 3), np.float64),
                num_merges=int(moff[-1]), num_pairs_tried=int(tried[0]))


class Scene:
    """A model and a correspondence graph held by the reference: cameras {id: (model, width, height, params)}, images
    {id: (camera_id, qvec xyzw, tvec, xy (N, 2) pixels, point3D ids (N,) or NO_POINT)}, points {id: (xyz, rgb, error,
    [(image, point2D)])}, graph_images {id: num_points2D} and matches [(id1, id2, (M, 2))] in insertion order."""

    def __init__(self, cameras, images, points, graph_images, matches, modified=(), finalize=True):
        lib = load()
        self._lib, self._s = lib, lib.tracksref_scene_new()
        self._npoints2D = {iid: len(im[3]) for iid, im in images.items()}
        for cid, (model, w, h, prm) in cameras.items():
            p = _f(prm, (-1,))
            lib.tracksref_add_camera(self._s, cid, int(model), int(w), int(h), _p(p), p.size)
        for iid, (cid, q, t, xy, pids) in images.items():
            xy = _f(xy, (-1, 2))
            ids = np.ascontiguousarray(pids, dtype=np.uint64)
            lib.tracksref_add_image(self._s, iid, cid, _p(_f(q, (4,))), _p(_f(t, (3,))), len(xy), _p(xy), _p(ids))
        for pid, (xyz, rgb, err, track) in points.items():
            ti = np.array([e[0] for e in track], np.uint32)
            tk = np.array([e[1] for e in track], np.uint32)
            lib.tracksref_add_point(self._s, pid, _p(_f(xyz, (3,))), _p(np.ascontiguousarray(rgb, np.uint8)), float(err),
                                    len(track), _p(ti), _p(tk))
        for iid, n in graph_images.items():
            lib.tracksref_graph_add_image(self._s, iid, n)
        for id1, id2, m in matches:
            m = np.ascontiguousarray(m, dtype=np.uint32).reshape(-1, 2)
            if lib.tracksref_graph_add_correspondences(self._s, id1, id2, _p(m), len(m)) != 0:
                raise ValueError("tracks reference: correspondences of an unknown image")
        if finalize:
            lib.tracksref_graph_finalize(self._s)
        for pid in modified:
            lib.tracksref_add_modified(self._s, pid)

    def __del__(self):
        try:
            self._lib.tracksref_scene_free(self._s)
        except Exception:  # interpreter shutdown
            pass

    def _run(self, fn, ids, options):
        a = None if ids is None else np.array(sorted(set(int(i) for i in ids)), np.uint64)
        if a is not None and a.size == 0:
            return 0
        n = int(fn(self._s, _p(options_array(**options)), _p(a), 0 if a is None else a.size))
        if n < 0:
            raise ValueError("tracks reference: the graph does not hold an image of a track")
        return n

    def complete(self, ids=None, **options):
        """complete_tracks(ids), or complete_all_tracks for ids=None"""
        return self._run(self._lib.tracksref_complete, ids, options)

    def merge(self, ids=None, **options):
        """merge_tracks(ids), or merge_all_tracks for ids=None"""
        return self._run(self._lib.tracksref_merge, ids, options)

    def points(self):
        """{id: (xyz (3,), rgb, error, [(image, point2D)])} in ascending id order"""
        n = int(self._lib.tracksref_num_points(self._s))
        m = max(n, 1)
        ids, xyz, err, lens, rgb = np.zeros(m, np.uint64), np.zeros((m, 3)), np.zeros(m), np.zeros(m, np.uint64), np.zeros((m, 3), np.uint8)
        self._lib.tracksref_get_points(self._s, _p(ids), _p(xyz), _p(err), _p(lens), _p(rgb))
        out = {}
        for i in range(n):
            a, b = np.zeros(max(int(lens[i]), 1), np.uint32), np.zeros(max(int(lens[i]), 1), np.uint32)
            self._lib.tracksref_get_track(self._s, int(ids[i]), _p(a), _p(b))
            out[int(ids[i])] = (xyz[i].copy(), tuple(int(v) for v in rgb[i]), float(err[i]),
                                [(int(a[k]), int(b[k])) for k in range(int(lens[i]))])
        return out

    def point2D_ids(self):
        """{image id: (N,) point3D ids}"""
        out = {}
        for iid, n in self._npoints2D.items():
            ids = np.zeros(max(n, 1), np.uint64)
            self._lib.tracksref_get_point2D_ids(self._s, iid, _p(ids))
            out[iid] = ids[:n]
        return out

    def modified(self):
        n = int(self._lib.tracksref_num_modified(self._s))
        ids = np.zeros(max(n, 1), np.uint64)
        self._lib.tracksref_get_modified(self._s, _p(ids))
        return set(int(i) for i in ids[:n])

    def min_margin(self):
        """the smallest |e - max^2| / max^2 over the finite errors that decided something so far"""
        return float(self._lib.tracksref_min_margin(self._s))

    def pairs_tried(self):
        return int(self._lib.tracksref_pairs_tried(self._s))


__all__ = ["NO_POINT", "Scene", "complete_tracks", "merge_tracks", "load", "options_array"]
