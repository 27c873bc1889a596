"""ctypes wrapper of the incremental triangulator's CPU reference (tests/triangulator_ref/triangulator_ref.cc, written
from DESIGN.md section 17 without any product header; it includes tests/tri_ref/tri_ref.cc for section 11's LO-RANSAC),
built on first use into tests/triangulator_ref/_build/ with the flags of tests/ba_ref_lib.py.  Pixels are lifted to the
normalised image plane here, with the oracle's Camera::CamFromImg (tests/oracle_lib.py)."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import oracle_lib

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "triangulator_ref" / "triangulator_ref.cc"
DEPS = [ROOT / "tests" / "tri_ref" / "tri_ref.cc"]
LIB = ROOT / "tests" / "triangulator_ref" / "_build" / "libtriangulatorref.so"
NO_POINT = 0xFFFFFFFFFFFFFFFF
OPTION_FIELDS = ("max_transitivity", "create_max_angle_error", "continue_max_angle_error", "merge_max_reproj_error",
                 "complete_max_reproj_error", "complete_max_transitivity", "re_max_angle_error", "re_min_ratio",
                 "re_max_trials", "min_angle", "ignore_two_view_tracks", "min_focal_length_ratio",
                 "max_focal_length_ratio", "max_extra_param")
OPTION_DEFAULTS = (1, 2.0, 2.0, 4.0, 4.0, 5, 5.0, 0.2, 1, 1.5, True, 0.1, 10.0, 1.0)
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
    V, Z, U32, U64, D = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_double
    sig = {
        "triref_observations": (C.c_int, [Z, V, V, Z, V, V, V, V, V, V, D, D, D, V, V, V, V, V]),
        "triref_angular_error": (D, [V, V, V, V]),
        "triref_scene_new": (V, []),
        "triref_scene_free": (None, [V]),
        "triref_add_camera": (None, [V, U32, C.c_int, U64, U64, V, C.c_int]),
        "triref_add_image": (None, [V, U32, U32, V, V, Z, V, V]),
        "triref_add_point": (None, [V, U64, V, Z, V, V]),
        "triref_graph_add_image": (None, [V, U32, Z]),
        "triref_graph_add_correspondences": (C.c_int, [V, U32, U32, V, Z]),
        "triref_graph_finalize": (None, [V]),
        "triref_graph_num_images": (Z, [V]),
        "triref_graph_exists_image": (C.c_int, [V, U32]),
        "triref_graph_image_counts": (C.c_int, [V, U32, V]),
        "triref_graph_pair_count": (U64, [V, U32, U32]),
        "triref_graph_transitive": (C.c_int64, [V, U32, U32, Z, V, V, Z]),
        "triref_graph_is_two_view": (C.c_int, [V, U32, U32]),
        "triref_triangulate_image": (C.c_int64, [V, V, U32]),
        "triref_num_points": (Z, [V]),
        "triref_get_points": (None, [V, V, V, V, V]),
        "triref_get_track": (None, [V, U64, V, V]),
        "triref_get_point2D_ids": (None, [V, U32, V]),
        "triref_num_modified": (Z, [V]),
        "triref_get_modified": (None, [V, V]),
        "triref_margins": (None, [V, V]),
    }
    for name, (res, args) in sig.items():
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    _lib = lib
    return lib


def _f(a, shape):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(shape)


def lift(model, params, xy):
    """Camera::CamFromImg of N x 2 pixels (the oracle's; width and height do not enter)."""
    xy = _f(xy, (-1, 2))
    if not len(xy):
        return xy.copy()
    with np.errstate(all="ignore"):
        return oracle_lib.cam_from_img(oracle_lib.make_camera(int(model), 0, 0, tuple(np.asarray(params, np.float64))), xy)


def angular_error(nxy, q, t, X) -> float:
    """Continue's angle: 11.2's residual before squaring, of the normalised point under the pose (q x y z w, t)"""
    return float(load().triref_angular_error(_p(_f(nxy, (2,))), _p(_f(q, (4,))), _p(_f(t, (3,))), _p(_f(X, (3,)))))


def round_slots(item_offsets):
    """The offsets of the items' round slots: an item of n candidates can create n // 2 tracks."""
    off = np.asarray(item_offsets, np.int64)
    return np.concatenate([[0], np.cumsum((off[1:] - off[:-1]) // 2)]).astype(np.uint64)


def triangulate_observations(camera_models, camera_params, image_cameras, qvec, tvec, item_offsets, cand_image, cand_xy,
                             cand_has_point, cand_xyz, no_create_two_view=None, create_max_angle_error=2.0,
                             continue_max_angle_error=2.0, min_angle=1.5):
    """The reference on a flat problem, in Context.triangulate_observations's result form (without timings and batches)."""
    models = np.array(camera_models, dtype=np.int32).reshape(-1)
    icam = np.array(image_cameras, dtype=np.int64).reshape(-1)
    q, t = _f(qvec, (-1, 4)), _f(tvec, (-1, 3))
    off = np.array(item_offsets, dtype=np.uint64).reshape(-1)
    ci = np.array(cand_image, dtype=np.uint32).reshape(-1)
    xy, X = _f(cand_xy, (-1, 2)), _f(cand_xyz, (-1, 3))
    has = np.ascontiguousarray(np.asarray(cand_has_point).reshape(-1) != 0, dtype=np.uint8)
    two = None if no_create_two_view is None else np.ascontiguousarray(np.asarray(no_create_two_view).reshape(-1) != 0, dtype=np.uint8)
    n, nit = ci.size, off.size - 1
    if not (q.shape[0] == t.shape[0] == icam.size and xy.shape[0] == X.shape[0] == has.size == n == int(off[-1])):
        raise ValueError("triangulator reference: array lengths disagree")
    nxy = np.zeros((n, 2))
    ccam = icam[ci] if n else np.zeros(0, np.int64)
    for c in np.unique(ccam):
        sel = ccam == c
        nxy[sel] = lift(models[c], camera_params[c], xy[sel])
    slots = round_slots(off)
    cont, rnd = np.zeros(max(nit, 1), np.int32), np.zeros(max(n, 1), np.uint32)
    nr, rxyz = np.zeros(max(nit, 1), np.uint32), np.zeros((max(int(slots[-1]), 1), 3))
    rc = load().triref_observations(icam.size, _p(q), _p(t), nit, _p(off), _p(ci), _p(nxy), _p(has), _p(X), _p(two),
                                    float(create_max_angle_error), float(continue_max_angle_error), float(min_angle),
                                    _p(cont), _p(rnd), _p(nr), _p(slots), _p(rxyz))
    if rc != 0:
        raise ValueError("triangulator reference: invalid input")
    nr = nr[:nit]
    roff = np.concatenate([[0], np.cumsum(nr)]).astype(np.uint64)
    out_xyz = np.zeros((int(roff[-1]), 3))
    for i in range(nit):
        out_xyz[int(roff[i]):int(roff[i + 1])] = rxyz[int(slots[i]):int(slots[i]) + int(nr[i])]
    return dict(continued=cont[:nit], cand_round=rnd[:n], round_offsets=roff, round_xyz=out_xyz,
                num_created=int(roff[-1]), num_continued=int((cont[:nit] >= 0).sum()))


def options_array(**kw):
    o = dict(zip(OPTION_FIELDS, OPTION_DEFAULTS))
    for k, v in kw.items():
        if k not in o:
            raise KeyError(k)
        o[k] = v
    return np.array([float(o[k]) for k in OPTION_FIELDS])


class Scene:
    """A model and a correspondence graph held by the reference: cameras {id: (model, width, height, params)}, images
    {id: (camera_id, qvec xyzw, tvec, xy (N, 2) pixels, point3D ids (N,) or NO_POINT)}, points {id: (xyz, [(image,
    point2D)])}, graph_images {id: num_points2D} and matches [(id1, id2, (M, 2))] in insertion order."""

    def __init__(self, cameras, images, points, graph_images, matches, finalize=True):
        lib = load()
        self._lib, self._s = lib, lib.triref_scene_new()
        for cid, (model, w, h, prm) in cameras.items():
            p = _f(prm, (-1,))
            lib.triref_add_camera(self._s, cid, int(model), int(w), int(h), _p(p), p.size)
        for iid, (cid, q, t, xy, pids) in images.items():
            xy = _f(xy, (-1, 2))
            nxy = lift(cameras[cid][0], cameras[cid][3], xy)
            ids = np.ascontiguousarray(pids, dtype=np.uint64)
            lib.triref_add_image(self._s, iid, cid, _p(_f(q, (4,))), _p(_f(t, (3,))), len(xy), _p(nxy), _p(ids))
        for pid, (xyz, track) in points.items():
            ti = np.array([e[0] for e in track], np.uint32)
            tk = np.array([e[1] for e in track], np.uint32)
            lib.triref_add_point(self._s, pid, _p(_f(xyz, (3,))), len(track), _p(ti), _p(tk))
        for iid, n in graph_images.items():
            lib.triref_graph_add_image(self._s, iid, n)
        for id1, id2, m in matches:
            m = np.ascontiguousarray(m, dtype=np.uint32).reshape(-1, 2)
            if lib.triref_graph_add_correspondences(self._s, id1, id2, _p(m), len(m)) != 0:
                raise ValueError("triangulator reference: correspondences of an unknown image")
        if finalize:
            lib.triref_graph_finalize(self._s)

    def __del__(self):
        try:
            self._lib.triref_scene_free(self._s)
        except Exception:  # interpreter shutdown
            pass

    # the graph
    def finalize(self):
        self._lib.triref_graph_finalize(self._s)

    def num_images(self):
        return int(self._lib.triref_graph_num_images(self._s))

    def exists_image(self, iid):
        return bool(self._lib.triref_graph_exists_image(self._s, iid))

    def image_counts(self, iid):
        out = np.zeros(2, np.uint64)
        if self._lib.triref_graph_image_counts(self._s, iid, _p(out)) != 0:
            raise ValueError("unknown image")
        return int(out[0]), int(out[1])

    def pair_count(self, id1, id2):
        return int(self._lib.triref_graph_pair_count(self._s, id1, id2))

    def transitive(self, iid, idx, transitivity):
        cap = 4096
        a, b = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        n = int(self._lib.triref_graph_transitive(self._s, iid, idx, transitivity, _p(a), _p(b), cap))
        if n < 0:
            raise ValueError("unknown image or point2D")
        assert n <= cap
        return [(int(a[i]), int(b[i])) for i in range(n)]

    def is_two_view(self, iid, idx):
        return bool(self._lib.triref_graph_is_two_view(self._s, iid, idx))

    # the triangulator
    def triangulate_image(self, image_id, **options):
        n = int(self._lib.triref_triangulate_image(self._s, _p(options_array(**options)), image_id))
        if n < 0:
            raise ValueError("triangulator reference: the model or the graph does not hold the image")
        return n

    def points(self):
        """{id: (xyz (3,), error, [(image, point2D)])} in ascending id order"""
        n = int(self._lib.triref_num_points(self._s))
        ids, xyz, err, lens = np.zeros(max(n, 1), np.uint64), np.zeros((max(n, 1), 3)), np.zeros(max(n, 1)), np.zeros(max(n, 1), np.uint64)
        self._lib.triref_get_points(self._s, _p(ids), _p(xyz), _p(err), _p(lens))
        out = {}
        for i in range(n):
            a, b = np.zeros(max(int(lens[i]), 1), np.uint32), np.zeros(max(int(lens[i]), 1), np.uint32)
            self._lib.triref_get_track(self._s, int(ids[i]), _p(a), _p(b))
            out[int(ids[i])] = (xyz[i].copy(), float(err[i]), [(int(a[k]), int(b[k])) for k in range(int(lens[i]))])
        return out

    def point2D_ids(self, image_id, n):
        ids = np.zeros(max(n, 1), np.uint64)
        self._lib.triref_get_point2D_ids(self._s, image_id, _p(ids))
        return ids[:n]

    def modified(self):
        n = int(self._lib.triref_num_modified(self._s))
        ids = np.zeros(max(n, 1), np.uint64)
        self._lib.triref_get_modified(self._s, _p(ids))
        return set(int(i) for i in ids[:n])

    def margins(self):
        """(Continue's, Create's) smallest distance of a deciding angle from its threshold so far, radians"""
        out = np.zeros(2)
        self._lib.triref_margins(self._s, _p(out))
        return float(out[0]), float(out[1])
