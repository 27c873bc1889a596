"""ctypes wrapper of retriangulate's CPU reference (tests/retri_ref/retri_ref.cc, written from DESIGN.md section 19
without any product header; it includes tests/triangulator_ref/triangulator_ref.cc for section 17's Continue, Create, graph
and scene), built on first use into tests/retri_ref/_build/ with the flags of tests/ba_ref_lib.py.  Pixels are lifted to
the normalised image plane here, with the oracle's Camera::CamFromImg (tests/oracle_lib.py)."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import triangulator_ref_lib as tref

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "retri_ref" / "retri_ref.cc"
DEPS = [ROOT / "tests" / "triangulator_ref" / "triangulator_ref.cc", ROOT / "tests" / "tri_ref" / "tri_ref.cc"]
LIB = ROOT / "tests" / "retri_ref" / "_build" / "libretriref.so"
NO_POINT = tref.NO_POINT
NONE, CONTINUE_1TO2, CONTINUE_2TO1, CREATED = 0, 1, 2, 3
OPTION_FIELDS, OPTION_DEFAULTS, options_array, lift = tref.OPTION_FIELDS, tref.OPTION_DEFAULTS, tref.options_array, tref.lift
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
    V, Z, U32, U64, D = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_double
    sig = {
        "retriref_pairs": (C.c_int, [Z, V, V, Z, V, V, V, Z, V, Z, V, V, V, Z, V, D, D, D, D, V, V, V, V, V]),
        "retriref_colour": (None, [Z, V, V]),
        "retriref_scene_new": (V, []),
        "retriref_scene_free": (None, [V]),
        "retriref_retriangulate": (C.c_int64, [V, V]),
        "retriref_num_trials": (Z, [V]),
        "retriref_get_trials": (None, [V, V, V, V]),
        "retriref_scene_margins": (None, [V, V]),
        # section 17's scene (triangulator_ref.cc)
        "triref_add_camera": (None, [V, U32, C.c_int, U64, U64, V, C.c_int]),
        "triref_add_image": (None, [V, U32, U32, V, V, Z, V, V]),
        "triref_add_point": (None, [V, U64, V, Z, V, V]),
        "triref_graph_add_image": (None, [V, U32, Z]),
        "triref_graph_add_correspondences": (C.c_int, [V, U32, U32, V, Z]),
        "triref_graph_finalize": (None, [V]),
        "triref_num_points": (Z, [V]),
        "triref_get_points": (None, [V, V, V, V, V]),
        "triref_get_track": (None, [V, U64, V, V]),
        "triref_get_point2D_ids": (None, [V, U32, V]),
        "triref_num_modified": (Z, [V]),
        "triref_get_modified": (None, [V, V]),
    }
    for name, (res, args) in sig.items():
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    _lib = lib
    return lib


def colour(pairs):
    """the round of every (image 1, image 2) pair under 19.3's greedy colouring, pairs in the given order"""
    pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    out = np.zeros(max(len(pr), 1), np.uint32)
    load().retriref_colour(len(pr), _p(pr), _p(out))
    return out[:len(pr)]


def retriangulate_pairs(camera_models, camera_params, image_cameras, qvec, tvec, obs_image, obs_xy, obs_point, point_xyz,
                        pair_images, pair_offsets, corr_obs, round_offsets, corr_two_view=None, create_max_angle_error=2.0,
                        re_max_angle_error=5.0, min_angle=1.5, re_min_ratio=0.2):
    """The reference on a flat problem, in Context.retriangulate_pairs's result form (without timings and launches), plus
    margins: the smallest relative distance of a Continue angle, a created point's observation error and a tri_ratio from
    its threshold."""
    models = np.array(camera_models, dtype=np.int32).reshape(-1)
    icam = np.array(image_cameras, dtype=np.int64).reshape(-1)
    q, t = _f(qvec, (-1, 4)), _f(tvec, (-1, 3))
    oi = np.array(obs_image, dtype=np.uint32).reshape(-1)
    xy = _f(obs_xy, (-1, 2))
    op = np.array(obs_point, dtype=np.int32).reshape(-1)
    X = _f(point_xyz, (-1, 3))
    poff = np.array(pair_offsets, dtype=np.uint64).reshape(-1)
    co = np.ascontiguousarray(corr_obs, dtype=np.uint32).reshape(-1, 2)
    roff = np.array(round_offsets, dtype=np.uint64).reshape(-1)
    two = None if corr_two_view is None else np.ascontiguousarray(np.asarray(corr_two_view).reshape(-1) != 0, dtype=np.uint8)
    n, npairs, nc = oi.size, poff.size - 1, co.shape[0]
    if not (q.shape[0] == t.shape[0] == icam.size and xy.shape[0] == op.size == n and int(poff[-1]) == nc and
            np.asarray(pair_images).reshape(-1, 2).shape[0] == npairs):
        raise ValueError("retriangulate reference: array lengths disagree")
    nxy = np.zeros((n, 2))
    ocam = icam[oi] if n else np.zeros(0, np.int64)
    for c in np.unique(ocam):
        sel = ocam == c
        nxy[sel] = lift(models[c], camera_params[c], xy[sel])
    ran, ntri = np.zeros(max(npairs, 1), np.uint8), np.zeros(max(npairs, 1), np.uint32)
    act, cxyz, margins = np.zeros(max(nc, 1), np.uint8), np.zeros((max(nc, 1), 3)), np.zeros(3)
    rc = load().retriref_pairs(icam.size, _p(q), _p(t), n, _p(oi), _p(nxy), _p(op), X.shape[0], _p(X), npairs, _p(poff), _p(co),
                               _p(two), roff.size - 1, _p(roff), float(create_max_angle_error), float(re_max_angle_error),
                               float(min_angle), float(re_min_ratio), _p(ran), _p(ntri), _p(act), _p(cxyz), _p(margins))
    if rc != 0:
        raise ValueError("retriangulate reference: invalid input")
    act, ran, ntri = act[:nc], ran[:npairs].astype(bool), ntri[:npairs]
    made = act == CREATED
    per_pair = np.array([int(made[int(poff[p]):int(poff[p + 1])].sum()) for p in range(npairs)], np.uint64)
    return dict(pair_ran=ran, pair_num_tri=ntri, corr_action=act,
                created_offsets=np.concatenate([[0], np.cumsum(per_pair)]).astype(np.uint64), created_xyz=cxyz[:nc][made].copy(),
                num_pairs_run=int(ran.sum()), num_continued=int(((act == CONTINUE_1TO2) | (act == CONTINUE_2TO1)).sum()),
                num_created=int(made.sum()), margins=margins)


class Scene:
    """A model and a correspondence graph held by the reference, with retriangulate's trial counters: cameras {id: (model,
    width, height, params)}, images {id: (camera_id, qvec xyzw, tvec, xy (N, 2) pixels, point3D ids (N,) or NO_POINT)},
    points {id: (xyz, [(image, point2D)])}, graph_images {id: num_points2D} and matches [(id1, id2, (M, 2))]."""

    def __init__(self, cameras, images, points, graph_images, matches, finalize=True):
        lib = load()
        self._lib, self._s = lib, lib.retriref_scene_new()
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
                raise ValueError("retriangulate reference: correspondences of an unknown image")
        if finalize:
            lib.triref_graph_finalize(self._s)

    def __del__(self):
        try:
            self._lib.retriref_scene_free(self._s)
        except Exception:  # interpreter shutdown
            pass

    def retriangulate(self, **options):
        return int(self._lib.retriref_retriangulate(self._s, _p(options_array(**options))))

    def trials(self):
        """{(image 1, image 2): trials spent}, the pairs that spent any"""
        n = int(self._lib.retriref_num_trials(self._s))
        a, b, c = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.int32)
        self._lib.retriref_get_trials(self._s, _p(a), _p(b), _p(c))
        return {(int(a[i]), int(b[i])): int(c[i]) for i in range(n) if c[i]}

    def margins(self):
        out = np.zeros(3)
        self._lib.retriref_scene_margins(self._s, _p(out))
        return out

    points = tref.Scene.points
    point2D_ids = tref.Scene.point2D_ids
    modified = tref.Scene.modified
