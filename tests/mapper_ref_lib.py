"""ctypes wrapper of the mapper's CPU reference (tests/mapper_ref/mapper_ref.cc, written from DESIGN.md section 20 without
any product header; it includes tests/filter_ref/filter_ref.cc for section 16's projection centre and triangulation
angle), built on first use into tests/mapper_ref/_build/ with the flags of tests/ba_ref_lib.py."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "mapper_ref" / "mapper_ref.cc"
DEPS = [ROOT / "tests" / "filter_ref" / "filter_ref.cc", ROOT / "tests" / "ba_ref" / "ba_ref.cc"]
LIB = ROOT / "tests" / "mapper_ref" / "_build" / "libmapperref.so"
NO_POINT = (1 << 64) - 1
MAX_SCORE = 17895696
_lib = None
_p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
_f = lambda a, shape: np.ascontiguousarray(a, dtype=np.float64).reshape(shape)  # noqa: E731
_u32 = lambda a: np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.uint32)  # noqa: E731
_u64 = lambda a: np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.uint64)  # noqa: E731


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
    V, Z, D, U32, U64 = C.c_void_p, C.c_size_t, C.c_double, C.c_uint32, C.c_uint64
    sig = {
        "mapper_ref_cell": (Z, [D, D]),
        "mapper_ref_max_score": (C.c_uint64, []),
        "mapper_ref_percentile": (D, [V, Z, D]),
        "mapper_ref_visibility": (C.c_int, [Z, V, V, Z, V, V, V, V, V, V, V, V, V, V]),
        "mapper_ref_pair_angles": (C.c_int, [Z, V, V, Z, V, Z, V, V, V, D, V, V]),
        # the scene
        "mapper_ref_scene_new": (V, []),
        "mapper_ref_scene_free": (None, [V]),
        "mapper_ref_add_camera": (None, [V, U32, C.c_int, U64, U64, V, C.c_int, C.c_int]),
        "mapper_ref_add_image": (None, [V, U32, U32, V, V, Z, V, V]),
        "mapper_ref_add_candidate": (None, [V, U32, U32, Z, V]),
        "mapper_ref_add_point": (None, [V, U64, V, Z, V, V]),
        "mapper_ref_graph_add_image": (None, [V, U32, Z]),
        "mapper_ref_graph_add_correspondences": (C.c_int, [V, U32, U32, V, Z]),
        "mapper_ref_graph_finalize": (None, [V]),
        "mapper_ref_find_next_images": (C.c_int64, [V, V, V, Z]),
        "mapper_ref_candidate_statistics": (None, [V, U32, V]),
        "mapper_ref_register_next_image": (C.c_int, [V, V, U32]),
        "mapper_ref_last_registration": (None, [V, V]),
        "mapper_ref_find_local_bundle": (C.c_int64, [V, V, U32, V, V, V, V, Z, V]),
        "mapper_ref_num_trials": (C.c_int, [V, U32]),
        "mapper_ref_num_total_reg_images": (U64, [V]),
        "mapper_ref_num_candidates": (Z, [V]),
        "mapper_ref_get_candidates": (None, [V, V]),
        "mapper_ref_is_registered": (C.c_int, [V, U32]),
        "mapper_ref_get_image": (None, [V, U32, V, V]),
        "mapper_ref_camera_params": (Z, [V, U32, V]),
        "mapper_ref_track_length": (Z, [V, U64]),
        "mapper_ref_get_track": (None, [V, U64, V, V]),
        "mapper_ref_num_modified": (Z, [V]),
        "mapper_ref_get_modified": (None, [V, V]),
    }
    for name, (res, args) in sig.items():
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    _lib = lib
    return lib


def cell(x, extent):
    return int(load().mapper_ref_cell(float(x), float(extent)))


def percentile(values, p=75.0):
    v = _f(values, (-1,))
    return float(load().mapper_ref_percentile(_p(v), v.size, float(p)))


def image_visibility(image_point_offsets, point2D_point3D, cand_width, cand_height, cand_point_offsets, cand_xy, corr_offsets,
                     corr_image, corr_point2D):
    """The reference on the flat problem of Context.image_visibility, in its result form (without timings)."""
    ipoff, table, cw, ch = _u64(image_point_offsets), _u64(point2D_point3D), _u32(cand_width), _u32(cand_height)
    cpoff, xy, coff, ci, cp = _u64(cand_point_offsets), _f(cand_xy, (-1, 2)), _u64(corr_offsets), _u32(corr_image), _u32(corr_point2D)
    nc = cw.size
    if not (ipoff.size >= 1 and int(ipoff[-1]) == table.size and ch.size == nc and cpoff.size == nc + 1 and int(cpoff[-1]) == len(xy) and
            coff.size == len(xy) + 1 and int(coff[-1]) == ci.size == cp.size):
        raise ValueError("mapper reference: array lengths disagree")
    nobs, nvis, score = np.zeros(max(nc, 1), np.uint32), np.zeros(max(nc, 1), np.uint32), np.zeros(max(nc, 1), np.uint64)
    if load().mapper_ref_visibility(ipoff.size - 1, _p(ipoff), _p(table), nc, _p(cw), _p(ch), _p(cpoff), _p(xy), _p(coff), _p(ci),
                                    _p(cp), _p(nobs), _p(nvis), _p(score)) != 0:
        raise ValueError("mapper reference: invalid input")
    return dict(num_observations=nobs[:nc], num_visible_points3D=nvis[:nc], score=score[:nc], max_score=int(load().mapper_ref_max_score()))


def shared_point_angles(qvec, tvec, point_xyz, pair_images, pair_offsets, shared_points, percentile=75.0, all_angles=False):
    """The reference on the flat problem of Context.shared_point_angles: {angle (K,)}; all_angles=True adds every shared
    point's own angle as `angles` (S,)."""
    q, t, X = _f(qvec, (-1, 4)), _f(tvec, (-1, 3)), _f(point_xyz, (-1, 3))
    pi, poff, sp = _u32(pair_images).reshape(-1, 2), _u64(pair_offsets), _u32(shared_points)
    np_ = pi.shape[0]
    if not (q.shape[0] == t.shape[0] and poff.size == np_ + 1 and int(poff[-1]) == sp.size):
        raise ValueError("mapper reference: array lengths disagree")
    out = np.zeros(max(np_, 1))
    every = np.zeros(max(sp.size, 1)) if all_angles else None
    if load().mapper_ref_pair_angles(q.shape[0], _p(q), _p(t), X.shape[0], _p(X), np_, _p(pi), _p(poff), _p(sp), float(percentile),
                                     _p(out), _p(every)) != 0:
        raise ValueError("mapper reference: invalid input")
    res = dict(angle=out[:np_])
    if all_angles:
        res["angles"] = every[:sp.size]
    return res


# ---- the three methods on a scene -------------------------------------------------------------------------------------------
OPTION_FIELDS = ("init_min_num_inliers", "init_max_error", "init_max_forward_motion", "init_min_tri_angle", "init_max_reg_trials",
                 "abs_pose_max_error", "abs_pose_min_num_inliers", "abs_pose_min_inlier_ratio", "abs_pose_refine_focal_length",
                 "abs_pose_refine_extra_params", "local_ba_num_images", "local_ba_min_tri_angle", "min_focal_length_ratio",
                 "max_focal_length_ratio", "max_extra_param", "filter_max_reproj_error", "filter_min_tri_angle", "max_reg_trials",
                 "fix_existing_images", "num_threads", "image_selection_method")
OPTION_DEFAULTS = (100, 4.0, 0.95, 16.0, 2, 12.0, 30, 0.25, True, True, 6, 6.0, 0.1, 10.0, 1.0, 4.0, 1.5, 3, False, -1, "MIN_UNCERTAINTY")
METHODS = ("MAX_VISIBLE_POINTS_NUM", "MAX_VISIBLE_POINTS_RATIO", "MIN_UNCERTAINTY")
LAST_FIELDS = ("success", "num_visible_points3D", "num_pairs", "num_inliers", "focal_factor", "estimate_focal_length",
               "would_refine_focal_length", "would_refine_extra_params")


def options_array(**options):
    unknown = set(options) - set(OPTION_FIELDS)
    if unknown:
        raise ValueError(f"mapper reference: unknown options {sorted(unknown)}")
    v = dict(zip(OPTION_FIELDS, OPTION_DEFAULTS))
    v.update(options)
    v["image_selection_method"] = METHODS.index(str(v["image_selection_method"]).split(".")[-1])
    return np.array([float(v[f]) for f in OPTION_FIELDS], np.float64)


class Scene:
    """A model, candidates and a correspondence graph held by the reference: cameras {id: (model, width, height, params[,
    has_prior_focal_length])}, images {id: (camera_id, qvec xyzw, tvec, xy (N, 2) pixels, point3D ids (N,) or NO_POINT)},
    points {id: (xyz, [(image, point2D)])}, candidates {id: (camera_id, xy (N, 2))}, graph_images {id: num_points2D} and
    matches [(id1, id2, (M, 2))]."""

    def __init__(self, cameras, images, points, candidates, graph_images, matches, finalize=True):
        lib = load()
        self._lib, self._s = lib, lib.mapper_ref_scene_new()
        self.sizes = {}
        for cid, cam in cameras.items():
            p = _f(cam[3], (-1,))
            lib.mapper_ref_add_camera(self._s, cid, int(cam[0]), int(cam[1]), int(cam[2]), _p(p), p.size, int(bool(cam[4])) if len(cam) > 4 else 0)
        for iid, (cid, q, t, xy, pids) in images.items():
            xy = _f(xy, (-1, 2))
            self.sizes[iid] = len(xy)
            lib.mapper_ref_add_image(self._s, iid, cid, _p(_f(q, (4,))), _p(_f(t, (3,))), len(xy), _p(xy), _p(_u64(pids)))
        for pid, (xyz, track) in points.items():
            ti, tk = _u32([e[0] for e in track]), _u32([e[1] for e in track])
            lib.mapper_ref_add_point(self._s, pid, _p(_f(xyz, (3,))), len(track), _p(ti), _p(tk))
        for iid, (cid, xy) in candidates.items():
            xy = _f(xy, (-1, 2))
            self.sizes[iid] = len(xy)
            lib.mapper_ref_add_candidate(self._s, iid, cid, len(xy), _p(xy))
        for iid, n in graph_images.items():
            lib.mapper_ref_graph_add_image(self._s, iid, n)
        for id1, id2, m in matches:
            m = np.ascontiguousarray(m, dtype=np.uint32).reshape(-1, 2)
            if lib.mapper_ref_graph_add_correspondences(self._s, id1, id2, _p(m), len(m)) != 0:
                raise ValueError("mapper reference: correspondences of an unknown image")
        if finalize:
            lib.mapper_ref_graph_finalize(self._s)
        self.point_ids = sorted(points)

    def __del__(self):
        try:
            self._lib.mapper_ref_scene_free(self._s)
        except Exception:  # interpreter shutdown
            pass

    def find_next_images(self, **options):
        out = np.zeros(max(len(self.sizes), 1), np.uint32)
        n = int(self._lib.mapper_ref_find_next_images(self._s, _p(options_array(**options)), _p(out), out.size))
        return [int(v) for v in out[:n]]

    def candidate_statistics(self, image_id):
        """(num_observations, num_visible_points3D, score)"""
        out = np.zeros(3, np.uint64)
        self._lib.mapper_ref_candidate_statistics(self._s, image_id, _p(out))
        return tuple(int(v) for v in out)

    def register_next_image(self, image_id, **options):
        rc = int(self._lib.mapper_ref_register_next_image(self._s, _p(options_array(**options)), image_id))
        if rc < 0:
            raise ValueError("mapper reference: not a candidate")
        return bool(rc)

    def last_registration(self):
        out = np.zeros(8)
        self._lib.mapper_ref_last_registration(self._s, _p(out))
        d = dict(zip(LAST_FIELDS, out.tolist()))
        return {k: (v if k == "focal_factor" else (bool(v) if k in ("success", "estimate_focal_length", "would_refine_focal_length", "would_refine_extra_params") else int(v)))
                for k, v in d.items()}

    def find_local_bundle(self, image_id, overlap=False, **options):
        """the bundle; overlap=True: (bundle, [(image, shared observations, angle or -1)])"""
        cap = max(len(self.sizes), 1)
        out, ov_i, ov_n, ov_a, n_ov = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint64), np.zeros(cap), np.zeros(1, np.uint64)
        n = int(self._lib.mapper_ref_find_local_bundle(self._s, _p(options_array(**options)), image_id, _p(out), _p(ov_i), _p(ov_n), _p(ov_a), cap, _p(n_ov)))
        if n < 0:
            raise ValueError("mapper reference: the model has no such image")
        bundle = [int(v) for v in out[:n]]
        k = int(n_ov[0])
        return (bundle, [(int(ov_i[i]), int(ov_n[i]), float(ov_a[i])) for i in range(k)]) if overlap else bundle

    def num_reg_trials(self, image_id):
        return int(self._lib.mapper_ref_num_trials(self._s, image_id))

    def num_total_reg_images(self):
        return int(self._lib.mapper_ref_num_total_reg_images(self._s))

    def candidates(self):
        n = int(self._lib.mapper_ref_num_candidates(self._s))
        out = np.zeros(max(n, 1), np.uint32)
        self._lib.mapper_ref_get_candidates(self._s, _p(out))
        return [int(v) for v in out[:n]]

    def is_registered(self, image_id):
        return bool(self._lib.mapper_ref_is_registered(self._s, image_id))

    def image(self, image_id):
        """(qvec xyzw, tvec, point3D ids) of a model image"""
        pose, ids = np.zeros(7), np.zeros(max(self.sizes[image_id], 1), np.uint64)
        self._lib.mapper_ref_get_image(self._s, image_id, _p(pose), _p(ids))
        return pose[:4].copy(), pose[4:].copy(), ids[:self.sizes[image_id]]

    def camera_params(self, camera_id):
        out = np.zeros(12)
        n = int(self._lib.mapper_ref_camera_params(self._s, camera_id, _p(out)))
        return out[:n]

    def tracks(self):
        out = {}
        for pid in self.point_ids:
            n = int(self._lib.mapper_ref_track_length(self._s, pid))
            a, b = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
            self._lib.mapper_ref_get_track(self._s, pid, _p(a), _p(b))
            out[pid] = [(int(a[i]), int(b[i])) for i in range(n)]
        return out

    def modified(self):
        n = int(self._lib.mapper_ref_num_modified(self._s))
        out = np.zeros(max(n, 1), np.uint64)
        self._lib.mapper_ref_get_modified(self._s, _p(out))
        return {int(v) for v in out[:n]}
