"""Shared cases of the initial pair: flat problems of Context.triangulate_pairs on the smallest shapes
at which the kernel can go wrong, the reference's results on them (computed once per case), an independent numpy
restatement, the solvers that stand in for the library in the `_with` hooks, and the walk from an empty model through
register_initial_image_pair, adjust_global_bundle, the filters and the mapper's loop."""
import functools
import hashlib

import numpy as np

import ba_cases
import initpair_ref_lib as ref
import triangulator_cases as tc

PI = 3.14159265358979311600e+00
DEFAULT_ANGLE = ref.DEFAULT_MIN_TRI_ANGLE
CORR_SIZES = (0, 1, 63, 64, 65, 257)
PAIR_COUNTS = (0, 1, 64, 65)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- flat problems ---------------------------------------------------------------------------------------------------------------
def problem(seed=0, sizes=(8,), models=(2,), nimg=6, noise=0.5, min_tri_angle=DEFAULT_ANGLE, radius=6.0):
    """pairs of the given numbers of correspondences between random distinct images of a ring: a point in the unit cube,
    its two projections plus noise"""
    rng = np.random.default_rng(seed)
    prm = [ba_cases.model_params(m) for m in models]
    poses = tc.ring(nimg, radius=radius, seed=seed)
    icam = np.arange(nimg, dtype=np.uint32) % len(models)
    q, t = np.array([p[0] for p in poses]), np.array([p[1] for p in poses])
    pi, xy1, xy2 = [], [], []
    for n in sizes:
        a, b = (int(v) for v in rng.choice(nimg, 2, replace=False))
        pi.append((a, b))
        X = rng.uniform(-1, 1, (n, 3))
        if n:
            xy1.append(tc.project(models[icam[a]], prm[icam[a]], q[a], t[a], X) + rng.normal(0, noise, (n, 2)))
            xy2.append(tc.project(models[icam[b]], prm[icam[b]], q[b], t[b], X) + rng.normal(0, noise, (n, 2)))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    cat = lambda v: np.concatenate(v) if v else np.zeros((0, 2))  # noqa: E731
    return (list(models), prm, icam, q, t, np.array(pi, np.uint32).reshape(-1, 2), off, cat(xy1), cat(xy2)), dict(min_tri_angle=min_tri_angle)


# SIMPLE_PINHOLE with f = 1 and the principal point at 0: a pixel is its normalised point
UNIT_CAMERA = ([0], [np.array([1.0, 0.0, 0.0])])
IDENTITY, TURNED = [0.0, 0.0, 0.0, 1.0], [0.0, 1.0, 0.0, 0.0]  # TURNED: half a turn about y, R = diag(-1, 1, -1)


def hand_problem(poses, corrs, min_tri_angle=DEFAULT_ANGLE):
    """one pair of unit cameras at the given (q x y z w, t) poses with the given ((x1, y1), (x2, y2)) correspondences"""
    q, t = np.array([p[0] for p in poses], np.float64), np.array([p[1] for p in poses], np.float64)
    xy1 = np.array([c[0] for c in corrs], np.float64).reshape(-1, 2)
    xy2 = np.array([c[1] for c in corrs], np.float64).reshape(-1, 2)
    return (UNIT_CAMERA[0], UNIT_CAMERA[1], np.zeros(2, np.uint32), q, t, np.array([[0, 1]], np.uint32), np.array([0, len(xy1)], np.uint64), xy1, xy2), \
        dict(min_tri_angle=min_tri_angle)


def _pixel(q, t, X):
    """the unit camera's pixel of X under the pose; exact for the dyadic coordinates used here"""
    Xc = ref.rotation_matrix(q) @ np.asarray(X, np.float64) + np.asarray(t, np.float64)
    return (Xc[0] / Xc[2], Xc[1] / Xc[2])


def _symmetric():
    """centres (-1, 0, 0) and (1, 0, 0), the point (0, 0, 1): the rays meet at a right angle"""
    return hand_problem([(IDENTITY, [1.0, 0.0, 0.0]), (IDENTITY, [-1.0, 0.0, 0.0])], [((1.0, 0.0), (-1.0, 0.0))])


def _depths():
    """the point (0, 0, 2) seen from centres (-1, 0, 0) and (1, 0, 0): in front of both; behind camera 1 only (camera 1
    turned away); behind camera 2 only; behind both.  One problem per row would need four calls: here four pairs share
    four images."""
    X = [0.0, 0.0, 2.0]
    front1, front2 = (IDENTITY, [1.0, 0.0, 0.0]), (IDENTITY, [-1.0, 0.0, 0.0])
    back1, back2 = (TURNED, [-1.0, 0.0, 0.0]), (TURNED, [1.0, 0.0, 0.0])  # t = -R C with R = diag(-1, 1, -1)
    poses = [front1, front2, back1, back2]
    q, t = np.array([p[0] for p in poses]), np.array([p[1] for p in poses])
    pairs = np.array([[0, 1], [2, 1], [0, 3], [2, 3]], np.uint32)
    xy1 = np.array([_pixel(*poses[a], X) for a, _ in pairs])
    xy2 = np.array([_pixel(*poses[b], X) for _, b in pairs])
    return (UNIT_CAMERA[0], UNIT_CAMERA[1], np.zeros(4, np.uint32), q, t, pairs, np.arange(5, dtype=np.uint64), xy1, xy2), dict(min_tri_angle=DEFAULT_ANGLE)


def _parallel():
    return hand_problem([(IDENTITY, [1.0, 0.0, 0.0]), (IDENTITY, [-1.0, 0.0, 0.0])], [((0.0, 0.0), (0.0, 0.0)), ((0.25, 0.5), (0.25, 0.5))])


def _coincident():
    return hand_problem([(IDENTITY, [0.5, 0.0, 0.0]), (IDENTITY, [0.5, 0.0, 0.0])], [((0.0, 0.0), (0.0, 0.0)), ((0.25, 0.0), (-0.25, 0.0)), ((0.5, 0.25), (0.5, 0.25))])


def _nonfinite():
    a, kw = problem(seed=11, sizes=(6, 6, 6, 6), models=(2, 4), nimg=8)
    a = [np.array(v, copy=True) if isinstance(v, np.ndarray) else v for v in a]
    q, t, pi, xy1, xy2 = a[3], a[4], a[5], a[7], a[8]
    xy1[0, 0], xy2[1, 1], xy1[2] = np.nan, np.inf, (-np.inf, np.nan)
    q[pi[1, 0], 0] = np.nan       # pair 1: a NaN rotation
    t[pi[2, 1], 2] = np.inf       # pair 2: an infinite translation
    q[pi[3, 0]] = 0.0             # pair 3: the zero quaternion
    return tuple(a), kw


CASES = {f"corrs_{n}": functools.partial(problem, seed=40 + n, sizes=(n,)) for n in CORR_SIZES}
CASES.update({f"pairs_{k}": functools.partial(problem, seed=50 + k, sizes=tuple(1 + (i % 3) for i in range(k)), nimg=9) for k in PAIR_COUNTS})
CASES.update({f"model_{ba_cases.MODEL_NAMES[m]}": functools.partial(problem, seed=20 + m, sizes=(9, 5), models=(m,)) for m in range(11)})
CASES["mixed_models"] = functools.partial(problem, seed=31, sizes=(7, 9, 4), models=(4, 7, 0, 5), nimg=8)
CASES["angle_zero"] = functools.partial(problem, seed=32, sizes=(20,), min_tri_angle=0.0)
CASES["angle_pi"] = functools.partial(problem, seed=32, sizes=(20,), min_tri_angle=PI)
CASES["symmetric"] = _symmetric
CASES["depths"] = _depths
CASES["parallel"] = _parallel
CASES["coincident"] = _coincident
CASES["nonfinite"] = _nonfinite
CASES["random"] = functools.partial(problem, seed=33, sizes=(70, 1, 0, 130, 64, 3), models=(2, 1, 4), nimg=10)
# what the numpy restatement is compared on: well-conditioned pairs only (21.6)
RESTATEMENT_CASES = ("random", "corrs_257", "mixed_models", "model_OPENCV")


@functools.lru_cache(maxsize=None)
def call(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    a, kw = call(name)
    return ref.triangulate_pairs(*a, depths=True, **kw)


def same(got, want):
    return (np.array_equal(got["accepted"], want["accepted"]) and np.array_equal(bits(got["xyz"]), bits(want["xyz"])) and
            np.array_equal(bits(got["tri_angle"]), bits(want["tri_angle"])) and got["num_accepted"] == want["num_accepted"])


def digest(r):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(r["accepted"], dtype=np.uint8).tobytes())
    h.update(bits(r["xyz"]).tobytes())
    h.update(bits(r["tri_angle"]).tobytes())
    return h.hexdigest()


def permuted(args, seed):
    """the pairs in another order, and within every pair its correspondences in another order; `order` maps a new
    correspondence to the old one"""
    rng = np.random.default_rng(seed)
    models, prm, icam, q, t, pi, off, xy1, xy2 = args
    off = np.asarray(off, np.int64)
    pairs = rng.permutation(len(pi))
    order = np.concatenate([off[p] + rng.permutation(int(off[p + 1] - off[p])) for p in pairs]).astype(np.int64) if len(pi) else np.zeros(0, np.int64)
    new_off = np.concatenate([[0], np.cumsum([off[p + 1] - off[p] for p in pairs])]).astype(np.uint64)
    return (models, prm, icam, q, t, pi[pairs], new_off, xy1[order], xy2[order]), order


def num_batches(num_corrs, bound):
    return -(-num_corrs // bound)


# ---- 21.2 restated independently in numpy (SVD for the DLT) ------------------------------------------------------------------
def np_triangulate_pairs(camera_models, camera_params, image_cameras, qvec, tvec, pair_images, pair_offsets, corr_xy1, corr_xy2, min_tri_angle=DEFAULT_ANGLE):
    """accepted, xyz, tri_angle and depths with numpy's SVD, arccos and matrix products; only the lift of the pixels is the
    reference's (it is not what 21.2 is about)"""
    n1, n2 = ref.lift_pairs(camera_models, camera_params, image_cameras, pair_images, pair_offsets, corr_xy1, corr_xy2)
    q, t = np.asarray(qvec, np.float64).reshape(-1, 4), np.asarray(tvec, np.float64).reshape(-1, 3)
    P, C = [], []
    for i in range(len(q)):
        x, y, z, w = q[i]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        P.append(np.c_[R, t[i]])
        C.append(-R.T @ t[i])
    n = len(n1)
    xyz, ang, dep = np.zeros((n, 3)), np.zeros(n), np.zeros((n, 2))
    off = np.asarray(pair_offsets, np.int64)
    for p, (a, b) in enumerate(np.asarray(pair_images, np.int64).reshape(-1, 2)):
        for k in range(off[p], off[p + 1]):
            A = np.stack([n1[k, 0] * P[a][2] - P[a][0], n1[k, 1] * P[a][2] - P[a][1], n2[k, 0] * P[b][2] - P[b][0], n2[k, 1] * P[b][2] - P[b][1]])
            v = np.linalg.svd(A)[2][3]
            X = v[:3] / v[3]
            r1, r2, base = X - C[a], X - C[b], C[a] - C[b]
            den = 2 * np.sqrt((r1 @ r1) * (r2 @ r2))
            angle = 0.0 if den == 0 else abs(np.arccos((r1 @ r1 + r2 @ r2 - base @ base) / den))
            xyz[k], ang[k] = X, min(angle, np.pi - angle)
            dep[k] = (P[a][2, :3] @ X + P[a][2, 3], P[b][2, :3] @ X + P[b][2, 3])
    eps = np.finfo(np.float64).eps
    return dict(accepted=(ang >= min_tri_angle) & (dep[:, 0] >= eps) & (dep[:, 1] >= eps), xyz=xyz, tri_angle=ang, depths=dep)


def measure_deviation():
    """the largest |xyz| and |angle| difference between the reference and the restatement over RESTATEMENT_CASES"""
    worst = dict(xyz=0.0, tri_angle=0.0)
    for name in RESTATEMENT_CASES:
        a, kw = call(name)
        got, want = np_triangulate_pairs(*a, **kw), reference(name)
        for f in worst:
            if len(want[f]):
                worst[f] = max(worst[f], float(np.max(np.abs(got[f] - want[f]))))
    return worst


# ---- the references in the library's place (pycolmap_amd._register_initial_image_pair_with) -----------------------------------
def pair_solver(d):
    r = ref.triangulate_pairs(d["camera_models"].reshape(-1), d["camera_params"], d["image_cameras"].reshape(-1), d["qvec"], d["tvec"],
                              d["pair_images"], d["pair_offsets"].reshape(-1), d["corr_xy1"], d["corr_xy2"], min_tri_angle=d["min_tri_angle"])
    return dict(accepted=r["accepted"].astype(np.uint8), xyz=r["xyz"], tri_angle=r["tri_angle"])


def oracle_two_view_solver(camera1, points1, camera2, points2, matches, options):
    """EstimateCalibratedTwoViewGeometry and EstimateTwoViewGeometryPose of the CPU oracle (tests/oracle_lib.py)"""
    import oracle_lib as o
    cams = [o.make_camera(int(c.model), c.width, c.height, tuple(c.params), prior=True) for c in (camera1, camera2)]
    r = options.ransac
    opts = o.tvg_default_options(
        min_num_inliers=options.min_num_inliers, min_E_F_inlier_ratio=options.min_E_F_inlier_ratio, max_H_inlier_ratio=options.max_H_inlier_ratio,
        watermark_min_inlier_ratio=options.watermark_min_inlier_ratio, watermark_border_size=options.watermark_border_size,
        detect_watermark=int(options.detect_watermark), multiple_ignore_watermark=int(options.multiple_ignore_watermark), force_H_use=0,
        compute_relative_pose=0, multiple_models=0, max_error=r.max_error, min_inlier_ratio=r.min_inlier_ratio, confidence=r.confidence,
        dyn_num_trials_multiplier=r.dyn_num_trials_multiplier, min_num_trials=int(r.min_num_trials), max_num_trials=int(min(r.max_num_trials, 1 << 30)))
    m = np.asarray(matches, np.uint32).reshape(-1, 2)
    w = o.estimate_two_view_geometry(cams[0], points1, cams[1], points2, m, opts, seed=0)
    inl = m[w["inlier_mask"]]
    wp = o.estimate_two_view_geometry_pose(cams[0], points1, cams[1], points2, inl, w["config"], E=w["E"], H=w["H"])
    ok = bool(wp["pose_ok"])
    return dict(pose_ok=ok, config=int(wp["config"]) if ok else int(w["config"]), inlier_matches=inl,
                qvec=wp["qvec"][[1, 2, 3, 0]] if ok else np.array([0.0, 0.0, 0.0, 1.0]), tvec=wp["tvec"] if ok else np.zeros(3),
                tri_angle=float(wp["tri_angle"]) if ok else 0.0)


def forced_two_view_solver(pose_ok=True, num_inliers=50, tz=0.0, tri_angle=0.5, qvec=(0.0, 0.0, 0.0, 1.0), tx=-1.0):
    """a two-view solver that answers as told: the first num_inliers matches as inliers"""
    def solve(camera1, points1, camera2, points2, matches, options):
        m = np.asarray(matches, np.uint32).reshape(-1, 2)
        return dict(pose_ok=pose_ok, config=2, inlier_matches=m[:num_inliers], qvec=np.array(qvec), tvec=np.array([tx, 0.0, tz]), tri_angle=tri_angle)
    return solve


# ---- from an empty model ---------------------------------------------------------------------------------------------------------
# the scenes plant 25 to 40 points and their image pairs share fewer: the thresholds come down (21.6)
START_OPTIONS = dict(init_min_num_inliers=8, init_min_tri_angle=4.0, abs_pose_min_num_inliers=5, local_ba_num_images=4)


def empty_state(name):
    """a scene of triangulator_cases.SCENES with every image a candidate and only the cameras in the model"""
    sc, _ = tc.scene_case(name)
    cameras = {c: (cam[0], cam[1], cam[2], cam[3], True) for c, cam in sc["cameras"].items()}
    return dict(cameras=cameras, images={}, points={}, candidates={i: (im[0], im[3]) for i, im in sc["images"].items()},
                graph_images=sc["graph_images"], matches=sc["matches"])


def best_pair(graph, image_ids):
    """the pair with the most correspondences, the lowest ids among equals: COLMAP's search, in a few lines over public calls"""
    ids = sorted(image_ids)
    return max(((a, b) for a in ids for b in ids if a < b), key=lambda ab: (graph.num_correspondences_between_images(*ab), -ab[0], -ab[1]))
