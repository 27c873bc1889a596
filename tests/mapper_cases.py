"""The flat cases of the mapper's two device calls, shared by the CPU tests, the GPU tests and the
fixture generator: the smallest shapes at which csrc/mapper.hip can go wrong.  vis_call(name) returns the arguments of
Context.image_visibility, angle_call(name) those of Context.shared_point_angles with its keywords."""
from __future__ import annotations

import functools
import hashlib

import numpy as np

import mapper_ref_lib as ref

NO_POINT = ref.NO_POINT
NAN, INF = float("nan"), float("inf")


# ---- image_visibility ------------------------------------------------------------------------------------------------------
def _vis_problem(graph_sizes, table, cands):
    """graph_sizes: points2D per graph image; table: their point3D ids, concatenated; cands: [(width, height, xy (N, 2),
    [per point2D: [(graph image, point2D), ...]])]"""
    ipoff = np.concatenate([[0], np.cumsum(graph_sizes)]).astype(np.uint64)
    cw = np.array([c[0] for c in cands], np.uint32)
    ch = np.array([c[1] for c in cands], np.uint32)
    cpoff = np.concatenate([[0], np.cumsum([len(c[2]) for c in cands])]).astype(np.uint64)
    xy = np.concatenate([np.asarray(c[2], np.float64).reshape(-1, 2) for c in cands]) if cands else np.zeros((0, 2))
    lists = [l for c in cands for l in c[3]]
    coff = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    flat = [e for l in lists for e in l]
    ci = np.array([e[0] for e in flat], np.uint32)
    cp = np.array([e[1] for e in flat], np.uint32)
    return ipoff, np.asarray(table, np.uint64), cw, ch, cpoff, xy, coff, ci, cp


def _graph(rng, sizes, share=0.5):
    table = np.full(int(np.sum(sizes)), NO_POINT, np.uint64)
    have = rng.random(table.size) < share
    table[have] = rng.integers(1, 1000, int(have.sum()))
    return list(sizes), table


def _random_cand(rng, sizes, n, width=640, height=480, max_corrs=3, spread=1.0):
    xy = np.column_stack([rng.uniform(0, width * spread, n), rng.uniform(0, height * spread, n)])
    lists = []
    for _ in range(n):
        m = int(rng.integers(0, max_corrs + 1))
        imgs = rng.choice(len(sizes), size=min(m, len(sizes)), replace=False)
        lists.append([(int(g), int(rng.integers(0, sizes[g]))) for g in imgs])
    return width, height, xy, lists


def _vis_sizes():
    rng = np.random.default_rng(2001)
    sizes, table = _graph(rng, [40, 70, 5, 130])
    return _vis_problem(sizes, table, [_random_cand(rng, sizes, n) for n in (0, 1, 63, 64, 65, 257)])


def _vis_cands(k):
    def build():
        rng = np.random.default_rng(2100 + k)
        sizes, table = _graph(rng, [30, 50, 20])
        return _vis_problem(sizes, table, [_random_cand(rng, sizes, int(rng.integers(0, 40)), width=int(rng.integers(1, 900)),
                                                        height=int(rng.integers(1, 900))) for _ in range(k)])
    return build


def _vis_corr_counts():
    """points2D with 0, 1 and 65 correspondences; of the long lists one carries a point only at its end, one nowhere"""
    sizes = [2] * 65
    table = np.full(130, NO_POINT, np.uint64)
    table[2 * 64] = 7   # image 64, point2D 0
    table[2 * 3 + 1] = 9  # image 3, point2D 1
    long_last = [(g, 0) for g in range(65)]   # only the last carries a point
    long_none = [(g, 1) for g in range(65) if g != 3] + [(0, 0)]  # 65 correspondences, none carries one
    xy = [[10, 10], [100, 100], [200, 200], [300, 300], [400, 400]]
    lists = [[], [(3, 1)], long_last, long_none, [(5, 0)]]
    return _vis_problem(sizes, table, [(640, 480, xy, lists)])


def _vis_edges():
    """pixels at 0, at width and at height exactly, beyond them, negative, NaN and inf; extents of 1, of 0 and odd ones"""
    sizes, table = [1], np.array([5], np.uint64)
    vals = [0.0, -0.0, 5e-324, 9.999, 10.0, 639.999, 640.0, 640.001, 480.0, 479.99, 1e300, -1e-300, -3.0, -INF, INF, NAN, 320.0, 7.5]
    xy = [[a, b] for a in vals for b in (0.0, 480.0, NAN, -1.0, 1e9, 240.0)] + [[b, a] for a in vals for b in (0.0, 640.0, NAN, 100.0)]
    cands = []
    for w, h in ((640, 480), (1, 1), (0, 480), (640, 0), (63, 65), (4294967295, 3)):
        cands.append((w, h, xy, [[(0, 0)]] * len(xy)))
    return _vis_problem(sizes, table, cands)


def _vis_one_cell():
    rng = np.random.default_rng(2300)
    sizes, table = [3], np.array([1, NO_POINT, 2], np.uint64)
    n = 200
    xy = np.column_stack([rng.uniform(100, 109.9, n), rng.uniform(75, 82.4, n)])  # cell (10, 10) of 640 x 480
    lists = [[(0, int(i % 3))] for i in range(n)]
    return _vis_problem(sizes, table, [(640, 480, xy, lists)])


def _vis_every_cell():
    """every finest cell hit once, at its centre: the maximum score; and the same with the cells' first corners"""
    sizes, table = [1], np.array([1], np.uint64)
    cx, cy = np.meshgrid(np.arange(64), np.arange(64))
    centre = np.column_stack([(cx.ravel() + 0.5) * 10, (cy.ravel() + 0.5) * 7.5])
    corner = np.column_stack([cx.ravel() * 10.0, cy.ravel() * 7.5])
    lists = [[(0, 0)]] * 4096
    return _vis_problem(sizes, table, [(640, 480, centre, lists), (640, 480, corner, lists)])


def _vis_random():
    rng = np.random.default_rng(2400)
    sizes, table = _graph(rng, rng.integers(1, 300, 12), share=0.4)
    cands = [_random_cand(rng, sizes, int(rng.integers(0, 600)), width=int(rng.integers(100, 2000)), height=int(rng.integers(100, 2000)),
                          max_corrs=6, spread=rng.choice([0.2, 1.0, 1.2])) for _ in range(20)]
    return _vis_problem(sizes, table, cands)


def _vis_empty_graph():
    return _vis_problem([], np.zeros(0, np.uint64), [(640, 480, [[1.0, 2.0], [3.0, 4.0]], [[], []]), (10, 10, np.zeros((0, 2)), [])])


VIS_CASES = {"sizes": _vis_sizes, "cands_0": _vis_cands(0), "cands_1": _vis_cands(1), "cands_64": _vis_cands(64), "cands_65": _vis_cands(65),
             "corr_counts": _vis_corr_counts, "edges": _vis_edges, "one_cell": _vis_one_cell, "every_cell": _vis_every_cell,
             "random": _vis_random, "empty_graph": _vis_empty_graph}


@functools.lru_cache(maxsize=None)
def vis_call(name):
    return VIS_CASES[name]()


@functools.lru_cache(maxsize=None)
def vis_reference(name):
    return ref.image_visibility(*vis_call(name))


def vis_same(a, b):
    return all(np.array_equal(np.asarray(a[f]), np.asarray(b[f])) for f in ("num_observations", "num_visible_points3D", "score")) and \
        int(a["max_score"]) == int(b["max_score"])


def vis_digest(r):
    h = hashlib.sha256()
    for f, dt in (("num_observations", np.uint32), ("num_visible_points3D", np.uint32), ("score", np.uint64)):
        h.update(np.ascontiguousarray(r[f], dtype=dt).tobytes())
    h.update(str(int(r["max_score"])).encode())
    return h.hexdigest()


def vis_permuted(args, seed):
    """the candidates in another order: (arguments, order)"""
    ipoff, table, cw, ch, cpoff, xy, coff, ci, cp = args
    order = np.random.default_rng(seed).permutation(len(cw))
    cands = []
    for c in order:
        p0, p1 = int(cpoff[c]), int(cpoff[c + 1])
        lists = [[(int(ci[k]), int(cp[k])) for k in range(int(coff[j]), int(coff[j + 1]))] for j in range(p0, p1)]
        cands.append((int(cw[c]), int(ch[c]), xy[p0:p1], lists))
    return _vis_problem(np.diff(ipoff.astype(np.int64)), table, cands), order


# ---- shared_point_angles ---------------------------------------------------------------------------------------------------
def _poses(rng, n, radius=4.0):
    """cameras on a circle around the origin, looking roughly inwards; qvec x y z w (not normalised exactly), tvec"""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q *= rng.uniform(0.9, 1.1, (n, 1))  # 16.2 divides by the squared norm
    t = rng.normal(size=(n, 3)) * radius
    return q, t


def _ang_problem(q, t, X, pairs):
    """pairs: [(image 1, image 2, [point indices])]"""
    pi = np.array([[a, b] for a, b, _ in pairs], np.uint32).reshape(-1, 2)
    poff = np.concatenate([[0], np.cumsum([len(p) for _, _, p in pairs])]).astype(np.uint64)
    sp = np.concatenate([np.asarray(p, np.uint32) for _, _, p in pairs]) if pairs else np.zeros(0, np.uint32)
    return np.asarray(q, np.float64), np.asarray(t, np.float64), np.asarray(X, np.float64).reshape(-1, 3), pi, poff, sp


PAIR_SIZES = (1, 2, 3, 5, 63, 64, 65, 257)


def _ang_sizes():
    rng = np.random.default_rng(3001)
    q, t = _poses(rng, 6)
    X = rng.normal(size=(400, 3))
    pairs = [(int(rng.integers(0, 6)), int(rng.integers(0, 6)), rng.integers(0, 400, n)) for n in PAIR_SIZES]
    return _ang_problem(q, t, X, pairs), {}


def _ang_bound():
    rng = np.random.default_rng(3002)
    q, t = _poses(rng, 2)
    n = 1 << 20
    X = rng.normal(size=(n, 3))
    return _ang_problem(q, t, X, [(0, 1, np.arange(n)), (1, 0, np.arange(7))]), {}


def _ang_all_equal():
    rng = np.random.default_rng(3003)
    q, t = _poses(rng, 3)
    X = rng.normal(size=(4, 3))
    return _ang_problem(q, t, X, [(0, 1, [2] * 70), (1, 2, [3] * 5), (0, 2, [1])]), {}


def _ang_nonfinite():
    """NaN and inf in a point and in a pose: a pair's angles are then partly or wholly NaN, and NaN sorts last"""
    rng = np.random.default_rng(3004)
    q, t = _poses(rng, 6)
    q[3, 1] = NAN
    t[4, 0] = INF
    q[5] = 0.0  # the zero quaternion: Eigen's inverse is zero, the centre the origin
    X = rng.normal(size=(80, 3))
    X[0, 0] = NAN
    X[1, 2] = INF
    X[2] = [-INF, INF, NAN]
    pairs = [(0, 1, [0, 5, 6, 7]), (0, 1, [0, 1, 2, 8]), (0, 1, [0]), (0, 1, list(range(3, 70)) + [0] * 30), (0, 1, [0] * 3 + list(range(3, 12))),
             (3, 1, [5, 6, 7]), (0, 4, [5, 6, 7, 8]), (5, 1, [5, 6, 7, 8, 9]), (3, 4, [0, 1, 2])]
    return _ang_problem(q, t, X, pairs), {}


def _ang_coincident():
    """both centres on the point (a zero denominator: angle 0), one centre on it, and the same image twice (no baseline)"""
    q = np.array([[0, 0, 0, 1.0], [0, 0, 0, 1.0], [0, 0, 0, 2.0]])
    t = np.array([[-1.0, -2.0, -3.0], [-1.0, -2.0, -3.0], [0.5, 0.25, -4.0]])
    X = np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 1.0], [5.0, -1.0, 2.0], [-0.5, -0.25, 4.0]])
    pairs = [(0, 1, [0]), (0, 1, [0, 1, 2]), (0, 2, [0, 1, 2, 3]), (2, 2, [1, 2]), (0, 0, [0, 0, 1])]
    return _ang_problem(q, t, X, pairs), {}


def _ang_pairs(k):
    def build():
        rng = np.random.default_rng(3100 + k)
        q, t = _poses(rng, 9)
        X = rng.normal(size=(50, 3))
        return _ang_problem(q, t, X, [(int(rng.integers(0, 9)), int(rng.integers(0, 9)), rng.integers(0, 50, int(rng.integers(1, 30)))) for _ in range(k)]), {}
    return build


def _ang_percentiles(p):
    def build():
        a, _ = _ang_sizes()
        return a, dict(percentile=p)
    return build


def _ang_random():
    rng = np.random.default_rng(3200)
    q, t = _poses(rng, 30)
    X = rng.normal(size=(3000, 3)) * 2
    pairs = [(int(rng.integers(0, 30)), int(rng.integers(0, 30)), rng.integers(0, 3000, int(rng.integers(1, 1500)))) for _ in range(40)]
    return _ang_problem(q, t, X, pairs), {}


ANGLE_CASES = {"sizes": _ang_sizes, "bound": _ang_bound, "all_equal": _ang_all_equal, "nonfinite": _ang_nonfinite, "coincident": _ang_coincident,
               "pairs_0": _ang_pairs(0), "pairs_1": _ang_pairs(1), "pairs_64": _ang_pairs(64), "pairs_65": _ang_pairs(65),
               "percentile_0": _ang_percentiles(0.0), "percentile_50": _ang_percentiles(50.0), "percentile_100": _ang_percentiles(100.0),
               "random": _ang_random}


@functools.lru_cache(maxsize=None)
def angle_call(name):
    return ANGLE_CASES[name]()


@functools.lru_cache(maxsize=None)
def angle_reference(name):
    a, kw = angle_call(name)
    return ref.shared_point_angles(*a, **kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def angle_same(a, b):
    """bit for bit; the reference and the library both write the one quiet NaN"""
    return np.array_equal(bits(a["angle"]), bits(b["angle"]))


def angle_digest(r):
    return hashlib.sha256(bits(r["angle"]).tobytes()).hexdigest()


def angle_permuted(args, seed):
    q, t, X, pi, poff, sp = args
    order = np.random.default_rng(seed).permutation(len(pi))
    pairs = [(int(pi[p, 0]), int(pi[p, 1]), sp[int(poff[p]):int(poff[p + 1])]) for p in order]
    return _ang_problem(q, t, X, pairs), order


def rank_of(n, p=75.0):
    """Percentile's index: round(p / 100 * (n - 1)), half away from zero"""
    v = p / 100 * (n - 1)
    return int(np.floor(v + 0.5))


# ---- the three methods on scenes ---------------------------------------------------------------------------------------------
# the five scenes of tests/golden/scenes.py's kind that sections 17 to 19 use (triangulator_cases.SCENES); the mapper's
# options for them: the scenes plant 25 to 40 points, so the inlier threshold comes down from 30
SCENE_OPTIONS = dict(abs_pose_min_num_inliers=5, local_ba_num_images=4)


def scene_names():
    import triangulator_cases as tc
    return sorted(tc.SCENES)


@functools.lru_cache(maxsize=None)
def mapper_state(name, num_model_images=2, has_prior_focal_length=True):
    """A scene cut into a model and candidates: `num_model_images` images at their true poses with the planted
    points at least two of them see (true positions, point ids 1, 2, ... in the planted order), every other image a candidate.  Returns a dict:
    cameras (with the prior flag), images, points, candidates, graph_images, matches (the forms of mapper_ref_lib.Scene)."""
    import triangulator_cases as tc
    sc, _ = tc.scene_case(name)
    # the pair of images that shares the most planted points (the lowest ids among equals), then the image that shares
    # the most with those taken, and so on
    seen = {i: {j for j, obs in sc["planted"].items() if any(e[0] == i for e in obs)} for i in sorted(sc["images"])}
    ids = sorted(seen)
    model_ids = list(max(((a, b) for a in ids for b in ids if a < b), key=lambda ab: (len(seen[ab[0]] & seen[ab[1]]), -ab[0], -ab[1])))
    while len(model_ids) < num_model_images:
        taken = set().union(*(seen[i] for i in model_ids))
        model_ids.append(max((i for i in ids if i not in model_ids), key=lambda i: (len(seen[i] & taken), -i)))
    model_ids = sorted(model_ids)
    images = {i: [sc["images"][i][0], sc["images"][i][1], sc["images"][i][2], sc["images"][i][3], np.full(len(sc["images"][i][3]), NO_POINT, np.uint64)]
              for i in model_ids}
    points = {}
    for j, obs in sc["planted"].items():
        track = [(i, k) for i, k in obs if i in images]
        if len(track) >= 2:
            pid = len(points) + 1  # Reconstruction.add_point3D's ids
            points[pid] = (sc["xyz"][j].copy(), track)
            for i, k in track:
                images[i][4][k] = pid
    candidates = {i: (im[0], im[3]) for i, im in sc["images"].items() if i not in images}
    cameras = {c: (cam[0], cam[1], cam[2], cam[3], has_prior_focal_length) for c, cam in sc["cameras"].items()}
    return dict(cameras=cameras, images={i: tuple(v) for i, v in images.items()}, points=points, candidates=candidates,
                graph_images=sc["graph_images"], matches=sc["matches"])


def ref_scene(st):
    return ref.Scene(st["cameras"], st["images"], st["points"], st["candidates"], st["graph_images"], st["matches"])


def mapper(st):
    """(Reconstruction, CorrespondenceGraph, IncrementalTriangulator, IncrementalMapper) of a state through the public
    methods, every image outside the model a candidate"""
    import pycolmap_amd as pc
    import triangulator_cases as tc
    r = pc.Reconstruction()
    for cid, cam in st["cameras"].items():
        r.add_camera(pc.Camera(model=tc.MODEL_NAMES[cam[0]], width=cam[1], height=cam[2], params=list(cam[3]), camera_id=cid,
                               has_prior_focal_length=bool(cam[4])))
    for iid, (cid, q, t, xy, _) in st["images"].items():
        im = pc.Image(name=f"image{iid}.png", camera_id=cid, id=iid)
        im.cam_from_world = pc.Rigid3d(pc.Rotation3d(np.array(q)), np.array(t))
        im.points2D = [pc.Point2D(p) for p in xy]
        r.add_image(im)
    for pid, (xyz, track) in sorted(st["points"].items()):
        got = r.add_point3D(np.array(xyz), pc.Track([pc.TrackElement(i, k) for i, k in track]))
        assert got == pid, (got, pid)
    g = pc.CorrespondenceGraph()
    for iid, n in st["graph_images"].items():
        g.add_image(iid, n)
    for a, b, m in st["matches"]:
        g.add_correspondences(a, b, m)
    g.finalize()
    t = pc.IncrementalTriangulator(g, r)
    mp = pc.IncrementalMapper(t)
    for iid, (cid, xy) in st["candidates"].items():
        im = pc.Image(name=f"image{iid}.png", camera_id=cid, id=iid)
        im.points2D = [pc.Point2D(p) for p in xy]
        mp.add_candidate(im)
    return r, g, t, mp


# the references in the library's place (IncrementalMapper._*_with)
def vis_solver(d):
    return ref.image_visibility(d["image_point_offsets"], d["point2D_point3D"], d["cand_width"], d["cand_height"], d["cand_point_offsets"],
                                d["cand_xy"], d["corr_offsets"], d["corr_image"], d["corr_point2D"])


def pose_solver(d):
    import abspose_ref_lib
    n = len(d["points2D"])
    r = abspose_ref_lib.estimate([0, n], [int(d["camera_model"])], [np.asarray(d["camera_params"]).reshape(-1)], d["points2D"], d["points3D"],
                                 estimation={k: (int(v) if isinstance(v, bool) else v) for k, v in d["estimation"].items()})
    return dict(success=bool(r["success"][0]), qvec=r["qvec"][0], tvec=r["tvec"][0], num_inliers=int(r["num_inliers"][0]),
                focal_factor=float(r["focal_factor"][0]), inlier_mask=r["inlier_mask"].astype(np.uint8))


def angle_solver(d):
    return ref.shared_point_angles(d["qvec"], d["tvec"], d["point_xyz"], d["pair_images"], d["pair_offsets"].reshape(-1),
                                   d["shared_points"].reshape(-1), percentile=d["percentile"])


def model_snapshot(r):
    """what the tests compare of a Reconstruction: poses and point3D ids per image, camera parameters, tracks and positions"""
    return dict(images={i: (bits(np.concatenate([im.cam_from_world.rotation.quat, im.cam_from_world.translation])).tolist(),
                            [p.point3D_id for p in im.points2D]) for i, im in r.images.items()},
                cameras={c: bits(cam.params).tolist() for c, cam in r.cameras.items()},
                points={p: (bits(pt.xyz).tolist(), [(e.image_id, e.point2D_idx) for e in pt.track.elements]) for p, pt in r.points3D.items()})


def ref_snapshot(rs, st):
    """model_snapshot's view of a reference scene (points keep their positions: nothing here moves them)"""
    images = {}
    for i in sorted(rs.sizes):
        if rs.is_registered(i):
            q, t, ids = rs.image(i)
            images[i] = (bits(np.concatenate([q, t])).tolist(), [int(v) for v in ids])
    return dict(images=images, cameras={c: bits(rs.camera_params(c)).tolist() for c in st["cameras"]},
                points={p: (bits(st["points"][p][0]).tolist(), tr) for p, tr in rs.tracks().items()})


# ---- section 20 restated independently in Python / numpy -----------------------------------------------------------------------
def np_cells(x, extent):
    with np.errstate(all="ignore"):
        v = 64.0 * np.asarray(x, np.float64) / np.float64(extent)
    out = np.zeros(v.shape, np.int64)
    mid = (v >= 1.0) & (v < 64.0)
    out[mid] = np.floor(v[mid]).astype(np.int64)
    out[v >= 64.0] = 63
    return out


def np_score(cx, cy):
    """a level's distinct cells times its cell count, over the six levels"""
    return sum(len({(int(a) >> s, int(b) >> s) for a, b in zip(cx, cy)}) * 4 ** (6 - s) for s in range(6))


def np_visibility(image_point_offsets, point2D_point3D, cand_width, cand_height, cand_point_offsets, cand_xy, corr_offsets, corr_image, corr_point2D):
    ipoff, cpoff, coff = (np.asarray(a, np.int64) for a in (image_point_offsets, cand_point_offsets, corr_offsets))
    has = np.asarray(point2D_point3D, np.uint64) != np.uint64(NO_POINT)
    carries = has[ipoff[np.asarray(corr_image, np.int64)] + np.asarray(corr_point2D, np.int64)] if len(corr_image) else np.zeros(0, bool)
    nobs, nvis, score = [], [], []
    for c in range(len(cand_width)):
        idx = np.arange(cpoff[c], cpoff[c + 1])
        with_corr = np.array([coff[j + 1] > coff[j] for j in idx], bool)
        visible = np.array([carries[coff[j]:coff[j + 1]].any() for j in idx], bool)
        xy = np.asarray(cand_xy, np.float64).reshape(-1, 2)[idx][visible] if len(idx) else np.zeros((0, 2))
        nobs.append(int(with_corr.sum()))
        nvis.append(int(visible.sum()))
        score.append(np_score(np_cells(xy[:, 0], cand_width[c]), np_cells(xy[:, 1], cand_height[c])))
    return dict(num_observations=np.array(nobs, np.uint32), num_visible_points3D=np.array(nvis, np.uint32), score=np.array(score, np.uint64),
                max_score=sum(16 ** l for l in range(1, 7)))


def np_centre(q, t):
    """16.2: rotation.inverse() * -translation, the inverse being the conjugate over the squared norm (the zero quaternion
    when that is not positive, NaN included) and the product Eigen's v + w (2 u x v) + u x (2 u x v); the quaternion is not
    normalised"""
    q, v = np.asarray(q, np.float64), -np.asarray(t, np.float64)
    n2 = float(q @ q)
    if not n2 > 0:
        return v
    u, w = -q[:3] / n2, q[3] / n2
    with np.errstate(all="ignore"):
        uv = 2.0 * np.cross(u, v)
        return v + w * uv + np.cross(u, uv)


def np_angles(c1, c2, X):
    """the angle at X between the rays to c1 and c2, folded to [0, pi / 2]; 0 where a ray has no length"""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        r1, r2, b2 = ((X - c1) ** 2).sum(1), ((X - c2) ** 2).sum(1), ((c1 - c2) ** 2).sum()
        den = 2.0 * np.sqrt(r1 * r2)
        a = np.abs(np.arccos((r1 + r2 - b2) / den))
        a = np.minimum(a, np.pi - a)
        a[np.isnan(a) & ~np.isnan(den) & ~np.isnan(r1 + r2 - b2) & (den != 0)] = NAN  # a ratio outside [-1, 1] stays NaN
    a[den == 0] = 0.0
    return a


def np_percentile(values, p=75.0):
    v = np.sort(np.asarray(values, np.float64))  # numpy sorts NaN last
    return float(v[min(len(v) - 1, max(0, rank_of(len(v), p)))])


def np_pair_angles(qvec, tvec, point_xyz, pair_images, pair_offsets, shared_points, percentile=75.0):
    q, t, X = np.asarray(qvec, np.float64).reshape(-1, 4), np.asarray(tvec, np.float64).reshape(-1, 3), np.asarray(point_xyz, np.float64).reshape(-1, 3)
    centres = [np_centre(q[i], t[i]) for i in range(len(q))]
    out, every = [], []
    for p, (a, b) in enumerate(np.asarray(pair_images).reshape(-1, 2)):
        ang = np_angles(centres[a], centres[b], X[np.asarray(shared_points[int(pair_offsets[p]):int(pair_offsets[p + 1])], np.int64)])
        every.append(ang)
        out.append(np_percentile(ang, percentile))
    return dict(angle=np.array(out), angles=np.concatenate(every) if every else np.zeros(0))


def state_point2D_ids(st):
    return {i: np.array(im[4], np.uint64).copy() for i, im in st["images"].items()}


def np_find_next_images(st, trials=None, **options):
    """20.1 on a state, from a dict-of-lists graph (triangulator_cases.PyGraph)"""
    import triangulator_cases as tc
    o = dict(zip(ref.OPTION_FIELDS, ref.OPTION_DEFAULTS), **options)
    g = tc.py_graph(dict(graph_images=st["graph_images"], matches=st["matches"]))
    ids = state_point2D_ids(st)
    fresh, tried = [], []
    for iid, (cid, xy) in st["candidates"].items():
        n = len(xy)
        corr = [g.direct(iid, p) for p in range(n)]
        nobs = sum(1 for c in corr if c)
        vis = [any(a in ids and ids[a][b] != NO_POINT for a, b in c) for c in corr]
        nvis = sum(vis)
        done = (trials or {}).get(iid, 0)
        if nvis < o["abs_pose_min_num_inliers"] or done >= o["max_reg_trials"]:
            continue
        w, h = st["cameras"][cid][1], st["cameras"][cid][2]
        pts = np.asarray(xy, np.float64).reshape(-1, 2)[np.array(vis, bool)]
        method = str(o["image_selection_method"]).split(".")[-1]
        rank = {"MAX_VISIBLE_POINTS_NUM": np.float32(nvis), "MAX_VISIBLE_POINTS_RATIO": np.float32(nvis) / np.float32(nobs),
                "MIN_UNCERTAINTY": np.float32(np_score(np_cells(pts[:, 0], w), np_cells(pts[:, 1], h)))}[method]
        (tried if done else fresh).append((-float(rank), iid))
    return [i for _, i in sorted(fresh)] + [i for _, i in sorted(tried)]


BUNDLE_ROWS = ((1.0, 0.6), (1.5, 0.6), (2.0, 0.5), (2.5, 0.4), (3.0, 0.3), (4.0, 0.2), (5.0, 0.1), (6.0, 0.1))


def np_find_local_bundle(st, image_id, **options):
    """20.3 on a state, eagerly: (bundle, the smallest distance of a used angle from a threshold it was compared with)"""
    o = dict(zip(ref.OPTION_FIELDS, ref.OPTION_DEFAULTS), **options)
    cid, q, t, xy, pids = st["images"][image_id]
    mine = [int(p) for p in pids if p != NO_POINT]
    shared = {}
    for p in mine:
        for i, _ in st["points"][p][1]:
            if i != image_id:
                shared[i] = shared.get(i, 0) + 1
    ov = sorted(shared.items(), key=lambda e: (-e[1], e[0]))
    want = min(o["local_ba_num_images"] - 1, len(ov))
    if len(ov) == want:
        return [i for i, _ in ov], float("inf")
    c0, mine_set = np_centre(q, t), set(mine)
    angle = {}
    for i, _ in ov:
        X = [st["points"][int(p)][0] for p in st["images"][i][4] if p != NO_POINT and int(p) in mine_set]
        angle[i] = np_percentile(np_angles(c0, np_centre(st["images"][i][1], st["images"][i][2]), X))
    out, margin = [], float("inf")
    deg = np.pi / 180.0
    for div, share in BUNDLE_ROWS:
        if len(out) >= want:
            break
        for i, n in ov:
            if n < share * len(mine):
                break
            if i in out:
                continue
            thr = o["local_ba_min_tri_angle"] * deg / div
            margin = min(margin, abs(angle[i] - thr))
            if angle[i] >= thr:
                out.append(i)
                if len(out) >= want:
                    break
    out += [i for i, _ in ov if i not in out][:want - len(out)]
    return out, margin


# ---- what the fixture freezes and the budget records ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_loop_reference(name, num_model_images=2):
    """The reference's loop on a state until find_next_images returns nothing: the log [(ranked ids, the image tried,
    registered, its local bundle or None)], the trial counts and the final snapshot"""
    st = mapper_state(name, num_model_images)
    rs = ref_scene(st)
    log = []
    while True:
        ranked = rs.find_next_images(**SCENE_OPTIONS)
        if not ranked:
            break
        ok = rs.register_next_image(ranked[0], **SCENE_OPTIONS)
        log.append((ranked, ranked[0], ok, rs.find_local_bundle(ranked[0], **SCENE_OPTIONS) if ok else None))
    return log, {i: rs.num_reg_trials(i) for i in sorted(st["candidates"])}, ref_snapshot(rs, st)


def loop_digest(log, trials, snapshot):
    return hashlib.sha256(repr((log, sorted(trials.items()), sorted(snapshot["images"].items()), sorted(snapshot["cameras"].items()),
                                sorted(snapshot["points"].items()))).encode()).hexdigest()


def measure_angle_difference():
    """the largest absolute difference between the reference's and the restatement's angles over ANGLE_CASES, per shared
    point and per pair (both NaN, or neither)"""
    worst = 0.0
    for name in sorted(ANGLE_CASES):
        a, kw = angle_call(name)
        r, m = ref.shared_point_angles(*a, all_angles=True, **kw), np_pair_angles(*a, **kw)
        for f in ("angles", "angle"):
            assert np.array_equal(np.isnan(r[f]), np.isnan(m[f])), (name, f)
            ok = ~np.isnan(r[f])
            if ok.any():
                worst = max(worst, float(np.abs(r[f][ok] - m[f][ok]).max()))
    return worst
