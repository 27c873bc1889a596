"""Deterministic synthetic inputs of the incremental triangulator for tests/test_triangulator_cpu.py,
tests/test_triangulator_gpu.py and tests/golden/make_triangulator_ref_golden.py: seeded scenes of planted points seen by
4 to 12 cameras with a correspondence graph from the planted tracks plus wrong matches; a brute-force restatement of the
graph and an independent Python restatement of Find, Continue and Create; flat problems of
Context.triangulate_observations built by hand for the edge cases; and the lists the fixture freezes."""
from __future__ import annotations

import hashlib

import numpy as np

import ba_cases
import oracle_lib
import triangulator_ref_lib as ref

MODEL_NAMES = ba_cases.MODEL_NAMES
WIDTH, HEIGHT = 1000, 800
NO_POINT = ref.NO_POINT
DEG = 0.0174532925199432954743716805978692718781530857086181640625


# ---- geometry ----------------------------------------------------------------------------------------------------------
def look_at(centre, target=(0.0, 0.0, 0.0)):
    """cam_from_world (qvec x y z w, tvec) of a camera at `centre` looking at `target`, y down"""
    c = np.asarray(centre, np.float64)
    z = np.asarray(target, np.float64) - c
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    if w > 1e-6:
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    else:  # a half turn: not produced by the rings below
        raise ValueError("look_at: degenerate rotation")
    q /= np.linalg.norm(q)
    return q, -pose_matrix(q, np.zeros(3))[:, :3] @ c


def pose_matrix(q, t):
    """11.1: [R | t] from q = (x, y, z, w) with the Rigid3d binding's arithmetic, one rounding per operation"""
    x, y, z, w = (np.float64(v) for v in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                  [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])
    return np.concatenate([R, np.asarray(t, np.float64).reshape(3, 1)], axis=1)


def project(model, params, q, t, X):
    """pixels of world points X (N, 3) (the oracle's Camera::ImgFromCam)"""
    P = pose_matrix(q, t)
    Xc = np.asarray(X, np.float64).reshape(-1, 3) @ P[:, :3].T + P[:, 3]
    cam = oracle_lib.make_camera(int(model), WIDTH, HEIGHT, tuple(params))
    return oracle_lib.img_from_cam(cam, Xc[:, :2] / Xc[:, 2:3])


def ring(nimg, radius=6.0, seed=0):
    """nimg poses on a ring around the origin, at varying heights"""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for i in range(nimg):
        a = 2 * np.pi * i / nimg + rng.uniform(-0.02, 0.02)
        out.append(look_at([radius * np.cos(a), radius * np.sin(a), rng.uniform(-1.5, 1.5)]))
    return out


# ---- 17.7: scenes --------------------------------------------------------------------------------------------------------
def scene(seed=0, nimg=12, npts=30, models=(2,), noise=0.3, views=(4, 12), wrong=2, drop=0.0, extra_keypoints=3,
          bogus_camera=None):
    """A seeded scene.  Returns a dict: cameras {id: (model, width, height, params)}, images {id: (camera id, qvec, tvec,
    xy (N, 2), point3D ids (N,) all NO_POINT)}, planted {point: [(image id, point2D index)]}, xyz (npts, 3),
    graph_images {id: N}, matches [(id1, id2, (M, 2) uint32)]: per image pair the planted matches (each dropped with
    probability `drop`) followed by `wrong` wrong ones between random keypoints.  Camera and image ids start at 1.
    bogus_camera: the index into `models` of a camera whose focal length is made bogus."""
    rng = np.random.default_rng(seed)
    cameras = {}
    for c, m in enumerate(models):
        prm = ba_cases.model_params(m)
        if bogus_camera == c:
            prm = prm.copy()
            prm[0] = 0.01 * WIDTH  # ratio 0.01 < min_focal_length_ratio
        cameras[c + 1] = (int(m), WIDTH, HEIGHT, prm)
    poses = ring(nimg, seed=seed)
    xyz = rng.uniform(-1.0, 1.0, (npts, 3))
    lo, hi = views
    seen = [sorted(rng.choice(nimg, size=int(rng.integers(lo, min(hi, nimg) + 1)), replace=False).tolist()) for _ in range(npts)]
    per_image = [[] for _ in range(nimg)]  # (point or -1) per point2D
    for j, imgs in enumerate(seen):
        for i in imgs:
            per_image[i].append(j)
    images, planted, index_of = {}, {j: [] for j in range(npts)}, {}
    for i in range(nimg):
        order = per_image[i] + [-1] * extra_keypoints
        order = [order[k] for k in rng.permutation(len(order))]
        cam_id = i % len(models) + 1
        model, _, _, prm = cameras[cam_id]
        good_prm = ba_cases.model_params(model)
        q, t = poses[i]
        xy = np.zeros((len(order), 2))
        for k, j in enumerate(order):
            if j < 0:
                xy[k] = rng.uniform([50, 50], [WIDTH - 50, HEIGHT - 50])
            else:
                xy[k] = project(model, good_prm, q, t, xyz[j])[0] + rng.normal(0, noise, 2) if noise else project(model, good_prm, q, t, xyz[j])[0]
                planted[j].append((i + 1, k))
                index_of[(i, j)] = k
        images[i + 1] = (cam_id, q, t, xy, np.full(len(order), NO_POINT, np.uint64))
    matches = []
    for a in range(nimg):
        for b in range(a + 1, nimg):
            m = [(index_of[(a, j)], index_of[(b, j)]) for j in range(npts) if (a, j) in index_of and (b, j) in index_of
                 and not (drop and rng.random() < drop)]
            for _ in range(wrong):
                m.append((int(rng.integers(len(images[a + 1][3]))), int(rng.integers(len(images[b + 1][3])))))
            if m:
                matches.append((a + 1, b + 1, np.array(m, np.uint32).reshape(-1, 2)))
    return dict(cameras=cameras, images=images, planted=planted, xyz=xyz, points={},
                graph_images={i: len(im[3]) for i, im in images.items()}, matches=matches)


def ref_scene(sc, finalize=True):
    return ref.Scene(sc["cameras"], sc["images"], sc["points"], sc["graph_images"], sc["matches"], finalize=finalize)


# ---- 17.1 restated by brute force ------------------------------------------------------------------------------------------
class PyGraph:
    """dict-of-lists restatement of the correspondence graph: corrs[(image, point2D)] = [(image, point2D)]"""

    def __init__(self):
        self.npts, self.corrs, self.ncorr, self.pairs, self.nobs = {}, {}, {}, {}, {}

    def add_image(self, iid, n):
        self.npts[iid] = n
        self.ncorr[iid] = 0

    def add_correspondences(self, a, b, m):
        if a == b:
            return
        key = (min(a, b), max(a, b))
        self.pairs.setdefault(key, 0)
        for p, q in np.asarray(m).reshape(-1, 2).tolist():
            if p >= self.npts[a] or q >= self.npts[b]:
                continue
            if any(c[0] == b for c in self.corrs.get((a, p), [])) or any(c[0] == a for c in self.corrs.get((b, q), [])):
                continue
            self.corrs.setdefault((a, p), []).append((b, q))
            self.corrs.setdefault((b, q), []).append((a, p))
            self.ncorr[a] += 1
            self.ncorr[b] += 1
            self.pairs[key] += 1

    def finalize(self):
        for iid in list(self.npts):
            self.nobs[iid] = sum(1 for p in range(self.npts[iid]) if self.corrs.get((iid, p)))
            if self.nobs[iid] == 0:
                del self.npts[iid]

    def direct(self, iid, p):
        if iid not in self.npts or p >= self.npts[iid]:
            raise ValueError("unknown image or point2D")
        return list(self.corrs.get((iid, p), []))

    def transitive(self, iid, p, transitivity):
        if transitivity == 1:
            return self.direct(iid, p)
        if not self.direct(iid, p):
            return []
        levels, seen = [[(iid, p)]], {(iid, p)}
        for _ in range(transitivity):
            nxt = []
            for o in levels[-1]:
                for c in self.corrs.get(o, []):
                    if c not in seen:
                        seen.add(c)
                        nxt.append(c)
            if not nxt:
                break
            levels.append(nxt)
        found = [o for lv in levels for o in lv]
        found[0] = found[-1]
        return found[:-1]

    def is_two_view(self, iid, p):
        c = self.direct(iid, p)
        return len(c) == 1 and len(self.direct(*c[0])) == 1


def py_graph(sc, finalize=True):
    g = PyGraph()
    for iid, n in sc["graph_images"].items():
        g.add_image(iid, n)
    for a, b, m in sc["matches"]:
        g.add_correspondences(a, b, m)
    if finalize:
        g.finalize()
    return g


# ---- 17.2 restated independently: numpy for the angle, tests/tri_ref for the RANSAC ----------------------------------------
def bogus(cam, o):
    model, w, h, prm = cam
    nf = ba_cases.NUM_FOCAL[model]
    if not (0 <= prm[nf] <= w and 0 <= prm[nf + 1] <= h):
        return True
    if any(not (o["min_focal_length_ratio"] <= f / max(w, h) <= o["max_focal_length_ratio"]) for f in prm[:nf]):
        return True
    return any(abs(e) > o["max_extra_param"] for e in prm[nf + 2:])


def np_angular_error(nxy, P, X):
    a = np.array([nxy[0], nxy[1], 1.0])
    b = P[:, :3] @ X + P[:, 3]
    return float(np.arccos(np.clip(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)), -1.0, 1.0)))


class PyState:
    """the model as plain Python: point2D ids per image, points {id: [xyz, [(image, point2D)]]}"""

    def __init__(self, sc):
        self.sc = sc
        self.ids = {i: [int(v) for v in im[4]] for i, im in sc["images"].items()}
        self.points = {pid: [np.array(xyz, np.float64), list(track)] for pid, (xyz, track) in sc["points"].items()}
        self.nxy = {i: ref.lift(sc["cameras"][im[0]][0], sc["cameras"][im[0]][3], im[3]) for i, im in sc["images"].items()}
        self.P = {i: pose_matrix(im[1], im[2]) for i, im in sc["images"].items()}
        self.decisions = []  # (image, point2D, continued to (image, point2D) or None, [created tracks])

    def triangulate_image(self, graph, image_id, **kw):
        import tri_ref_lib
        o = dict(zip(ref.OPTION_FIELDS, ref.OPTION_DEFAULTS))
        o.update(kw)
        sc = self.sc
        if bogus(sc["cameras"][sc["images"][image_id][0]], o):
            return 0
        count = 0
        for p in range(len(self.ids[image_id])):
            found = [c for c in graph.transitive(image_id, p, o["max_transitivity"])
                     if c[0] in sc["images"] and not bogus(sc["cameras"][sc["images"][c[0]][0]], o)]
            if not found:
                continue
            with_point = [c for c in found if self.ids[c[0]][c[1]] != NO_POINT]
            ref_obs, cont = (image_id, p), None
            if with_point and self.ids[image_id][p] == NO_POINT:
                angles = [np_angular_error(self.nxy[image_id][p], self.P[image_id], self.points[self.ids[c[0]][c[1]]][0]) for c in with_point]
                k = int(np.argmin(angles))  # the first minimum
                if angles[k] <= DEG * o["continue_max_angle_error"]:
                    cont = with_point[k]
                    pid = self.ids[cont[0]][cont[1]]
                    self.points[pid][1].append(ref_obs)
                    self.ids[image_id][p] = pid
                    count += 1
            kept = [c for c in found + [ref_obs] if self.ids[c[0]][c[1]] == NO_POINT]
            created, first = [], True
            while len(kept) >= 2:
                if first and len(kept) == 2 and o["ignore_two_view_tracks"] and graph.is_two_view(*kept[0]):
                    break
                first = False
                n = len(kept)
                imgs = sorted({c[0] for c in kept})
                poses = np.array([self.P[i].reshape(-1) for i in imgs])
                xyz, ok, mask, _ = tri_ref_lib.triangulate(
                    poses, [0, n], [imgs.index(c[0]) for c in kept], [self.nxy[c[0]][c[1]] for c in kept],
                    min_tri_angle=DEG * o["min_angle"], max_error=DEG * o["create_max_angle_error"], min_inlier_ratio=0.02,
                    confidence=0.9999, dyn_num_trials_multiplier=3.0, max_num_trials=10000,
                    min_num_trials=n * (n - 1) // 2 if n <= 15 else 0)
                if not ok[0]:
                    break
                track = [c for c, m in zip(kept, mask) if m]
                pid = max([0] + list(self.points)) + 1
                self.points[pid] = [xyz[0].copy(), track]
                for c in track:
                    self.ids[c[0]][c[1]] = pid
                created.append(track)
                count += len(track)
                kept = [c for c, m in zip(kept, mask) if not m]
                if len(kept) < 3:
                    break
            self.decisions.append((image_id, p, cont, created))
        return count

    def tracks(self):
        return {pid: list(t) for pid, (_, t) in self.points.items()}


# ---- the flat problem of one image, as the host plans it at max_transitivity 1 (17.4) ---------------------------------------
def flat_problem(sc, graph, image_ids, state=None, **kw):
    """(positional arguments of triangulate_observations, keywords, items [(image, point2D)], candidates [(image,
    point2D)]) for every point2D with found correspondences of the given images, in order, on the model as it stands."""
    o = dict(zip(ref.OPTION_FIELDS, ref.OPTION_DEFAULTS))
    o.update(kw)
    cam_ids, img_ids = list(sc["cameras"]), list(sc["images"])
    ids = state.ids if state else {i: [int(v) for v in im[4]] for i, im in sc["images"].items()}
    points = state.points if state else {pid: [np.asarray(x), t] for pid, (x, t) in sc["points"].items()}
    off, ci, xy, has, X, two, items, cands = [0], [], [], [], [], [], [], []
    for image_id in image_ids:
        if bogus(sc["cameras"][sc["images"][image_id][0]], o):
            continue
        for p in range(len(ids[image_id])):
            found = [c for c in graph.transitive(image_id, p, o["max_transitivity"])
                     if c[0] in sc["images"] and not bogus(sc["cameras"][sc["images"][c[0]][0]], o)]
            if not found:
                continue
            first = next((c for c in found if ids[c[0]][c[1]] == NO_POINT), None)
            two.append(bool(o["ignore_two_view_tracks"] and first is not None and graph.is_two_view(*first)))
            for c in found + [(image_id, p)]:
                pid = ids[c[0]][c[1]]
                ci.append(img_ids.index(c[0]))
                xy.append(sc["images"][c[0]][3][c[1]])
                has.append(pid != NO_POINT)
                X.append(points[pid][0] if pid != NO_POINT else np.zeros(3))
                cands.append(c)
            off.append(len(ci))
            items.append((image_id, p))
    args = ([sc["cameras"][c][0] for c in cam_ids], [sc["cameras"][c][3] for c in cam_ids],
            np.array([cam_ids.index(sc["images"][i][0]) for i in img_ids], np.uint32),
            np.array([sc["images"][i][1] for i in img_ids]).reshape(-1, 4), np.array([sc["images"][i][2] for i in img_ids]).reshape(-1, 3),
            np.array(off, np.uint64), np.array(ci, np.uint32), np.array(xy).reshape(-1, 2), np.array(has, np.uint8),
            np.array(X).reshape(-1, 3))
    kwargs = dict(no_create_two_view=np.array(two, np.uint8), create_max_angle_error=o["create_max_angle_error"],
                  continue_max_angle_error=o["continue_max_angle_error"], min_angle=o["min_angle"])
    return args, kwargs, items, cands


# ---- flat problems built by hand (17.7's edge cases) -----------------------------------------------------------------------
def hand_problem(seed=0, sizes=(4,), models=(2,), nimg=70, noise=0.3, p_has=0.0, p_out=0.1, groups=1, two_view=None,
                 ref_has=False):
    """A flat problem with one item per entry of `sizes` (candidates, the reference included), every candidate in another
    image.  Each item plants `groups` points and deals its candidates to them in turn; a candidate is an outlier (a random
    pixel) with probability p_out and carries a point (the planted one plus 1e-3 noise) with probability p_has."""
    rng = np.random.default_rng(seed)
    poses = ring(nimg, seed=seed)
    cams = [(int(m), ba_cases.model_params(m)) for m in models]
    icam = np.arange(nimg) % len(models)
    off, ci, xy, has, X = [0], [], [], [], []
    for n in sizes:
        pts = rng.uniform(-1.0, 1.0, (groups, 3))
        imgs = rng.choice(nimg, size=n, replace=False) if n <= nimg else rng.integers(0, nimg, n)
        for k in range(n):
            i = int(imgs[k])
            P = pts[k % groups]
            m, prm = cams[icam[i]]
            if rng.random() < p_out:
                pix = rng.uniform([50, 50], [WIDTH - 50, HEIGHT - 50])
            else:
                pix = project(m, prm, *poses[i], P)[0] + rng.normal(0, noise, 2)
            carries = (rng.random() < p_has) if k + 1 < n else ref_has
            ci.append(i)
            xy.append(pix)
            has.append(carries)
            X.append(P + rng.normal(0, 1e-3, 3) if carries else np.zeros(3))
        off.append(len(ci))
    args = [[c[0] for c in cams], [c[1] for c in cams], icam.astype(np.uint32), np.array([p[0] for p in poses]),
            np.array([p[1] for p in poses]), np.array(off, np.uint64), np.array(ci, np.uint32).reshape(-1),
            np.array(xy, np.float64).reshape(-1, 2), np.array(has, np.uint8).reshape(-1), np.array(X, np.float64).reshape(-1, 3)]
    kw = {}
    if two_view is not None:
        kw["no_create_two_view"] = np.array(two_view, np.uint8)
    return args, kw


def _threshold_problem(above):
    """one item whose Continue angle A is exactly DegToRad(continue_max_angle_error) (above = False), or one double above
    it: the reference pixel is moved until some option value e has DegToRad(e) == A in doubles"""
    args, kw = hand_problem(seed=31, sizes=(3,), models=(1,), noise=0.0, p_out=0.0)
    args[8][:] = [1, 1, 0]
    X = np.array([0.1, -0.2, 0.3])
    args[9][0] = X
    args[9][1] = X + [0.5, 0.0, 0.0]  # farther from the ray: candidate 0 is the minimum
    i = int(args[6][2])
    m, prm = args[0][0], args[1][0]
    pix0 = project(m, prm, args[3][i], args[4][i], X)[0]
    for k in range(256):
        pix = pix0 + [20.0 + k, 0.0]
        A = ref.angular_error(ref.lift(m, prm, [pix])[0], args[3][i], args[4][i], X)
        e = A / DEG
        hits = [v for v in _neighbours(e, 4) if DEG * v == A]
        if hits:
            break
    else:
        raise AssertionError("no pixel whose angle is a representable threshold")
    args[7][2] = pix
    thr = hits[0]
    if above:
        while DEG * thr >= A:
            thr = np.nextafter(thr, 0.0)
        assert np.nextafter(DEG * thr, 1.0) == A
    return args, dict(kw, continue_max_angle_error=float(thr))


def _neighbours(x, k):
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


def _special(what):
    if what == "behind":  # a candidate behind the camera: its image looks away from the point
        args, kw = hand_problem(seed=41, sizes=(5,), models=(2,), p_out=0.0)
        i = int(args[6][1])
        args[3][i] = args[3][i] * np.array([1.0, 1.0, 1.0, -1.0])  # the conjugate: another orientation altogether
        return args, kw
    args, kw = hand_problem(seed=42, sizes=(5, 6, 4), models=(2, 4), p_has=0.4, p_out=0.0)
    if what == "nan_pixel":
        args[7][1] = [np.nan, 100.0]
        args[7][7] = [np.inf, 100.0]
    elif what == "nan_pose":
        args[4][int(args[6][0])] = [np.nan, 0.0, 1.0]
        args[3][int(args[6][6])] = [np.inf, 0.0, 0.0, 1.0]
    elif what == "nan_point":
        args[8][0] = 1
        args[9][0] = [np.nan, 0.0, 0.0]
        args[8][5] = 1
        args[9][5] = [np.inf, 0.0, 0.0]
    return args, kw


_M = {n: k for k, n in enumerate(MODEL_NAMES)}
# name: (builder, keyword options)
CASES = {
    "mixed": (lambda: hand_problem(seed=1, sizes=[2, 3, 4, 5, 6, 8, 12, 20, 7, 3, 2, 9], models=(2, 1), p_has=0.25, p_out=0.15), {}),
    "two_groups": (lambda: hand_problem(seed=2, sizes=[6, 7, 8, 10, 12], models=(2,), groups=2, p_out=0.0), {}),
}
EDGE_CASES = {
    "sizes": (lambda: hand_problem(seed=3, sizes=[2, 3, 15, 16, 63, 64, 65], models=(2, 1), p_has=0.1, p_out=0.1), {}),
    "items_0": (lambda: hand_problem(seed=4, sizes=[]), {}),
    "items_1": (lambda: hand_problem(seed=5, sizes=[5]), {}),
    "items_64": (lambda: hand_problem(seed=6, sizes=[3, 4] * 32, p_has=0.2), {}),
    "items_65": (lambda: hand_problem(seed=7, sizes=[4, 3] * 32 + [5], p_has=0.2), {}),
    "items_257": (lambda: hand_problem(seed=8, sizes=[2, 3, 4, 5] * 64 + [6], p_has=0.2), {}),
    "all_models": (lambda: hand_problem(seed=9, sizes=[11, 12, 13, 22], models=tuple(range(11)), nimg=66, p_has=0.1), {}),
    "three_rounds": (lambda: hand_problem(seed=10, sizes=[12, 13], groups=3, p_out=0.0), {}),
    "left_over_2": (lambda: hand_problem(seed=11, sizes=[5], groups=2, p_out=0.0, noise=0.0), {}),
    "two_view_flag": (lambda: hand_problem(seed=12, sizes=[2, 2, 3], p_out=0.0, two_view=[1, 0, 1]), {}),
    "ref_has_point": (lambda: hand_problem(seed=13, sizes=[5, 6], p_has=0.5, ref_has=True, p_out=0.0), {}),
    "continue_at_threshold": (lambda: _threshold_problem(False), {}),
    "continue_above_threshold": (lambda: _threshold_problem(True), {}),
    "behind": (lambda: _special("behind"), {}),
    "nan_pixel": (lambda: _special("nan_pixel"), {}),
    "nan_pose": (lambda: _special("nan_pose"), {}),
    "nan_point": (lambda: _special("nan_point"), {}),
    "min_angle_0": (lambda: hand_problem(seed=14, sizes=[3, 4, 6], p_out=0.0), dict(min_angle=0.0)),
    "min_angle_180": (lambda: hand_problem(seed=14, sizes=[3, 4, 6], p_out=0.0), dict(min_angle=180.0)),
}
for _m in range(11):
    EDGE_CASES[f"model_{MODEL_NAMES[_m]}"] = ((lambda m=_m: hand_problem(seed=20 + m, sizes=[4, 6, 9], models=(m,), p_has=0.2)), {})
ALL_CASES = {**CASES, **EDGE_CASES}
RESULT_KEYS = ("continued", "cand_round", "round_offsets", "round_xyz")
_cache = {}


def case_call(name):
    """(positional arguments, keywords) of triangulate_observations; built once, read-only"""
    if name not in _cache:
        builder, opts = ALL_CASES[name]
        args, kw = builder()
        for a in list(args) + list(kw.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = (tuple(args), {**kw, **opts})
    return _cache[name]


_ref_cache = {}


def reference(name):
    if name not in _ref_cache:
        args, kw = case_call(name)
        _ref_cache[name] = ref.triangulate_observations(*args, **kw)
    return _ref_cache[name]


def bits(a):
    """the doubles' bits, every NaN as the one canonical NaN (16.6 F6)"""
    a = np.array(a, dtype=np.float64).reshape(-1)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def same(a, b) -> bool:
    return (np.array_equal(a["continued"], b["continued"]) and np.array_equal(a["cand_round"], b["cand_round"]) and
            np.array_equal(np.asarray(a["round_offsets"], np.uint64), np.asarray(b["round_offsets"], np.uint64)) and
            np.array_equal(bits(a["round_xyz"]), bits(b["round_xyz"])))


def digest(result) -> str:
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(result["continued"], np.int32).tobytes())
    h.update(np.ascontiguousarray(result["cand_round"], np.uint32).tobytes())
    h.update(np.ascontiguousarray(result["round_offsets"], np.uint64).tobytes())
    h.update(bits(result["round_xyz"]).tobytes())
    return h.hexdigest()


# ---- through Python ----------------------------------------------------------------------------------------------------
def reconstruction(sc):
    """(Reconstruction, CorrespondenceGraph) of a scene through the public methods"""
    import pycolmap_amd as pc
    r = pc.Reconstruction()
    for cid, (model, w, h, prm) in sc["cameras"].items():
        r.add_camera(pc.Camera(model=MODEL_NAMES[model], width=w, height=h, params=list(prm), camera_id=cid))
    for iid, (cid, q, t, xy, _) in sc["images"].items():
        im = pc.Image(name=f"image{iid}.png", camera_id=cid, id=iid)
        im.cam_from_world = pc.Rigid3d(pc.Rotation3d(np.array(q)), np.array(t))
        im.points2D = [pc.Point2D(p) for p in xy]
        r.add_image(im)
    g = pc.CorrespondenceGraph()
    for iid, n in sc["graph_images"].items():
        g.add_image(iid, n)
    for a, b, m in sc["matches"]:
        g.add_correspondences(a, b, m)
    g.finalize()
    return r, g


# ---- whole scenes through the sequential reference (17.7) ------------------------------------------------------------------
# name: (scene keywords, triangulate_image options)
SCENES = {
    "direct": (dict(seed=3, nimg=12, npts=30, models=(2, 4), wrong=3, drop=0.3), dict(max_transitivity=1)),
    "transitive_2": (dict(seed=3, nimg=12, npts=30, models=(2, 4), wrong=3, drop=0.3), dict(max_transitivity=2)),
    "all_models": (dict(seed=5, nimg=22, npts=40, models=tuple(range(11)), wrong=2, drop=0.1), dict(max_transitivity=1)),
    "bogus_camera": (dict(seed=6, nimg=12, npts=25, models=(2, 1), wrong=2, bogus_camera=1), dict(max_transitivity=1)),
    "two_view_off": (dict(seed=7, nimg=12, npts=25, models=(2,), wrong=4, views=(4, 6)), dict(ignore_two_view_tracks=False)),
}
_scene_cache = {}


def scene_case(name):
    if name not in _scene_cache:
        _scene_cache[name] = scene(**SCENES[name][0])
    return _scene_cache[name], SCENES[name][1]


_scene_ref_cache = {}


def scene_reference(name):
    """the reference's sequential result over all images in id order: (counts per image, points, point2D ids per image,
    modified ids, margins)"""
    if name not in _scene_ref_cache:
        sc, opts = scene_case(name)
        rs = ref_scene(sc)
        counts = [rs.triangulate_image(i, **opts) for i in sc["images"]]
        _scene_ref_cache[name] = (counts, rs.points(), {i: rs.point2D_ids(i, len(im[3])) for i, im in sc["images"].items()},
                                  rs.modified(), rs.margins())
    return _scene_ref_cache[name]


def scene_digest(counts, points) -> str:
    """sha256 over the counts and the points (ids, positions bit for bit, errors, tracks)"""
    h = hashlib.sha256()
    h.update(np.asarray(counts, np.int64).tobytes())
    for pid, (xyz, err, track) in points.items():
        h.update(np.uint64(pid).tobytes())
        h.update(bits(xyz).tobytes())
        h.update(bits([err]).tobytes())
        h.update(np.asarray(track, np.uint32).tobytes())
    return h.hexdigest()


def reconstruction_points(r):
    """{id: (xyz, error, track)} of a pycolmap Reconstruction, in the map's order"""
    return {pid: (np.array(p.xyz), float(p.error), [(e.image_id, e.point2D_idx) for e in p.track.elements])
            for pid, p in r.points3D.items()}


def reference_solver(d):
    """the reference in the library's place for IncrementalTriangulator._triangulate_image_with"""
    return ref.triangulate_observations(
        d["camera_models"].reshape(-1), d["camera_params"], d["image_cameras"].reshape(-1), d["qvec"], d["tvec"],
        d["item_offsets"].reshape(-1), d["cand_image"].reshape(-1), d["cand_xy"], d["cand_has_point"].reshape(-1), d["cand_xyz"],
        d["no_create_two_view"].reshape(-1), create_max_angle_error=d["create_max_angle_error"],
        continue_max_angle_error=d["continue_max_angle_error"], min_angle=d["min_angle"])


EMPTY_IMAGE, UNMATCHED_IMAGE = 100, 101


def reconstruction_with_empty_images(finalize):
    """(Reconstruction, CorrespondenceGraph) of a small scene plus image 100 without points2D and image 101 with three
    points2D and no correspondences, both in the model and added to the graph; finalize() erases both from the graph"""
    import pycolmap_amd as pc
    sc = scene(seed=9, nimg=5, npts=6, views=(4, 5), wrong=1)
    r, _ = reconstruction(sc)
    for iid, pts in ((EMPTY_IMAGE, []), (UNMATCHED_IMAGE, [[10.0, 20.0], [30.0, 40.0], [50.0, 60.0]])):
        im = pc.Image(name=f"image{iid}.png", camera_id=1, id=iid)
        im.cam_from_world = pc.Rigid3d(pc.Rotation3d(np.array(sc["images"][1][1])), np.array(sc["images"][1][2]))
        im.points2D = [pc.Point2D(p) for p in pts]
        r.add_image(im)
    g = pc.CorrespondenceGraph()
    for iid, n in list(sc["graph_images"].items()) + [(EMPTY_IMAGE, 0), (UNMATCHED_IMAGE, 3)]:
        g.add_image(iid, n)
    for a, b, m in sc["matches"]:
        g.add_correspondences(a, b, m)
    if finalize:
        g.finalize()
    return r, g


def check_empty_images(triangulate):
    """an image without points2D and an image without correspondences (17.2): on a graph that was not finalized the call
    returns 0 without a device call; finalize() erases both images from the graph, and the call raises (G5).  Either way
    the model is untouched.  triangulate(triangulator, options, image_id) is the call under test."""
    import pycolmap_amd as pc
    import pytest
    for finalize in (False, True):
        r, g = reconstruction_with_empty_images(finalize)
        t = pc.IncrementalTriangulator(g, r)
        for iid in (EMPTY_IMAGE, UNMATCHED_IMAGE):
            assert g.exists_image(iid) == (not finalize)
            if finalize:
                with pytest.raises(ValueError, match=r"\[correspondence_graph.h:\d+\] Check Failed: ExistsImage"):
                    triangulate(t, {}, iid)
            else:
                assert triangulate(t, {}, iid) == 0
                st = pc.last_run_stats()
                assert st["call"] == "triangulate_image" and st["num_device_calls"] == 0 and st["num_items"] == 0
            assert len(r.points3D) == 0 and t.get_modified_points3D() == set()
        assert triangulate(t, {}, 1) > 0  # the other images are not affected
