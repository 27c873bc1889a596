"""Deterministic synthetic inputs of track completion and track merging for tests/test_tracks_cpu.py,
tests/test_tracks_gpu.py and tests/golden/make_tracks_ref_golden.py: the scenes of tests/triangulator_cases.py after the
reference's triangulate_image, with observations detached and points duplicated; hand-built worlds with exact pixels for
the answers worked out by hand; an independent Python restatement of 18.1 and 18.2; flat problems of
Context.complete_tracks and Context.merge_tracks for the shapes at which the kernels can go wrong; and the lists the
fixture freezes."""
from __future__ import annotations

import copy
import hashlib

import numpy as np

import ba_cases
import tracks_ref_lib as ref
import triangulator_cases as tc

NO_POINT = ref.NO_POINT
DBL_MAX, DBL_EPSILON = np.finfo(np.float64).max, np.finfo(np.float64).eps
MAX_COMPONENT_OBS = 4096
bits = tc.bits


def colour(pid):
    return ((7 * pid) % 256, (13 * pid + 5) % 256, (29 * pid + 11) % 256)


# ---- states: a scene with points ------------------------------------------------------------------------------------------
def make_state(sc, points, point2D_ids):
    """cameras, images (with the points2D's point ids), points {id: (xyz, rgb, error, track)}, graph_images, matches"""
    images = {iid: (cid, q, t, xy, np.array(point2D_ids[iid], np.uint64)) for iid, (cid, q, t, xy, _) in sc["images"].items()}
    return dict(cameras=sc["cameras"], images=images, points=points, graph_images=sc["graph_images"], matches=sc["matches"])


def triangulated_state(name):
    """a scene of triangulator_cases after the reference's triangulate_image over all its images"""
    sc, _ = tc.scene_case(name)
    _, points, ids, _, _ = tc.scene_reference(name)
    pts = {pid: (xyz.copy(), colour(pid), err, list(track)) for pid, (xyz, err, track) in points.items()}
    return make_state(sc, pts, ids)


def perturbed(state, seed, detach=0.3, duplicate=0.3):
    """18.6: every element of a track beyond its second is detached with probability `detach`; then a share `duplicate`
    of the points with four elements or more is split in two, the second half under a new id at a position 1e-3 away"""
    rng = np.random.default_rng(seed)
    st = copy.deepcopy(state)
    ids = {iid: im[4] for iid, im in st["images"].items()}
    for pid in sorted(st["points"]):
        xyz, rgb, err, track = st["points"][pid]
        keep = track[:2]
        for e in track[2:]:
            if rng.random() < detach:
                ids[e[0]][e[1]] = NO_POINT
            else:
                keep.append(e)
        st["points"][pid] = (xyz, rgb, err, keep)
    for pid in sorted(st["points"]):
        xyz, rgb, err, track = st["points"][pid]
        if len(track) >= 4 and rng.random() < duplicate:
            new = max(st["points"]) + 1
            half = len(track) // 2
            st["points"][pid] = (xyz, rgb, err, track[:half])
            st["points"][new] = (xyz + rng.normal(0, 1e-3, 3), colour(new), err, track[half:])
            for e in track[half:]:
                ids[e[0]][e[1]] = new
    return st


def ref_scene(st, modified=(), finalize=True):
    return ref.Scene(st["cameras"], st["images"], st["points"], st["graph_images"], st["matches"], modified=modified, finalize=finalize)


def reconstruction(st, finalize=True):
    """(Reconstruction, CorrespondenceGraph, IncrementalTriangulator) of a state through the public methods; the points'
    ids must be 1 .. N"""
    import pycolmap_amd as pc
    r, _ = tc.reconstruction(st)
    assert sorted(st["points"]) == list(range(1, len(st["points"]) + 1))
    for pid in sorted(st["points"]):
        xyz, rgb, err, track = st["points"][pid]
        got = r.add_point3D(np.array(xyz), pc.Track([pc.TrackElement(i, k) for i, k in track]), list(rgb))
        assert got == pid
        r.points3D[pid].error = err
    g = pc.CorrespondenceGraph()
    for iid, n in st["graph_images"].items():
        g.add_image(iid, n)
    for a, b, m in st["matches"]:
        g.add_correspondences(a, b, m)
    if finalize:
        g.finalize()
    return r, g, pc.IncrementalTriangulator(g, r)


def recon_points(r):
    """{id: (xyz, rgb, error, track)} of a Reconstruction in ascending id order"""
    return {pid: (np.array(p.xyz), tuple(int(c) for c in p.color), float(p.error), [(e.image_id, e.point2D_idx) for e in p.track.elements])
            for pid, p in sorted(r.points3D.items())}


def recon_point2D_ids(r):
    return {iid: np.array([p.point3D_id for p in im.points2D], np.uint64) for iid, im in r.images.items()}


def same_points(got, want):
    if list(got) != list(want):
        return False
    for pid in want:
        g, w = got[pid], want[pid]
        if not (np.array_equal(bits(g[0]), bits(w[0])) and tuple(g[1]) == tuple(w[1]) and np.array_equal(bits([g[2]]), bits([w[2]])) and g[3] == w[3]):
            return False
    return True


def same_point2D_ids(got, want):
    return set(got) == set(want) and all(np.array_equal(np.asarray(got[i], np.uint64), np.asarray(want[i], np.uint64)) for i in want)


def state_digest(count, points) -> str:
    h = hashlib.sha256()
    h.update(np.int64(count).tobytes())
    for pid, (xyz, rgb, err, track) in points.items():
        h.update(np.uint64(pid).tobytes())
        h.update(bits(xyz).tobytes())
        h.update(np.asarray(rgb, np.uint8).tobytes())
        h.update(bits([err]).tobytes())
        h.update(np.asarray(track, np.uint32).tobytes())
    return h.hexdigest()


# ---- the reference in the library's place ---------------------------------------------------------------------------------
def complete_solver(d):
    return ref.complete_tracks(d["camera_models"].reshape(-1), d["camera_params"], d["image_cameras"].reshape(-1), d["qvec"], d["tvec"],
                               d["item_xyz"], d["item_offsets"].reshape(-1), d["cand_image"].reshape(-1), d["cand_xy"],
                               complete_max_reproj_error=d["complete_max_reproj_error"])


def merge_solver(d):
    return ref.merge_tracks(d["camera_models"].reshape(-1), d["camera_params"], d["image_cameras"].reshape(-1), d["qvec"], d["tvec"],
                            d["comp_point_offsets"].reshape(-1), d["comp_root_offsets"].reshape(-1), d["roots"].reshape(-1),
                            d["point_xyz"], d["point_obs_offsets"].reshape(-1), d["obs_image"].reshape(-1), d["obs_xy"],
                            d["obs_corr_offsets"].reshape(-1), d["corr_obs"].reshape(-1),
                            merge_max_reproj_error=d["merge_max_reproj_error"])


# ---- 18.1 and 18.2 restated in Python -------------------------------------------------------------------------------------
class PyTracks:
    """An independent restatement on dicts: the graph by tc.PyGraph's brute force, the error by the oracle's camera
    models through tc.project (another arithmetic: equal decisions where no error is within 1e-9 of its threshold)."""

    def __init__(self, st, modified=(), **options):
        self.o = dict(zip(ref.options_array.__globals__["OPTION_FIELDS"], ref.options_array.__globals__["OPTION_DEFAULTS"]))
        self.o.update(options)
        self.cameras, self.images = st["cameras"], {i: (c, q, t, xy, np.array(ids, np.uint64)) for i, (c, q, t, xy, ids) in st["images"].items()}
        self.points = {pid: [np.array(xyz, np.float64), tuple(rgb), err, list(track)] for pid, (xyz, rgb, err, track) in st["points"].items()}
        self.graph = tc.py_graph(st)
        self.modified = set(modified)

    def error(self, image_id, idx, X):
        cid, q, t, xy, _ = self.images[image_id]
        model, _, _, prm = self.cameras[cid]
        P = tc.pose_matrix(q, t)
        Xc = P[:, :3] @ X + P[:, 3]
        if Xc[2] < DBL_EPSILON:
            return DBL_MAX
        with np.errstate(all="ignore"):
            d = tc.project(model, prm, q, t, X)[0] - xy[idx]
        return float(d @ d)

    def corrs(self, image_id, idx):
        return self.graph.direct(image_id, idx)

    def complete(self, ids=None):
        o, total = self.o, 0
        max2 = o["complete_max_reproj_error"] ** 2
        for pid in sorted(set(self.points) if ids is None else set(ids)):
            if pid not in self.points:
                continue
            P = self.points[pid]
            queue = list(P[3])
            for t in range(o["complete_max_transitivity"]):
                if not queue:
                    break
                nxt = []
                for ref_obs in queue:
                    for (j, a) in self.corrs(*ref_obs):
                        if j not in self.images or self.images[j][4][a] != NO_POINT:
                            continue
                        if tc.bogus(self.cameras[self.images[j][0]], o):
                            continue
                        if self.error(j, a, P[0]) > max2:
                            continue
                        P[3].append((j, a))
                        self.images[j][4][a] = pid
                        self.modified.add(pid)
                        total += 1
                        if t < o["complete_max_transitivity"] - 1:
                            nxt.append((j, a))
                queue = nxt
        return total

    def merge(self, ids=None):
        max2 = self.o["merge_max_reproj_error"] ** 2
        total = 0
        for pid in sorted(set(self.points) if ids is None else set(ids)):
            if pid not in self.points:
                continue
            current, ret, merged = pid, 0, True
            tried = set()
            while merged:
                merged = False
                for obs in list(self.points[current][3]):
                    for (j, a) in self.corrs(*obs):
                        q = int(self.images[j][4][a]) if j in self.images else NO_POINT
                        if q == NO_POINT or q == current or (current, q) in tried:
                            continue
                        tried.add((current, q))
                        A, B = self.points[current], self.points[q]
                        n1, n2 = len(A[3]), len(B[3])
                        X = (float(n1) * A[0] + float(n2) * B[0]) / float(n1 + n2)
                        if any(self.error(i, k, X) > max2 for i, k in A[3] + B[3]):
                            continue
                        new = max(self.points) + 1
                        rgb = tuple(int((float(n1) * A[1][c] + float(n2) * B[1][c]) / float(n1 + n2)) for c in range(3))
                        self.points[new] = [X, rgb, -1.0, A[3] + B[3]]
                        for i, k in A[3] + B[3]:
                            self.images[i][4][k] = new
                        del self.points[current], self.points[q]
                        self.modified -= {current, q}
                        self.modified.add(new)
                        current, ret, merged = new, n1 + n2, True
                        break
                    if merged:
                        break
            total += ret
        return total

    def state_points(self):
        return {pid: (p[0], p[1], p[2], p[3]) for pid, p in sorted(self.points.items())}


# ---- hand-built worlds with exact pixels -----------------------------------------------------------------------------------
def world(nimg, phys, views, tracks, edges=None, offsets=None, extra=None, bogus_images=(), nan_pixels=()):
    """A state built by hand.  phys: physical points (P, 3); views {p: [image ids]}: physical point p has one point2D in
    each of these images, at its exact projection plus offsets[(p, image)]; edges {p: [(image, image)]}: the
    correspondences among p's points2D (default: all pairs of its views, in lexicographic order); tracks: [(xyz, [(p,
    image)])]: the model's points 1, 2, ..; extra: [((p1, image1), (p2, image2))] further correspondences; bogus_images
    use camera 2, whose focal length is bogus; nan_pixels: (p, image) whose pixel is NaN.  Model 0 (SIMPLE_PINHOLE)."""
    prm = ba_cases.model_params(0)
    bad = prm.copy()
    bad[0] = 0.01 * tc.WIDTH
    cameras = {1: (0, tc.WIDTH, tc.HEIGHT, prm), 2: (0, tc.WIDTH, tc.HEIGHT, bad)}
    poses = tc.ring(nimg, seed=77)
    phys = np.asarray(phys, np.float64).reshape(-1, 3)
    index, per_image = {}, {i + 1: [] for i in range(nimg)}
    for p in sorted(views):
        for i in views[p]:
            q, t = poses[i - 1]
            xy = tc.project(0, prm, q, t, phys[p])[0] + np.asarray((offsets or {}).get((p, i), (0.0, 0.0)))
            if (p, i) in nan_pixels:
                xy = np.array([np.nan, xy[1]])
            index[(p, i)] = len(per_image[i])
            per_image[i].append(xy)
    images = {i: (2 if i in bogus_images else 1, poses[i - 1][0], poses[i - 1][1], np.array(per_image[i]).reshape(-1, 2),
                  np.full(len(per_image[i]), NO_POINT, np.uint64)) for i in per_image}
    matches = []
    for p in sorted(views):
        es = (edges or {}).get(p)
        if es is None:
            es = [(a, b) for k, a in enumerate(views[p]) for b in views[p][k + 1:]]
        for a, b in es:
            matches.append((a, b, np.array([[index[(p, a)], index[(p, b)]]], np.uint32)))
    for (p1, i1), (p2, i2) in extra or []:
        matches.append((i1, i2, np.array([[index[(p1, i1)], index[(p2, i2)]]], np.uint32)))
    points = {}
    for n, (xyz, obs) in enumerate(tracks):
        pid = n + 1
        track = [(i, index[(p, i)]) for p, i in obs]
        for i, k in track:
            images[i][4][k] = pid
        points[pid] = (np.asarray(xyz, np.float64), colour(pid), 0.0, track)
    st = dict(cameras=cameras, images=images, points=points, graph_images={i: len(per_image[i]) for i in per_image}, matches=matches)
    st["index"] = index
    return st


# ---- flat problems of Context.complete_tracks ----------------------------------------------------------------------------------
def _cameras_and_images(models, nimg, seed):
    prm = [ba_cases.model_params(m) for m in models]
    poses = tc.ring(nimg, seed=seed)
    icam = np.arange(nimg, dtype=np.uint32) % len(models)
    q = np.array([p[0] for p in poses])
    t = np.array([p[1] for p in poses])
    return list(models), prm, icam, q, t


def complete_problem(seed=0, sizes=(4,), models=(2,), nimg=12, special=None):
    """items of the given numbers of candidates: a point in the unit cube, candidates in random images at the projection
    plus noise of 0.5, 3 or 30 pixels, so that about a third fails a threshold of 4"""
    rng = np.random.default_rng(seed)
    models, prm, icam, q, t = _cameras_and_images(models, nimg, seed)
    X = rng.uniform(-1, 1, (len(sizes), 3))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ci, xy = [], []
    for i, n in enumerate(sizes):
        for _ in range(n):
            im = int(rng.integers(nimg))
            c = icam[im]
            ci.append(im)
            xy.append(tc.project(models[c], prm[c], q[im], t[im], X[i])[0] + rng.normal(0, rng.choice([0.5, 3.0, 30.0]), 2))
    ci, xy = np.array(ci, np.uint32), np.array(xy, np.float64).reshape(-1, 2)
    if special == "nonfinite" and len(ci) >= 8:
        xy[0, 0], xy[1, 1], xy[2] = np.nan, np.inf, (-np.inf, np.nan)
        q = q.copy()
        t = t.copy()
        X = X.copy()
        q[ci[3], 0], t[ci[4], 2], q[ci[5]] = np.nan, np.inf, 0.0
        X[len(sizes) - 1] = (np.nan, 0.0, np.inf)
        X[0] = -3.0 * X[0] + 20.0 * np.array([np.cos(0.0), np.sin(0.0), 0.0])  # behind some cameras
    return (models, prm, icam, q, t, X, off, ci, xy), {}


def threshold_problem():
    """one item on the optical axis of an identity pose: errors exactly 25, 25 at a threshold one double below 5, and a
    pixel one double further away"""
    prm = ba_cases.model_params(0)
    cx, cy = prm[1], prm[2]
    q, t = np.array([[0.0, 0.0, 0.0, 1.0]]), np.zeros((1, 3))
    X = np.array([[0.0, 0.0, 5.0], [0.0, 0.0, -5.0]])
    xy = np.array([[cx + 3.0, cy + 4.0], [cx + 3.0, np.nextafter(cy + 4.0, np.inf)], [cx - 3.0, cy - 4.0], [cx, cy]])
    return ([0], [prm], np.zeros(1, np.uint32), q, t, X, np.array([0, 3, 4], np.uint64), np.zeros(4, np.uint32), xy), {"complete_max_reproj_error": 5.0}


COMPLETE_CASES = {
    "c/items_0": lambda: complete_problem(1, ()),
    "c/item_of_1": lambda: complete_problem(2, (1,)),
    "c/sizes": lambda: complete_problem(3, (1, 63, 64, 65, 0, 7)),
    "c/items_257": lambda: complete_problem(4, (3,) * 257),
    "c/all_models": lambda: complete_problem(5, (9,) * 33, models=tuple(range(11)), nimg=22),
    "c/nonfinite": lambda: complete_problem(6, (8, 8, 8), special="nonfinite"),
    "c/threshold": threshold_problem,
    **{f"c/model_{m}": (lambda m=m: complete_problem(10 + m, (5, 70), models=(m,))) for m in range(11)},
}
COMPLETE_KEYS = ("cand_sq_error", "cand_pass")


# ---- flat problems of Context.merge_tracks ------------------------------------------------------------------------------------
def merge_problem(seed=0, comps=((2, 2),), models=(2,), nimg=12, spread=1e-3, outlier=0.0, roots="all", shuffle=False):
    """components (k points, n observations each): a physical point, the k points within `spread` of it, every
    observation in a random image at the physical point's projection plus 0.3 pixels of noise (with probability `outlier`
    plus 30 pixels), point j linked to point j + 1 through their first observations and to a random other point through
    random ones, symmetrically.  roots: "all", or "even" for every second point."""
    rng = np.random.default_rng(seed)
    models, prm, icam, q, t = _cameras_and_images(models, nimg, seed)
    cpo, cro, rt, X, poo, oi, xy, corr = [0], [0], [], [], [0], [], [], []
    for k, n in comps:
        phys = rng.uniform(-1, 1, 3)
        first_point, first_obs = len(X), len(oi)
        for j in range(k):
            X.append(phys + rng.normal(0, spread, 3))
            if roots == "all" or j % 2 == 0:
                rt.append(first_point + j)
            for _ in range(n):
                im = int(rng.integers(nimg))
                c = icam[im]
                noise = rng.normal(0, 0.3, 2) + (rng.normal(0, 30.0, 2) if rng.random() < outlier else 0.0)
                oi.append(im)
                xy.append(tc.project(models[c], prm[c], q[im], t[im], phys)[0] + noise)
                corr.append([])
            poo.append(len(oi))
        for j in range(k - 1):
            a, b = first_obs + j * n, first_obs + (j + 1) * n
            corr[a].append(b)
            corr[b].append(a)
            if k > 2:
                o = int(rng.integers(k))
                if o != j:
                    a, b = first_obs + j * n + int(rng.integers(n)), first_obs + o * n + int(rng.integers(n))
                    corr[a].append(b)
                    corr[b].append(a)
        if shuffle:
            for lst in corr[first_obs:]:
                rng.shuffle(lst)
        cpo.append(len(X))
        cro.append(len(rt))
    oco = np.concatenate([[0], np.cumsum([len(c) for c in corr])]).astype(np.uint64)
    co = np.array([v for c in corr for v in c], np.uint32)
    return (models, prm, icam, q, t, np.array(cpo, np.uint64), np.array(cro, np.uint64), np.array(rt, np.uint32),
            np.array(X, np.float64).reshape(-1, 3), np.array(poo, np.uint64), np.array(oi, np.uint32),
            np.array(xy, np.float64).reshape(-1, 2), oco, co), {}


MERGE_CASES = {
    "m/comps_0": lambda: merge_problem(1, ()),
    "m/comps_1": lambda: merge_problem(2, ((2, 2),)),
    "m/comps_63": lambda: merge_problem(3, ((2, 2),) * 63, outlier=0.1),
    "m/comps_64": lambda: merge_problem(4, ((2, 2),) * 64, outlier=0.1),
    "m/comps_65": lambda: merge_problem(5, ((2, 2),) * 65, outlier=0.1),
    "m/comps_257": lambda: merge_problem(6, ((2, 2),) * 257, outlier=0.1),
    "m/chain_5": lambda: merge_problem(7, ((6, 3),)),
    "m/mixed": lambda: merge_problem(8, ((7, 5), (2, 2), (12, 3), (1, 4), (3, 9), (5, 2)) * 6, outlier=0.08, shuffle=True),
    "m/roots_even": lambda: merge_problem(9, ((7, 4), (4, 3), (9, 2)) * 5, outlier=0.05, roots="even", shuffle=True),
    "m/far_apart": lambda: merge_problem(10, ((4, 3),) * 8, spread=0.3),
    "m/all_models": lambda: merge_problem(11, ((4, 4),) * 22, models=tuple(range(11)), nimg=22, outlier=0.05),
    "m/obs_4096": lambda: merge_problem(12, ((64, 64), (2, 2)), outlier=0.01, shuffle=True),
}
MERGE_KEYS = ("root_return", "root_merge_offsets", "merge_current", "merge_other", "merge_xyz")
ALL_CASES = {**COMPLETE_CASES, **MERGE_CASES}
_case_cache, _ref_cache = {}, {}


def case_call(name):
    if name not in _case_cache:
        _case_cache[name] = ALL_CASES[name]()
    return _case_cache[name]


def reference(name):
    if name not in _ref_cache:
        args, kw = case_call(name)
        _ref_cache[name] = (ref.complete_tracks if name.startswith("c/") else ref.merge_tracks)(*args, **kw)
    return _ref_cache[name]


def same(name, got, want) -> bool:
    if name.startswith("c/"):
        return (np.array_equal(bits(got["cand_sq_error"]), bits(want["cand_sq_error"])) and
                np.array_equal(np.asarray(got["cand_pass"], bool), np.asarray(want["cand_pass"], bool)) and got["num_passed"] == want["num_passed"])
    return (all(np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)) for k in MERGE_KEYS[:4]) and
            np.array_equal(bits(got["merge_xyz"]), bits(want["merge_xyz"])) and got["num_merges"] == want["num_merges"])


def digest(name, result) -> str:
    h = hashlib.sha256()
    if name.startswith("c/"):
        h.update(bits(result["cand_sq_error"]).tobytes())
        h.update(np.ascontiguousarray(result["cand_pass"], np.uint8).tobytes())
    else:
        h.update(np.ascontiguousarray(result["root_return"], np.uint32).tobytes())
        h.update(np.ascontiguousarray(result["root_merge_offsets"], np.uint64).tobytes())
        h.update(np.ascontiguousarray(result["merge_current"], np.uint32).tobytes())
        h.update(np.ascontiguousarray(result["merge_other"], np.uint32).tobytes())
        h.update(bits(result["merge_xyz"]).tobytes())
    return h.hexdigest()


# ---- whole scenes through the sequential reference (18.6) --------------------------------------------------------------------
# name: (scene of triangulator_cases, seed of the perturbation, options)
SCENES = {
    "direct": ("direct", 1, {}),
    "transitive_2": ("transitive_2", 2, dict(complete_max_transitivity=2)),
    "all_models": ("all_models", 3, {}),
    "bogus_camera": ("bogus_camera", 4, dict(complete_max_reproj_error=6.0, merge_max_reproj_error=6.0)),
    "two_view_off": ("two_view_off", 5, dict(complete_max_transitivity=1, merge_max_reproj_error=2.5)),
}
_state_cache, _scene_ref_cache = {}, {}


def scene_state(name):
    if name not in _state_cache:
        base, seed, opts = SCENES[name]
        _state_cache[name] = (perturbed(triangulated_state(base), seed), opts)
    return _state_cache[name]


def subset_ids(st):
    """every third id, a few that do not exist, one twice"""
    ids = sorted(st["points"])
    return ids[::3] + [max(ids) + 5, 10 ** 9, ids[0]]


def scene_reference(name, op, ids="all"):
    """the sequential reference on the scene's state.  op: "complete", "merge" or "both" (complete, then merge, the
    mapper's order); ids: "all" or "subset".  Returns (counts, points, point2D ids, modified, smallest margin)."""
    key = (name, op, ids)
    if key not in _scene_ref_cache:
        st, opts = scene_state(name)
        rs = ref_scene(st)
        listed = None if ids == "all" else subset_ids(st)
        counts = []
        if op in ("complete", "both"):
            counts.append(rs.complete(listed, **opts))
        if op in ("merge", "both"):
            counts.append(rs.merge(listed, **opts))
        _scene_ref_cache[key] = (counts, rs.points(), rs.point2D_ids(), rs.modified(), rs.min_margin())
    return _scene_ref_cache[key]
