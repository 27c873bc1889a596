"""Deterministic synthetic inputs of retriangulate for tests/test_retriangulate_cpu.py,
tests/test_retriangulate_gpu.py and tests/golden/make_retri_ref_golden.py: flat problems of Context.retriangulate_pairs
for the shapes at which the kernels can go wrong; the scenes of tests/triangulator_cases.py after the reference's
triangulate_image with tracks cut so that pairs fall under re_min_ratio; hand-built worlds with exact pixels for the
answers worked out by hand; an independent Python restatement of 19.2 on the flat problem; a brute-force restatement of
19.3's colouring; and the lists the fixture freezes."""
from __future__ import annotations

import copy
import hashlib

import numpy as np

import ba_cases
import retri_ref_lib as ref
import tracks_cases as trc
import triangulator_cases as tc

NO_POINT = ref.NO_POINT
DEG = tc.DEG
bits = tc.bits
ARG_NAMES = ("camera_models", "camera_params", "image_cameras", "qvec", "tvec", "obs_image", "obs_xy", "obs_point", "point_xyz",
             "pair_images", "pair_offsets", "corr_obs", "round_offsets")
OPT_NAMES = ("create_max_angle_error", "re_max_angle_error", "min_angle", "re_min_ratio")
RESULT_KEYS = ("pair_ran", "pair_num_tri", "corr_action", "created_offsets", "created_xyz")


# ---- flat problems ---------------------------------------------------------------------------------------------------------
def flat_problem(seed=0, rounds=(((0, 1, 8),),), models=(2,), nimg=None, noise=0.3, p_one=0.3, p_same=0.1, p_diff=0.1,
                 p_out=0.1, p_share=0.0, p_two_view=0.0):
    """A flat problem: `rounds` lists per round the pairs (image a, image b, correspondences).  Every correspondence plants
    a point and observes it in both images (a random pixel with probability p_out); with probability p_share its first
    observation is instead one that an earlier round made in image a, so that rounds depend on one another.  A fresh
    correspondence has one point on both observations (p_same), two different points (p_diff), a point on one side
    (p_one) or none.  Returns (args in ARG_NAMES order, keywords)."""
    rng = np.random.default_rng(seed)
    if nimg is None:
        nimg = 1 + max([max(a, b) for r in rounds for a, b, _ in r] + [1])
    poses = tc.ring(nimg, seed=seed)
    cams = [(int(m), ba_cases.model_params(m)) for m in models]
    icam = np.arange(nimg) % len(models)
    oi, xy, op, planted, X = [], [], [], [], []
    earlier = {i: [] for i in range(nimg)}  # observations of earlier rounds per image
    pimg, poff, co, two, roff = [], [0], [], [], [0]

    def observe(i, P, outlier):
        m, prm = cams[icam[i]]
        pix = rng.uniform([50, 50], [tc.WIDTH - 50, tc.HEIGHT - 50]) if outlier else tc.project(m, prm, *poses[i], P)[0] + rng.normal(0, noise, 2)
        oi.append(i)
        xy.append(pix)
        op.append(-1)
        planted.append(P)
        return len(oi) - 1

    def point(P):
        X.append(P + rng.normal(0, 1e-3, 3))
        return len(X) - 1

    for r in rounds:
        made = {i: [] for i in range(nimg)}
        for a, b, n in r:
            used = set()
            for _ in range(n):
                free = [o for o in earlier[a] if o not in used]
                if free and rng.random() < p_share:
                    o1 = free[int(rng.integers(len(free)))]
                    P = planted[o1]
                    o2 = observe(b, P, False)
                else:
                    P = rng.uniform(-1.0, 1.0, 3)
                    o1 = observe(a, P, rng.random() < p_out)
                    o2 = observe(b, P, rng.random() < p_out)
                    made[a].append(o1)
                    u = rng.random()
                    if u < p_same:
                        op[o1] = op[o2] = point(P)
                    elif u < p_same + p_diff:
                        op[o1], op[o2] = point(P), point(P)
                    elif u < p_same + p_diff + p_one:
                        if rng.random() < 0.5:
                            op[o1] = point(P)
                        else:
                            op[o2] = point(P)
                used.add(o1)
                made[b].append(o2)
                co.append((o1, o2))
                two.append(rng.random() < p_two_view)
            pimg.append((a, b))
            poff.append(len(co))
        for i in made:
            earlier[i] += made[i]
        roff.append(len(pimg))
    args = [[c[0] for c in cams], [c[1] for c in cams], icam.astype(np.uint32), np.array([p[0] for p in poses]),
            np.array([p[1] for p in poses]), np.array(oi, np.uint32), np.array(xy, np.float64).reshape(-1, 2),
            np.array(op, np.int32), np.array(X, np.float64).reshape(-1, 3), np.array(pimg, np.uint32).reshape(-1, 2),
            np.array(poff, np.uint64), np.array(co, np.uint32).reshape(-1, 2), np.array(roff, np.uint64)]
    return args, dict(corr_two_view=np.array(two, np.uint8))


def _one_corr(seed, model=1):
    """one pair of images 0 and 1 with one exact correspondence and one point (index 0) at the planted position"""
    args, kw = flat_problem(seed=seed, rounds=(((0, 1, 1),),), models=(model,), nimg=6, noise=0.0, p_one=0.0, p_same=0.0,
                            p_diff=0.0, p_out=0.0)
    return args, kw


def _threshold_problem(above):
    """one correspondence whose Continue angle A is exactly DegToRad(re_max_angle_error) (above = False), or one double
    above it: observation 2's pixel is moved until some option value e has DegToRad(e) == A in doubles"""
    args, kw = _one_corr(31)
    X = np.array([0.1, -0.2, 0.3])
    args[8] = X.reshape(1, 3)
    args[7][:] = [0, -1]
    m, prm = args[0][0], args[1][0]
    pix0 = tc.project(m, prm, args[3][1], args[4][1], X)[0]
    for k in range(256):
        pix = pix0 + [40.0 + k, 0.0]
        A = ref.tref.angular_error(ref.lift(m, prm, [pix])[0], args[3][1], args[4][1], X)
        hits = [v for v in tc._neighbours(A / DEG, 4) if DEG * v == A]
        if hits:
            break
    else:
        raise AssertionError("no pixel whose angle is a representable threshold")
    args[6][1] = pix
    thr = hits[0]
    if above:
        while DEG * thr >= A:
            thr = np.nextafter(thr, 0.0)
        assert np.nextafter(DEG * thr, 1.0) == A
    return args, dict(kw, re_max_angle_error=float(thr))


def _special(what):
    args, kw = flat_problem(seed=42, rounds=(((0, 1, 9), (2, 3, 7)), ((1, 2, 8),)), models=(2, 4), p_one=0.4, p_out=0.0, p_share=0.4)
    if what == "behind":  # image 1 looks away from everything it observes
        args[3][1] = args[3][1] * np.array([1.0, 1.0, 1.0, -1.0])
    elif what == "nan_pixel":
        args[6][1] = [np.nan, 100.0]
        args[6][20] = [np.inf, 100.0]
    elif what == "nan_pose":
        args[4][0] = [np.nan, 0.0, 1.0]
        args[3][3] = [np.inf, 0.0, 0.0, 1.0]
    elif what == "nan_point":
        args[8][0] = [np.nan, 0.0, 0.0]
        args[8][2] = [np.inf, 0.0, 0.0]
    return args, kw


def _between_thresholds():
    """one correspondence without points whose two rays miss one another by about 7 degrees: each observation's error
    under the triangulated point is about 3.5 degrees, between create_max_angle_error 2 and re_max_angle_error 5"""
    args, kw = _one_corr(33, model=0)
    f = args[1][0][0]
    args[6][1] = args[6][1] + [0.0, f * np.tan(7.0 * DEG)]  # across the (nearly horizontal) epipolar line
    return args, kw


def _ratio_fifth():
    """a pair of five correspondences of which exactly one carries a common point: tri_ratio is 1 / 5"""
    args, kw = flat_problem(seed=34, rounds=(((0, 1, 5),),), nimg=6, p_one=0.0, p_same=0.0, p_diff=0.0, p_out=0.0)
    args[8] = np.array([[0.0, 0.1, 0.2]])
    args[7][0:2] = 0  # the first correspondence's two observations
    return args, kw


def _filled_by_earlier_rounds(seen_by_image_0):
    """Rounds (0, 1), (0, 2), (1, 2) on six planted points that images 1 and 2 all see, without points there; image 0
    sees the first `seen_by_image_0` of them and carries their points.  The first two rounds continue those points into
    images 1 and 2, so pair (1, 2), whose num_tri_corrs is 0 on the uploaded state, has `seen_by_image_0` of 6 when its
    round comes: with all six it is no longer under-reconstructed and must not run; with one it runs, at 1 / 6, and
    creates the other five."""
    n, m = 6, seen_by_image_0
    rng = np.random.default_rng(50 + m)
    poses = tc.ring(6, seed=50)
    prm = ba_cases.model_params(2)
    P = rng.uniform(-0.8, 0.8, (n, 3))
    oi, xy, op = [], [], []
    obs = {}
    for i, pts in ((0, range(m)), (1, range(n)), (2, range(n))):
        for p in pts:
            obs[(i, p)] = len(oi)
            oi.append(i)
            xy.append(tc.project(2, prm, *poses[i], P[p])[0] + rng.normal(0, 0.3, 2))
            op.append(p if i == 0 else -1)
    co = [(obs[(0, p)], obs[(1, p)]) for p in range(m)] + [(obs[(0, p)], obs[(2, p)]) for p in range(m)] + \
         [(obs[(1, p)], obs[(2, p)]) for p in range(n)]
    args = [[2], [prm], np.zeros(6, np.uint32), np.array([q for q, _ in poses]), np.array([t for _, t in poses]),
            np.array(oi, np.uint32), np.array(xy), np.array(op, np.int32), P[:m] + rng.normal(0, 1e-3, (m, 3)),
            np.array([[0, 1], [0, 2], [1, 2]], np.uint32), np.array([0, m, 2 * m, 2 * m + n], np.uint64),
            np.array(co, np.uint32), np.array([0, 1, 2, 3], np.uint64)]
    return args, dict(corr_two_view=np.zeros(len(co), np.uint8))


def initial_num_tri(args):
    """num_tri_corrs of every pair on the uploaded state, before any round"""
    op, poff, co = np.asarray(args[7], np.int64), [int(v) for v in args[10]], np.asarray(args[11]).reshape(-1, 2)
    return [sum(1 for k in range(poff[p], poff[p + 1]) if op[co[k][0]] >= 0 and op[co[k][0]] == op[co[k][1]])
            for p in range(len(poff) - 1)]


_R65 = tuple(((r % 7, (r + 1) % 7, (3, 4, 6, 7)[r % 4]),) for r in range(65))
# name: (builder, keyword options)
CASES = {
    "mixed": (lambda: flat_problem(seed=1, rounds=(((0, 1, 40), (2, 3, 25)), ((0, 2, 30), (1, 3, 20)), ((0, 3, 15),)),
                                   models=(2, 1), p_share=0.4, p_two_view=0.1), {}),
    "sparse": (lambda: flat_problem(seed=2, rounds=(((0, 1, 30),), ((1, 2, 30),), ((2, 0, 30),)), p_one=0.1, p_same=0.0, p_diff=0.0,
                                    p_share=0.6, p_out=0.0), {}),
}
EDGE_CASES = {
    "sizes": (lambda: flat_problem(seed=3, rounds=(((0, 1, 0), (2, 3, 1), (4, 5, 63), (6, 7, 64), (8, 9, 65), (10, 11, 257)),),
                                   models=(2, 1)), {}),
    "rounds_0": (lambda: flat_problem(seed=4, rounds=()), {}),
    "rounds_1": (lambda: flat_problem(seed=4, rounds=(((0, 1, 12),),)), {}),
    "rounds_2": (lambda: flat_problem(seed=5, rounds=(((0, 1, 12),), ((1, 2, 12),)), p_share=0.5), {}),
    "rounds_65": (lambda: flat_problem(seed=6, rounds=_R65, nimg=7, p_share=0.5), {}),
    "pairs_0": (lambda: flat_problem(seed=7, rounds=((), ((0, 1, 7),), ())), {}),
    "pairs_257": (lambda: flat_problem(seed=8, rounds=(tuple((2 * k, 2 * k + 1, k % 3) for k in range(257)),), p_one=0.4), {}),
    "all_models": (lambda: flat_problem(seed=9, rounds=(tuple((2 * k, 2 * k + 1, 9) for k in range(11)), tuple((2 * k + 1, 2 * k + 2, 9) for k in range(10))),
                                        models=tuple(range(11)), nimg=22, p_share=0.4), {}),
    "continue_at_threshold": (lambda: _threshold_problem(False), {}),
    "continue_above_threshold": (lambda: _threshold_problem(True), {}),
    "behind": (lambda: _special("behind"), {}),
    "nan_pixel": (lambda: _special("nan_pixel"), {}),
    "nan_pose": (lambda: _special("nan_pose"), {}),
    "nan_point": (lambda: _special("nan_point"), {}),
    "between_thresholds": (_between_thresholds, {}),
    "between_thresholds_wide": (_between_thresholds, dict(create_max_angle_error=5.0)),
    "ratio_fifth_skipped": (_ratio_fifth, dict(re_min_ratio=0.2)),
    "ratio_fifth_runs": (_ratio_fifth, dict(re_min_ratio=float(np.nextafter(0.2, 1.0)))),
    "two_view_all": (lambda: flat_problem(seed=12, rounds=(((0, 1, 6),),), p_one=0.3, p_out=0.0, p_two_view=1.0), {}),
    "min_angle_180": (lambda: flat_problem(seed=14, rounds=(((0, 1, 6),),), p_out=0.0), dict(min_angle=180.0)),
    "filled_pair_skipped": (lambda: _filled_by_earlier_rounds(6), {}),
    "filled_pair_runs": (lambda: _filled_by_earlier_rounds(1), {}),
    "ratio_0": (lambda: flat_problem(seed=15, rounds=(((0, 1, 6),),), p_same=0.0), dict(re_min_ratio=0.0)),
}
for _m in range(11):
    EDGE_CASES[f"model_{tc.MODEL_NAMES[_m]}"] = ((lambda m=_m: flat_problem(seed=20 + m, rounds=(((0, 1, 9),), ((1, 2, 9),)), models=(m,),
                                                                              p_share=0.4)), {})
ALL_CASES = {**CASES, **EDGE_CASES}
_cache, _ref_cache = {}, {}


def case_call(name):
    """(positional arguments, keywords) of retriangulate_pairs; built once, read-only"""
    if name not in _cache:
        builder, opts = ALL_CASES[name]
        args, kw = builder()
        for a in list(args) + list(kw.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = (tuple(args), {**kw, **opts})
    return _cache[name]


def reference(name):
    if name not in _ref_cache:
        args, kw = case_call(name)
        _ref_cache[name] = ref.retriangulate_pairs(*args, **kw)
    return _ref_cache[name]


def same(a, b) -> bool:
    return (np.array_equal(np.asarray(a["pair_ran"], bool), np.asarray(b["pair_ran"], bool)) and
            np.array_equal(a["pair_num_tri"], b["pair_num_tri"]) and np.array_equal(a["corr_action"], b["corr_action"]) and
            np.array_equal(np.asarray(a["created_offsets"], np.uint64), np.asarray(b["created_offsets"], np.uint64)) and
            np.array_equal(bits(a["created_xyz"]), bits(b["created_xyz"])))


def digest(result) -> str:
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(result["pair_ran"], np.uint8).tobytes())
    h.update(np.ascontiguousarray(result["pair_num_tri"], np.uint32).tobytes())
    h.update(np.ascontiguousarray(result["corr_action"], np.uint8).tobytes())
    h.update(np.ascontiguousarray(result["created_offsets"], np.uint64).tobytes())
    h.update(bits(result["created_xyz"]).tobytes())
    return h.hexdigest()


# ---- 19.2 restated independently on the flat problem: numpy for the angle and the ratio, tests/tri_ref for the RANSAC -------
def py_retriangulate_pairs(args, kw):
    import tri_ref_lib
    a = dict(zip(ARG_NAMES, args))
    o = dict(create_max_angle_error=2.0, re_max_angle_error=5.0, min_angle=1.5, re_min_ratio=0.2)
    o.update({k: v for k, v in kw.items() if k in o})
    two = kw.get("corr_two_view")
    icam, oi = np.asarray(a["image_cameras"]), np.asarray(a["obs_image"])
    nxy = np.zeros((len(oi), 2))
    for k in range(len(oi)):
        c = icam[oi[k]]
        nxy[k] = ref.lift(a["camera_models"][c], a["camera_params"][c], [a["obs_xy"][k]])[0]
    P = [tc.pose_matrix(q, t) for q, t in zip(a["qvec"], a["tvec"])]
    point = [int(v) for v in a["obs_point"]]
    xyz = {i: np.array(x) for i, x in enumerate(np.asarray(a["point_xyz"]).reshape(-1, 3))}
    npoints = len(xyz)
    poff, roff, co = [int(v) for v in a["pair_offsets"]], [int(v) for v in a["round_offsets"]], np.asarray(a["corr_obs"]).reshape(-1, 2)
    ran, ntri, act, made = [], [], np.zeros(len(co), np.uint8), []
    with np.errstate(all="ignore"):
        for r in range(len(roff) - 1):
            before = list(point)  # the model as it stood before the round (19.3)
            updates = []
            for p in range(roff[r], roff[r + 1]):
                ks = range(poff[p], poff[p + 1])
                n = sum(1 for k in ks if before[co[k][0]] >= 0 and before[co[k][0]] == before[co[k][1]])
                ntri.append(n)
                ratio = np.float64(n) / np.float64(len(ks)) if len(ks) else np.nan
                ran.append(not ratio >= o["re_min_ratio"])
                if not ran[-1]:
                    continue
                for k in ks:
                    o1, o2 = int(co[k][0]), int(co[k][1])
                    s1, s2 = before[o1], before[o2]
                    if s1 >= 0 and s2 >= 0:
                        continue
                    if s1 >= 0 or s2 >= 0:
                        refo, slot = (o2, s1) if s1 >= 0 else (o1, s2)
                        e = tc.np_angular_error(nxy[refo], P[oi[refo]], xyz[slot])
                        if e <= DEG * o["re_max_angle_error"]:
                            updates.append((refo, slot))
                            act[k] = ref.CONTINUE_1TO2 if s1 >= 0 else ref.CONTINUE_2TO1
                        continue
                    if two is not None and two[k]:
                        continue
                    X, ok, mask, _ = tri_ref_lib.triangulate(
                        np.array([P[oi[o1]].reshape(-1), P[oi[o2]].reshape(-1)]), [0, 2], [0, 1], [nxy[o1], nxy[o2]],
                        min_tri_angle=DEG * o["min_angle"], max_error=DEG * o["create_max_angle_error"], min_inlier_ratio=0.02,
                        confidence=0.9999, dyn_num_trials_multiplier=3.0, max_num_trials=10000, min_num_trials=1)
                    if ok[0] and mask[0] and mask[1]:
                        xyz[npoints + k] = X[0].copy()
                        updates += [(o1, npoints + k), (o2, npoints + k)]
                        act[k] = ref.CREATED
            for obs, slot in updates:
                point[obs] = slot
    made = [xyz[npoints + k] for k in range(len(co)) if act[k] == ref.CREATED]
    per_pair = [int((act[poff[p]:poff[p + 1]] == ref.CREATED).sum()) for p in range(len(poff) - 1)]
    return dict(pair_ran=np.array(ran, bool), pair_num_tri=np.array(ntri, np.uint32), corr_action=act,
                created_offsets=np.concatenate([[0], np.cumsum(per_pair)]).astype(np.uint64),
                created_xyz=np.array(made, np.float64).reshape(-1, 3))


# ---- 19.3 restated by brute force --------------------------------------------------------------------------------------------
def brute_colour(pairs):
    """every pair, in order, into the lowest round none of whose earlier pairs shares an image with it"""
    rounds = []
    for i, (a, b) in enumerate(pairs):
        r = 0
        while any(rounds[j] == r and {a, b} & set(pairs[j]) for j in range(i)):
            r += 1
        rounds.append(r)
    return rounds


# ---- the equivalent item of Context.triangulate_observations (19.5) ------------------------------------------------------------
def equivalent_items(args, kw, result):
    """Replays the result round by round and builds, for every correspondence of a pair that ran and that does not carry
    two points, its two-candidate item on the state at the start of its round: [the observation with a point or
    observation 1, the reference observation or observation 2].  Returns (arguments and keywords of
    triangulate_observations, per item the expected (continued, created position or None))."""
    a = dict(zip(ARG_NAMES, args))
    o = dict(create_max_angle_error=2.0, re_max_angle_error=5.0, min_angle=1.5)
    o.update({k: v for k, v in kw.items() if k in o})
    two = kw.get("corr_two_view")
    point = [int(v) for v in a["obs_point"]]
    X = [np.array(x) for x in np.asarray(a["point_xyz"]).reshape(-1, 3)]
    npoints = len(X)
    poff, roff, co = [int(v) for v in a["pair_offsets"]], [int(v) for v in a["round_offsets"]], np.asarray(a["corr_obs"]).reshape(-1, 2)
    xyz = dict(enumerate(X))
    created = iter(np.asarray(result["created_xyz"]).reshape(-1, 3))
    off, ci, cxy, has, cX, flags, want = [0], [], [], [], [], [], []
    for r in range(len(roff) - 1):
        before = list(point)
        for p in range(roff[r], roff[r + 1]):
            for k in range(poff[p], poff[p + 1]):
                act = int(result["corr_action"][k])
                pos = next(created) if act == ref.CREATED else None
                o1, o2 = int(co[k][0]), int(co[k][1])
                if not result["pair_ran"][p]:
                    assert act == ref.NONE
                    continue
                s1, s2 = before[o1], before[o2]
                if s1 >= 0 and s2 >= 0:
                    assert act == ref.NONE
                    continue
                first, second = (o2, o1) if (s2 >= 0 and s1 < 0) else (o1, o2)
                for ob in (first, second):
                    ci.append(int(a["obs_image"][ob]))
                    cxy.append(a["obs_xy"][ob])
                    has.append(before[ob] >= 0)
                    cX.append(xyz[before[ob]] if before[ob] >= 0 else np.zeros(3))
                off.append(len(ci))
                flags.append(bool(two is not None and two[k]))
                want.append((0 if act in (ref.CONTINUE_1TO2, ref.CONTINUE_2TO1) else -1, pos))
                if act == ref.CONTINUE_1TO2:
                    point[o2] = s1
                elif act == ref.CONTINUE_2TO1:
                    point[o1] = s2
                elif act == ref.CREATED:
                    xyz[npoints + k] = pos
                    point[o1] = point[o2] = npoints + k
    targs = (a["camera_models"], a["camera_params"], a["image_cameras"], a["qvec"], a["tvec"], np.array(off, np.uint64),
             np.array(ci, np.uint32), np.array(cxy, np.float64).reshape(-1, 2), np.array(has, np.uint8), np.array(cX, np.float64).reshape(-1, 3))
    tkw = dict(no_create_two_view=np.array(flags, np.uint8), create_max_angle_error=o["create_max_angle_error"],
               continue_max_angle_error=o["re_max_angle_error"], min_angle=o["min_angle"])
    return targs, tkw, want


def check_equivalent(want, got):
    """the items' results of triangulate_observations against the correspondences' outcomes, bit for bit"""
    n = len(want)
    assert len(got["continued"]) == n
    for i, (cont, pos) in enumerate(want):
        assert int(got["continued"][i]) == cont, i
        nr = int(got["round_offsets"][i + 1]) - int(got["round_offsets"][i])
        assert nr == (0 if pos is None else 1), i
        if pos is not None:
            assert np.array_equal(bits(got["round_xyz"][int(got["round_offsets"][i])]), bits(pos)), i
            assert list(got["cand_round"][2 * i:2 * i + 2]) == [1, 1], i


def permuted(args, kw, seed=0):
    """the same problem with the pairs shuffled inside their rounds; returns (args, kw, new pair -> old pair)"""
    rng = np.random.default_rng(seed)
    a = dict(zip(ARG_NAMES, args))
    poff, roff = [int(v) for v in a["pair_offsets"]], [int(v) for v in a["round_offsets"]]
    order = []
    for r in range(len(roff) - 1):
        order += [roff[r] + int(i) for i in rng.permutation(roff[r + 1] - roff[r])]
    co, two = np.asarray(a["corr_obs"]).reshape(-1, 2), kw.get("corr_two_view")
    new_co, new_two, new_off, corr_map = [], [], [0], []
    for p in order:
        ks = list(range(poff[p], poff[p + 1]))
        new_co += [co[k] for k in ks]
        corr_map += ks
        if two is not None:
            new_two += [two[k] for k in ks]
        new_off.append(len(new_co))
    b = dict(a, pair_images=np.asarray(a["pair_images"]).reshape(-1, 2)[order].reshape(-1, 2), pair_offsets=np.array(new_off, np.uint64),
             corr_obs=np.array(new_co, np.uint32).reshape(-1, 2))
    nkw = dict(kw)
    if two is not None:
        nkw["corr_two_view"] = np.array(new_two, np.uint8)
    return tuple(b[n] for n in ARG_NAMES), nkw, order, corr_map


# ---- scenes: triangulated, then cut -------------------------------------------------------------------------------------------
def cut_state(state, seed, delete=0.45, detach=0.35):
    """19.6: a share `delete` of the points is deleted with its whole track; every element of a remaining track beyond its
    second is detached with probability `detach`; the points are renumbered 1 .. N in their old order"""
    rng = np.random.default_rng(seed)
    st = copy.deepcopy(state)
    ids = {iid: im[4] for iid, im in st["images"].items()}
    kept = {}
    for pid in sorted(st["points"]):
        xyz, rgb, err, track = st["points"][pid]
        if rng.random() < delete:
            for e in track:
                ids[e[0]][e[1]] = NO_POINT
            continue
        keep = track[:2]
        for e in track[2:]:
            if rng.random() < detach:
                ids[e[0]][e[1]] = NO_POINT
            else:
                keep.append(e)
        new = len(kept) + 1
        for e in keep:
            ids[e[0]][e[1]] = new
        kept[new] = (xyz, trc.colour(new), err, keep)
    st["points"] = kept
    return st


SCENES = ("direct", "transitive_2", "all_models", "bogus_camera", "two_view_off")
_state_cache = {}


def scene_state(name):
    """(the cut state, retriangulate's options) of a scene of triangulator_cases"""
    if name not in _state_cache:
        opts = {k: v for k, v in tc.SCENES[name][1].items() if k != "max_transitivity"}
        _state_cache[name] = (cut_state(trc.triangulated_state(name), seed=100 + SCENES.index(name)), dict(opts, re_max_trials=2))
    return _state_cache[name]


def ref_scene(st, finalize=True):
    pts = {pid: (p[0], p[3]) for pid, p in st["points"].items()}
    return ref.Scene(st["cameras"], st["images"], pts, st["graph_images"], st["matches"], finalize=finalize)


_scene_ref_cache = {}


def scene_reference(name):
    """the sequential reference called twice on the cut scene: per call (count, points, point2D ids, modified, trials),
    and the margins after both"""
    if name not in _scene_ref_cache:
        st, opts = scene_state(name)
        rs = ref_scene(st)
        calls = []
        for _ in range(2):
            n = rs.retriangulate(**opts)
            calls.append((n, rs.points(), {i: rs.point2D_ids(i, len(im[3])) for i, im in st["images"].items()}, rs.modified(), rs.trials()))
        _scene_ref_cache[name] = (calls, rs.margins())
    return _scene_ref_cache[name]


def options(**kw):
    import pycolmap_amd as pc
    o = pc.IncrementalTriangulatorOptions()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def same_model(r, want_points, want_ids):
    """a Reconstruction against the reference's points {id: (xyz, error, track)} and point2D ids: positions bit for bit"""
    got = trc.recon_points(r)
    if list(got) != list(want_points):
        return False
    for pid, (xyz, err, track) in want_points.items():
        g = got[pid]
        if not (np.array_equal(bits(g[0]), bits(xyz)) and g[3] == track):
            return False
    return trc.same_point2D_ids(trc.recon_point2D_ids(r), want_ids)


def reference_solver(d):
    """the flat reference in the library's place for _retriangulate_with"""
    return ref.retriangulate_pairs(*[d[n] for n in ARG_NAMES], corr_two_view=d["corr_two_view"], **{n: d[n] for n in OPT_NAMES})


def state_digest(count, points, trials) -> str:
    h = hashlib.sha256()
    h.update(np.int64(count).tobytes())
    for pid, (xyz, err, track) in points.items():
        h.update(np.uint64(pid).tobytes())
        h.update(bits(xyz).tobytes())
        h.update(np.asarray(track, np.uint32).tobytes())
    for k in sorted(trials):
        h.update(np.asarray([k[0], k[1], trials[k]], np.int64).tobytes())
    return h.hexdigest()
