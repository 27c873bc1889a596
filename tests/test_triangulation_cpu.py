"""Triangulation without a GPU: the pycolmap surface (PointData, EstimateTriangulationOptions, the argument checks of
estimate_triangulation), and the CPU reference (tests/tri_ref/tri_ref.cc) that the GPU kernel is held to - against
known answers, against an independent numpy / LAPACK restatement, and against its frozen fixture."""
import json
import math
import pickle
from pathlib import Path

import numpy as np
import pytest

import tri_cases
import tri_ref_lib as ref

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"


# ---- the pycolmap surface ------------------------------------------------------------------------------------------
def test_options_defaults_and_dataclass_protocol():
    import pycolmap
    o = pycolmap.EstimateTriangulationOptions()
    assert o.min_tri_angle == 0.0
    r = o.ransac
    assert (r.max_error, r.min_inlier_ratio, r.confidence, r.min_num_trials, r.max_num_trials) == (4.0, 0.01, 0.9999, 1000, 100000)
    d = o.todict()
    assert d == {"min_tri_angle": 0.0, "ransac": {"max_error": 4.0, "min_inlier_ratio": 0.01, "confidence": 0.9999,
                                                  "dyn_num_trials_multiplier": 3.0, "min_num_trials": 1000,
                                                  "max_num_trials": 100000}}
    o2 = pycolmap.EstimateTriangulationOptions({"min_tri_angle": 0.1, "ransac": {"max_error": 0.01}})
    assert o2.min_tri_angle == 0.1 and o2.ransac.max_error == 0.01 and o2.ransac.min_num_trials == 1000
    o3 = pycolmap.EstimateTriangulationOptions(min_tri_angle=0.2)
    o3.mergedict({"ransac": {"confidence": 0.99}})
    assert o3.min_tri_angle == 0.2 and o3.ransac.confidence == 0.99 and o3.ransac.max_error == 4.0
    assert pickle.loads(pickle.dumps(o3)).todict() == o3.todict()
    s = o.summary()
    assert s.startswith("EstimateTriangulationOptions:") and "min_tri_angle = 0.0" in s and "max_error = 4.0" in s
    with pytest.raises(ValueError, match="unknown option"):
        pycolmap.EstimateTriangulationOptions(min_angle=1.0)


def test_point_data():
    import pycolmap
    p = pycolmap.PointData([10.0, 20.0], [0.01, -0.02])
    assert list(p.point) == [10.0, 20.0] and list(p.point_normalized) == [0.01, -0.02]
    p2 = pycolmap.PointData(np.array([1.0, 2.0]), np.array([3.0, 4.0]))
    assert list(p2.point_normalized) == [3.0, 4.0]


def _inputs(n, m=None, k=None):
    import pycolmap
    pts = [pycolmap.PointData([0.0, 0.0], [0.0, 0.0])] * n
    ims = [pycolmap.Image()] * (n if m is None else m)
    cams = [pycolmap.Camera(model="SIMPLE_PINHOLE", width=10, height=10, params=[1.0, 5.0, 5.0])] * (n if k is None else k)
    return pts, ims, cams


def test_argument_checks_raise_before_any_device_work():
    import pycolmap
    with pytest.raises(ValueError, match=r"^\[module\.cc:\d+\] Check Failed: images\.size\(\) == cameras\.size\(\) \(3 vs\. 2\)$"):
        pycolmap.estimate_triangulation(*_inputs(3, 3, 2))
    with pytest.raises(ValueError, match=r"^\[module\.cc:\d+\] Check Failed: images\.size\(\) == point_data\.size\(\) \(2 vs\. 3\)$"):
        pycolmap.estimate_triangulation(*_inputs(3, 2, 2))
    with pytest.raises(ValueError, match=r"Check Failed: point_data\.size\(\) >= 2 \(1 vs\. 2\)"):
        pycolmap.estimate_triangulation(*_inputs(1), opions=pycolmap.EstimateTriangulationOptions())
    with pytest.raises(ValueError, match=r"Check Failed: point_data\.size\(\) >= 2 \(0 vs\. 2\)"):
        pycolmap.estimate_triangulation([], [], [])
    with pytest.raises(TypeError):  # the keyword is spelled as in the reference
        pycolmap.estimate_triangulation(*_inputs(1), options=pycolmap.EstimateTriangulationOptions())


def test_names_resolve_through_import_pycolmap():
    import pycolmap
    import pycolmap_amd
    for n in ("estimate_triangulation", "PointData", "EstimateTriangulationOptions"):
        assert getattr(pycolmap, n) is getattr(pycolmap_amd, n)


# ---- numerics of DESIGN.md 11.4 ----------------------------------------------------------------------------------------
def test_own_acos_is_within_one_ulp_and_nan_outside():
    xs = np.concatenate([np.linspace(-1.0, 1.0, 20001), [0.5, -0.5, np.nextafter(0.5, 0), np.nextafter(1.0, 0), 1e-300]])
    got = np.array([ref.acos(x) for x in xs])
    want = np.arccos(xs)
    assert (np.abs(got - want) <= np.spacing(np.maximum(want, 1e-300))).all()
    assert ref.acos(1.0) == 0.0 and ref.acos(-1.0) == math.pi
    for bad in (np.nextafter(1.0, 2.0), -np.nextafter(1.0, 2.0), np.nan, np.inf):
        assert math.isnan(ref.acos(bad))


def test_triangulation_angle():
    c1, c2 = np.array([0.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0])
    assert ref.angle(c1, c2, np.array([0.5, 0.0, 0.5])) == pytest.approx(math.pi / 2)
    assert ref.angle(c1, c2, c1) == 0.0  # zero denominator
    # obtuse: min(angle, pi - angle)
    assert ref.angle(c1, c2, np.array([0.5, 0.0, 0.1])) == pytest.approx(math.pi - 2 * math.atan2(0.5, 0.1))


# ---- the CPU reference against known answers --------------------------------------------------------------------------
def _cosines(sc, xyz):
    """The cosine of every observation at its track's xyz, in DESIGN.md 11.2's operation order."""
    off = sc["offsets"].astype(np.int64)
    t = np.repeat(np.arange(len(off) - 1), np.diff(off))
    x, y = sc["obs_xy"][:, 0], sc["obs_xy"][:, 1]
    na = np.sqrt(x * x + y * y + 1.0)
    P = sc["poses"][sc["obs_pose"]]
    X = xyz[t]
    q = [P[:, r, 0] * X[:, 0] + P[:, r, 1] * X[:, 1] + P[:, r, 2] * X[:, 2] + P[:, r, 3] for r in range(3)]
    nb = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
    return (x / na) * (q[0] / nb) + (y / na) * (q[1] / nb) + (1.0 / na) * (q[2] / nb)


def test_reference_noise_free_known_answers():
    sc = tri_cases.scene(101, 300, noise_px=0.0, outlier_frac=0.0)
    xyz, ok, mask, st = ref.triangulate(sc["poses"], sc["offsets"], sc["obs_pose"], sc["obs_xy"], max_error=tri_cases.TIGHT)
    rel = np.linalg.norm(xyz[ok] - sc["xyz"][ok], axis=1) / np.linalg.norm(sc["xyz"][ok], axis=1)
    assert ok.mean() > 0.8 and rel.max() < 1e-9
    # every observation is an inlier, except where the cosine of a perfect observation rounds above 1: acos gives NaN
    # and NaN is an outlier (COLMAP's std::acos does the same)
    off = sc["offsets"].astype(np.int64)
    okm = np.repeat(ok, np.diff(off))
    c = _cosines(sc, xyz)
    assert np.array_equal(mask[okm], c[okm] <= 1.0)
    assert mask[okm].mean() > 0.85
    failed = np.flatnonzero(~ok)
    for t in failed:  # a failure is a track with fewer than two finite residuals
        assert (c[off[t]:off[t + 1]] <= 1.0).sum() < 2 or st["num_inliers"][t] < 2


def test_reference_flags_planted_outliers():
    sc = tri_cases.scene(102, 300, outlier_frac=0.25, mean_len=8.0)
    xyz, ok, mask, st = ref.triangulate(sc["poses"], sc["offsets"], sc["obs_pose"], sc["obs_xy"], max_error=tri_cases.TIGHT)
    lens = np.diff(sc["offsets"].astype(np.int64))
    okm = np.repeat(ok & (lens >= 5), lens)
    assert (~mask[okm & sc["outlier"]]).mean() > 0.97  # planted outliers are flagged
    assert mask[okm & ~sc["outlier"]].mean() > 0.9
    good = ok & (lens >= 5)
    err = np.linalg.norm(xyz[good] - sc["xyz"][good], axis=1)
    assert np.median(err) < 0.02


def _single_track(P_list, X):
    poses = np.stack(P_list)
    xy = []
    for P in P_list:
        q = P[:, :3] @ X + P[:, 3]
        xy.append(q[:2] / q[2])
    return poses, np.array([0, len(P_list)], np.uint64), np.arange(len(P_list), dtype=np.uint32), np.array(xy)


def _cam(center, R=np.eye(3)):
    P = np.zeros((3, 4))
    P[:, :3] = R
    P[:, 3] = -R @ np.asarray(center, float)
    return P


def test_reference_behind_camera_and_zero_baseline_fail():
    X = np.array([0.2, -0.1, 5.0])
    # all cameras look along +z; a point behind them (z < 0 in every camera) projects, but fails the depth check
    P = [_cam([0, 0, 0]), _cam([1, 0, 0]), _cam([0, 1, 0])]
    poses, off, op, xy = _single_track(P, np.array([0.2, -0.1, -5.0]))
    assert not ref.triangulate(poses, off, op, xy)[1][0]
    # the same cameras in front: success, all inliers
    poses, off, op, xy = _single_track(P, X)
    xyz, ok, mask, st = ref.triangulate(poses, off, op, xy, max_error=1e-3)
    assert ok[0] and np.allclose(xyz[0], X, rtol=1e-9)
    # zero baseline: one centre for every observation; min_tri_angle > 0 refuses the angle of 0
    poses, off, op, xy = _single_track([_cam([0, 0, 0])] * 3, X)
    assert not ref.triangulate(poses, off, op, xy, min_tri_angle=1e-6)[1][0]


@pytest.mark.parametrize("n", [2, 3, 4, 7, 12, 30, 45])
def test_reference_runs_every_combination_for_small_tracks(n):
    """With min_num_trials = 1000 above n(n-1)/2 no RANSAC stops early: num_trials is the CombinationSampler's
    number of pairs."""
    sc = tri_cases.fixed_length(200 + n, 20, n, outlier_frac=0.2)
    xyz, ok, mask, st = ref.triangulate(sc["poses"], sc["offsets"], sc["obs_pose"], sc["obs_xy"], max_error=tri_cases.TIGHT)
    assert (st["num_trials"] == n * (n - 1) // 2).all()


def test_reference_trial_caps():
    sc = tri_cases.fixed_length(301, 3, 80, outlier_frac=0.3)
    a = ref.triangulate(sc["poses"], sc["offsets"], sc["obs_pose"], sc["obs_xy"], max_error=tri_cases.TIGHT,
                        min_num_trials=10, max_num_trials=50)
    assert (a[3]["num_trials"] <= 50).all()
    b = ref.triangulate(sc["poses"], sc["offsets"], sc["obs_pose"], sc["obs_xy"], max_error=tri_cases.TIGHT)
    assert (b[3]["num_trials"] == 1002).all()  # 3160 pairs; stops right after min_num_trials (LORANSAC's abort step)


# ---- an independent restatement: numpy / LAPACK ------------------------------------------------------------------------
def _np_triangulate_track(P, C, xy, min_tri_angle, max_error, conf=0.9999, mult=3.0, min_trials=1000, max_trials=100000):
    n = len(xy)
    maxres = max_error * max_error

    def angle(c1, c2, X):
        b2, r1, r2 = np.sum((c1 - c2) ** 2), np.sum((X - c1) ** 2), np.sum((X - c2) ** 2)
        den = 2.0 * np.sqrt(r1 * r2)
        if den == 0.0:
            return 0.0
        with np.errstate(invalid="ignore"):
            a = abs(np.arccos((r1 + r2 - b2) / den))
        return min(a, np.pi - a) if not np.isnan(a) else np.nan

    def residuals(X):
        a = np.c_[xy, np.ones(n)]
        a /= np.linalg.norm(a, axis=1, keepdims=True)
        q = P[:, :, :3] @ X + P[:, :, 3]
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        with np.errstate(invalid="ignore"):
            return np.arccos(np.sum(a * q, axis=1)) ** 2

    def estimate(idx):
        if len(idx) == 2:
            i, j = idx
            A = np.stack([xy[i, 0] * P[i, 2] - P[i, 0], xy[i, 1] * P[i, 2] - P[i, 1],
                          xy[j, 0] * P[j, 2] - P[j, 0], xy[j, 1] * P[j, 2] - P[j, 1]])
            v = np.linalg.svd(A)[2][-1]
            X = v[:3] / v[3]
            if P[i, 2] @ np.r_[X, 1] >= 2.2e-16 and P[j, 2] @ np.r_[X, 1] >= 2.2e-16 and angle(C[i], C[j], X) >= min_tri_angle:
                return X
            return None
        A = np.zeros((4, 4))
        for k in idx:
            h = np.r_[xy[k], 1.0]
            h /= np.linalg.norm(h)
            T = P[k] - np.outer(h, h) @ P[k]
            A += T.T @ T
        v = np.linalg.eigh(A)[1][:, 0]
        X = v[:3] / v[3]
        if not all(P[k, 2] @ np.r_[X, 1] >= 2.2e-16 for k in idx):
            return None
        for a in range(len(idx)):
            for b in range(a):
                if angle(C[idx[a]], C[idx[b]], X) >= min_tri_angle:
                    return X
        return None

    def support(r):
        inl = r <= maxres
        return int(inl.sum()), float(r[inl].sum())

    def better(s, b):
        return s[0] > b[0] or (s[0] == b[0] and s[1] < b[1])

    def num_trials(k):
        nom = 1 - conf
        if nom <= 0:
            return 1 << 64
        denom = 1 - (k / n) ** 2
        if denom <= 0:
            return 1
        if denom == 1.0:
            return 1 << 64
        return int(math.ceil(math.log(nom) / math.log(denom) * mult))

    cap = min(max_trials, num_trials_cfg(conf, mult, max_trials), n * (n - 1) // 2)
    best, best_X = (0, np.finfo(float).max), None
    dyn = cap
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    trial, abort = 0, False
    while trial < cap:
        if abort:
            trial += 1
            break
        X = estimate(list(pairs[trial]))
        if X is not None:
            r = residuals(X)
            s = support(r)
            if better(s, best):
                best, best_X = s, X
                if s[0] > 2:
                    for _ in range(10):
                        prev = best[0]
                        L = estimate(list(np.flatnonzero(residuals(best_X) <= maxres)))
                        if L is not None:
                            ls = support(residuals(L))
                            if better(ls, best):
                                best, best_X = ls, L
                        if best[0] <= prev:
                            break
                dyn = num_trials(best[0])
            if trial >= dyn and trial >= min_trials:
                abort = True
        trial += 1
    if best[0] < 2:
        return None, np.zeros(n, bool)
    return best_X, residuals(best_X) <= maxres


def num_trials_cfg(conf, mult, max_trials, min_inlier_ratio=0.01):
    r = int(min_inlier_ratio * 100000) / 100000
    return int(math.ceil(math.log(1 - conf) / math.log(1 - r * r) * mult))


def _np_batch(sc, min_tri_angle=0.0, max_error=tri_cases.TIGHT):
    Pall = sc["poses"]
    Call = -np.einsum("cji,cj->ci", Pall[:, :, :3], Pall[:, :, 3])
    off = sc["offsets"].astype(np.int64)
    out = []
    for t in range(len(off) - 1):
        sl = slice(off[t], off[t + 1])
        idx = sc["obs_pose"][sl]
        out.append(_np_triangulate_track(Pall[idx], Call[idx], sc["obs_xy"][sl], min_tri_angle, max_error))
    return out


def test_reference_agrees_with_numpy_restatement():
    # clear cases: well-conditioned tracks of 3-8 observations, 0.5 px noise, far-off outliers - identical masks
    sc = tri_cases.scene(401, 150, outlier_frac=0.0, mean_len=5.0, max_len=8)
    xyz, ok, mask, st = ref.triangulate(sc["poses"], sc["offsets"], sc["obs_pose"], sc["obs_xy"], max_error=tri_cases.TIGHT)
    off = sc["offsets"].astype(np.int64)
    for t, (X, m) in enumerate(_np_batch(sc)):
        assert (X is not None) == ok[t]
        assert np.array_equal(m, mask[off[t]:off[t + 1]])
        if X is not None:
            assert np.allclose(X, xyz[t], rtol=1e-6, atol=1e-9)
    # a seeded random set with outliers and an angle limit: report the agreement, expect nearly all
    sc = tri_cases.scene(402, 300, outlier_frac=0.2, mean_len=6.0, max_len=12)
    xyz, ok, mask, st = ref.triangulate(sc["poses"], sc["offsets"], sc["obs_pose"], sc["obs_xy"], max_error=tri_cases.TIGHT,
                                        min_tri_angle=0.05)
    off = sc["offsets"].astype(np.int64)
    agree = 0
    for t, (X, m) in enumerate(_np_batch(sc, min_tri_angle=0.05)):
        agree += int((X is not None) == ok[t] and np.array_equal(m, mask[off[t]:off[t + 1]]))
    rate = agree / (len(off) - 1)
    print(f"reference vs numpy restatement: {agree} of {len(off) - 1} tracks identical ({rate:.3f})")
    assert rate > 0.95


# ---- the frozen fixture and the recording ------------------------------------------------------------------------------
def test_reference_against_frozen_fixture():
    fx = np.load(GOLDEN / "tri_ref_v1.npz")
    names = sorted({k.split("/")[0] for k in fx.files})
    assert len(names) >= 5
    for name in names:
        opts = json.loads(bytes(fx[f"{name}/options"]).decode())
        xyz, ok, mask, st = ref.triangulate(fx[f"{name}/poses"], fx[f"{name}/offsets"], fx[f"{name}/obs_pose"],
                                            fx[f"{name}/obs_xy"], **opts)
        assert np.array_equal(xyz.view(np.uint64), fx[f"{name}/xyz"].view(np.uint64)), name
        assert np.array_equal(ok, fx[f"{name}/success"]) and np.array_equal(mask, fx[f"{name}/inlier_mask"]), name
        assert np.array_equal(st["num_trials"], fx[f"{name}/num_trials"]), name
        assert np.array_equal(st["num_inliers"], fx[f"{name}/num_inliers"]), name


def test_reference_against_pycolmap_recording():
    """Agreement with the real pycolmap 0.6.x estimate_triangulation, recorded by
    tests/golden/make_triangulation_reference_golden.py on the fixture's tracks."""
    rec = GOLDEN / "tri_pycolmap_v1.npz"
    if not rec.exists():
        pytest.skip("no recording of pycolmap's estimate_triangulation (tests/golden/make_triangulation_reference_golden.py)")
    fx, rc = np.load(GOLDEN / "tri_ref_v1.npz"), np.load(rec)
    names = sorted({k.split("/")[0] for k in rc.files})
    for name in names:
        ok, rok = fx[f"{name}/success"], rc[f"{name}/success"]
        assert (ok == rok).mean() > 0.95, name
        both = ok & rok
        assert np.allclose(fx[f"{name}/xyz"][both], rc[f"{name}/xyz"][both], rtol=1e-6, atol=1e-8), name
