"""Named, deterministic relative-pose cases shared by the CPU and GPU suites ("what is pinned"):
the inputs of amc_pose_pairs (cases) and of homography_decomposition (homography_cases).

Every case is built from planted geometry - R, t, points, and E or H computed from them - so no RANSAC decides what a
case contains.  cases() maps a name to a dict:

    cam1, cam2   (model, width, height, params) of the two slots
    pts1, pts2   the slots' image points; f32: they go up through upload_keypoints (float32) instead of
                 upload_points_f64
    matches      (n, 2) uint32; config, E, H: the geometry handed to EstimateTwoViewGeometryPose
    kind         "clean" | "garbage" (rows planted to fail the cheirality test of every candidate: garbage()) |
                 "degenerate"
    survivors    the number of points the winner must keep, where the case fixes it
    truth        (R, t) where the planted motion must come back

build_cases() adds the oracle's result for each and asserts what the cases are there for: the survivor counts, that
the rotation cases reach all four branches of Eigen's matrix-to-quaternion conversion, that the three planar scenes
pick the three formula sets of the homography decomposition, that the two nearly pure rotations stand 10 % clear of
its 1e-3 threshold on either side, and that the case with points on the line between facing cameras has negative
cosines.  A fixture that drifts then fails loudly instead of covering less.

Degenerate input (zero E, NaN in E, Inf in H, rank-one H, a NaN point, configs without a geometry) cannot keep the
kernel running: jacobi_eigen_t leaves its sweep loop on !(off > tol), which a NaN satisfies, and is bounded by 40
sweeps; select_cosine is 63 steps over n / 64 chunks whatever the keys are.  The oracle's result on each of them is
well defined because none lets a NaN reach its std::sort: a non-finite candidate keeps no point (every comparison of
the cheirality test is false), so the angle list is empty, and the NaN point is dropped by the same comparisons
before its angle is taken.  The all-zero E decomposes to proper rotations (U = V = I) and finite points.  NaNs in R, t
and q are compared as NaNs, not by payload.
"""
from __future__ import annotations

import functools

import numpy as np

from ref2 import pose_ref2 as r2

CALIBRATED, UNCALIBRATED, PLANAR, PANORAMIC, PLANAR_OR_PANORAMIC = 2, 3, 4, 5, 6
CAM_A = ("PINHOLE", 1600, 1200, (1200.0, 1190.0, 800.0, 600.0))
CAM_B = ("SIMPLE_PINHOLE", 1600, 1200, (1210.0, 801.0, 599.0))
CAM_RADIAL = ("SIMPLE_RADIAL", 1600, 1200, (1195.0, 802.0, 598.0, 0.05))
CAM_OPENCV = ("OPENCV", 1600, 1200, (1205.0, 1198.0, 799.0, 601.0, 0.04, -0.02, 0.001, -0.002))
COUNTS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 257)
EDGE_ROWS = (0, 63, 64, 127, 129)
# the largest |entry| of S on either side of the decomposition's 1e-3: 10 % clear of it and no more, so that a threshold
# moved by more than that changes a result
THRESHOLD_SIDES = (("below", 0.899e-3), ("above", 1.101e-3))
Z3 = np.zeros((3, 3))


def bits(a):
    """the bit patterns of float64 values, NaNs as one pattern whatever their payload"""
    a = np.ascontiguousarray(a, dtype=np.float64).copy()
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def K_of(cam):
    return r2.calibration_matrix(cam[0], cam[3])


def project(cam, X):
    return r2.img_from_cam(cam[0], cam[3], X[:, :2] / X[:, 2:])


def ident(n):
    return np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.uint32)


def garbage(scene, rows):
    """pts2 with the second point of `rows` replaced by the image of a point 5000 units down the row's first ray.  Such
    a row satisfies the epipolar constraint, so it triangulates where it was planted: beyond 1000 baselines for the
    planted pose, and behind a camera for each of the other three candidates.  (Mirroring and scaling the second point,
    which is enough on the homography path, leaves most rows of a general scene in front of both cameras.)"""
    out = scene["pts2"].copy()
    rows = list(rows)
    if rows:
        uv = r2.cam_from_img(scene["cam1"][0], scene["cam1"][3], scene["pts1"][rows])
        far = np.column_stack([uv, np.ones(len(rows))]) * 5000.0
        out[rows] = project(scene["cam2"], far @ scene["R"].T + scene["t"])
    return out


def case(cam1, cam2, pts1, pts2, matches, config, E=None, H=None, kind="clean", survivors=None, truth=None, f32=False):
    return dict(cam1=cam1, cam2=cam2, pts1=np.ascontiguousarray(pts1, np.float64),
                pts2=np.ascontiguousarray(pts2, np.float64), matches=np.ascontiguousarray(matches, np.uint32).reshape(-1, 2),
                config=int(config), E=np.array(Z3 if E is None else E, np.float64),
                H=np.array(Z3 if H is None else H, np.float64), kind=kind, survivors=survivors, truth=truth, f32=f32)


# ---------------------------------------------------------------------------------------------- scenes
def general_scene(seed, n, cam1=CAM_A, cam2=CAM_B, R=None, t=None):
    """n points 4 to 9 units in front of camera 1, seen by camera 2 = [R | t]"""
    rng = np.random.default_rng(seed)
    R = rodrigues((0.2, -1.0, 0.3), 0.3) if R is None else R
    t = np.array([0.8, -0.1, 0.15]) if t is None else np.asarray(t, np.float64)
    X = rng.uniform([-2.0, -1.5, 4.0], [2.0, 1.5, 9.0], size=(n, 3))
    X2 = X @ R.T + t
    assert (X2[:, 2] > 0.5).all()
    return dict(cam1=cam1, cam2=cam2, pts1=project(cam1, X), pts2=project(cam2, X2), R=R, t=t, E=skew(t) @ R, X=X)


def facing_scene(seed, n, axis, angle, centre=(0.0, 0.0, 10.0), spread=1.2):
    """camera 2 sits at `centre`, turned by `angle` about `axis`; n points 3 to 7 units in front of camera 1"""
    rng = np.random.default_rng(seed)
    R = rodrigues(axis, angle)
    t = -R @ np.asarray(centre, np.float64)
    X = rng.uniform([-spread, -spread, 3.0], [spread, spread, 7.0], size=(n, 3))
    X2 = X @ R.T + t
    assert (X2[:, 2] > 0.5).all(), "the points must be in front of the second camera"
    return dict(cam1=CAM_A, cam2=CAM_A, pts1=project(CAM_A, X), pts2=project(CAM_A, X2), R=R, t=t, E=skew(t) @ R, X=X)


def plane_scene(seed, n, nrm, a, angle=0.2, d=5.0, cam1=CAM_A, cam2=CAM_B, axis=(0.3, 1.0, -0.2)):
    """n points on the plane nrm . X = d seen by [I | 0] and [R | t] with R^T t = d a; H maps pixels of 1 to pixels of 2"""
    rng = np.random.default_rng(seed)
    nrm = np.asarray(nrm, np.float64) / np.linalg.norm(nrm)
    R = rodrigues(axis, angle)
    t = d * (R @ np.asarray(a, np.float64))
    rays = np.column_stack([rng.uniform(-0.4, 0.4, (n, 2)), np.ones(n)])
    X = rays * (d / (rays @ nrm))[:, None]
    X2 = X @ R.T + t
    assert (X[:, 2] > 0.5).all() and (X2[:, 2] > 0.5).all()
    Hn = R + np.outer(t, nrm) / d
    return dict(cam1=cam1, cam2=cam2, pts1=project(cam1, X), pts2=project(cam2, X2), R=R, t=t, n=nrm, d=d, Hn=Hn,
                H=K_of(cam2) @ Hn @ np.linalg.inv(K_of(cam1)), x1=X[:, :2] / X[:, 2:], x2=X2[:, :2] / X2[:, 2:])


PLANES = {0: dict(nrm=(0.6, 0.1, 0.79), a=(0.10, 0.01, 0.02)),     # the largest |S_ii| at index 0, 1, 2
          1: dict(nrm=(0.1, 0.6, 0.79), a=(0.01, 0.10, 0.02)),
          2: dict(nrm=(0.1, -0.2, 1.0), a=(0.01, 0.02, 0.08))}


def threshold_scene(seed, n, target, **kw):
    """a nearly pure rotation: the translation of plane 2 scaled until the largest |entry| of S is `target`"""
    s = 1.0
    for _ in range(6):
        sc = plane_scene(seed, n, PLANES[2]["nrm"], np.asarray(PLANES[2]["a"]) * s, **kw)
        s *= target / r2.homography_S(sc["H"], K_of(sc["cam1"]), K_of(sc["cam2"]))[1]
    return sc


SURVIVOR_SETS = {
    "edges": sorted(set(range(130)) - set(EDGE_ROWS)),           # all rows but 0, 63, 64, 127, 129
    "64": list(range(1, 128, 2)),                                # the odd rows below 128
    "65": list(range(1, 128, 2)) + [128],
    "1": [128],
    "2": [63, 64],
    "0": [],
}


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    # counts: the first n matches of one scene, calibrated and planar
    g = general_scene(7101, 257)
    p = plane_scene(7102, 257, **PLANES[2])
    for n in COUNTS:
        c[f"count_calibrated_{n}"] = case(g["cam1"], g["cam2"], g["pts1"], g["pts2"], ident(257)[:n], CALIBRATED, E=g["E"],
                                          survivors=n, truth=(g["R"], g["t"]) if n >= 2 else None)
        c[f"count_planar_{n}"] = case(p["cam1"], p["cam2"], p["pts1"], p["pts2"], ident(257)[:n], PLANAR, H=p["H"],
                                      survivors=n)
    # survivors: 130 rows, garbage everywhere but at the listed rows
    g = general_scene(7103, 130)
    for name, keep in SURVIVOR_SETS.items():
        bad = sorted(set(range(130)) - set(keep))
        c[f"survivors_{name}"] = case(g["cam1"], g["cam2"], g["pts1"], garbage(g, bad), ident(130),
                                      CALIBRATED, E=g["E"], kind="garbage", survivors=len(keep))
    # duplicates: equal cosines
    g = general_scene(7104, 2)
    for n in (64, 65, 130):
        c[f"duplicates_one_{n}"] = case(g["cam1"], g["cam2"], g["pts1"], g["pts2"], np.zeros((n, 2)), CALIBRATED, E=g["E"],
                                        survivors=n, truth=(g["R"], g["t"]))
    for n, first in ((64, 32), (130, 65), (65, 49)):
        rows = np.repeat(np.arange(n) >= first, 2).reshape(n, 2)
        tag = "halves" if 2 * first == n else "quarters"
        c[f"duplicates_{tag}_{n}"] = case(g["cam1"], g["cam2"], g["pts1"], g["pts2"], rows, CALIBRATED, E=g["E"],
                                          survivors=n, truth=(g["R"], g["t"]))
    # rotations: camera 2 at z = 10 facing camera 1, turned about x, y and an oblique axis; a turn about z leaves the
    # optical axis where it was, so that camera stands beside the first and is rolled
    near = np.deg2rad(175.0)
    rot = {"x": facing_scene(7110, 130, (1, 0, 0), near), "y": facing_scene(7111, 130, (0, 1, 0), np.deg2rad(172.0)),
           "z": facing_scene(7112, 130, (0, 0, 1), np.deg2rad(178.0), centre=(1.0, 0.2, 0.0)),
           "oblique": facing_scene(7113, 130, (1.0, 1.0, 0.15), np.deg2rad(170.0)),
           "x180": facing_scene(7114, 130, (1, 0, 0), np.pi)}
    for name, s in rot.items():
        c[f"rotation_{name}"] = case(s["cam1"], s["cam2"], s["pts1"], s["pts2"], ident(130), CALIBRATED, E=s["E"],
                                     survivors=130, truth=(s["R"], s["t"]))
    s = general_scene(7115, 130, cam2=CAM_A, R=rodrigues((1, 1, 1), 2 * np.pi / 3), t=(-5.0, 0.0, 6.0))
    c["rotation_120_about_111"] = case(s["cam1"], s["cam2"], s["pts1"], s["pts2"], ident(130), CALIBRATED, E=s["E"],
                                       survivors=130, truth=(s["R"], s["t"]))
    s = general_scene(7116, 130)
    c["rotation_small"] = case(s["cam1"], s["cam2"], s["pts1"], s["pts2"], ident(130), CALIBRATED, E=s["E"], survivors=130,
                               truth=(s["R"], s["t"]))
    # angles above 90 degrees: facing cameras, points close to the line between them
    s = facing_scene(7117, 130, (1, 0, 0), near, spread=0.05)
    c["angles_above_90"] = case(s["cam1"], s["cam2"], s["pts1"], s["pts2"], ident(130), CALIBRATED, E=s["E"], survivors=130,
                                truth=(s["R"], s["t"]))
    # homographies
    for i, kw in PLANES.items():
        s = plane_scene(7120 + i, 130, **kw)
        c[f"homography_S{i}"] = case(s["cam1"], s["cam2"], s["pts1"], s["pts2"], ident(130), PLANAR, H=s["H"], survivors=130)
    s = plane_scene(7123, 130, **PLANES[0])
    for name, f in (("plus", 1.0), ("minus", -1.0), ("half", 0.5), ("double", 2.0)):
        c[f"homography_{name}"] = case(s["cam1"], s["cam2"], s["pts1"], s["pts2"], ident(130), PLANAR, H=f * s["H"],
                                       survivors=130)
    s = plane_scene(7124, 130, PLANES[2]["nrm"], (0.0, 0.0, 0.0))
    for name, cfg in (("por", PLANAR_OR_PANORAMIC), ("planar", PLANAR), ("panoramic", PANORAMIC)):
        c[f"homography_pure_rotation_{name}"] = case(s["cam1"], s["cam2"], s["pts1"], s["pts2"], ident(130), cfg, H=s["H"],
                                                     survivors=0)
    for name, target in THRESHOLD_SIDES:
        s = threshold_scene(7125, 130, target)
        c[f"homography_threshold_{name}"] = case(s["cam1"], s["cam2"], s["pts1"], s["pts2"], ident(130), PLANAR_OR_PANORAMIC,
                                                 H=s["H"], survivors=0)
    # cameras
    for name, (c1, c2) in (("pinhole_pinhole", (CAM_A, CAM_A)), ("pinhole_simple", (CAM_A, CAM_B)),
                           ("simple_pinhole", (CAM_B, CAM_A)), ("distorted", (CAM_RADIAL, CAM_OPENCV))):
        s = general_scene(7130, 130, cam1=c1, cam2=c2)
        c[f"cameras_{name}"] = case(c1, c2, s["pts1"], s["pts2"], ident(130), CALIBRATED, E=s["E"], survivors=130,
                                    truth=(s["R"], s["t"]))
    s = general_scene(7131, 130)
    q1, q2 = s["pts1"].astype(np.float32).astype(np.float64), s["pts2"].astype(np.float32).astype(np.float64)
    for name, f32 in (("float32", True), ("float64", False)):   # the same values through either upload: equal results
        c[f"cameras_{name}"] = case(s["cam1"], s["cam2"], q1, q2, ident(130), CALIBRATED, E=s["E"], survivors=130, f32=f32)
    # degenerate input
    s = general_scene(7140, 71)
    p = plane_scene(7141, 71, **PLANES[1])
    deg = functools.partial(case, kind="degenerate")
    c["degenerate_zero_E"] = deg(s["cam1"], s["cam2"], s["pts1"], s["pts2"], ident(71), UNCALIBRATED)
    E = s["E"].copy()
    E[1, 2] = np.nan
    c["degenerate_nan_E"] = deg(s["cam1"], s["cam2"], s["pts1"], s["pts2"], ident(71), CALIBRATED, E=E)
    H = p["H"].copy()
    H[0, 1] = np.inf
    c["degenerate_inf_H"] = deg(p["cam1"], p["cam2"], p["pts1"], p["pts2"], ident(71), PLANAR, H=H)
    c["degenerate_rank_one_H"] = deg(p["cam1"], p["cam2"], p["pts1"], p["pts2"], ident(71), PLANAR,
                                     H=np.outer([1.0, 2.0, 0.5], [0.3, -0.1, 1.0]))
    bad = s["pts2"].copy()
    bad[35] = np.nan
    c["degenerate_nan_point"] = deg(s["cam1"], s["cam2"], s["pts1"], bad, ident(71), CALIBRATED, E=s["E"], survivors=70)
    for cfg, name in ((0, "undefined"), (1, "degenerate"), (7, "watermark"), (8, "multiple")):
        c[f"degenerate_config_{name}"] = deg(s["cam1"], s["cam2"], s["pts1"], s["pts2"], ident(71), cfg, E=s["E"], H=p["H"])
    assert all(len(v["matches"]) <= 260 for v in c.values())
    return c


MASKED_SIZES = (63, 64, 65, 129, 130)


def masked_holes(M):
    return sorted({0, 63, 64, M - 1} & set(range(M)))


@functools.lru_cache(maxsize=None)
def masked_scenes():
    """M -> dict(cam, pts1, pts2 (float32 values), matches, holes): the input of amc_verify_pairs with
    compute_relative_pose, the only way to a non-null mask in the pose kernel.  Exact correspondences of a general
    scene, but for the rows `holes` = {0, 63, 64, M - 1}, whose second point is moved hundreds of pixels off its
    epipolar line: the estimation's inlier mask then has a cleared row in each 64-row chunk (the callers assert it)."""
    out = {}
    for M in MASKED_SIZES:
        s = general_scene(7300 + M, M, cam2=CAM_A)
        p2 = s["pts2"].copy()
        holes = masked_holes(M)
        p2[holes] = np.mod(p2[holes] + np.array([317.0, 411.0]), [1600.0, 1200.0])
        out[M] = dict(cam=CAM_A, pts1=s["pts1"].astype(np.float32).astype(np.float64),
                      pts2=p2.astype(np.float32).astype(np.float64), matches=ident(M), holes=holes)
    return out


def oracle_verify(sc):
    """the oracle's EstimateTwoViewGeometry with the relative pose on a masked scene"""
    import oracle_lib as o
    cam = ocam(sc["cam"])
    return o.estimate_two_view_geometry(cam, sc["pts1"], cam, sc["pts2"], sc["matches"],
                                        o.tvg_default_options(compute_relative_pose=1), seed=0)


def check_masked(sc, mask):
    """the inlier mask is the planted one: exactly the holes cleared, so one cleared row in every 64-row chunk"""
    M = len(sc["matches"])
    assert list(np.flatnonzero(~np.asarray(mask, bool))) == sc["holes"], (M, np.flatnonzero(~np.asarray(mask, bool)))
    for base in range(0, M, 64):
        assert not np.asarray(mask, bool)[base:base + 64].all(), (M, base)


K1H = np.array([[900.0, 0, 640], [0, 910.0, 360], [0, 0, 1]])
K2H = np.array([[1100.0, 0, 600], [0, 1090.0, 400], [0, 0, 1]])
CAM_1H = ("PINHOLE", 1280, 720, (900.0, 910.0, 640.0, 360.0))
CAM_2H = ("PINHOLE", 1280, 720, (1100.0, 1090.0, 600.0, 400.0))


@functools.lru_cache(maxsize=None)
def homography_cases():
    """name -> dict(H, K1, K2, p1, p2 (normalised points), kind, survivors): the inputs of homography_decomposition"""
    c = {}

    def hcase(s, n=None, H=None, p2=None, kind="clean", survivors=None):
        n = len(s["x1"]) if n is None else n
        p2 = s["x2"] if p2 is None else p2
        return dict(H=np.array(s["H"] if H is None else H), K1=K1H, K2=K2H, p1=np.ascontiguousarray(s["x1"][:n]),
                    p2=np.ascontiguousarray(p2[:n]), kind=kind, survivors=n if survivors is None else survivors)

    kw = dict(cam1=CAM_1H, cam2=CAM_2H)
    s = plane_scene(7201, 129, **PLANES[2], **kw)
    for n in (0, 1, 63, 64, 65, 129):
        c[f"count_{n}"] = hcase(s, n)
    s = plane_scene(7202, 130, **PLANES[2], **kw)
    p2 = s["x2"].copy()
    p2[list(EDGE_ROWS)] *= -5.0
    c["garbage_edges"] = hcase(s, p2=p2, kind="garbage", survivors=125)
    for i, pk in PLANES.items():
        c[f"S{i}"] = hcase(plane_scene(7210 + i, 130, **pk, **kw))
    s = plane_scene(7213, 130, **PLANES[0], **kw)
    c["plus"], c["minus"] = hcase(s), hcase(s, H=-s["H"])
    c["pure_rotation"] = hcase(plane_scene(7214, 130, PLANES[2]["nrm"], (0.0, 0.0, 0.0), **kw), survivors=0)
    for name, target in THRESHOLD_SIDES:
        c[f"threshold_{name}"] = hcase(threshold_scene(7215, 130, target, **kw), survivors=0)
    return c


# ---------------------------------------------------------------------------------------------- references
def ocam(cam, prior=True):
    import oracle_lib as o
    return o.make_camera(cam[0], cam[1], cam[2], cam[3], prior=prior)


def oracle(c):
    import oracle_lib as o
    return o.estimate_two_view_geometry_pose(ocam(c["cam1"]), c["pts1"], ocam(c["cam2"]), c["pts2"], c["matches"], c["config"],
                                             E=c["E"], H=c["H"])


def oracle_h(c):
    import oracle_lib as o
    return o.pose_from_homography(c["H"], c["K1"], c["K2"], c["p1"], c["p2"])


def restated(c):
    return r2.relative_pose((c["cam1"][0], c["cam1"][3]), c["pts1"], (c["cam2"][0], c["cam2"][3]), c["pts2"], c["matches"],
                            c["config"], c["E"], c["H"])


def restated_h(c):
    return r2.pose_from_homography(c["H"], c["K1"], c["K2"], c["p1"], c["p2"])


def coverage(cs, want):
    """what the cases reach, from the oracle's results `want` and the restatement"""
    branches = {n: r2.quaternion_branch(want[n]["R"]) for n in cs if n.startswith("rotation_")}
    s_index = {i: r2.homography_S(cs[f"homography_S{i}"]["H"], K_of(cs[f"homography_S{i}"]["cam1"]),
                                  K_of(cs[f"homography_S{i}"]["cam2"]))[2] for i in range(3)}
    inf_norm = {k: r2.homography_S(cs[f"homography_threshold_{k}"]["H"], K_of(cs[f"homography_threshold_{k}"]["cam1"]),
                                   K_of(cs[f"homography_threshold_{k}"]["cam2"]))[1] for k in ("below", "above")}
    cos = restated(cs["angles_above_90"])["cosines"]
    return dict(branches=branches, s_index=s_index, inf_norm=inf_norm, negative_cosines=int((cos < 0).sum()),
                survivors={n: want[n]["num_points3D"] for n in cs if cs[n]["survivors"] is not None})


def check_coverage(cs, cov):
    assert set(cov["branches"].values()) == {"trace", 0, 1, 2}, cov["branches"]
    assert cov["s_index"] == {0: 0, 1: 1, 2: 2}, cov["s_index"]
    assert cov["inf_norm"]["below"] <= 0.9e-3 and cov["inf_norm"]["above"] >= 1.1e-3, cov["inf_norm"]
    assert cov["negative_cosines"] >= 1
    for n, got in cov["survivors"].items():
        assert got == cs[n]["survivors"], f"{n}: the reference keeps {got} points, the case plants {cs[n]['survivors']}"


def check_homography_coverage(hs, want):
    s_index = {i: r2.homography_S(hs[f"S{i}"]["H"], K1H, K2H)[2] for i in range(3)}
    assert s_index == {0: 0, 1: 1, 2: 2}, s_index
    inf_norm = {k: r2.homography_S(hs[f"threshold_{k}"]["H"], K1H, K2H)[1] for k in ("below", "above")}
    assert inf_norm["below"] <= 0.9e-3 and inf_norm["above"] >= 1.1e-3, inf_norm
    for n, c in hs.items():
        assert len(want[n]["points3D"]) == c["survivors"], f"{n}: {len(want[n]['points3D'])} points, planted {c['survivors']}"
    keep = restated_h(hs["garbage_edges"])["keep"]
    assert sorted(np.flatnonzero(~keep)) == list(EDGE_ROWS)


@functools.lru_cache(maxsize=None)
def build_cases():
    """(cases, the oracle's result per case), with the coverage the cases are there for asserted"""
    cs = cases()
    want = {n: oracle(c) for n, c in cs.items()}
    check_coverage(cs, coverage(cs, want))
    return cs, want


@functools.lru_cache(maxsize=None)
def build_homography_cases():
    hs = homography_cases()
    want = {n: oracle_h(c) for n, c in hs.items()}
    check_homography_coverage(hs, want)
    return hs, want
