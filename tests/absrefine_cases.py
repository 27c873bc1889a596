"""Scenes of the joint pose and camera refinement shared by the CPU and GPU suites: the
localisation queries of abspose_cases with a camera that is wrong at the start, and the options each case runs under.
Every query has at most 200 correspondences."""
from __future__ import annotations

import numpy as np

from abspose_cases import FAST, FOCAL4, TIGHT, collinear, concat, empty_query, scene, start, subset

BOTH = dict(refine_focal_length=1, refine_extra_params=1)
BOTH_TIGHT = dict(BOTH, **TIGHT)
FLAGS = ((0, 0), (1, 0), (0, 1), (1, 1))
NUM_FOCAL = {0: 1, 1: 2, 2: 1, 3: 1, 4: 2, 5: 2, 6: 2, 7: 2, 8: 1, 9: 1, 10: 2}
NUM_PARAMS = {0: 3, 1: 4, 2: 4, 3: 5, 4: 8, 5: 8, 6: 12, 7: 5, 8: 4, 9: 5, 10: 12}
FIELDS = ("success", "qvec", "tvec", "camera_params", "num_inliers", "num_trials", "focal_factor", "inlier_mask",
          "covariance")


def flags(rf, re, **more):
    return dict(refine_focal_length=int(rf), refine_extra_params=int(re), **more)


def wrong_camera(sc, focal=1.0, extra=None):
    """The scene with every camera's focal lengths multiplied by `focal` and, with `extra`, its extra parameters
    multiplied by it (0: the distortion starts at zero).  The scene keeps the true cameras as true_params."""
    prm = []
    for m, p in zip(sc["camera_models"], sc["camera_params"]):
        p = np.array(p, np.float64)
        nf = NUM_FOCAL[int(m)]
        p[:nf] *= focal
        if extra is not None:
            p[nf + 2:] *= extra
        prm.append(p)
    return dict(sc, camera_params=prm, true_params=[np.array(p, np.float64) for p in sc["camera_params"]])


def refine_cases():
    """name -> ("refine", scene with start_q / start_t / mask, None, refinement options, return_covariance)"""
    c = {}
    # every model under every flag pattern (nv = 0 included), the focal length 5 % off
    for m in range(11):
        sc = wrong_camera(start(scene(1000 + m, 1, 120, outlier_frac=0.2, noise_px=1.0, model=m), m), focal=1.05)
        for rf, re in FLAGS:
            c[f"model{m}_f{rf}e{re}"] = ("refine", sc, None, flags(rf, re), (m + rf + re) % 2 == 0)
    # all eleven models in one call, in both orders
    every = wrong_camera(start(concat(*[scene(1020 + m, 1, 60 + 7 * m, outlier_frac=0.1, noise_px=0.5, model=m)
                                        for m in range(11)]), 20), focal=0.95)
    c["all_models"] = ("refine", every, None, BOTH, True)
    rev = subset(every, list(range(10, -1, -1)))
    off = every["offsets"].astype(np.int64)
    rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in range(10, -1, -1)])
    c["all_models_reversed"] = ("refine", dict(rev, start_q=every["start_q"][::-1].copy(),
                                               start_t=every["start_t"][::-1].copy(), mask=every["mask"][rows]),
                                None, BOTH, True)
    # the lane edges of the sums over inliers: set bits out of 65 / 130 correspondences (OPENCV, K = 12)
    for k, n in ((0, 65), (1, 65), (2, 65), (3, 65), (63, 65), (64, 65), (65, 65), (129, 130)):
        sc = wrong_camera(start(scene(1040, 1, n, outlier_frac=0.0, noise_px=1.0, model=4), 40, count=k), focal=1.02)
        c[f"mask{k}of{n}"] = ("refine", sc, None, BOTH, False)
        c[f"mask{k}of{n}_cov"] = ("refine", sc, None, BOTH, True)
    # fewer residuals than columns (K = 16): LM runs on its damping; the covariance's rank rule fails the query
    for k in (3, 7):
        sc = wrong_camera(start(scene(1050, 1, 60, outlier_frac=0.0, noise_px=0.5, model=6), 50, count=k), focal=1.02)
        c[f"few{k}"] = ("refine", sc, None, dict(BOTH, gradient_tolerance=0.0), False)
        c[f"few{k}_cov"] = ("refine", sc, None, dict(BOTH, gradient_tolerance=0.0), True)
    # a focal length far off; distortion starting at zero and at the truth
    for name, f in (("half", 0.5), ("double", 2.0)):
        sc = wrong_camera(start(scene(1060, 1, 150, outlier_frac=0.0, noise_px=0.0, model=2), 60), focal=f)
        c[f"focal_{name}"] = ("refine", sc, None, dict(BOTH, gradient_tolerance=0.0), True)
    base = start(scene(1061, 1, 150, outlier_frac=0.0, noise_px=0.3, model=4), 61)
    c["distortion_zero"] = ("refine", wrong_camera(base, extra=0.0), None, dict(BOTH, gradient_tolerance=0.0), True)
    c["distortion_truth"] = ("refine", wrong_camera(base), None, dict(BOTH, gradient_tolerance=0.0), True)
    # NaN / inf in the data: a failed query, never an error; the query beside it is untouched
    two = wrong_camera(start(scene(1062, 2, 60, outlier_frac=0.2, model=3), 62), focal=1.03)
    k_in = int(np.flatnonzero(two["mask"])[3])
    p2 = two["points2D"].copy()
    p2[k_in, 0] = np.nan
    c["nan_pixel"] = ("refine", dict(two, points2D=p2), None, BOTH, True)
    p3 = two["points3D"].copy()
    p3[k_in, 2] = np.inf
    c["inf_point"] = ("refine", dict(two, points3D=p3), None, BOTH, True)
    q = two["start_q"].copy()
    q[0, 1] = np.nan
    c["nan_pose"] = ("refine", dict(two, start_q=q), None, BOTH, True)
    prm = [p.copy() for p in two["camera_params"]]
    prm[0][3] = np.inf
    c["inf_param"] = ("refine", dict(two, camera_params=prm), None, BOTH, True)
    prm = [p.copy() for p in two["camera_params"]]
    prm[0][0] = np.nan
    c["nan_focal"] = ("refine", dict(two, camera_params=prm), None, BOTH, True)
    # a point behind the camera among the inliers
    sc = start(scene(1063, 1, 80, outlier_frac=0.0, noise_px=0.5, model=2, behind_frac=0.05), 63)
    c["behind"] = ("refine", wrong_camera(dict(sc, mask=np.ones(80, bool)), focal=1.02), None, BOTH, True)
    # the solver's exits, each with the options that force it (the CPU suite checks the names against the trace)
    near = wrong_camera(start(scene(1070, 1, 100, outlier_frac=0.2, noise_px=1.0, model=2), 70), focal=1.05)
    exact = wrong_camera(start(scene(1071, 1, 100, outlier_frac=0.0, noise_px=0.0, model=2), 71, rot=0, trans=0))
    c["exit_gradient_at_start"] = ("refine", exact, None, BOTH, True)
    c["exit_gradient_after_step"] = ("refine", near, None, dict(BOTH, gradient_tolerance=30.0), True)
    for it in (0, 1, 2):
        c[f"exit_max_iterations{it}"] = ("refine", near, None, dict(BOTH_TIGHT, max_num_iterations=it), True)
    c["exit_parameter_tolerance"] = ("refine", wrong_camera(start(scene(1072, 1, 100, outlier_frac=0.0, noise_px=0.0,
                                                                        model=2), 72), focal=1.05), None,
                                     dict(BOTH_TIGHT), True)
    c["exit_function_tolerance"] = ("refine", near, None, dict(BOTH_TIGHT), True)
    sc = wrong_camera(start(scene(1075, 1, 60, outlier_frac=0.0, noise_px=1.0), 75), focal=1.05)
    c["exit_invalid_steps"] = ("refine", dict(sc, start_t=np.zeros((1, 3))), None,
                               dict(BOTH_TIGHT, loss_function_scale=1e-120), True)
    t = near["start_t"].copy()
    t[0, 0] = np.inf
    c["exit_not_finite_start"] = ("refine", dict(near, start_t=t), None, BOTH, True)
    return c


EXPECTED_EXITS = {
    "exit_gradient_at_start": "GRADIENT_AT_START", "exit_gradient_after_step": "GRADIENT_AFTER_STEP",
    "exit_max_iterations0": "MAX_ITERATIONS", "exit_max_iterations1": "MAX_ITERATIONS",
    "exit_max_iterations2": "MAX_ITERATIONS", "exit_parameter_tolerance": "PARAMETER_TOLERANCE",
    "exit_function_tolerance": "FUNCTION_TOLERANCE", "exit_invalid_steps": "INVALID_STEPS",
    "exit_not_finite_start": "NOT_FINITE_START", "mask0of65": "NOTHING_TO_REFINE",
}


def estimate_cases():
    """name -> ("estimate", scene, estimation options, refinement options, return_covariance)"""
    c = {}
    sc = wrong_camera(scene(1080, 2, 150, outlier_frac=0.2, model=2), focal=1.0)
    c["estimate_plain"] = ("estimate", sc, FAST, BOTH, True)
    c["estimate_plain_fixed_camera"] = ("estimate", sc, FAST, {}, True)
    for m in (0, 4, 8):
        sc = wrong_camera(scene(1081 + m, 1, 150, outlier_frac=0.2, model=m), focal=0.7)
        c[f"estimate_focal_model{m}"] = ("estimate", sc, FOCAL4, BOTH, True)
    c["estimate_focal_fixed_camera"] = ("estimate", wrong_camera(scene(1081, 1, 150, outlier_frac=0.2, model=0), focal=0.7),
                                        FOCAL4, {}, True)
    c["estimate_all_factors_fail"] = ("estimate", concat(scene(901, 1, 2, outlier_frac=0.0, noise_px=0.0),
                                                         collinear(902, 60)), FOCAL4, BOTH, True)
    c["estimate_empty_and_two_points"] = ("estimate", concat(scene(1090, 1, 80, outlier_frac=0.2, model=3), empty_query(),
                                                             scene(1091, 1, 2, outlier_frac=0.0, noise_px=0.0),
                                                             scene(1092, 1, 90, outlier_frac=0.1, model=9)), FAST, BOTH,
                                          True)
    return c


CASES = {**refine_cases(), **estimate_cases()}


def run(name, estimate, refine, **kw):
    """The case through `estimate` / `refine`: the reference's functions or a Context's methods."""
    kind, sc, est, rf, cov = CASES[name]
    args = (sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"], sc["points3D"])
    if kind == "estimate":
        return estimate(*args, est, rf, cov, **kw)
    return refine(*args, sc["start_q"], sc["start_t"], sc["mask"], rf, cov, **kw)


def digest(result) -> str:
    """sha256 over the result's FIELDS, each as name, dtype, shape and bytes."""
    import hashlib
    h = hashlib.sha256()
    for k in FIELDS:
        if k in result:
            a = np.ascontiguousarray(result[k])
            h.update(f"{k}:{a.dtype.str}:{a.shape}:".encode())
            h.update(a.tobytes())
    return h.hexdigest()


def same(a, b, fields=FIELDS):
    """The names of the fields (present in both) whose bytes differ."""
    return [k for k in fields if k in a and k in b
            and np.ascontiguousarray(a[k]).tobytes() != np.ascontiguousarray(b[k]).tobytes()]
