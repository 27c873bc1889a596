"""Independent checks of the joint pose and camera refinement's CPU reference (tests/absrefine_ref):

* derivatives: the reference's forward-mode Jacobian of a pixel by (qx, qy, qz, qw, tx, ty, tz, variable camera
  parameters) against central differences of the reference's own pixel, in float64 with a step per column;
* the solver: scipy.optimize.least_squares(loss="cauchy") over the pose tangent and the variable camera columns from the
  reference's start, against the reference's final cost, and the refined camera and pose against the truth.

    python tests/ref2/absrefine_ref2.py        # measures and writes tests/ref2/absrefine_deviation_budget.json
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
BUDGET = ROOT / "tests" / "ref2" / "absrefine_deviation_budget.json"
if __name__ == "__main__":
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import abspose_cases  # noqa: E402
import absrefine_cases as cases  # noqa: E402
import absrefine_ref_lib as ref  # noqa: E402

# camera parameters per model for the derivative probe; FOV three times, one per branch of its factor
PROBE_CAMERAS = [
    (0, [800.0, 500.0, 400.0]), (1, [800.0, 808.0, 500.0, 400.0]), (2, [800.0, 500.0, 400.0, 0.05]),
    (3, [800.0, 500.0, 400.0, 0.05, -0.02]), (4, [800.0, 808.0, 500.0, 400.0, 0.05, -0.02, 1e-3, -1e-3]),
    (5, [800.0, 808.0, 500.0, 400.0, 0.02, -0.01, 3e-3, -1e-3]),
    (6, [800.0, 808.0, 500.0, 400.0, 0.05, -0.02, 1e-3, -1e-3, 5e-3, 0.01, -5e-3, 2e-3]),
    (7, [800.0, 808.0, 500.0, 400.0, 0.6]),      # FOV: omega^2 >= 1e-4, radius^2 >= 1e-4
    (7, [800.0, 808.0, 500.0, 400.0, 0.005]),    # FOV: omega^2 < 1e-4
    (8, [800.0, 500.0, 400.0, 0.02]), (9, [800.0, 500.0, 400.0, 0.02, -0.01]),
    (10, [800.0, 808.0, 500.0, 400.0, 0.02, -0.01, 1e-3, -1e-3, 2e-3, 1e-3, 5e-4, -5e-4]),
]
FOV_NEAR_AXIS = (7, [800.0, 808.0, 500.0, 400.0, 0.6])  # with points of radius^2 < 1e-4: the third branch


def probe_points(rng, near_axis=False):
    """a pose near the identity and eight points in front of it"""
    q = np.array([0.02, -0.03, 0.01, 1.0]) + rng.normal(scale=0.01, size=4)
    t = np.array([0.1, -0.2, 0.3])
    spread = 0.004 if near_axis else 0.4
    X = np.column_stack([rng.uniform(-spread, spread, 8) * 5.0, rng.uniform(-spread, spread, 8) * 5.0,
                         rng.uniform(4.0, 6.0, 8)])
    if near_axis:  # undo the pose so that the camera-frame points stay near the axis
        q, t = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
    return q, t, X


def derivative_deviation(model, params, near_axis=False, seed=0):
    """max over points, rows and columns of |J_forward - J_central| / max(1, |J_forward|)"""
    rng = np.random.default_rng(seed)
    q, t, X = probe_points(rng, near_axis)
    worst = 0.0
    for x in X:
        _, J, idx = ref.project(model, params, q, t, x, True, True)
        assert J.shape[1] == 7 + len(idx)
        if near_axis:
            assert (x[0] ** 2 + x[1] ** 2) / x[2] ** 2 < 1e-4
        for col in range(J.shape[1]):
            def at(h):
                qq, tt, pp = q.copy(), t.copy(), np.array(params, np.float64)
                if col < 4:
                    qq[col] += h
                elif col < 7:
                    tt[col - 4] += h
                else:
                    pp[idx[col - 7]] += h
                return ref.project(model, pp, qq, tt, x, True, True)[0]
            v = q[col] if col < 4 else t[col - 4] if col < 7 else params[idx[col - 7]]
            h = 1e-6 * max(1.0, abs(v))  # about eps^(1/3) of the variable's scale
            fd = (at(h) - at(-h)) / (2.0 * h)
            worst = max(worst, float(np.max(np.abs(J[:, col] - fd) / np.maximum(1.0, np.abs(J[:, col])))))
    return worst


def measure_derivatives():
    out = {}
    for i, (m, p) in enumerate(PROBE_CAMERAS):
        out[f"model{m}" + ("_small_omega" if m == 7 and p[4] < 0.01 else "")] = derivative_deviation(m, p, seed=i)
    out["model7_near_axis"] = derivative_deviation(*FOV_NEAR_AXIS, near_axis=True, seed=20)
    return out


# ---- scipy as the independent solver ---------------------------------------------------------------------------------------
def quat_plus(q, d):
    """EigenQuaternionManifold::Plus (12.7) in numpy"""
    nd = np.linalg.norm(d)
    if nd == 0.0:
        return q.copy()
    a = np.append(np.sin(nd) / nd * d, np.cos(nd))
    x1, y1, z1, w1 = a
    x2, y2, z2, w2 = q
    return np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])


def point_norms(model, params, q, t, sc):
    """the norm of every inlier's pixel residual (the reference's projection), so that scipy's per-entry Cauchy loss is
    Ceres' loss on the squared norm of the two-vector"""
    m = np.asarray(sc["mask"], bool)
    d = ref.project_points(model, params, q, t, sc["points3D"][m]) - sc["points2D"][m]
    return np.hypot(d[:, 0], d[:, 1])


def cost(model, params, q, t, sc, scale=1.0):
    r = point_norms(model, params, q, t, sc)
    return 0.5 * scale * scale * float(np.sum(np.log1p((r / scale) ** 2)))


def scipy_refine(sc, refine_focal_length=True, refine_extra_params=True):
    """least_squares over (pose tangent at the start, variable camera columns) of a one-query scene"""
    from scipy.optimize import least_squares
    model = int(sc["camera_models"][0])
    p0 = np.array(sc["camera_params"][0], np.float64)
    idx = ref.variable_params(model, refine_focal_length, refine_extra_params)
    q0, t0 = sc["start_q"][0], sc["start_t"][0]

    def unpack(x):
        p = p0.copy()
        p[idx] = p0[idx] + x[6:]
        return p, quat_plus(q0, x[:3]), t0 + x[3:6]

    def fun(x):
        p, q, t = unpack(x)
        return point_norms(model, p, q, t, sc)

    r = least_squares(fun, np.zeros(6 + len(idx)), loss="cauchy", f_scale=1.0, x_scale="jac", method="trf", xtol=1e-15,
                      ftol=1e-15, gtol=1e-15, max_nfev=2000)
    p, q, t = unpack(r.x)
    return dict(converged=r.status > 0, cost=float(r.cost), params=p, qvec=q, tvec=t)


SOLVER_MODELS = (0, 1, 2, 8)  # (on the noisy RADIAL, OPENCV and OPENCV_FISHEYE scenes scipy itself does not converge)


def solver_scene(model, noise_px):
    sc = abspose_cases.start(abspose_cases.scene(1200 + model, 1, 120, outlier_frac=0.0, noise_px=noise_px, model=model),
                             model)
    return cases.wrong_camera(sc, focal=1.2)


def reference_refine(sc):
    return ref.refine(sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"], sc["points3D"], sc["start_q"],
                      sc["start_t"], sc["mask"], dict(cases.BOTH, gradient_tolerance=0.0))


def measure_solver():
    """noisy scenes: the reference's final cost against scipy's, (ref - scipy) / scipy; noise-free scenes with the
    focal length 20 % off: the distance of the refined focal length (relative), distortion and pose from the truth"""
    excess, focal, extra, pose = {}, {}, {}, {}
    for m in SOLVER_MODELS:
        sc = solver_scene(m, 1.0)
        got, sp = reference_refine(sc), scipy_refine(sc)
        assert got["success"][0] and sp["converged"]
        n = cases.NUM_PARAMS[m]
        c = cost(m, got["camera_params"][0, :n], got["qvec"][0], got["tvec"][0], sc)
        excess[f"model{m}"] = (c - sp["cost"]) / sp["cost"]
        sc = solver_scene(m, 0.0)
        got, sp = reference_refine(sc), scipy_refine(sc)
        assert got["success"][0] and sp["converged"]
        true, nf = sc["true_params"][0], cases.NUM_FOCAL[m]
        focal[f"model{m}"] = float(np.max(np.abs(got["camera_params"][0, :nf] / true[:nf] - 1.0)))
        extra[f"model{m}"] = float(np.max(np.abs(got["camera_params"][0, nf + 2:n] - true[nf + 2:]), initial=0.0))
        sign = 1.0 if np.dot(got["qvec"][0], sc["qvec"][0]) >= 0 else -1.0
        pose[f"model{m}"] = float(max(np.max(np.abs(sign * got["qvec"][0] - sc["qvec"][0])),
                                      np.max(np.abs(got["tvec"][0] - sc["tvec"][0]))))
    return excess, focal, extra, pose


def main():
    der = measure_derivatives()
    excess, focal, extra, pose = measure_solver()
    worst = lambda d: max(d.values())  # noqa: E731
    budget = {
        "derivatives": {"measured": der, "measured_max": worst(der), "margin": 2.0 * worst(der),
                        "what": "max |J_forward - J_central| / max(1, |J_forward|), float64 central differences, step "
                                "1e-6 max(1, |x|)"},
        "cost_excess": {"measured": excess, "measured_max": worst(excess), "margin": 2.0 * max(worst(excess), 0.0),
                        "what": "(reference cost - scipy cost) / scipy cost on noisy scenes"},
        "focal_rel": {"measured": focal, "measured_max": worst(focal), "margin": 2.0 * worst(focal),
                      "what": "max |f / f_true - 1| on noise-free scenes, focal length 20 % off at the start"},
        "extra_abs": {"measured": extra, "measured_max": worst(extra), "margin": 2.0 * worst(extra),
                      "what": "max |extra - truth| on the same scenes"},
        "pose_abs": {"measured": pose, "measured_max": worst(pose), "margin": 2.0 * worst(pose),
                     "what": "max |q - q_true|, |t - t_true| on the same scenes"},
    }
    BUDGET.write_text(json.dumps(budget, indent=1, sort_keys=True) + "\n")
    print(json.dumps({k: (v["measured_max"], v["margin"]) for k, v in budget.items()}, indent=1))


if __name__ == "__main__":
    main()
