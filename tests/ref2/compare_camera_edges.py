"""Measure the CPU references against the mpmath restatement (tests/ref2/camera_edges_ref2.py) on every case of
tests/camera_edge_cases.py and record the worst deviation per (regime, model, quantity) in
tests/ref2/camera_edges_deviation_budget.json, which tests/test_camera_edges_cpu.py reads its bounds from.  Run by hand,
like tests/ref2/compare.py, after a change to a reference or to the cases:

    python tests/ref2/compare_camera_edges.py

Units.  A pixel value (residual, abspose_pixel) deviates in ulps of the coordinate's scale max(|x|, |c|, |f u|): the pixel
is the sum f (u + du) + c, rounded at the size of its terms, and the fisheye family's du is -u plus a small number, so for
a wide point u + du is rounded at the size of u.  A squared error deviates in units of what one such ulp in either
coordinate moves it by, 2 (|r_x| ulp_x + |r_y| ulp_y), plus its own ulp.  A Jacobian block deviates in units of
DBL_EPSILON times the largest entry of its row of the block.  The lift's reprojection is in pixels.

Jacobians.  Every case compares the three blocks of ba_ref_lib.observation as one row of 21 entries against the largest
entry of that whole row (jacobian_row): the row always holds the principal point's 1, so the measure stays defined where
a block's own rows are rounding noise (a radius beyond 2^66, tan(omega / 2) beyond 1e6, the rational pole).  The cases
that run iterations (camera_edge_cases.iteration_safe) are also compared block by block against the block row's own
largest entry (jacobian_pose, jacobian_camera, jacobian_point), and abspose_ref's 2 x 7 block likewise
(abspose_jacobian); that sharper measure is meaningless where the projection has lost its radial rank, which is why the
other 31 cases have only jacobian_row.  depth_tiny alone has no Jacobian comparison: at r >= 2^66 forward mode on
COLMAP's u + (u thetad / r - u) adds a derivative of 2^67 to a term of 2^133 whose ulp is 2^80, and the reference's pose
and point blocks come out as exact zeros where the function's slope is 1836; there is nothing to hold them to.
Every observation of a case is compared."""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import camera_edge_cases as ce  # noqa: E402
from ref2 import camera_edges_ref2 as r2  # noqa: E402

BUDGET = Path(__file__).resolve().parent / "camera_edges_deviation_budget.json"
EPS = float(np.finfo(np.float64).eps)
VALUE_QUANTITIES = ("residual", "sq_error_ba", "sq_error_filter", "abspose_pixel")
JACOBIAN_QUANTITIES = ("jacobian_pose", "jacobian_camera", "jacobian_point", "abspose_jacobian")
ROW_QUANTITY = "jacobian_row"
POLE = 1e-12  # |denominator| below this: the pixel is a quotient by a rounding error, compared with nothing


def jacobian_rows(sc):
    """the observations whose Jacobians are compared: all of them"""
    return list(range(len(sc["obs_image"])))


def _block_dev(A, B):
    scale = np.abs(B).max(axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        d = np.abs(A - B) / (EPS * np.where(scale > 0, scale, 1.0))
    return d


def measure(name):
    """{quantity: worst deviation}, the names of the reference's non-finite entries, of the ill-conditioned ones, and
    {quantity: number of entries compared}"""
    import abspose_ref_lib
    import ba_ref_lib
    sc = ce.case_scene(name)
    m, prm, nf = sc["model"], sc["camera_params"][0], ce.NUM_FOCAL[sc["model"]]
    op = ce.obs_point(sc)
    Xc = ce.camera_frame(sc)
    worst, counts, nonfinite, ill = {}, {}, [], []

    def note(q, dev, tag):
        dev = np.atleast_1d(np.asarray(dev, np.float64))
        fin = np.isfinite(dev)
        if not fin.all():
            nonfinite.append(f"{name}#{tag}:{q}")
        counts[q] = counts.get(q, 0) + int(fin.sum())
        if fin.any():
            worst[q] = max(worst.get(q, 0.0), float(dev[fin].max()))

    e2_filter = ce.filter_reference(name, True)["obs_sq_error"]
    jrows = set(jacobian_rows(sc)) if ce.regime(name) != "depth_tiny" else set()
    blocks = ce.iteration_safe(name)
    for k in range(len(op)):
        i = int(sc["obs_image"][k])
        q, t, X, xy = sc["qvec"][i], sc["tvec"][i], sc["xyz"][op[k]], sc["obs_xy"][k]
        if m == ce._M["FULL_OPENCV"]:
            with np.errstate(all="ignore"):
                u, v = Xc[k, 0] / Xc[k, 2], Xc[k, 1] / Xc[k, 2]
            if abs(ce.rational_denominator(prm[nf + 2:], u * u + v * v)) < POLE:
                ill.append(f"{name}#{k}")
                continue
        x, y, _ = r2.pixel(m, prm, q, t, X)
        with np.errstate(all="ignore"):
            u, v = Xc[k, 0] / Xc[k, 2], Xc[k, 1] / Xc[k, 2]
            ux = float(np.spacing(max(abs(float(x)), abs(prm[nf]), abs(prm[0] * u))))
            uy = float(np.spacing(max(abs(float(y)), abs(prm[nf + 1]), abs(prm[nf - 1] * v))))
        rx, ry = x - r2.M(xy[0]), y - r2.M(xy[1])
        e2 = rx * rx + ry * ry
        ue = 2.0 * (abs(float(rx)) * ux + abs(float(ry)) * uy) + float(np.spacing(float(e2)))
        _, r, Jp, Jc, Jx = ba_ref_lib.observation(m, prm, q, t, X, xy)
        note("residual", [abs(float(rx - r2.M(r[0]))) / ux, abs(float(ry - r2.M(r[1]))) / uy] if np.isfinite(r).all()
             else [np.nan], k)
        cost = ba_ref_lib.observation(m, prm, q, t, X, xy, jac=False)[0]
        note("sq_error_ba", abs(float(e2 - r2.M(2.0 * cost))) / ue if np.isfinite(cost) else np.nan, k)
        want = r2.sq_error(m, prm, q, t, X, xy)
        if float(want) == ce.DBL_MAX or e2_filter[k] == ce.DBL_MAX:
            note("sq_error_filter", 0.0 if float(want) == e2_filter[k] else np.inf, k)
            assert float(want) == e2_filter[k], (name, k, "the depth test")
        else:
            note("sq_error_filter", abs(float(want - r2.M(e2_filter[k]))) / ue if np.isfinite(e2_filter[k]) else np.nan, k)
        pxy, J7 = abspose_ref_lib.project(m, prm, q, t, X)
        note("abspose_pixel", [abs(float(x - r2.M(pxy[0]))) / ux, abs(float(y - r2.M(pxy[1]))) / uy]
             if np.isfinite(pxy).all() else [np.nan], k)
        if k in jrows:
            Bp, Bc, Bx = r2.jacobians(m, prm, q, t, X)
            note(ROW_QUANTITY, _block_dev(np.hstack([Jp, Jc, Jx]), np.hstack([Bp, Bc, Bx])), k)
        if k in jrows and blocks:
            for qn, A, B in (("jacobian_pose", Jp, Bp), ("jacobian_camera", Jc, Bc), ("jacobian_point", Jx, Bx),
                             ("abspose_jacobian", J7, r2.pose_jacobian7(m, prm, q, t, X))):
                note(qn, _block_dev(A, B), k)
    return worst, nonfinite, ill, counts


def lift_measure(model):
    """strong_poly's lifts: the float64 Newton restatement's iteration counts, whether it reproduces the oracle's bits,
    and the reprojection (mpmath) of the lifts in pixels"""
    prm = ce.strong_params(model)
    px = ce.strong_pixels(model)
    lifted, _ = ce.lift_reference(model)
    its, same = np.zeros(len(px), int), np.zeros(len(px), bool)
    res = np.full(len(px), np.nan)
    p = [r2.M(v) for v in prm]
    for k in range(len(px)):
        u, v, its[k] = r2.newton_lift(model, prm, px[k])
        same[k] = np.array_equal(ce.bits([u, v]), ce.bits(lifted[k]))
        if np.isfinite(lifted[k]).all():
            x, y, _ = r2.img_from_cam(model, p, r2.M(lifted[k, 0]), r2.M(lifted[k, 1]))
            res[k] = float(max(abs(x - r2.M(px[k, 0])), abs(y - r2.M(px[k, 1]))))
    return dict(iterations=its, same_bits=same, reprojection=res, nonfinite=~np.isfinite(lifted).all(axis=1))


def project_measure(model):
    """the oracle's img_from_cam on strong_uv against mpmath, in ulps of the coordinate's scale"""
    prm = ce.strong_params(model)
    nf = ce.NUM_FOCAL[model]
    uv = ce.strong_uv(model)
    _, got = ce.lift_reference(model)
    p = [r2.M(v) for v in prm]
    worst = 0.0
    for k in range(len(uv)):
        x, y, _ = r2.img_from_cam(model, p, r2.M(uv[k, 0]), r2.M(uv[k, 1]))
        ux = float(np.spacing(max(abs(float(x)), prm[nf], abs(prm[0] * uv[k, 0]))))
        uy = float(np.spacing(max(abs(float(y)), prm[nf + 1], abs(prm[nf - 1] * uv[k, 1]))))
        worst = max(worst, abs(float(x - r2.M(got[k, 0]))) / ux, abs(float(y - r2.M(got[k, 1]))) / uy)
    return worst


def key(name):
    return f"{ce.regime(name)}/{ce.MODEL_NAMES[ce.SPECS[name][1]]}"


def main():
    worst, nonfinite, ill = {}, [], []
    for name in ce.CASES:
        w, nfin, il, _ = measure(name)
        slot = worst.setdefault(key(name), {})
        for q, v in w.items():
            slot[q] = max(slot.get(q, 0.0), v)
        nonfinite += nfin
        ill += il
    lifts = {}
    for m in ce.POLYNOMIAL:
        lm = lift_measure(m)
        inside = np.arange(len(lm["iterations"])) < 126
        lifts[ce.MODEL_NAMES[m]] = dict(
            worst_reprojection_inside_fold_px=float(np.nanmax(lm["reprojection"][inside])),
            max_iterations_inside_fold=int(lm["iterations"][inside].max()),
            ran_100_iterations=int((lm["iterations"] == 100).sum()), nonfinite_lifts=int(lm["nonfinite"].sum()),
            newton_restatement_same_bits=int(lm["same_bits"].sum()), img_from_cam_ulps=project_measure(m))
    out = dict(units=dict(values="ulps of max(|x|, |c|, |f u|); squared errors: 2 (|r_x| ulp_x + |r_y| ulp_y) + ulp(e2)",
                          jacobians="DBL_EPSILON times the largest entry of the block's row", lifts="pixels"),
               worst={k: {q: round(v, 3) for q, v in sorted(w.items())} for k, w in sorted(worst.items())},
               nonfinite=sorted(nonfinite), ill_conditioned=sorted(ill), lifts=lifts)
    BUDGET.write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {BUDGET}")
    for q in VALUE_QUANTITIES + JACOBIAN_QUANTITIES + (ROW_QUANTITY,):
        vals = [(w[q], k) for k, w in worst.items() if q in w]
        print(f"{q:18s} worst {max(vals)[0]:.3g} in {max(vals)[1]}")


if __name__ == "__main__":
    main()
