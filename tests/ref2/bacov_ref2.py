"""An independent numpy restatement of the bundle-adjustment covariance for tests/test_ba_covariance_cpu.py:
a dense Jacobian of tests/ba_scipy.py's residual by central differences (the same parametrisation: Ceres' Plus on the
start quaternion, the same constant masks), the loss as section 15.4's corrector sqrt(rho') on each observation's rows,
then inv(J^T J + damping on the points' diagonal) restricted to the blocks.  No Schur complement, no Cholesky, no written
order: numpy's LAPACK on the full system.  ba_scipy restates the polynomial camera models 0 to 4; the other six are restated
here, again in numpy and not taken from the reference."""
from __future__ import annotations

import numpy as np

import ba_scipy
from ba_cases import NUM_FOCAL, quat_plus, rotate


def project(model, p, Xc):
    if model <= 4:
        return ba_scipy.project(model, p, Xc)
    u, v = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    nf = NUM_FOCAL[model]
    f1, f2, c1, c2 = p[0], p[nf - 1], p[nf], p[nf + 1]
    e = p[nf + 2:]
    r = np.sqrt(u * u + v * v)
    if model == 7:  # FOV (the general branch: omega and the radius away from 0)
        factor = np.arctan(r * 2.0 * np.tan(e[0] / 2.0)) / (r * e[0])
        return np.stack([f1 * u * factor + c1, f2 * v * factor + c2], axis=1)
    if model == 6:  # FULL_OPENCV
        r2 = r * r
        rad = (1 + e[0] * r2 + e[1] * r2 ** 2 + e[4] * r2 ** 3) / (1 + e[5] * r2 + e[6] * r2 ** 2 + e[7] * r2 ** 3)
        du = u * rad + 2 * e[2] * u * v + e[3] * (r2 + 2 * u * u) - u
        dv = v * rad + 2 * e[3] * u * v + e[2] * (r2 + 2 * v * v) - v
        return np.stack([f1 * (u + du) + c1, f2 * (v + dv) + c2], axis=1)
    theta = np.arctan(r)
    if model == 10:  # THIN_PRISM_FISHEYE: the equidistant point first, then the polynomial
        u, v = theta * u / r, theta * v / r
        r2 = u * u + v * v
        rad = e[0] * r2 + e[1] * r2 ** 2 + e[4] * r2 ** 3 + e[5] * r2 ** 4
        du = u * rad + 2 * e[2] * u * v + e[3] * (r2 + 2 * u * u) + e[6] * r2
        dv = v * rad + 2 * e[3] * u * v + e[2] * (r2 + 2 * v * v) + e[7] * r2
        return np.stack([f1 * (u + du) + c1, f2 * (v + dv) + c2], axis=1)
    k = {5: 4, 8: 1, 9: 2}[model]  # OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE
    thetad = theta * (1 + sum(e[n] * theta ** (2 * n + 2) for n in range(k)))
    return np.stack([f1 * u * thetad / r + c1, f2 * v * thetad / r + c2], axis=1)


def rho1(loss, scale, s):
    b = scale * scale
    if loss == 0:
        return np.ones_like(s)
    return 1.0 / np.sqrt(1.0 + s / b) if loss == 1 else 1.0 / (1.0 + s / b)


class Problem(ba_scipy.Problem):
    """ba_scipy's parametrisation with all eleven models and constant points; residuals of a subset of observations"""

    def __init__(self, *args, point_const=None):
        super().__init__(*args)
        npts = self.X0.shape[0]
        self.point_var = np.ones(npts, bool) if point_const is None else np.asarray(point_const).reshape(-1) == 0
        self.m = sum(len(v) for v in self.pvar) + sum(len(v) for v in self.cvar)

    def residuals_of(self, sel, image_delta=None, camera_delta=None, point_delta=None):
        """unweighted residuals (len(sel), 2) with one image's tangent step, one camera's parameter step or one point's
        step applied: (index, vector)"""
        out = np.zeros((sel.size, 2))
        for i in np.unique(self.oi[sel]):
            at = np.flatnonzero(self.oi[sel] == i)
            q, t = self.q0[i], self.t0[i]
            if image_delta is not None and image_delta[0] == i:
                q, t = quat_plus(q, image_delta[1][:3]), t + image_delta[1][3:]
            c = self.icam[i]
            prm = self.prm0[c]
            if camera_delta is not None and camera_delta[0] == c:
                prm = prm + camera_delta[1]
            X = self.X0[self.op[sel[at]]]
            if point_delta is not None:
                X = X + (self.op[sel[at]] == point_delta[0])[:, None] * point_delta[1]
            out[at] = project(self.models[c], prm, rotate(q, X) + t) - self.xy[sel[at]]
        return out

    def jacobian(self, loss=0, loss_scale=1.0):
        """(J, point column starts): the columns are the poses' variable coordinates image by image, the cameras'
        variable slots, then three per variable point"""
        nobs = self.oi.size
        every = np.arange(nobs)
        r0 = self.residuals_of(every)
        w = np.sqrt(rho1(loss, loss_scale, (r0 * r0).sum(axis=1)))
        pstart = {}
        n = self.m
        for j in np.flatnonzero(self.point_var):
            pstart[int(j)] = n
            n += 3
        J = np.zeros((2 * nobs, n))

        def column(col, sel, h, **kw_plus_minus):
            (name, (index, vec)), = kw_plus_minus.items()
            d = (self.residuals_of(sel, **{name: (index, vec * h)}) - self.residuals_of(sel, **{name: (index, -vec * h)})) / (2 * h)
            d = d * w[sel][:, None]
            J[2 * sel, col], J[2 * sel + 1, col] = d[:, 0], d[:, 1]
        col = 0
        for i, var in enumerate(self.pvar):
            sel = np.flatnonzero(self.oi == i)
            for k in var:
                column(col, sel, 1e-6, image_delta=(i, np.eye(6)[k]))
                col += 1
        for c, var in enumerate(self.cvar):
            sel = np.flatnonzero(self.icam[self.oi] == c)
            for k in var:
                column(col, sel, 1e-6 * max(1.0, abs(self.prm0[c][k])), camera_delta=(c, np.eye(len(self.prm0[c]))[k]))
                col += 1
        for j, at in pstart.items():
            sel = np.flatnonzero(self.op == j)
            for k in range(3):
                column(at + k, sel, 1e-6, point_delta=(j, np.eye(3)[k]))
        return J, pstart


def ba_covariance(camera_models, camera_params, camera_const, image_cameras, qvec, tvec, pose_const, xyz, obs_image,
                  obs_point, obs_xy, options=None, point_const=None):
    """matrix (m, m) and {point index: 3 x 3} of the problem by the dense inverse"""
    o = dict(loss_function_type=0, loss_function_scale=1.0, damping=1e-8)
    o.update(options or {})
    loss = o["loss_function_type"]
    loss = {"TRIVIAL": 0, "SOFT_L1": 1, "CAUCHY": 2}[loss.upper()] if isinstance(loss, str) else int(loss)
    pb = Problem(camera_models, camera_params, camera_const, image_cameras, qvec, tvec, pose_const, xyz, obs_image,
                 obs_point, obs_xy, point_const=point_const)
    J, pstart = pb.jacobian(loss, o["loss_function_scale"])
    H = J.T @ J
    for at in pstart.values():
        H[at:at + 3, at:at + 3] += o["damping"] * np.eye(3)
    # the columns mix units (radians, pixels, distortion coefficients): invert the system scaled to a unit diagonal
    d = 1.0 / np.sqrt(np.diag(H))
    cov = d[:, None] * np.linalg.inv(d[:, None] * H * d[None, :]) * d[None, :]
    cov = 0.5 * (cov + cov.T)
    return cov[:pb.m, :pb.m], {j: cov[at:at + 3, at:at + 3] for j, at in pstart.items()}


def deviation(result, matrix2, points2):
    """The largest deviation of a reference result from this restatement over the owners' diagonal blocks and the point
    blocks, each relative to the largest entry of this restatement's block."""
    worst = 0.0
    owner = np.asarray(result["column_owner"])
    for o in np.unique(owner):
        cols = np.flatnonzero(owner == o)
        a, b = result["matrix"][np.ix_(cols, cols)], matrix2[np.ix_(cols, cols)]
        worst = max(worst, float(np.abs(a - b).max() / np.abs(b).max()))
    for j, b in points2.items():
        worst = max(worst, float(np.abs(result["point_cov"][j] - b).max() / np.abs(b).max()))
    return worst
