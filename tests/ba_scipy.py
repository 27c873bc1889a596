"""An independent solver for the accuracy checks of tests/test_ba_cpu.py: scipy.optimize.least_squares
on the same parametrisation as section 15: the rotation as a 3-vector update of the start quaternion (Ceres' Plus), the
same constant masks, the same loss as a rescaling of each observation's residual so that its squared norm is rho(|r|^2).
The camera models are restated here in numpy (the polynomial ones the accuracy cases use), not taken from the
reference."""
from __future__ import annotations

import numpy as np
from scipy.optimize import least_squares

from ba_cases import NUM_FOCAL, quat_plus, rotate


def project(model, p, Xc):
    u, v = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    nf = NUM_FOCAL[model]
    f1, f2, c1, c2 = p[0], p[nf - 1], p[nf], p[nf + 1]
    e = p[nf + 2:]
    r2 = u * u + v * v
    if model in (0, 1):
        du = dv = 0.0
    elif model == 2:
        du, dv = u * e[0] * r2, v * e[0] * r2
    elif model == 3:
        rad = e[0] * r2 + e[1] * r2 * r2
        du, dv = u * rad, v * rad
    elif model == 4:
        rad = e[0] * r2 + e[1] * r2 * r2
        du = u * rad + 2 * e[2] * u * v + e[3] * (r2 + 2 * u * u)
        dv = v * rad + 2 * e[3] * u * v + e[2] * (r2 + 2 * v * v)
    else:
        raise NotImplementedError(model)
    return np.stack([f1 * (u + du) + c1, f2 * (v + dv) + c2], axis=1)


def rho(loss, scale, s):
    b = scale * scale
    if loss == "TRIVIAL":
        return s
    if loss == "SOFT_L1":
        return 2.0 * b * (np.sqrt(1.0 + s / b) - 1.0)
    return b * np.log1p(s / b)


class Problem:
    def __init__(self, models, camera_params, camera_const, image_cameras, qvec, tvec, pose_const, xyz, obs_image,
                 obs_point, obs_xy, loss="TRIVIAL", loss_scale=1.0):
        self.models = list(models)
        self.prm0 = [np.array(p, np.float64) for p in camera_params]
        self.cvar = [np.flatnonzero(np.asarray(camera_const)[c, :len(p)] == 0) for c, p in enumerate(self.prm0)]
        self.icam = np.asarray(image_cameras)
        self.q0, self.t0 = np.array(qvec, np.float64), np.array(tvec, np.float64)
        self.pvar = [np.flatnonzero(np.asarray(pose_const)[i] == 0) for i in range(len(self.icam))]
        self.X0 = np.array(xyz, np.float64)
        self.oi, self.op, self.xy = np.asarray(obs_image), np.asarray(obs_point), np.asarray(obs_xy, np.float64)
        self.loss, self.loss_scale = loss, loss_scale
        self.n = sum(len(v) for v in self.pvar) + sum(len(v) for v in self.cvar) + self.X0.size

    def unpack(self, x):
        at = 0
        q, t = self.q0.copy(), self.t0.copy()
        for i, var in enumerate(self.pvar):
            d = np.zeros(6)
            d[var] = x[at:at + len(var)]
            at += len(var)
            q[i] = quat_plus(self.q0[i], d[:3])
            t[i] = self.t0[i] + d[3:]
        prm = [p.copy() for p in self.prm0]
        for c, var in enumerate(self.cvar):
            prm[c][var] += x[at:at + len(var)]
            at += len(var)
        X = self.X0 + x[at:].reshape(-1, 3)
        return q, t, prm, X

    def residuals(self, x):
        q, t, prm, X = self.unpack(x)
        out = np.zeros((self.oi.size, 2))
        for i in range(len(self.icam)):
            sel = np.flatnonzero(self.oi == i)
            if sel.size == 0:
                continue
            qi = q[i]
            Xc = rotate(qi, X[self.op[sel]]) + t[i]
            c = self.icam[i]
            out[sel] = project(self.models[c], prm[c], Xc) - self.xy[sel]
        s = (out * out).sum(axis=1)
        w = np.sqrt(np.where(s > 0, rho(self.loss, self.loss_scale, s) / np.where(s > 0, s, 1.0), 1.0))
        return (out * w[:, None]).reshape(-1)

    def solve(self, tol):
        r = least_squares(self.residuals, np.zeros(self.n), method="trf", x_scale="jac", ftol=tol, xtol=tol, gtol=tol,
                          max_nfev=2000)
        return r.cost, self.unpack(r.x)
