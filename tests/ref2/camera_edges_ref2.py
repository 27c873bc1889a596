"""An independent restatement of Camera::ImgFromCam for the eleven camera models in mpmath at 60 digits, for
tests/test_camera_edges_cpu.py and tests/ref2/compare_camera_edges.py.  It is written from COLMAP's
definition of the models (DESIGN.md 12.7 / 15.3 name them) with COLMAP's branch structure, because the series branches of
FOV and the `r > epsilon` branches of the fisheye family are part of the specification; atan, tan, sin, cos and sqrt are
mpmath's own.  Nothing here shares text with tests/abspose_ref, tests/ba_ref, tests/filter_ref or the kernels' headers.

A branch is taken on the value rounded to a double (the code under test decides on doubles), and the derivatives are
central differences of the branch that the undisturbed point takes: a jet differentiates the branch it runs, and a
difference across a cut would measure the jump between a series and its function, not a slope.

newton_lift is IterativeUndistortion in float64 with its iteration count, which no reference reports."""
from __future__ import annotations

import numpy as np
from mpmath import mp, mpf

mp.dps = 60

NUM_FOCAL = [1, 2, 1, 1, 2, 2, 2, 2, 1, 1, 2]
NUM_PARAMS = [3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12]
EPS = float(np.finfo(np.float64).eps)
DBL_MAX = float(np.finfo(np.float64).max)
STEP = mpf(10) ** -15  # relative step of the central differences: truncation 1e-30, 15 of the 60 digits cancel


def M(x):
    return mpf(float(x)) if not isinstance(x, mpf) else x


def _tangential(e2, e3, u, v, r2):
    return (2 * e2 * u * v + e3 * (r2 + 2 * u * u), 2 * e3 * u * v + e2 * (r2 + 2 * v * v))


def img_from_cam(model, p, u, v, branch=None):
    """(x, y, branch) of the normalised point (u, v): branch is what the selectors chose, or, given, what they must
    choose."""
    nf = NUM_FOCAL[model]
    f1, f2, c1, c2 = p[0], p[nf - 1], p[nf], p[nf + 1]
    e = p[nf + 2:]
    r2 = u * u + v * v
    if model in (0, 1):
        return f1 * u + c1, f2 * v + c2, ()
    if model == 7:
        om = e[0]
        om2 = om * om
        if branch is None:
            branch = ("series",) if float(om2) < 1e-4 else ("radius_series",) if float(r2) < 1e-4 else ("atan",)
        if branch[0] == "series":
            factor = (om2 * r2) / 3 - om2 / 12 + 1
        elif branch[0] == "radius_series":
            th = mp.tan(om / 2)
            factor = (-2 * th * (4 * r2 * th * th - 3)) / (3 * om)
        else:
            radius = mp.sqrt(r2)
            factor = mp.atan(radius * 2 * mp.tan(om / 2)) / (radius * om)
        return f1 * (u * factor) + c1, f2 * (v * factor) + c2, branch
    if model in (5, 8, 9, 10):
        r = mp.sqrt(r2)
        if branch is None:
            branch = ("atan",) if float(r) > EPS else ("axis",)
    if model == 10:
        if branch[0] == "atan":
            th = mp.atan(r)
            u, v = th * u / r, th * v / r
        r2 = u * u + v * v
        r4 = r2 * r2
        radial = e[0] * r2 + e[1] * r4 + e[4] * r4 * r2 + e[5] * r4 * r4
        tu, tv = _tangential(e[2], e[3], u, v, r2)
        du, dv = u * radial + tu + e[6] * r2, v * radial + tv + e[7] * r2
    elif model in (5, 8, 9):
        if branch[0] == "atan":
            th = mp.atan(r)
            t2 = th * th
            k = list(e) + [0, 0, 0]
            if model == 8:
                thd = th * (1 + k[0] * t2)
            elif model == 9:
                thd = th * (1 + k[0] * t2 + k[1] * t2 * t2)
            else:
                thd = th * (1 + k[0] * t2 + k[1] * t2 ** 2 + k[2] * t2 ** 3 + k[3] * t2 ** 4)
            du, dv = u * thd / r - u, v * thd / r - v
        else:
            du, dv = mpf(0), mpf(0)
    elif model == 2:
        du, dv = u * (e[0] * r2), v * (e[0] * r2)
    elif model == 3:
        radial = e[0] * r2 + e[1] * r2 * r2
        du, dv = u * radial, v * radial
    elif model == 4:
        radial = e[0] * r2 + e[1] * r2 * r2
        tu, tv = _tangential(e[2], e[3], u, v, r2)
        du, dv = u * radial + tu, v * radial + tv
    elif model == 6:
        r4 = r2 * r2
        r6 = r4 * r2
        radial = (1 + e[0] * r2 + e[1] * r4 + e[4] * r6) / (1 + e[5] * r2 + e[6] * r4 + e[7] * r6)
        tu, tv = _tangential(e[2], e[3], u, v, r2)
        du, dv = u * radial + tu - u, v * radial + tv - v
    else:
        raise ValueError(model)
    return f1 * (u + du) + c1, f2 * (v + dv) + c2, branch if branch is not None else ()


def quat_plus(q, d):
    """EigenQuaternionManifold::Plus, q = (x, y, z, w)"""
    n = mp.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    if n == 0:
        return list(q)
    s = mp.sin(n) / n
    a = [s * d[0], s * d[1], s * d[2], mp.cos(n)]
    return [a[3] * q[0] + a[0] * q[3] + a[1] * q[2] - a[2] * q[1],
            a[3] * q[1] - a[0] * q[2] + a[1] * q[3] + a[2] * q[0],
            a[3] * q[2] + a[0] * q[1] - a[1] * q[0] + a[2] * q[3],
            a[3] * q[3] - a[0] * q[0] - a[1] * q[1] - a[2] * q[2]]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def camera_frame(q, t, X):
    """Eigen's q * X + t for a quaternion that is not normalised: X + w uv + q_v x uv, uv = 2 q_v x X"""
    uv = [2 * c for c in _cross(q[:3], X)]
    c2 = _cross(q[:3], uv)
    return [X[i] + q[3] * uv[i] + c2[i] + t[i] for i in range(3)]


def project(model, p, q, t, X, branch=None):
    Xc = camera_frame(q, t, X)
    return img_from_cam(model, p, Xc[0] / Xc[2], Xc[1] / Xc[2], branch)


def as_mp(model, params, q, t, X):
    return ([M(v) for v in list(params)[:NUM_PARAMS[model]]], [M(v) for v in q], [M(v) for v in t], [M(v) for v in X])


def pixel(model, params, q, t, X):
    """the projection (x, y) as mpf, and the branch"""
    return project(model, *as_mp(model, params, q, t, X))


def sq_error(model, params, q, t, X, xy):
    """the filter's squared reprojection error: DBL_MAX for a depth below DBL_EPSILON (decided on the double)"""
    p, q, t, X = as_mp(model, params, q, t, X)
    if float(camera_frame(q, t, X)[2]) < EPS:
        return mpf(DBL_MAX)
    x, y, _ = project(model, p, q, t, X)
    return (x - M(xy[0])) ** 2 + (y - M(xy[1])) ** 2


def jacobians(model, params, q, t, X):
    """(2, 6) by the pose tangent (rotation, translation), (2, 12) by the parameter slots, (2, 3) by the point, as
    float64 arrays rounded from 60-digit central differences of the undisturbed point's branch."""
    p, q, t, X = as_mp(model, params, q, t, X)
    Xc = camera_frame(q, t, X)
    _, _, branch = project(model, p, q, t, X)
    big = max(abs(c) for c in Xc)
    rr = mp.sqrt(Xc[0] ** 2 + Xc[1] ** 2) / abs(Xc[2])
    # the steps' scales: a coordinate across the axis moves u or v, at the size of the largest coordinate; the one along the
    # axis moves the depth, at the depth's own size (under a rotation that tilts the axis every coordinate does)
    tilted = any(abs(v) > 1e-12 for v in list(q)[:2])
    s_point = [abs(Xc[2])] * 3 if tilted else [big, big, abs(Xc[2])]
    s_rot = 1 / max(mpf(1), rr)
    if model == 7:  # FOV is a function of u * 2 tan(omega / 2): next to tan's pole its scale in u is that much smaller
        narrow = 1 / max(mpf(1), abs(2 * mp.tan(p[4] / 2)))
        s_point, s_rot = [v * narrow for v in s_point], s_rot * narrow

    def diff(fn, h):
        a, b = fn(h), fn(-h)
        return [(a[0] - b[0]) / (2 * h), (a[1] - b[1]) / (2 * h)]

    Jp, Jc, Jx = np.zeros((2, 6)), np.zeros((2, 12)), np.zeros((2, 3))
    for k in range(6):
        def fn(h, k=k):
            d = [mpf(0)] * 6
            d[k] = h
            return project(model, p, quat_plus(q, d[:3]), [t[i] + d[3 + i] for i in range(3)], X, branch)[:2]
        g = diff(fn, STEP * (s_rot if k < 3 else s_point[k - 3]))
        Jp[:, k] = [float(g[0]), float(g[1])]
    for k in range(len(p)):
        s = max(abs(p[k]), mpf(1))
        if model == 7 and k == 4:
            s = min(s, abs(mp.cos(p[k] / 2)))  # stay on this side of tan's pole
        def fn(h, k=k):
            pp = list(p)
            pp[k] = pp[k] + h
            return project(model, pp, q, t, X, branch)[:2]
        g = diff(fn, STEP * s)
        Jc[:, k] = [float(g[0]), float(g[1])]
    for k in range(3):
        def fn(h, k=k):
            XX = list(X)
            XX[k] = XX[k] + h
            return project(model, p, q, t, XX, branch)[:2]
        g = diff(fn, STEP * s_point[k])
        Jx[:, k] = [float(g[0]), float(g[1])]
    return Jp, Jc, Jx


def pose_jacobian7(model, params, q, t, X):
    """(2, 7) by the ambient pose parameters (qx, qy, qz, qw, tx, ty, tz) of the formula for q not normalised"""
    p, q, t, X = as_mp(model, params, q, t, X)
    Xc = camera_frame(q, t, X)
    _, _, branch = project(model, p, q, t, X)
    rr = mp.sqrt(Xc[0] ** 2 + Xc[1] ** 2) / abs(Xc[2])
    h0 = STEP / max(mpf(1), rr)
    if model == 7:
        h0 = h0 / max(mpf(1), abs(2 * mp.tan(p[4] / 2)))
    J = np.zeros((2, 7))
    for k in range(7):
        h = h0 * (1 if k < 4 else min(abs(c) for c in Xc if c != 0))
        out = []
        for sgn in (1, -1):
            qq, tt = list(q), list(t)
            if k < 4:
                qq[k] = qq[k] + sgn * h
            else:
                tt[k - 4] = tt[k - 4] + sgn * h
            out.append(project(model, p, qq, tt, X, branch)[:2])
        J[:, k] = [float((out[0][i] - out[1][i]) / (2 * h)) for i in range(2)]
    return J


# ---- IterativeUndistortion in float64, with its iteration count ----------------------------------------------------------
def _distortion(model, e, u, v):
    u2, uv, v2 = u * u, u * v, v * v
    r2 = u2 + v2
    if model == 2:
        rad = e[0] * r2
        return u * rad, v * rad
    if model == 3:
        rad = e[0] * r2 + e[1] * r2 * r2
        return u * rad, v * rad
    if model == 4:
        rad = e[0] * r2 + e[1] * r2 * r2
        return (u * rad + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2), v * rad + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2))
    r4 = r2 * r2
    r6 = r4 * r2
    rad = (1.0 + e[0] * r2 + e[1] * r4 + e[4] * r6) / (1.0 + e[5] * r2 + e[6] * r4 + e[7] * r6)
    return (u * rad + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2) - u, v * rad + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2) - v)


def newton_lift(model, params, xy):
    """(u, v, iterations) of one pixel for the polynomial models 2, 3, 4, 6: iterations = 100 means that the step never
    fell below the bound"""
    p = [float(v) for v in params]
    nf = NUM_FOCAL[model]
    e = p[nf + 2:]
    with np.errstate(all="ignore"):
        x0 = np.float64(xy[0] - p[nf]) / np.float64(p[0])
        y0 = np.float64(xy[1] - p[nf + 1]) / np.float64(p[nf - 1])
        u, v = x0, y0
        for it in range(100):
            s0, s1 = max(EPS, abs(1e-6 * u)), max(EPS, abs(1e-6 * v))
            d = _distortion(model, e, u, v)
            b0, f0 = _distortion(model, e, u - s0, v), _distortion(model, e, u + s0, v)
            b1, f1 = _distortion(model, e, u, v - s1), _distortion(model, e, u, v + s1)
            J00, J01 = 1.0 + (f0[0] - b0[0]) / (2.0 * s0), (f1[0] - b1[0]) / (2.0 * s1)
            J10, J11 = (f0[1] - b0[1]) / (2.0 * s0), 1.0 + (f1[1] - b1[1]) / (2.0 * s1)
            idet = np.float64(1.0) / np.float64(J00 * J11 - J10 * J01)
            r0, r1 = u + d[0] - x0, v + d[1] - y0
            st0, st1 = (J11 * idet) * r0 + (-J01 * idet) * r1, (-J10 * idet) * r0 + (J00 * idet) * r1
            u, v = u - st0, v - st1
            if st0 * st0 + st1 * st1 < 1e-10:
                return float(u), float(v), it + 1
    return float(u), float(v), 100
