// ba_core.h — bundle adjustment (include/amc_ba.h): the per-observation arithmetic of DESIGN.md section 15, for the
// device and the host alike.  One observation's residual through the camera model with forward-mode derivatives by the
// camera-frame point and the camera's parameters (15 partials), the chain rule to the pose tangent and the point
// (15.3), the loss corrector (15.4), and the small symmetric solves of the point, pose and camera blocks (15.6).
// FP contraction is off and every transcendental is the project's own (12.9), so the bits equal tests/ba_ref.
#pragma once

#include "abspose_core.h"

namespace amc {
namespace ba {

using ap::ap_atan;
using ap::ap_cos;
using ap::ap_log;
using ap::ap_sin;
using tvg::dabs;
using tvg::dsqrt;

constexpr int kMaxParams = cam::kMaxParams;  // 12
constexpr int kND = 3 + kMaxParams;          // partials: camera-frame point (3), camera parameters (12)
enum : int { LOSS_TRIVIAL = 0, LOSS_SOFT_L1 = 1, LOSS_CAUCHY = 2 };

struct BJet {
    double a;
    double d[kND];
};
AMC_HD BJet bconst(double a) {
    BJet r;
    r.a = a;
    for (int i = 0; i < kND; ++i) r.d[i] = 0.0;
    return r;
}
AMC_HD BJet operator+(const BJet& x, const BJet& y) {
    BJet r;
    r.a = x.a + y.a;
    for (int i = 0; i < kND; ++i) r.d[i] = x.d[i] + y.d[i];
    return r;
}
AMC_HD BJet operator-(const BJet& x, const BJet& y) {
    BJet r;
    r.a = x.a - y.a;
    for (int i = 0; i < kND; ++i) r.d[i] = x.d[i] - y.d[i];
    return r;
}
AMC_HD BJet operator*(const BJet& x, const BJet& y) {
    BJet r;
    r.a = x.a * y.a;
    for (int i = 0; i < kND; ++i) r.d[i] = x.a * y.d[i] + x.d[i] * y.a;
    return r;
}
AMC_HD BJet operator/(const BJet& x, const BJet& y) {  // (x' - (x / y) y') / y
    BJet r;
    r.a = x.a / y.a;
    for (int i = 0; i < kND; ++i) r.d[i] = (x.d[i] - r.a * y.d[i]) / y.a;
    return r;
}
AMC_HD BJet operator+(const BJet& x, double c) { BJet r = x; r.a = x.a + c; return r; }
AMC_HD BJet operator+(double c, const BJet& x) { BJet r = x; r.a = c + x.a; return r; }
AMC_HD BJet operator-(const BJet& x, double c) { BJet r = x; r.a = x.a - c; return r; }
AMC_HD BJet operator*(const BJet& x, double c) {
    BJet r;
    r.a = x.a * c;
    for (int i = 0; i < kND; ++i) r.d[i] = x.d[i] * c;
    return r;
}
AMC_HD BJet operator*(double c, const BJet& x) {
    BJet r;
    r.a = c * x.a;
    for (int i = 0; i < kND; ++i) r.d[i] = c * x.d[i];
    return r;
}
AMC_HD BJet operator/(const BJet& x, double c) {
    BJet r;
    r.a = x.a / c;
    for (int i = 0; i < kND; ++i) r.d[i] = x.d[i] / c;
    return r;
}
AMC_HD double bval(double x) { return x; }
AMC_HD double bval(const BJet& x) { return x.a; }
AMC_HD double bsqrt(double x) { return dsqrt(x); }
AMC_HD BJet bsqrt(const BJet& x) {
    BJet r;
    r.a = dsqrt(x.a);
    const double h = 2.0 * r.a;
    for (int i = 0; i < kND; ++i) r.d[i] = x.d[i] / h;
    return r;
}
AMC_HD double batan(double x) { return ap_atan(x); }
AMC_HD BJet batan(const BJet& x) {
    BJet r;
    r.a = ap_atan(x.a);
    const double h = 1.0 + x.a * x.a;
    for (int i = 0; i < kND; ++i) r.d[i] = x.d[i] / h;
    return r;
}
AMC_HD double btan(double x) { return ap_sin(x) / ap_cos(x); }
AMC_HD BJet btan(const BJet& x) {  // sin / cos; derivative 1 + tan^2
    BJet r;
    r.a = ap_sin(x.a) / ap_cos(x.a);
    const double h = 1.0 + r.a * r.a;
    for (int i = 0; i < kND; ++i) r.d[i] = x.d[i] * h;
    return r;
}

// Camera::ImgFromCam of the camera-frame point (pu, pv, pw) with the parameters p as the scalar type T (15.3): the
// operation order of abspose_core.h's img_from_cam_t (12.7), the parameters taking part in the derivatives
template <class T>
AMC_HD void img_from_cam_p(int model, const T* p, const T& pu, const T& pv, const T& pw, T& x, T& y) {
    using namespace cam;
    T u = pu / pw, v = pv / pw;
    const int nf = num_focal(model);
    const T f1 = p[0], f2 = p[nf - 1], c1 = p[nf], c2 = p[nf + 1];
    const T* e = p + nf + 2;
    if (model == FOV) {
        const T omega = e[0];
        const double kEpsilon = 1e-4;
        const T radius2 = u * u + v * v;
        const T omega2 = omega * omega;
        T factor;
        if (bval(omega2) < kEpsilon) {
            factor = (omega2 * radius2) / 3.0 - omega2 / 12.0 + 1.0;
        } else {
            const T tan_half_omega = btan(omega / 2.0);
            if (bval(radius2) < kEpsilon) {
                factor = (-2.0 * tan_half_omega * (4.0 * radius2 * tan_half_omega * tan_half_omega - 3.0)) / (3.0 * omega);
            } else {
                const T radius = bsqrt(radius2);
                const T numerator = batan(radius * 2.0 * tan_half_omega);
                factor = numerator / (radius * omega);
            }
        }
        x = f1 * (u * factor) + c1;
        y = f2 * (v * factor) + c2;
        return;
    }
    if (model == THIN_PRISM_FISHEYE) {
        const T r = bsqrt(u * u + v * v);
        if (bval(r) > DBL_EPSILON) {
            const T theta = batan(r);
            u = theta * u / r;
            v = theta * v / r;
        }
    }
    T du, dv;
    switch (model) {
        case SIMPLE_PINHOLE:
        case PINHOLE:
            x = f1 * u + c1;
            y = f2 * v + c2;
            return;
        case SIMPLE_RADIAL: {
            const T r2 = u * u + v * v;
            const T radial = e[0] * r2;
            du = u * radial;
            dv = v * radial;
            break;
        }
        case RADIAL: {
            const T r2 = u * u + v * v;
            const T radial = e[0] * r2 + e[1] * r2 * r2;
            du = u * radial;
            dv = v * radial;
            break;
        }
        case OPENCV: {
            const T u2 = u * u, uv = u * v, v2 = v * v;
            const T r2 = u2 + v2;
            const T radial = e[0] * r2 + e[1] * r2 * r2;
            du = u * radial + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2);
            dv = v * radial + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2);
            break;
        }
        case FULL_OPENCV: {
            const T u2 = u * u, uv = u * v, v2 = v * v;
            const T r2 = u2 + v2;
            const T r4 = r2 * r2;
            const T r6 = r4 * r2;
            const T radial = (1.0 + e[0] * r2 + e[1] * r4 + e[4] * r6) / (1.0 + e[5] * r2 + e[6] * r4 + e[7] * r6);
            du = u * radial + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2) - u;
            dv = v * radial + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2) - v;
            break;
        }
        case THIN_PRISM_FISHEYE: {
            const T u2 = u * u, uv = u * v, v2 = v * v;
            const T r2 = u2 + v2;
            const T r4 = r2 * r2;
            const T r6 = r4 * r2;
            const T r8 = r6 * r2;
            const T radial = e[0] * r2 + e[1] * r4 + e[4] * r6 + e[5] * r8;
            du = u * radial + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2) + e[6] * r2;
            dv = v * radial + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2) + e[7] * r2;
            break;
        }
        default: {  // OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE
            const int nk = model == SIMPLE_RADIAL_FISHEYE ? 1 : model == RADIAL_FISHEYE ? 2 : 4;
            const T r = bsqrt(u * u + v * v);
            if (bval(r) > DBL_EPSILON) {
                const T theta = batan(r);
                const T theta2 = theta * theta;
                T thetad;
                if (nk == 1) {
                    thetad = theta * (1.0 + e[0] * theta2);
                } else if (nk == 2) {
                    const T theta4 = theta2 * theta2;
                    thetad = theta * (1.0 + e[0] * theta2 + e[1] * theta4);
                } else {
                    const T theta4 = theta2 * theta2;
                    const T theta6 = theta4 * theta2;
                    const T theta8 = theta4 * theta4;
                    thetad = theta * (1.0 + e[0] * theta2 + e[1] * theta4 + e[2] * theta6 + e[3] * theta8);
                }
                du = u * thetad / r - u;
                dv = v * thetad / r - v;
            } else {
                du = u * 0.0;
                dv = v * 0.0;
            }
            break;
        }
    }
    x = f1 * (u + du) + c1;
    y = f2 * (v + dv) + c2;
}

AMC_HD void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
// Eigen's q * v for q = (x, y, z, w), not normalised: v + w uv + q_v x uv, uv = 2 q_v x v
AMC_HD void quat_rotate(const double* q, const double* v, double* o) {
    double uv[3], c[3];
    cross3(q, v, uv);
    for (int i = 0; i < 3; ++i) uv[i] = uv[i] + uv[i];
    cross3(q, uv, c);
    for (int i = 0; i < 3; ++i) o[i] = (v[i] + q[3] * uv[i]) + c[i];
}

// rho(s) and rho'(s) of the loss at s = |r|^2 (15.4); b = scale^2
AMC_HD void loss_eval(int loss, double scale, double s, double& rho, double& rho1) {
    if (loss == LOSS_TRIVIAL) {
        rho = s;
        rho1 = 1.0;
        return;
    }
    const double b = scale * scale, c = 1.0 / b;
    const double sum = 1.0 + s * c;
    if (loss == LOSS_SOFT_L1) {
        const double tmp = dsqrt(sum);
        rho = 2.0 * b * (tmp - 1.0);
        rho1 = 1.0 / tmp;
    } else {
        rho = b * ap_log(sum);
        rho1 = 1.0 / sum;
    }
}

// One observation (15.3, 15.4).  cost = rho / 2.  With jac: the loss-corrected residual r (2) and the loss-corrected
// Jacobian blocks by the pose tangent Jp (2 x 6, rotation first), the camera parameters Jc (2 x 12) and the point Jx
// (2 x 3), unscaled and unmasked.
AMC_HD double observation(int model, const double* prm, const double* q, const double* t, const double* X,
                          const double* xy, int loss, double loss_scale, bool jac, double* r, double* Jp, double* Jc,
                          double* Jx) {
    double Xc[3];
    quat_rotate(q, X, Xc);
    for (int i = 0; i < 3; ++i) Xc[i] = Xc[i] + t[i];
    if (!jac) {
        double p[kMaxParams], x, y;
        for (int i = 0; i < kMaxParams; ++i) p[i] = prm[i];
        img_from_cam_p<double>(model, p, Xc[0], Xc[1], Xc[2], x, y);
        const double rx = x - xy[0], ry = y - xy[1];
        double rho, rho1;
        loss_eval(loss, loss_scale, rx * rx + ry * ry, rho, rho1);
        return 0.5 * rho;
    }
    BJet p[kMaxParams], pc[3], x, y;
    for (int i = 0; i < kMaxParams; ++i) {
        p[i] = bconst(prm[i]);
        p[i].d[3 + i] = 1.0;
    }
    for (int i = 0; i < 3; ++i) {
        pc[i] = bconst(Xc[i]);
        pc[i].d[i] = 1.0;
    }
    img_from_cam_p<BJet>(model, p, pc[0], pc[1], pc[2], x, y);
    const double rx = x.a - xy[0], ry = y.a - xy[1];
    double rho, rho1;
    loss_eval(loss, loss_scale, rx * rx + ry * ry, rho, rho1);
    const double w = dsqrt(rho1);
    r[0] = w * rx;
    r[1] = w * ry;
    // d Xc / d q (3 x 4: A | uv) times PlusJacobian (4 x 3) = G, and d Xc / d X = M (columns: the rotation of e_k)
    double uv[3];
    cross3(q, X, uv);
    for (int i = 0; i < 3; ++i) uv[i] = uv[i] + uv[i];
    double A[3][4], M[3][3];
    for (int k = 0; k < 3; ++k) {
        double ek[3] = {0.0, 0.0, 0.0}, xe[3], ue[3], qxe[3], col[3];
        ek[k] = 1.0;
        cross3(X, ek, xe);
        cross3(uv, ek, ue);
        cross3(q, xe, qxe);
        for (int i = 0; i < 3; ++i) A[i][k] = (-2.0 * q[3]) * xe[i] - ue[i] - 2.0 * qxe[i];
        quat_rotate(q, ek, col);
        for (int i = 0; i < 3; ++i) M[i][k] = col[i];
    }
    for (int i = 0; i < 3; ++i) A[i][3] = uv[i];
    double Jm[12], G[3][3];
    ap::quat_plus_jacobian(q, Jm);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            G[i][j] = A[i][0] * Jm[j] + A[i][1] * Jm[3 + j] + A[i][2] * Jm[6 + j] + A[i][3] * Jm[9 + j];
    const BJet* rr[2] = {&x, &y};
    for (int a = 0; a < 2; ++a) {
        const double* d = rr[a]->d;
        for (int j = 0; j < 3; ++j) Jp[6 * a + j] = w * (d[0] * G[0][j] + d[1] * G[1][j] + d[2] * G[2][j]);
        for (int j = 0; j < 3; ++j) Jp[6 * a + 3 + j] = w * d[j];
        for (int j = 0; j < kMaxParams; ++j) Jc[kMaxParams * a + j] = w * d[3 + j];
        for (int j = 0; j < 3; ++j) Jx[3 * a + j] = w * (d[0] * M[0][j] + d[1] * M[1][j] + d[2] * M[2][j]);
    }
    return 0.5 * rho;
}

// the LM diagonal entry of a Jacobi-scaled column with squared norm h (12.7)
AMC_HD double lm_diag(double h, double radius) {
    const double c = h < 1e-6 ? 1e-6 : h > 1e32 ? 1e32 : h;
    return c / radius;
}

// inverse of the symmetric 3 x 3 (upper: 00 01 02 11 12 22) by the adjugate; the same packing out
AMC_HD void sym3_inverse(const double* s, double* o) {
    const double a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5];
    const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
    const double det = a * c00 + b * c01 + c * c02;
    o[0] = c00 / det;
    o[1] = c01 / det;
    o[2] = c02 / det;
    o[3] = (a * f - c * c) / det;
    o[4] = (b * c - a * e) / det;
    o[5] = (a * d - b * b) / det;
}
AMC_HD void sym3_mul(const double* s, const double* v, double* o) {
    o[0] = s[0] * v[0] + s[1] * v[1] + s[2] * v[2];
    o[1] = s[1] * v[0] + s[3] * v[1] + s[4] * v[2];
    o[2] = s[2] * v[0] + s[4] * v[1] + s[5] * v[2];
}

// In-place inverse of the symmetric positive definite n x n (row-major, stride n, n <= 12) by Cholesky: A = L L^T, then
// the columns of the inverse by two triangular solves each.  A pivot that is not positive makes the block the identity
// (the preconditioner then leaves that block's residual as it is); returns whether that happened.
AMC_HD bool spd_inverse(double* A, int n) {
    double L[kMaxParams * kMaxParams];
    bool ok = true;
    for (int j = 0; j < n && ok; ++j) {
        double s = A[j * n + j];
        for (int k = 0; k < j; ++k) s = s - L[j * n + k] * L[j * n + k];
        if (!(s > 0.0)) {
            ok = false;
            break;
        }
        const double ljj = dsqrt(s);
        L[j * n + j] = ljj;
        for (int i = j + 1; i < n; ++i) {
            double v = A[i * n + j];
            for (int k = 0; k < j; ++k) v = v - L[i * n + k] * L[j * n + k];
            L[i * n + j] = v / ljj;
        }
    }
    if (!ok) {
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) A[i * n + j] = i == j ? 1.0 : 0.0;
        return false;
    }
    for (int c = 0; c < n; ++c) {
        double y[kMaxParams];
        for (int i = 0; i < n; ++i) {
            double v = i == c ? 1.0 : 0.0;
            for (int k = 0; k < i; ++k) v = v - L[i * n + k] * y[k];
            y[i] = v / L[i * n + i];
        }
        for (int i = n - 1; i >= 0; --i) {
            double v = y[i];
            for (int k = i + 1; k < n; ++k) v = v - L[k * n + i] * A[k * n + c];
            A[i * n + c] = v / L[i * n + i];
        }
    }
    return true;
}

}  // namespace ba
}  // namespace amc
