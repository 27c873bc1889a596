// absrefine_core.h — RefineAbsolutePose with a variable camera (include/amc_absrefine.h): COLMAP 3.9.1's joint
// refinement of the pose, the focal lengths and the distortion, restated in DESIGN.md section 25.  One 64-lane wave runs
// one query, as in abspose_core.h, whose reduction order (12.10), transcendentals (12.9), quaternion manifold and dense
// solve it reuses.
//
// The solver has K = 6 + NV columns: the six pose tangent columns of 12.7, then the camera's variable parameters in
// ascending index.  NV is a template parameter, so every loop over columns is compile-time and no jet or solver array
// is indexed by a run-time column (the twelve parameters themselves are looked up by the model's layout, as in
// img_from_cam_t).  A camera parameter is a Par: a value, the derivative with respect to itself and the jet column it owns
// (-1 for a constant).  An operation between a Par and a jet evaluates the product / quotient rule in the Par's own
// column only and the constant-operand rule of abspose_core.h in every other column, so with NV = 0 every operation is
// abspose_core.h's, in its order: the results then equal 12.7 / 12.8 bit for bit.
#pragma once

#include "abspose_core.h"

namespace amc {
namespace apr {

using ap::finite;
using ap::kDblEps;
using ap::kDblMax;
using ap::kLanes;
using tvg::dabs;
using tvg::dsqrt;

constexpr int kPose = 7;  // jet columns of the pose: qx qy qz qw tx ty tz

// the camera's variable parameter indices, ascending (25.1): focal lengths iff refine_focal, extra parameters iff
// refine_extra, the principal point never; returns NV and fills idx
AMC_HD int variable_params(int model, bool refine_focal, bool refine_extra, int* idx) {
    const int nf = cam::num_focal(model), np = cam::num_params(model);
    int nv = 0;
    if (refine_focal)
        for (int i = 0; i < nf; ++i) idx[nv++] = i;
    if (refine_extra)
        for (int i = nf + 2; i < np; ++i) idx[nv++] = i;
    return nv;
}

template <int W>
struct JetW {
    double a;
    double d[W];
};
struct Par {
    double a;
    double da;
    int col;
};

#define APR_T template <int W> AMC_HD
APR_T JetW<W> jconstw(double a) {
    JetW<W> r;
    r.a = a;
    for (int i = 0; i < W; ++i) r.d[i] = 0.0;
    return r;
}
APR_T JetW<W> operator+(const JetW<W>& x, const JetW<W>& y) {
    JetW<W> r;
    r.a = x.a + y.a;
    for (int i = 0; i < W; ++i) r.d[i] = x.d[i] + y.d[i];
    return r;
}
APR_T JetW<W> operator-(const JetW<W>& x, const JetW<W>& y) {
    JetW<W> r;
    r.a = x.a - y.a;
    for (int i = 0; i < W; ++i) r.d[i] = x.d[i] - y.d[i];
    return r;
}
APR_T JetW<W> operator*(const JetW<W>& x, const JetW<W>& y) {
    JetW<W> r;
    r.a = x.a * y.a;
    for (int i = 0; i < W; ++i) r.d[i] = x.a * y.d[i] + x.d[i] * y.a;
    return r;
}
APR_T JetW<W> operator/(const JetW<W>& x, const JetW<W>& y) {
    JetW<W> r;
    r.a = x.a / y.a;
    for (int i = 0; i < W; ++i) r.d[i] = (x.d[i] - r.a * y.d[i]) / y.a;
    return r;
}
APR_T JetW<W> operator+(const JetW<W>& x, double c) { JetW<W> r = x; r.a = x.a + c; return r; }
APR_T JetW<W> operator+(double c, const JetW<W>& x) { JetW<W> r = x; r.a = c + x.a; return r; }
APR_T JetW<W> operator-(const JetW<W>& x, double c) { JetW<W> r = x; r.a = x.a - c; return r; }
APR_T JetW<W> operator*(const JetW<W>& x, double c) {
    JetW<W> r;
    r.a = x.a * c;
    for (int i = 0; i < W; ++i) r.d[i] = x.d[i] * c;
    return r;
}
APR_T JetW<W> operator*(double c, const JetW<W>& x) {
    JetW<W> r;
    r.a = c * x.a;
    for (int i = 0; i < W; ++i) r.d[i] = c * x.d[i];
    return r;
}
APR_T JetW<W> operator/(const JetW<W>& x, double c) {
    JetW<W> r;
    r.a = x.a / c;
    for (int i = 0; i < W; ++i) r.d[i] = x.d[i] / c;
    return r;
}
APR_T JetW<W> tsqrt(const JetW<W>& x) {
    JetW<W> r;
    r.a = dsqrt(x.a);
    const double h = 2.0 * r.a;
    for (int i = 0; i < W; ++i) r.d[i] = x.d[i] / h;
    return r;
}
APR_T JetW<W> tatan(const JetW<W>& x) {
    JetW<W> r;
    r.a = ap::ap_atan(x.a);
    const double h = 1.0 + x.a * x.a;
    for (int i = 0; i < W; ++i) r.d[i] = x.d[i] / h;
    return r;
}

// Par with a scalar and with a Par of the same column (FOV's omega is the only parameter that meets itself)
AMC_HD Par operator*(double c, const Par& p) { return Par{c * p.a, c * p.da, p.col}; }
AMC_HD Par operator/(const Par& p, double c) { return Par{p.a / c, p.da / c, p.col}; }
AMC_HD Par operator*(const Par& x, const Par& y) { return Par{x.a * y.a, x.a * y.da + x.da * y.a, x.col}; }
AMC_HD Par operator/(const Par& x, const Par& y) {
    const double a = x.a / y.a;
    return Par{a, (x.da - a * y.da) / y.a, x.col};
}
AMC_HD Par psin(const Par& p) { return Par{ap::ap_sin(p.a), ap::ap_cos(p.a) * p.da, p.col}; }
AMC_HD Par pcos(const Par& p) { return Par{ap::ap_cos(p.a), -(ap::ap_sin(p.a) * p.da), p.col}; }

// Par with a jet: the full rule in the Par's column, the constant-operand rule elsewhere
APR_T JetW<W> operator*(const Par& p, const JetW<W>& x) {
    JetW<W> r;
    r.a = p.a * x.a;
    for (int i = 0; i < W; ++i) r.d[i] = i == p.col ? p.a * x.d[i] + p.da * x.a : p.a * x.d[i];
    return r;
}
APR_T JetW<W> operator*(const JetW<W>& x, const Par& p) {
    JetW<W> r;
    r.a = x.a * p.a;
    for (int i = 0; i < W; ++i) r.d[i] = i == p.col ? x.a * p.da + x.d[i] * p.a : x.d[i] * p.a;
    return r;
}
APR_T JetW<W> operator/(const JetW<W>& x, const Par& p) {
    JetW<W> r;
    r.a = x.a / p.a;
    for (int i = 0; i < W; ++i) r.d[i] = i == p.col ? (x.d[i] - r.a * p.da) / p.a : x.d[i] / p.a;
    return r;
}
APR_T JetW<W> operator+(const JetW<W>& x, const Par& p) {
    JetW<W> r;
    r.a = x.a + p.a;
    for (int i = 0; i < W; ++i) r.d[i] = i == p.col ? x.d[i] + p.da : x.d[i];
    return r;
}
APR_T JetW<W> operator-(const JetW<W>& x, const Par& p) {
    JetW<W> r;
    r.a = x.a - p.a;
    for (int i = 0; i < W; ++i) r.d[i] = i == p.col ? x.d[i] - p.da : x.d[i];
    return r;
}

// img_from_cam_t of abspose_core.h with the camera's parameters as Pars: the same expression trees, operand by operand
template <int W>
AMC_HD void img_from_cam_p(int model, const double* pv_, const int* pcol, const JetW<W>& pu, const JetW<W>& pv,
                           const JetW<W>& pw, JetW<W>& x, JetW<W>& y) {
    using namespace cam;
    using T = JetW<W>;
    T u = pu / pw, v = pv / pw;
    const int nf = num_focal(model);
    auto par = [&](int i) { return Par{pv_[i], pcol[i] >= 0 ? 1.0 : 0.0, pcol[i]}; };
    const Par f1 = par(0), f2 = par(nf - 1), c1 = par(nf), c2 = par(nf + 1);
    auto e = [&](int i) { return par(nf + 2 + i); };
    if (model == FOV) {
        const Par omega = e(0);
        const double kEpsilon = 1e-4;
        const T radius2 = u * u + v * v;
        const Par omega2 = omega * omega;
        T factor;
        if (omega2.a < kEpsilon) {
            factor = (omega2 * radius2) / 3.0 - omega2 / 12.0 + 1.0;
        } else {
            const Par tan_half_omega = psin(omega / 2.0) / pcos(omega / 2.0);
            if (radius2.a < kEpsilon) {
                factor = (-2.0 * tan_half_omega * (4.0 * radius2 * tan_half_omega * tan_half_omega - 3.0)) / (3.0 * omega);
            } else {
                const T radius = tsqrt(radius2);
                const T numerator = tatan(radius * 2.0 * tan_half_omega);
                factor = numerator / (radius * omega);
            }
        }
        x = f1 * (u * factor) + c1;
        y = f2 * (v * factor) + c2;
        return;
    }
    if (model == THIN_PRISM_FISHEYE) {
        const T r = tsqrt(u * u + v * v);
        if (r.a > kDblEps) {
            const T theta = tatan(r);
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
            const T radial = e(0) * r2;
            du = u * radial;
            dv = v * radial;
            break;
        }
        case RADIAL: {
            const T r2 = u * u + v * v;
            const T radial = e(0) * r2 + e(1) * r2 * r2;
            du = u * radial;
            dv = v * radial;
            break;
        }
        case OPENCV: {
            const T u2 = u * u, uv = u * v, v2 = v * v;
            const T r2 = u2 + v2;
            const T radial = e(0) * r2 + e(1) * r2 * r2;
            du = u * radial + 2.0 * e(2) * uv + e(3) * (r2 + 2.0 * u2);
            dv = v * radial + 2.0 * e(3) * uv + e(2) * (r2 + 2.0 * v2);
            break;
        }
        case FULL_OPENCV: {
            const T u2 = u * u, uv = u * v, v2 = v * v;
            const T r2 = u2 + v2;
            const T r4 = r2 * r2;
            const T r6 = r4 * r2;
            const T radial = (1.0 + e(0) * r2 + e(1) * r4 + e(4) * r6) / (1.0 + e(5) * r2 + e(6) * r4 + e(7) * r6);
            du = u * radial + 2.0 * e(2) * uv + e(3) * (r2 + 2.0 * u2) - u;
            dv = v * radial + 2.0 * e(3) * uv + e(2) * (r2 + 2.0 * v2) - v;
            break;
        }
        case THIN_PRISM_FISHEYE: {
            const T u2 = u * u, uv = u * v, v2 = v * v;
            const T r2 = u2 + v2;
            const T r4 = r2 * r2;
            const T r6 = r4 * r2;
            const T r8 = r6 * r2;
            const T radial = e(0) * r2 + e(1) * r4 + e(4) * r6 + e(5) * r8;
            du = u * radial + 2.0 * e(2) * uv + e(3) * (r2 + 2.0 * u2) + e(6) * r2;
            dv = v * radial + 2.0 * e(3) * uv + e(2) * (r2 + 2.0 * v2) + e(7) * r2;
            break;
        }
        default: {  // OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE
            const int nk = model == SIMPLE_RADIAL_FISHEYE ? 1 : model == RADIAL_FISHEYE ? 2 : 4;
            const T r = tsqrt(u * u + v * v);
            if (r.a > kDblEps) {
                const T theta = tatan(r);
                const T theta2 = theta * theta;
                T thetad;
                if (nk == 1) {
                    thetad = theta * (1.0 + e(0) * theta2);
                } else if (nk == 2) {
                    const T theta4 = theta2 * theta2;
                    thetad = theta * (1.0 + e(0) * theta2 + e(1) * theta4);
                } else {
                    const T theta4 = theta2 * theta2;
                    const T theta6 = theta4 * theta2;
                    const T theta8 = theta4 * theta4;
                    thetad = theta * (1.0 + e(0) * theta2 + e(1) * theta4 + e(2) * theta6 + e(3) * theta8);
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

// pixel_residual of abspose_core.h over W columns: the residual of one correspondence with d/d(q, t, camera columns)
template <int W>
AMC_HD void pixel_residual_w(int model, const double* prm, const int* pcol, const double* q, const double* t,
                             const double* X, double ox, double oy, JetW<W>& rx, JetW<W>& ry) {
    using T = JetW<W>;
    T qv[4], tv[3];
    for (int i = 0; i < 4; ++i) {
        qv[i] = jconstw<W>(q[i]);
        qv[i].d[i] = 1.0;
    }
    for (int i = 0; i < 3; ++i) {
        tv[i] = jconstw<W>(t[i]);
        tv[i].d[4 + i] = 1.0;
    }
    T uv0 = qv[1] * X[2] - qv[2] * X[1];
    T uv1 = qv[2] * X[0] - qv[0] * X[2];
    T uv2 = qv[0] * X[1] - qv[1] * X[0];
    uv0 = uv0 + uv0;
    uv1 = uv1 + uv1;
    uv2 = uv2 + uv2;
    const T c0 = qv[1] * uv2 - qv[2] * uv1;
    const T c1 = qv[2] * uv0 - qv[0] * uv2;
    const T c2 = qv[0] * uv1 - qv[1] * uv0;
    const T p0 = (X[0] + qv[3] * uv0) + c0 + tv[0];
    const T p1 = (X[1] + qv[3] * uv1) + c1 + tv[1];
    const T p2 = (X[2] + qv[3] * uv2) + c2 + tv[2];
    img_from_cam_p<W>(model, prm, pcol, p0, p1, p2, rx, ry);
    rx = rx - ox;
    ry = ry - oy;
}

// the query a wave refines
struct Query {
    int model;
    int idx[10];        // the variable parameter indices (NV of them)
    const double* xy;   // n x 2 pixels
    const double* X;    // n x 3
    const uint8_t* mask;
    uint32_t n;
};

template <int K>
struct EvalK {
    double cost;
    double H[K * (K + 1) / 2];  // upper triangle, row by row
    double g[K];
};
template <int K>
AMC_HD double symk(const double* H, int i, int j) {
    if (i > j) {
        const int t = i;
        i = j;
        j = t;
    }
    return H[i * K - i * (i - 1) / 2 + (j - i)];
}

// evaluate_t of abspose_core.h over K = 6 + NV columns
template <int NV>
AMC_HD void evaluate_k(const Query& Q, const int* pcol, double loss_scale, const double* q, const double* t,
                       const double* prm, bool jac, EvalK<6 + NV>& ev) {
    constexpr int K = 6 + NV, W = kPose + NV, NH = K * (K + 1) / 2, NS = 1 + NH + K;
    const double b = loss_scale * loss_scale, c = 1.0 / b;
    double Jm[12];
    ap::quat_plus_jacobian(q, Jm);
    double s[NS];
    ap::wave_sum<NS>(
        [&](int l, double (&o)[NS]) {
            for (int i = 0; i < NS; ++i) o[i] = 0.0;
            for (uint32_t k = (uint32_t)l; k < Q.n; k += kLanes) {
                if (!Q.mask[k]) continue;
                JetW<W> rx, ry;
                pixel_residual_w<W>(Q.model, prm, pcol, q, t, Q.X + 3 * k, Q.xy[2 * k], Q.xy[2 * k + 1], rx, ry);
                const double sq = rx.a * rx.a + ry.a * ry.a;
                const double sum = 1.0 + sq * c;
                const double inv = 1.0 / sum;
                o[0] = o[0] + 0.5 * (b * ap::ap_log(sum));
                if (!jac) continue;
                const double w = dsqrt(inv);
                double J[2][K];
                const JetW<W>* rr[2] = {&rx, &ry};
                for (int r = 0; r < 2; ++r) {
                    for (int j = 0; j < 3; ++j)
                        J[r][j] = w * (rr[r]->d[0] * Jm[j] + rr[r]->d[1] * Jm[3 + j] + rr[r]->d[2] * Jm[6 + j] +
                                       rr[r]->d[3] * Jm[9 + j]);
                    for (int j = 0; j < 3; ++j) J[r][3 + j] = w * rr[r]->d[4 + j];
                    for (int j = 0; j < NV; ++j) J[r][6 + j] = w * rr[r]->d[kPose + j];
                }
                const double f[2] = {w * rx.a, w * ry.a};
                int tt = 1;
                for (int i = 0; i < K; ++i)
                    for (int j = i; j < K; ++j, ++tt) o[tt] = o[tt] + (J[0][i] * J[0][j] + J[1][i] * J[1][j]);
                for (int i = 0; i < K; ++i) o[1 + NH + i] = o[1 + NH + i] + (J[0][i] * f[0] + J[1][i] * f[1]);
            }
        },
        s);
    ev.cost = s[0];
    for (int i = 0; i < NH; ++i) ev.H[i] = s[1 + i];
    for (int i = 0; i < K; ++i) ev.g[i] = s[1 + NH + i];
}

struct LmOpts {
    double gradient_tolerance;
    int64_t max_num_iterations;
    double loss_scale;
    bool covariance;
};
struct Out {
    bool success;
    double q[4];
    double t[3];
    double prm[cam::kMaxParams];
    double cov[36];
    int iterations;
};

// refine_t of abspose_core.h over K columns (25.2): the same statements in the same order, the camera columns added
// after the pose's wherever the pose's six are walked
template <int NV>
AMC_HD void refine_k(const Query& Q, const LmOpts& rp, const double* q0, const double* t0, const double* prm0, Out& out) {
    constexpr int K = 6 + NV;
    const int np = cam::num_params(Q.model);
    int pcol[cam::kMaxParams];
    for (int i = 0; i < cam::kMaxParams; ++i) {
        pcol[i] = -1;
        for (int j = 0; j < NV; ++j)
            if (Q.idx[j] == i) pcol[i] = kPose + j;
    }
    out.success = false;
    out.iterations = 0;
    double q[4] = {q0[0], q0[1], q0[2], q0[3]}, t[3] = {t0[0], t0[1], t0[2]};
    double prm[cam::kMaxParams];
    for (int i = 0; i < cam::kMaxParams; ++i) prm[i] = prm0[i];
    for (int i = 0; i < 36; ++i) out.cov[i] = 0.0;
    double cnt[1];
    ap::wave_sum<1>(
        [&](int l, double (&o)[1]) {
            o[0] = 0.0;
            for (uint32_t k = (uint32_t)l; k < Q.n; k += kLanes) o[0] = o[0] + (Q.mask[k] ? 1.0 : 0.0);
        },
        cnt);
    bool usable = true;
    if (cnt[0] > 0.0) {
        EvalK<K> ev;
        evaluate_k<NV>(Q, pcol, rp.loss_scale, q, t, prm, true, ev);
        if (!finite(ev.cost)) usable = false;
        double scale[K];
        for (int i = 0; i < K; ++i) scale[i] = 1.0 / (1.0 + dsqrt(symk<K>(ev.H, i, i)));
        double radius = 1e4, decrease = 2.0;
        int invalid_run = 0;
        auto gmax = [&](const EvalK<K>& e) {
            double m = ap::gradient_max_norm(q, t, e.g);
            for (int j = 0; j < NV; ++j) m = tvg::dmax(m, dabs(e.g[6 + j]));
            return m;
        };
        bool done = !usable || gmax(ev) <= rp.gradient_tolerance;
        for (int64_t it = 1; !done && it <= rp.max_num_iterations; ++it) {
            out.iterations = (int)it;
            double A[K * K], y[K], Hs[K * K];
            for (int i = 0; i < K; ++i) {
                for (int j = 0; j < K; ++j) Hs[K * i + j] = scale[i] * symk<K>(ev.H, i, j) * scale[j];
                y[i] = -(scale[i] * ev.g[i]);
            }
            for (int i = 0; i < K * K; ++i) A[i] = Hs[i];
            for (int i = 0; i < K; ++i) {
                double dgl = Hs[(K + 1) * i];
                dgl = dgl < 1e-6 ? 1e-6 : dgl > 1e32 ? 1e32 : dgl;
                A[(K + 1) * i] = A[(K + 1) * i] + dgl / radius;
            }
            bool valid = ap::solve_gauss<K>(A, y);
            double mcc = 0.0;
            if (valid) {
                double gy = 0.0, yhy = 0.0;
                for (int i = 0; i < K; ++i) {
                    gy = gy + (scale[i] * ev.g[i]) * y[i];
                    double hy = 0.0;
                    for (int j = 0; j < K; ++j) hy = hy + Hs[K * i + j] * y[j];
                    yhy = yhy + y[i] * hy;
                }
                mcc = -(gy + 0.5 * yhy);
                valid = mcc > 0.0;
            }
            if (!valid) {
                radius = radius / decrease;
                decrease = 2.0 * decrease;
                if (++invalid_run >= 5) {
                    usable = false;
                    break;
                }
                if (radius < 1e-32) break;
                continue;
            }
            invalid_run = 0;
            double delta[K], qn[4], tn[3], pn[cam::kMaxParams];
            for (int i = 0; i < K; ++i) delta[i] = scale[i] * y[i];
            ap::quat_plus(q, delta, qn);
            for (int i = 0; i < 3; ++i) tn[i] = t[i] + delta[3 + i];
            for (int i = 0; i < cam::kMaxParams; ++i) {
                pn[i] = prm[i];
                for (int j = 0; j < NV; ++j)
                    if (Q.idx[j] == i) pn[i] = prm[i] + delta[6 + j];
            }
            // parameter tolerance over the pose and, when the camera varies, its whole block (25.2)
            double sn = 0.0, xn = 0.0;
            for (int i = 0; i < 4; ++i) {
                sn = sn + (q[i] - qn[i]) * (q[i] - qn[i]);
                xn = xn + q[i] * q[i];
            }
            for (int i = 0; i < 3; ++i) {
                sn = sn + (t[i] - tn[i]) * (t[i] - tn[i]);
                xn = xn + t[i] * t[i];
            }
            if (NV > 0)
                for (int i = 0; i < cam::kMaxParams; ++i)
                    if (i < np) {
                        sn = sn + (prm[i] - pn[i]) * (prm[i] - pn[i]);
                        xn = xn + prm[i] * prm[i];
                    }
            if (dsqrt(sn) <= 1e-8 * (dsqrt(xn) + 1e-8)) break;
            EvalK<K> cand;
            evaluate_k<NV>(Q, pcol, rp.loss_scale, qn, tn, pn, false, cand);
            const double new_cost = finite(cand.cost) ? cand.cost : kDblMax;
            const double cost_change = ev.cost - new_cost;
            if (dabs(cost_change) <= 1e-6 * ev.cost) break;  // function tolerance
            const double rel = cost_change / mcc;
            if (rel > 1e-3) {
                for (int i = 0; i < 4; ++i) q[i] = qn[i];
                for (int i = 0; i < 3; ++i) t[i] = tn[i];
                for (int i = 0; i < cam::kMaxParams; ++i) prm[i] = pn[i];
                evaluate_k<NV>(Q, pcol, rp.loss_scale, q, t, prm, true, ev);
                const double z = 2.0 * rel - 1.0;
                const double f = 1.0 - z * z * z;
                radius = radius / (f > 1.0 / 3.0 ? f : 1.0 / 3.0);
                radius = radius < 1e16 ? radius : 1e16;
                decrease = 2.0;
                if (gmax(ev) <= rp.gradient_tolerance) break;
            } else {
                radius = radius / decrease;
                decrease = 2.0 * decrease;
                if (radius < 1e-32) break;
            }
        }
        if (usable && rp.covariance) {
            // the pose block of (J^T J)^-1 over all K columns; rank rule of 12.8 on the K x K matrix
            double H[K * K], V[K * K];
            for (int i = 0; i < K; ++i)
                for (int j = 0; j < K; ++j) H[K * i + j] = symk<K>(ev.H, i, j);
            tvg::jacobi_eigen_t<K>(H, V);
            double lmin = H[0], lmax = H[0];
            for (int i = 1; i < K; ++i) {
                lmin = H[(K + 1) * i] < lmin ? H[(K + 1) * i] : lmin;
                lmax = H[(K + 1) * i] > lmax ? H[(K + 1) * i] : lmax;
            }
            if (!(lmax > 0.0) || !(lmin > 1e-28 * lmax) || !finite(lmax)) {
                usable = false;
            } else {
                for (int i = 0; i < 6; ++i)
                    for (int j = 0; j < 6; ++j) {
                        double s2 = 0.0;
                        for (int k = 0; k < K; ++k) s2 = s2 + V[K * i + k] * (V[K * j + k] / H[(K + 1) * k]);
                        out.cov[6 * i + j] = s2;
                    }
            }
        }
    }
    out.success = usable;
    for (int i = 0; i < 4; ++i) out.q[i] = q[i];
    for (int i = 0; i < 3; ++i) out.t[i] = t[i];
    for (int i = 0; i < cam::kMaxParams; ++i) out.prm[i] = prm[i];
}
#undef APR_T

}  // namespace apr
}  // namespace amc
