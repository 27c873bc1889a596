// rigpose_core.h — the numerics of the rig absolute pose (include/amc_rigpose.h) that are not
// already abspose_core.h's: the generalised P3P, the residual through cam_from_rig, the unique-inlier support and the
// refinement's residual with a camera per correspondence.  Compiles for host and device like abspose_core.h; FP
// contraction is off, so the bits equal those of the CPU reference written from section 13 (tests/rigpose_ref).
#pragma once

#include "abspose_core.h"

namespace amc {
namespace rp {

using ap::finite;
using ap::Jet;
using ap::kDblEps;
using ap::kDblMax;
using ap::kLanes;
using tvg::dsqrt;

// one camera of a rig as the kernels read it (built on the host, 13.2)
struct RigCam {
    int32_t model;
    uint32_t lift_on_device;  // 0: the pixels of this camera were lifted with host libm
    double params[cam::kMaxParams];
    double Rt[12];            // cam_from_rig.matrix(), row-major 3 x 4
    double origin[3];         // -Rc^T tc
    double q[4];              // cam_from_rig rotation, x y z w
};

// ---- 13.2: the ray of a normalised point in the rig frame ------------------------------------------------------------
AMC_HD void rig_ray(const double* Rt, double u, double v, double* d) {
    const double nn = dsqrt(u * u + v * v + 1.0);
    const double r0 = u / nn, r1 = v / nn, r2 = 1.0 / nn;
    for (int j = 0; j < 3; ++j) d[j] = (Rt[j] * r0 + Rt[4 + j] * r1) + Rt[8 + j] * r2;
}

// ---- 13.3: GP3P ------------------------------------------------------------------------------------------------------
// f_ij(li, lj) = li^2 + lj^2 + m li lj + u li + v lj + k
struct Quadric {
    double m, u, v, k;
};
AMC_HD Quadric gp3p_quadric(const double* ci, const double* di, const double* Xi, const double* cj, const double* dj,
                            const double* Xj) {
    const double e[3] = {ci[0] - cj[0], ci[1] - cj[1], ci[2] - cj[2]};
    const double x[3] = {Xi[0] - Xj[0], Xi[1] - Xj[1], Xi[2] - Xj[2]};
    Quadric f;
    f.m = -2.0 * ((di[0] * dj[0] + di[1] * dj[1]) + di[2] * dj[2]);
    f.u = 2.0 * ((e[0] * di[0] + e[1] * di[1]) + e[2] * di[2]);
    f.v = -2.0 * ((e[0] * dj[0] + e[1] * dj[1]) + e[2] * dj[2]);
    f.k = ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) - ((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    return f;
}
AMC_HD double quadric_value(const Quadric& f, double li, double lj) {
    return ((((li * li + lj * lj) + f.m * li * lj) + f.u * li) + f.v * lj) + f.k;
}
// product of two polynomials in (x, y), coefficient [x degree][y degree]
template <int AX, int AY, int BX, int BY>
AMC_HD void bimul(const double (&a)[AX][AY], const double (&b)[BX][BY], double (&r)[AX + BX - 1][AY + BY - 1]) {
    for (int i = 0; i < AX + BX - 1; ++i)
        for (int j = 0; j < AY + BY - 1; ++j) r[i][j] = 0.0;
    for (int i = 0; i < AX; ++i)
        for (int j = 0; j < AY; ++j)
            for (int k = 0; k < BX; ++k)
                for (int l = 0; l < BY; ++l) r[i + k][j + l] = r[i + k][j + l] + a[i][j] * b[k][l];
}

// c, d: origins and unit directions of the three rays (rig frame), X: the three world points; models ascending by the
// octic's root (rig_from_world, 3 x 4 row-major); returns the count (<= 8)
AMC_HD int gp3p(const double (&c)[3][3], const double (&d)[3][3], const double (&X)[3][3], double (*models)[12]) {
    const Quadric f12 = gp3p_quadric(c[0], d[0], X[0], c[1], d[1], X[1]);
    const Quadric f13 = gp3p_quadric(c[0], d[0], X[0], c[2], d[2], X[2]);
    const Quadric f23 = gp3p_quadric(c[1], d[1], X[1], c[2], d[2], X[2]);
    // x = lambda2, y = lambda3.  f12 = l1^2 + a1(x) l1 + a0(x), f13 = l1^2 + b1(y) l1 + b0(y);
    // D0 = a0 - b0, D1 = a1 - b1, E = a1 b0 - a0 b1, g = D0^2 + D1 E
    const double D0[3][3] = {{f12.k - f13.k, -f13.v, -1.0}, {f12.v, 0.0, 0.0}, {1.0, 0.0, 0.0}};
    const double D1[2][2] = {{f12.u - f13.u, -f13.m}, {f12.m, 0.0}};
    const double E[3][3] = {{f12.u * f13.k - f12.k * f13.u, f12.u * f13.v - f12.k * f13.m, f12.u},
                            {f12.m * f13.k - f12.v * f13.u, f12.m * f13.v - f12.v * f13.m, f12.m},
                            {-f13.u, -f13.m, 0.0}};
    double DD[5][5], DE[4][4];
    bimul<3, 3, 3, 3>(D0, D0, DD);
    bimul<2, 2, 3, 3>(D1, E, DE);
    double rows[5][5];
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 5; ++j) rows[i][j] = (i < 4 && j < 4) ? DD[i][j] + DE[i][j] : DD[i][j];
    // g mod f23 in x, f23 = x^2 + p1(y) x + p0(y): x^4, x^3, x^2 in turn
    const double p1[2] = {f23.u, f23.m}, p0[3] = {f23.k, f23.v, 1.0};
    {
        const double L = rows[4][0];
        for (int j = 0; j < 2; ++j) rows[3][j] = rows[3][j] - L * p1[j];
        for (int j = 0; j < 3; ++j) rows[2][j] = rows[2][j] - L * p0[j];
    }
    {
        const double L[2] = {rows[3][0], rows[3][1]};
        double t3[3], t4[4];
        ap::pmul(L, 2, p1, 2, t3);
        ap::pmul(L, 2, p0, 3, t4);
        for (int j = 0; j < 3; ++j) rows[2][j] = rows[2][j] - t3[j];
        for (int j = 0; j < 4; ++j) rows[1][j] = rows[1][j] - t4[j];
    }
    {
        const double L[3] = {rows[2][0], rows[2][1], rows[2][2]};
        double t4[4], t5[5];
        ap::pmul(L, 3, p1, 2, t4);
        ap::pmul(L, 3, p0, 3, t5);
        for (int j = 0; j < 4; ++j) rows[1][j] = rows[1][j] - t4[j];
        for (int j = 0; j < 5; ++j) rows[0][j] = rows[0][j] - t5[j];
    }
    const double r1[4] = {rows[1][0], rows[1][1], rows[1][2], rows[1][3]};
    const double r0[5] = {rows[0][0], rows[0][1], rows[0][2], rows[0][3], rows[0][4]};
    // the octic r0^2 - p1 r0 r1 + p0 r1^2
    double r0r0[9], r0r1[8], p1r0r1[9], r1r1[7], p0r1r1[9], oct[9];
    ap::pmul(r0, 5, r0, 5, r0r0);
    ap::pmul(r0, 5, r1, 4, r0r1);
    ap::pmul(p1, 2, r0r1, 8, p1r0r1);
    ap::pmul(r1, 4, r1, 4, r1r1);
    ap::pmul(p0, 3, r1r1, 7, p0r1r1);
    bool ok = true;
    for (int i = 0; i < 9; ++i) {
        oct[i] = (r0r0[i] - p1r0r1[i]) + p0r1r1[i];
        ok = ok && finite(oct[i]);
    }
    if (!ok) return 0;
    double roots[8];
    const int nr = tvg::real_roots_t<8>(oct, roots);
    int nm = 0;
    for (int k = 0; k < nr; ++k) {
        const double y = roots[k];
        const double r1v = ((r1[3] * y + r1[2]) * y + r1[1]) * y + r1[0];
        const double r0v = (((r0[4] * y + r0[3]) * y + r0[2]) * y + r0[1]) * y + r0[0];
        if (r1v == 0.0 || !finite(r1v)) continue;
        const double x = -r0v / r1v;
        const double a1 = f12.u + f12.m * x, a0 = (f12.k + f12.v * x) + x * x;
        const double b1 = f13.u + f13.m * y, b0 = (f13.k + f13.v * y) + y * y;
        const double den = a1 - b1;
        if (den == 0.0 || !finite(den)) continue;
        double l[3] = {-(a0 - b0) / den, x, y};
        // two Newton steps on (f12, f13, f23)
        bool good = true;
        for (int it = 0; it < 2 && good; ++it) {
            double J[9] = {2.0 * l[0] + f12.m * l[1] + f12.u, 2.0 * l[1] + f12.m * l[0] + f12.v, 0.0,
                           2.0 * l[0] + f13.m * l[2] + f13.u, 0.0, 2.0 * l[2] + f13.m * l[0] + f13.v,
                           0.0, 2.0 * l[1] + f23.m * l[2] + f23.u, 2.0 * l[2] + f23.m * l[1] + f23.v};
            double F[3] = {quadric_value(f12, l[0], l[1]), quadric_value(f13, l[0], l[2]),
                           quadric_value(f23, l[1], l[2])};
            good = ap::solve_gauss<3>(J, F);
            for (int i = 0; i < 3; ++i) l[i] = l[i] - F[i];
        }
        if (!good || !finite(l[0]) || !finite(l[1]) || !finite(l[2])) continue;
        double dst[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) dst[i][j] = c[i][j] + l[i] * d[i][j];
        ap::umeyama3(X, dst, models[nm]);
        ++nm;
    }
    return nm;
}

// ---- 13.4: the squared reprojection error of X under rig_from_world P in the camera Rt ---------------------------------
AMC_HD double sq_reproj_rig(const double* P, const double* Rt, const double* X, double u, double v) {
    const double Y0 = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
    const double Y1 = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
    const double Y2 = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
    const double z = Rt[8] * Y0 + Rt[9] * Y1 + Rt[10] * Y2 + Rt[11];
    if (!(z > kDblEps)) return kDblMax;
    const double x = Rt[0] * Y0 + Rt[1] * Y1 + Rt[2] * Y2 + Rt[3];
    const double y = Rt[4] * Y0 + Rt[5] * Y1 + Rt[6] * Y2 + Rt[7];
    const double du = x / z - u, dv = y / z - v;
    return du * du + dv * dv;
}

// ---- 13.5: the unique-inlier support ---------------------------------------------------------------------------------
struct Support {
    uint32_t cnt;
    uint32_t uniq;
    double sum;
};
AMC_HD bool better(const Support& a, const Support& b) {
    if (a.uniq != b.uniq) return a.uniq > b.uniq;
    if (a.cnt != b.cnt) return a.cnt > b.cnt;
    return a.sum < b.sum;
}
constexpr uint32_t kNoPrev = 0xffffffffu;
// an inlier counts once per 3D point: not when an earlier correspondence of the same point is flagged too
AMC_HD bool first_flagged_of_its_point(const uint8_t* flag, const uint32_t* prev_same, uint32_t k) {
    for (uint32_t j = prev_same[k]; j != kNoPrev; j = prev_same[j])
        if (flag[j]) return false;
    return true;
}

// ---- 13.7: the residual of one correspondence (pixels) with d/d(q, t) of rig_from_world -------------------------------
// Eigen's q * X + t, then the constant q_c * Y + t_c in the same product form, then the correspondence's camera
AMC_HD void rig_pixel_residual(const RigCam& cm, const double* q, const double* t, const double* X, double ox, double oy,
                               Jet& rx, Jet& ry) {
    Jet qv[4], tv[3];
    for (int i = 0; i < 4; ++i) {
        qv[i] = ap::jconst(q[i]);
        qv[i].d[i] = 1.0;
    }
    for (int i = 0; i < 3; ++i) {
        tv[i] = ap::jconst(t[i]);
        tv[i].d[4 + i] = 1.0;
    }
    Jet uv0 = qv[1] * X[2] - qv[2] * X[1];
    Jet uv1 = qv[2] * X[0] - qv[0] * X[2];
    Jet uv2 = qv[0] * X[1] - qv[1] * X[0];
    uv0 = uv0 + uv0;
    uv1 = uv1 + uv1;
    uv2 = uv2 + uv2;
    const Jet c0 = qv[1] * uv2 - qv[2] * uv1;
    const Jet c1 = qv[2] * uv0 - qv[0] * uv2;
    const Jet c2 = qv[0] * uv1 - qv[1] * uv0;
    const Jet Y0 = (X[0] + qv[3] * uv0) + c0 + tv[0];
    const Jet Y1 = (X[1] + qv[3] * uv1) + c1 + tv[1];
    const Jet Y2 = (X[2] + qv[3] * uv2) + c2 + tv[2];
    const double* qc = cm.q;
    Jet w0 = qc[1] * Y2 - qc[2] * Y1;
    Jet w1 = qc[2] * Y0 - qc[0] * Y2;
    Jet w2 = qc[0] * Y1 - qc[1] * Y0;
    w0 = w0 + w0;
    w1 = w1 + w1;
    w2 = w2 + w2;
    const Jet e0 = qc[1] * w2 - qc[2] * w1;
    const Jet e1 = qc[2] * w0 - qc[0] * w2;
    const Jet e2 = qc[0] * w1 - qc[1] * w0;
    const Jet Z0 = (Y0 + qc[3] * w0) + e0 + cm.Rt[3];
    const Jet Z1 = (Y1 + qc[3] * w1) + e1 + cm.Rt[7];
    const Jet Z2 = (Y2 + qc[3] * w2) + e2 + cm.Rt[11];
    ap::img_from_cam_t<Jet>(cm.model, cm.params, Z0, Z1, Z2, rx, ry);
    rx = rx - ox;
    ry = ry - oy;
}

}  // namespace rp
}  // namespace amc
