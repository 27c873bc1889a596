// rigpose_ref.cc — CPU reference of the rig absolute pose: plain sequential C++ written from the
// section, no product header.  The pieces section 13 shares with section 12 (the 64-way sum, Jacobi, the root finder's
// bracket step, the SVD, the Procrustes rotation, the cameras, the forward-mode scalar, Gaussian elimination, the
// trial-count formula, the manifold) are those of the absolute pose reference, included unmodified.
#include "../abspose_ref/abspose_ref.cc"

#include <set>

namespace {

// ---- D2 for degree <= 8: the derivative chain of abspose_ref.cc's RealRoots, longer -----------------------------------
int RealRoots8(const double* cin, int deg, double* roots) {
    while (deg > 0 && cin[deg] == 0.0) --deg;
    if (deg == 0) return 0;
    double chain[9][9];
    for (int i = 0; i <= deg; ++i) chain[0][i] = cin[i];
    for (int j = 1; j < deg; ++j)
        for (int i = 1; i <= deg - j + 1; ++i) chain[j][i - 1] = chain[j - 1][i] * i;
    double crit[8], cur[8];
    int nc = 0;
    for (int j = deg - 1; j >= 0; --j) {
        nc = RootsBetween(chain[j], j + 1 < deg ? chain[j + 1] : nullptr, deg - j, crit, nc, cur);
        for (int i = 0; i < nc; ++i) crit[i] = cur[i];
    }
    for (int i = 0; i < nc; ++i) roots[i] = crit[i];
    return nc;
}

// ---- 13.2 -------------------------------------------------------------------------------------------------------------
struct RigCamera {
    int model;
    double params[12];
    double Rt[12];     // cam_from_rig.matrix()
    double origin[3];  // -Rc^T tc
    double q[4];       // x y z w
};
RigCamera MakeRigCamera(int model, const double* params, const double* g) {
    RigCamera c{};
    c.model = model;
    for (int i = 0; i < NumParams(model); ++i) c.params[i] = params[i];
    const double x = g[0], y = g[1], z = g[2], w = g[3];  // Eigen::Quaterniond::toRotationMatrix
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double R[9] = {1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx,
                         txz - twy, tyz + twx, 1.0 - (txx + tyy)};
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) c.Rt[4 * r + k] = R[3 * r + k];
        c.Rt[4 * r + 3] = g[4 + r];
    }
    for (int j = 0; j < 3; ++j) c.origin[j] = -((R[j] * g[4] + R[3 + j] * g[5]) + R[6 + j] * g[6]);
    for (int i = 0; i < 4; ++i) c.q[i] = g[i];
    return c;
}
void RigRay(const double* Rt, double u, double v, double* d) {
    const double nn = std::sqrt(u * u + v * v + 1.0);
    const double r0 = u / nn, r1 = v / nn, r2 = 1.0 / nn;
    for (int j = 0; j < 3; ++j) d[j] = (Rt[j] * r0 + Rt[4 + j] * r1) + Rt[8 + j] * r2;
}

// ---- 13.3: GP3P -------------------------------------------------------------------------------------------------------
struct Quadric {  // li^2 + lj^2 + m li lj + u li + v lj + k
    double m, u, v, k;
};
Quadric MakeQuadric(const double* ci, const double* di, const double* Xi, const double* cj, const double* dj,
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
double QuadricValue(const Quadric& f, double li, double lj) {
    return ((((li * li + lj * lj) + f.m * li * lj) + f.u * li) + f.v * lj) + f.k;
}
// polynomials in (x, y) as [x degree][y degree], row stride 5
void BiMul(const double* a, int ax, int ay, const double* b, int bx, int by, double* r) {
    for (int i = 0; i < ax + bx - 1; ++i)
        for (int j = 0; j < ay + by - 1; ++j) r[5 * i + j] = 0.0;
    for (int i = 0; i < ax; ++i)
        for (int j = 0; j < ay; ++j)
            for (int k = 0; k < bx; ++k)
                for (int l = 0; l < by; ++l) r[5 * (i + k) + j + l] = r[5 * (i + k) + j + l] + a[5 * i + j] * b[5 * k + l];
}
struct Gp3pSolution {
    Model model;
    double depth[3];
};
// c, d: 3 x 3 ray origins and unit directions (rig frame); X: 3 x 3 world points
std::vector<Gp3pSolution> GP3P(const double* c, const double* d, const double* X) {
    std::vector<Gp3pSolution> out;
    const Quadric f12 = MakeQuadric(c, d, X, c + 3, d + 3, X + 3);
    const Quadric f13 = MakeQuadric(c, d, X, c + 6, d + 6, X + 6);
    const Quadric f23 = MakeQuadric(c + 3, d + 3, X + 3, c + 6, d + 6, X + 6);
    // x = lambda2, y = lambda3; D0 = a0 - b0, D1 = a1 - b1, E = a1 b0 - a0 b1, g = D0^2 + D1 E
    double D0[25] = {}, D1[25] = {}, E[25] = {}, DD[25] = {}, DE[25] = {}, rows[5][5];
    D0[0] = f12.k - f13.k; D0[1] = -f13.v; D0[2] = -1.0; D0[5] = f12.v; D0[10] = 1.0;
    D1[0] = f12.u - f13.u; D1[1] = -f13.m; D1[5] = f12.m;
    E[0] = f12.u * f13.k - f12.k * f13.u; E[1] = f12.u * f13.v - f12.k * f13.m; E[2] = f12.u;
    E[5] = f12.m * f13.k - f12.v * f13.u; E[6] = f12.m * f13.v - f12.v * f13.m; E[7] = f12.m;
    E[10] = -f13.u; E[11] = -f13.m; E[12] = 0.0;
    BiMul(D0, 3, 3, D0, 3, 3, DD);
    BiMul(D1, 2, 2, E, 3, 3, DE);
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 5; ++j) rows[i][j] = (i < 4 && j < 4) ? DD[5 * i + j] + DE[5 * i + j] : DD[5 * i + j];
    // g mod f23 in x, f23 = x^2 + p1(y) x + p0(y)
    const double p1[2] = {f23.u, f23.m}, p0[3] = {f23.k, f23.v, 1.0};
    {
        const double L = rows[4][0];
        for (int j = 0; j < 2; ++j) rows[3][j] = rows[3][j] - L * p1[j];
        for (int j = 0; j < 3; ++j) rows[2][j] = rows[2][j] - L * p0[j];
    }
    {
        const double L[2] = {rows[3][0], rows[3][1]};
        double t3[3], t4[4];
        PolyMul(L, 2, p1, 2, t3);
        PolyMul(L, 2, p0, 3, t4);
        for (int j = 0; j < 3; ++j) rows[2][j] = rows[2][j] - t3[j];
        for (int j = 0; j < 4; ++j) rows[1][j] = rows[1][j] - t4[j];
    }
    {
        const double L[3] = {rows[2][0], rows[2][1], rows[2][2]};
        double t4[4], t5[5];
        PolyMul(L, 3, p1, 2, t4);
        PolyMul(L, 3, p0, 3, t5);
        for (int j = 0; j < 4; ++j) rows[1][j] = rows[1][j] - t4[j];
        for (int j = 0; j < 5; ++j) rows[0][j] = rows[0][j] - t5[j];
    }
    const double* r1 = rows[1];  // degree 3
    const double* r0 = rows[0];  // degree 4
    double r0r0[9], r0r1[8], p1r0r1[9], r1r1[7], p0r1r1[9], oct[9];
    PolyMul(r0, 5, r0, 5, r0r0);
    PolyMul(r0, 5, r1, 4, r0r1);
    PolyMul(p1, 2, r0r1, 8, p1r0r1);
    PolyMul(r1, 4, r1, 4, r1r1);
    PolyMul(p0, 3, r1r1, 7, p0r1r1);
    for (int i = 0; i < 9; ++i) {
        oct[i] = (r0r0[i] - p1r0r1[i]) + p0r1r1[i];
        if (!std::isfinite(oct[i])) return out;
    }
    double roots[8];
    const int nr = RealRoots8(oct, 8, roots);
    for (int k = 0; k < nr; ++k) {
        const double y = roots[k];
        const double r1v = ((r1[3] * y + r1[2]) * y + r1[1]) * y + r1[0];
        const double r0v = (((r0[4] * y + r0[3]) * y + r0[2]) * y + r0[1]) * y + r0[0];
        if (r1v == 0.0 || !std::isfinite(r1v)) continue;
        const double x = -r0v / r1v;
        const double a1 = f12.u + f12.m * x, a0 = (f12.k + f12.v * x) + x * x;
        const double b1 = f13.u + f13.m * y, b0 = (f13.k + f13.v * y) + y * y;
        const double den = a1 - b1;
        if (den == 0.0 || !std::isfinite(den)) continue;
        double l[3] = {-(a0 - b0) / den, x, y};
        bool good = true;
        for (int it = 0; it < 2 && good; ++it) {
            double J[9] = {2.0 * l[0] + f12.m * l[1] + f12.u, 2.0 * l[1] + f12.m * l[0] + f12.v, 0.0,
                           2.0 * l[0] + f13.m * l[2] + f13.u, 0.0, 2.0 * l[2] + f13.m * l[0] + f13.v,
                           0.0, 2.0 * l[1] + f23.m * l[2] + f23.u, 2.0 * l[2] + f23.m * l[1] + f23.v};
            double F[3] = {QuadricValue(f12, l[0], l[1]), QuadricValue(f13, l[0], l[2]), QuadricValue(f23, l[1], l[2])};
            good = Gauss<3>(J, F);
            for (int i = 0; i < 3; ++i) l[i] = l[i] - F[i];
        }
        if (!good || !std::isfinite(l[0]) || !std::isfinite(l[1]) || !std::isfinite(l[2])) continue;
        // rig_from_world: the Procrustes of 12.3 from X_i to p_i = c_i + l_i d_i
        double p[3][3], ms[3], md[3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) p[i][j] = c[3 * i + j] + l[i] * d[3 * i + j];
        for (int j = 0; j < 3; ++j) {
            ms[j] = (X[j] + X[3 + j] + X[6 + j]) / 3.0;
            md[j] = (p[0][j] + p[1][j] + p[2][j]) / 3.0;
        }
        double S[9], U[9], Sv[3], V[9], R[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double s = 0.0;
                for (int k2 = 0; k2 < 3; ++k2) s = s + (p[k2][i] - md[i]) * (X[3 * k2 + j] - ms[j]);
                S[3 * i + j] = s / 3.0;
            }
        Svd3(S, U, Sv, V);
        Procrustes(U, V, R);
        Gp3pSolution sol;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) sol.model[4 * i + j] = R[3 * i + j];
            sol.model[4 * i + 3] = md[i] - (R[3 * i] * ms[0] + R[3 * i + 1] * ms[1] + R[3 * i + 2] * ms[2]);
            sol.depth[i] = l[i];
        }
        out.push_back(sol);
    }
    return out;
}

// ---- 13.4 / 13.5 ------------------------------------------------------------------------------------------------------
struct RigCorr {
    size_t n;
    const RigCamera* cams;
    const int32_t* cidx;
    const double* uv;  // normalized
    const double* X;
    const uint32_t* id;  // point ids (13.2)
};
double RigResidual(const Model& P, const double* Rt, const double* X, double u, double v) {
    const double Y0 = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
    const double Y1 = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
    const double Y2 = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
    const double z = Rt[8] * Y0 + Rt[9] * Y1 + Rt[10] * Y2 + Rt[11];
    if (!(z > kEps)) return DBL_MAX;
    const double x = Rt[0] * Y0 + Rt[1] * Y1 + Rt[2] * Y2 + Rt[3];
    const double y = Rt[4] * Y0 + Rt[5] * Y1 + Rt[6] * Y2 + Rt[7];
    const double du = x / z - u, dv = y / z - v;
    return du * du + dv * dv;
}
struct RigSupport {
    size_t cnt = 0, uniq = 0;
    double sum = DBL_MAX;
};
bool RigBetter(const RigSupport& a, const RigSupport& b) {
    if (a.uniq != b.uniq) return a.uniq > b.uniq;
    if (a.cnt != b.cnt) return a.cnt > b.cnt;
    return a.sum < b.sum;
}
RigSupport RigScore(const RigCorr& c, const Model& P, double maxr, std::vector<char>* mask) {
    std::vector<char> in(c.n);
    const std::vector<double> s = Sum64<2>(c.n, [&](size_t k, double* o) {
        const double r = RigResidual(P, c.cams[c.cidx[k]].Rt, c.X + 3 * k, c.uv[2 * k], c.uv[2 * k + 1]);
        in[k] = r <= maxr;
        if (in[k]) {
            o[0] = o[0] + 1.0;
            o[1] = o[1] + r;
        }
    });
    std::set<uint32_t> ids;
    for (size_t k = 0; k < c.n; ++k)
        if (in[k]) ids.insert(c.id[k]);
    if (mask) *mask = in;
    RigSupport sp;
    sp.cnt = static_cast<size_t>(s[0]);
    sp.uniq = ids.size();
    sp.sum = s[1];
    return sp;
}
std::vector<uint32_t> PointIds(size_t n, const double* X) {
    std::vector<uint32_t> id(n);
    for (size_t k = 0; k < n; ++k) {
        id[k] = static_cast<uint32_t>(k);
        for (size_t j = 0; j < k; ++j)
            if (X[3 * j] == X[3 * k] && X[3 * j + 1] == X[3 * k + 1] && X[3 * j + 2] == X[3 * k + 2]) {
                id[k] = static_cast<uint32_t>(j);
                break;
            }
    }
    return id;
}

// ---- 13.6: RANSAC<GP3PEstimator, UniqueInlierSupportMeasurer> ------------------------------------------------------------
struct RigRansacReport {
    bool success = false;
    RigSupport support;
    uint64_t trials = 0;
    Model model{};
    std::vector<char> mask;
};
RigRansacReport RigRansac(const RigCorr& c, const RansacOpts& o) {
    RigRansacReport rep;
    rep.support = RigSupport();
    rep.support.sum = DBL_MAX;
    rep.mask.assign(c.n, 0);
    if (c.n < 3) return rep;
    std::mt19937 gen(0);
    std::vector<uint32_t> perm(c.n);
    for (size_t i = 0; i < c.n; ++i) perm[i] = static_cast<uint32_t>(i);
    RigSupport best;
    Model best_model{};
    uint64_t dyn = o.max_trials;
    bool abort = false;
    uint64_t t;
    for (t = 0; t < o.max_trials; ++t) {
        if (abort) {
            t += 1;
            break;
        }
        for (uint32_t i = 0; i < 3; ++i) {
            std::uniform_int_distribution<uint32_t> dist(i, static_cast<uint32_t>(c.n - 1));
            std::swap(perm[i], perm[dist(gen)]);
        }
        double cc[9], dd[9], X3[9];
        for (int i = 0; i < 3; ++i) {
            const uint32_t k = perm[i];
            const RigCamera& cm = c.cams[c.cidx[k]];
            RigRay(cm.Rt, c.uv[2 * k], c.uv[2 * k + 1], dd + 3 * i);
            for (int j = 0; j < 3; ++j) {
                cc[3 * i + j] = cm.origin[j];
                X3[3 * i + j] = c.X[3 * k + j];
            }
        }
        for (const Gp3pSolution& sol : GP3P(cc, dd, X3)) {
            const RigSupport s = RigScore(c, sol.model, o.maxr, nullptr);
            if (RigBetter(s, best)) {
                best = s;
                best_model = sol.model;
                dyn = o.max_trials > o.min_trials ? NumTrials(best.cnt, c.n, o.conf, o.mult) : o.max_trials;
            }
            if (t >= dyn && t >= o.min_trials) {
                abort = true;
                break;
            }
        }
    }
    rep.trials = t;
    if (best.cnt < 3) return rep;
    rep.success = true;
    rep.support = best;
    rep.model = best_model;
    RigScore(c, best_model, o.maxr, &rep.mask);
    return rep;
}

// ---- 13.7: RefineGeneralizedAbsolutePose ---------------------------------------------------------------------------------
// residual of correspondence k (pixels) with d/d(q, t) of rig_from_world
void RigPixelResidual(const RigCamera& cm, const double* q, const double* t, const double* P, double ox, double oy, D* rx,
                      D* ry) {
    D qv[4], tv[3];
    for (int i = 0; i < 4; ++i) { qv[i] = Cst(q[i]); qv[i].g[i] = 1.0; }
    for (int i = 0; i < 3; ++i) { tv[i] = Cst(t[i]); tv[i].g[4 + i] = 1.0; }
    D w0 = qv[1] * P[2] - qv[2] * P[1], w1 = qv[2] * P[0] - qv[0] * P[2], w2 = qv[0] * P[1] - qv[1] * P[0];
    w0 = w0 + w0;
    w1 = w1 + w1;
    w2 = w2 + w2;
    const D Y0 = (P[0] + qv[3] * w0) + (qv[1] * w2 - qv[2] * w1) + tv[0];
    const D Y1 = (P[1] + qv[3] * w1) + (qv[2] * w0 - qv[0] * w2) + tv[1];
    const D Y2 = (P[2] + qv[3] * w2) + (qv[0] * w1 - qv[1] * w0) + tv[2];
    const double* qc = cm.q;
    D v0 = qc[1] * Y2 - qc[2] * Y1, v1 = qc[2] * Y0 - qc[0] * Y2, v2 = qc[0] * Y1 - qc[1] * Y0;
    v0 = v0 + v0;
    v1 = v1 + v1;
    v2 = v2 + v2;
    const D Z0 = (Y0 + qc[3] * v0) + (qc[1] * v2 - qc[2] * v1) + cm.Rt[3];
    const D Z1 = (Y1 + qc[3] * v1) + (qc[2] * v0 - qc[0] * v2) + cm.Rt[7];
    const D Z2 = (Y2 + qc[3] * v2) + (qc[0] * v1 - qc[1] * v0) + cm.Rt[11];
    ImgFromCam(cm.model, cm.params, Z0, Z1, Z2, rx, ry);
    *rx = *rx - ox;
    *ry = *ry - oy;
}
struct RigRefOpts {
    double gtol, scale;
    int64_t iters;
    bool cov;
};
struct RigProblem {
    const RigCamera* cams;
    const int32_t* cidx;
    const double* xy;
    const double* X;
};
Eval RigEvaluate(const RigRefOpts& o, const RigProblem& pr, const double* q, const double* t, const std::vector<char>& mask,
                 bool jac) {
    const double b = o.scale * o.scale, c = 1.0 / b;
    const double Jm[4][3] = {{q[3], q[2], -q[1]}, {-q[2], q[3], q[0]}, {q[1], -q[0], q[3]}, {-q[0], -q[1], -q[2]}};
    const std::vector<double> s = Sum64<28>(mask.size(), [&](size_t k, double* acc) {
        if (!mask[k]) return;
        D rx, ry;
        RigPixelResidual(pr.cams[pr.cidx[k]], q, t, pr.X + 3 * k, pr.xy[2 * k], pr.xy[2 * k + 1], &rx, &ry);
        const double sq = rx.a * rx.a + ry.a * ry.a, sum = 1.0 + sq * c;
        acc[0] = acc[0] + 0.5 * (b * Log(sum));
        if (!jac) return;
        const double w = std::sqrt(1.0 / sum);
        double J[2][6];
        const D* rr[2] = {&rx, &ry};
        for (int r = 0; r < 2; ++r) {
            const double* g = rr[r]->g;
            for (int j = 0; j < 3; ++j) J[r][j] = w * (g[0] * Jm[0][j] + g[1] * Jm[1][j] + g[2] * Jm[2][j] + g[3] * Jm[3][j]);
            for (int j = 0; j < 3; ++j) J[r][3 + j] = w * g[4 + j];
        }
        const double f[2] = {w * rx.a, w * ry.a};
        int tt = 1;
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j, ++tt) acc[tt] = acc[tt] + (J[0][i] * J[0][j] + J[1][i] * J[1][j]);
        for (int i = 0; i < 6; ++i) acc[22 + i] = acc[22 + i] + (J[0][i] * f[0] + J[1][i] * f[1]);
    });
    Eval e;
    e.cost = s[0];
    for (int i = 0, tt = 1; i < 6; ++i)
        for (int j = i; j < 6; ++j, ++tt) e.H[i][j] = e.H[j][i] = s[tt];
    for (int i = 0; i < 6; ++i) e.g[i] = s[22 + i];
    return e;
}
// 12.7 / 12.8 with the rig residual: returns usable; q, t updated in place; cov (36) when asked; tr (abspose_ref.cc's
// Trace: recorded, never read back) filled when given
bool RigRefine(const RigRefOpts& o, const RigProblem& pr, double* q, double* t, const std::vector<char>& mask, double* cov,
               Trace* tr = nullptr) {
    Trace local;
    Trace& T = tr ? *tr : local;
    T = Trace();
    if (cov) std::fill(cov, cov + 36, 0.0);
    if (std::count(mask.begin(), mask.end(), 1) == 0) {
        T.exit = NOTHING_TO_REFINE;
        return true;
    }
    Eval ev = RigEvaluate(o, pr, q, t, mask, true);
    if (!std::isfinite(ev.cost)) {
        T.exit = NOT_FINITE_START;
        return false;
    }
    double sc[6];
    for (int i = 0; i < 6; ++i) sc[i] = 1.0 / (1.0 + std::sqrt(ev.H[i][i]));
    double radius = 1e4, decrease = 2.0;
    int invalid = 0;
    if (!(GradNorm(q, t, ev.g) <= o.gtol)) {
        for (int64_t it = 1; it <= o.iters; ++it) {
            T.iterations = static_cast<int32_t>(it);
            double Hs[36], A[36], y[6];
            for (int i = 0; i < 6; ++i) {
                for (int j = 0; j < 6; ++j) Hs[6 * i + j] = sc[i] * ev.H[i][j] * sc[j];
                y[i] = -(sc[i] * ev.g[i]);
            }
            std::memcpy(A, Hs, sizeof A);
            for (int i = 0; i < 6; ++i) A[7 * i] = A[7 * i] + std::min(std::max(Hs[7 * i], 1e-6), 1e32) / radius;
            bool valid = Gauss<6>(A, y);
            double mcc = 0.0;
            if (valid) {
                double gy = 0.0, yhy = 0.0;
                for (int i = 0; i < 6; ++i) {
                    gy = gy + (sc[i] * ev.g[i]) * y[i];
                    double hy = 0.0;
                    for (int j = 0; j < 6; ++j) hy = hy + Hs[6 * i + j] * y[j];
                    yhy = yhy + y[i] * hy;
                }
                mcc = -(gy + 0.5 * yhy);
                valid = mcc > 0.0;
            }
            if (!valid) {
                radius = radius / decrease;
                decrease = 2.0 * decrease;
                ++T.invalid;
                if (++invalid >= 5) {
                    T.exit = INVALID_STEPS;
                    return false;
                }
                if (radius < 1e-32) {
                    T.exit = MIN_RADIUS;
                    break;
                }
                continue;
            }
            invalid = 0;
            double d[6], qn[4], tn[3];
            for (int i = 0; i < 6; ++i) d[i] = sc[i] * y[i];
            QuatPlus(q, d, qn);
            for (int i = 0; i < 3; ++i) tn[i] = t[i] + d[3 + i];
            double sn = 0.0, xn = 0.0;
            for (int i = 0; i < 4; ++i) { sn = sn + (q[i] - qn[i]) * (q[i] - qn[i]); xn = xn + q[i] * q[i]; }
            for (int i = 0; i < 3; ++i) { sn = sn + (t[i] - tn[i]) * (t[i] - tn[i]); xn = xn + t[i] * t[i]; }
            if (std::sqrt(sn) <= 1e-8 * (std::sqrt(xn) + 1e-8)) {
                T.exit = PARAMETER_TOLERANCE;
                break;
            }
            const double cand = RigEvaluate(o, pr, qn, tn, mask, false).cost;
            const double change = ev.cost - (std::isfinite(cand) ? cand : DBL_MAX);
            if (std::fabs(change) <= 1e-6 * ev.cost) {
                T.exit = FUNCTION_TOLERANCE;
                break;
            }
            const double rel = change / mcc;
            if (rel > 1e-3) {
                std::memcpy(q, qn, sizeof qn);
                std::memcpy(t, tn, sizeof tn);
                ev = RigEvaluate(o, pr, q, t, mask, true);
                const double z = 2.0 * rel - 1.0, f = 1.0 - z * z * z;
                radius = std::min(radius / std::max(f, 1.0 / 3.0), 1e16);
                decrease = 2.0;
                ++T.accepted;
                if (GradNorm(q, t, ev.g) <= o.gtol) {
                    T.exit = GRADIENT_AFTER_STEP;
                    break;
                }
            } else {
                radius = radius / decrease;
                decrease = 2.0 * decrease;
                ++T.rejected;
                if (radius < 1e-32) {
                    T.exit = MIN_RADIUS;
                    break;
                }
            }
        }
    } else {
        T.exit = GRADIENT_AT_START;
    }
    if (!o.cov) return true;
    double H[36], V[36];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) H[6 * i + j] = ev.H[i][j];
    Jacobi(6, H, V);
    double lmin = H[0], lmax = H[0];
    for (int i = 1; i < 6; ++i) {
        lmin = std::min(lmin, H[7 * i]);
        lmax = std::max(lmax, H[7 * i]);
    }
    if (!(lmax > 0.0) || !(lmin > 1e-28 * lmax) || !std::isfinite(lmax)) {
        T.rank_failed = 1;
        return false;
    }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s = s + V[6 * i + k] * (V[6 * j + k] / H[7 * k]);
            cov[6 * i + j] = s;
        }
    return true;
}

}  // namespace

extern "C" {

// c, d, X: 3 x 3 each; models: 8 x 12, depths: 8 x 3; returns the solution count
int rigpose_ref_gp3p(const double* c, const double* d, const double* X, double* models, double* depths) {
    const std::vector<Gp3pSolution> s = GP3P(c, d, X);
    for (size_t i = 0; i < s.size(); ++i) {
        std::memcpy(models + 12 * i, s[i].model.data(), 12 * sizeof(double));
        std::memcpy(depths + 3 * i, s[i].depth, 3 * sizeof(double));
    }
    return static_cast<int>(s.size());
}

// the support (13.5) of `model` over one query with normalized points uv; out: cnt, uniq, sum; mask: n bytes
void rigpose_ref_support(size_t n, size_t ncam, const int32_t* models, const double* cparams, const double* rigs,
                         const int32_t* cidx, const double* uv, const double* X, const double* model, double maxr,
                         double* out, uint8_t* mask) {
    std::vector<RigCamera> cams;
    for (size_t i = 0; i < ncam; ++i) cams.push_back(MakeRigCamera(models[i], cparams + 12 * i, rigs + 7 * i));
    const std::vector<uint32_t> id = PointIds(n, X);
    Model P;
    std::memcpy(P.data(), model, sizeof(double) * 12);
    std::vector<char> m;
    const RigSupport s = RigScore(RigCorr{n, cams.data(), cidx, uv, X, id.data()}, P, maxr, &m);
    out[0] = static_cast<double>(s.cnt);
    out[1] = static_cast<double>(s.uniq);
    out[2] = s.sum;
    for (size_t k = 0; k < n; ++k) mask[k] = m[k];
}

// the point ids (13.2) of n world points
void rigpose_ref_point_ids(size_t n, const double* X, uint32_t* ids) {
    const std::vector<uint32_t> id = PointIds(n, X);
    std::copy(id.begin(), id.end(), ids);
}

// is the support a (cnt, uniq, sum) better than b
int rigpose_ref_better(const double* a, const double* b) {
    RigSupport x, y;
    x.cnt = static_cast<size_t>(a[0]); x.uniq = static_cast<size_t>(a[1]); x.sum = a[2];
    y.cnt = static_cast<size_t>(b[0]); y.uniq = static_cast<size_t>(b[1]); y.sum = b[2];
    return RigBetter(x, y) ? 1 : 0;
}

// residual (2) and its Jacobian (2 x 7, d/d(qx qy qz qw tx ty tz)) of one correspondence
void rigpose_ref_residual(int model, const double* cparams, const double* rig, const double* q, const double* t,
                          const double* X, const double* xy, double* res, double* jac) {
    const RigCamera cm = MakeRigCamera(model, cparams, rig);
    D rx, ry;
    RigPixelResidual(cm, q, t, X, xy[0], xy[1], &rx, &ry);
    res[0] = rx.a;
    res[1] = ry.a;
    for (int i = 0; i < 7; ++i) {
        jac[i] = rx.g[i];
        jac[7 + i] = ry.g[i];
    }
}

// est: max_error, min_inlier_ratio, confidence, dyn_num_trials_multiplier, min_num_trials, max_num_trials; ref:
// gradient_tolerance, max_num_iterations, loss_function_scale (all as doubles); trace: 6 int32 per query (iterations,
// accepted, rejected, invalid, exit, rank test failed; exit -1 where no refinement ran), or null
int rigpose_ref_estimate_trace(const uint64_t* off, size_t nq, const uint64_t* coff, const int32_t* models,
                         const double* cparams, const double* rigs, const int32_t* cidx, const double* p2,
                         const double* p3, const double* est, const double* ref, int want_cov, uint8_t* success,
                         double* qvec, double* tvec, uint32_t* num_inliers, uint32_t* num_all_inliers,
                               uint64_t* num_trials, double* covariance, uint8_t* mask, int32_t* trace) {
    const uint64_t min_t = static_cast<uint64_t>(est[4]);
    const uint64_t max_t = std::min(static_cast<uint64_t>(est[5]),
                                    NumTrials(static_cast<uint64_t>(est[1] * 100000), 100000, est[2], est[3]));
    for (size_t qi = 0; qi < nq; ++qi) {
        const size_t c0 = off[qi], n = off[qi + 1] - off[qi];
        std::vector<RigCamera> cams;
        for (uint64_t i = coff[qi]; i < coff[qi + 1]; ++i) cams.push_back(MakeRigCamera(models[i], cparams + 12 * i, rigs + 7 * i));
        const int32_t* ci = cidx + c0;
        double* cv = covariance ? covariance + 36 * qi : nullptr;
        if (cv) std::fill(cv, cv + 36, 0.0);
        if (trace) {
            const int32_t row[6] = {0, 0, 0, 0, -1, 0};
            std::memcpy(trace + 6 * qi, row, sizeof row);
        }
        std::vector<double> uv(2 * n);
        double sum = 0.0;
        for (size_t k = 0; k < n; ++k) {
            const RigCamera& cm = cams[ci[k]];
            CamFromImg(cm.model, cm.params, p2[2 * (c0 + k)], p2[2 * (c0 + k) + 1], &uv[2 * k], &uv[2 * k + 1]);
            const int nf = NumFocal(cm.model);
            double mf = 0.0;
            for (int i = 0; i < nf; ++i) mf += cm.params[i];
            sum += est[0] / (mf / nf);
        }
        const double thr = n ? sum / static_cast<double>(n) : 0.0;
        const std::vector<uint32_t> id = PointIds(n, p3 + 3 * c0);
        const RigRansacReport r = RigRansac(RigCorr{n, cams.data(), ci, uv.data(), p3 + 3 * c0, id.data()},
                                            RansacOpts{thr * thr, est[2], est[3], min_t, max_t});
        success[qi] = 0;
        std::fill(qvec + 4 * qi, qvec + 4 * qi + 4, 0.0);
        std::fill(tvec + 3 * qi, tvec + 3 * qi + 3, 0.0);
        num_trials[qi] = r.trials;
        num_inliers[qi] = r.success ? static_cast<uint32_t>(r.support.uniq) : 0;
        num_all_inliers[qi] = r.success ? static_cast<uint32_t>(r.support.cnt) : 0;
        for (size_t k = 0; k < n; ++k) mask[c0 + k] = r.mask[k];
        if (!r.success) continue;
        double* q = qvec + 4 * qi;
        double* t = tvec + 3 * qi;
        if (!ModelToPose(r.model, q, t)) continue;
        const RigRefOpts ro{ref[0], ref[2], static_cast<int64_t>(ref[1]), want_cov != 0};
        Trace tr;
        success[qi] = RigRefine(ro, RigProblem{cams.data(), ci, p2 + 2 * c0, p3 + 3 * c0}, q, t, r.mask, cv, &tr) ? 1 : 0;
        if (trace) {
            const int32_t row[6] = {tr.iterations, tr.accepted, tr.rejected, tr.invalid, tr.exit, tr.rank_failed};
            std::memcpy(trace + 6 * qi, row, sizeof row);
        }
    }
    return 0;
}
int rigpose_ref_estimate(const uint64_t* off, size_t nq, const uint64_t* coff, const int32_t* models,
                         const double* cparams, const double* rigs, const int32_t* cidx, const double* p2,
                         const double* p3, const double* est, const double* ref, int want_cov, uint8_t* success,
                         double* qvec, double* tvec, uint32_t* num_inliers, uint32_t* num_all_inliers,
                         uint64_t* num_trials, double* covariance, uint8_t* mask) {
    return rigpose_ref_estimate_trace(off, nq, coff, models, cparams, rigs, cidx, p2, p3, est, ref, want_cov, success, qvec,
                                      tvec, num_inliers, num_all_inliers, num_trials, covariance, mask, nullptr);
}

}  // extern "C"
