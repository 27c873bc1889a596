// absrefine_ref.cc — CPU reference of the joint pose and camera refinement, written from DESIGN.md section 25.  It
// includes no product header (nothing of pycolmap_amd/csrc or include/).  Section 25 is defined on top of section 12's
// primitives, and so is this file: it includes the section-12 reference beside it for the fdlibm transcendentals
// (12.9), the 64-way sum (12.10), the pivoted Gaussian elimination and the quaternion Plus, and writes everything of
// section 25 itself: the K-column jets with the camera parameters active, the eleven models over them, the LM loop
// over K columns, the K x K rank rule and the covariance's pose block.  Plain sequential C++; the 64 lanes run in turn.
// -ffp-contract=off: the GPU kernel (csrc/absrefine.hip) must match this bit for bit.
#include "../abspose_ref/abspose_ref.cc"

namespace {

constexpr int kMaxW = 17;   // 7 pose coordinates + 10 camera columns
constexpr int kMaxK = 16;

// 25.1: the variable parameter indices, ascending
int VariableParams(int model, bool rf, bool re, int* idx) {
    const int nf = NumFocal(model), np = NumParams(model);
    int nv = 0;
    if (rf)
        for (int i = 0; i < nf; ++i) idx[nv++] = i;
    if (re)
        for (int i = nf + 2; i < np; ++i) idx[nv++] = i;
    return nv;
}

// ---- 25.5: jets over W = 7 + nv columns; a camera parameter is a value, its own derivative and its column ------------
struct J {
    double a, g[kMaxW];
};
struct P {
    double a, da;
    int col;  // -1: constant
};
thread_local int gW = 7;

J JCst(double a) {
    J r;
    r.a = a;
    for (int i = 0; i < kMaxW; ++i) r.g[i] = 0.0;
    return r;
}
J operator+(const J& x, const J& y) { J r = JCst(x.a + y.a); for (int i = 0; i < gW; ++i) r.g[i] = x.g[i] + y.g[i]; return r; }
J operator-(const J& x, const J& y) { J r = JCst(x.a - y.a); for (int i = 0; i < gW; ++i) r.g[i] = x.g[i] - y.g[i]; return r; }
J operator*(const J& x, const J& y) {
    J r = JCst(x.a * y.a);
    for (int i = 0; i < gW; ++i) r.g[i] = x.a * y.g[i] + x.g[i] * y.a;
    return r;
}
J operator/(const J& x, const J& y) {
    J r = JCst(x.a / y.a);
    for (int i = 0; i < gW; ++i) r.g[i] = (x.g[i] - r.a * y.g[i]) / y.a;
    return r;
}
J operator+(const J& x, double c) { J r = x; r.a = x.a + c; return r; }
J operator+(double c, const J& x) { J r = x; r.a = c + x.a; return r; }
J operator-(const J& x, double c) { J r = x; r.a = x.a - c; return r; }
J operator*(const J& x, double c) { J r = JCst(x.a * c); for (int i = 0; i < gW; ++i) r.g[i] = x.g[i] * c; return r; }
J operator*(double c, const J& x) { J r = JCst(c * x.a); for (int i = 0; i < gW; ++i) r.g[i] = c * x.g[i]; return r; }
J operator/(const J& x, double c) { J r = JCst(x.a / c); for (int i = 0; i < gW; ++i) r.g[i] = x.g[i] / c; return r; }
J SqrtJ(const J& x) {
    J r = JCst(std::sqrt(x.a));
    const double h = 2.0 * r.a;
    for (int i = 0; i < gW; ++i) r.g[i] = x.g[i] / h;
    return r;
}
J AtanJ(const J& x) {
    J r = JCst(Atan(x.a));
    const double h = 1.0 + x.a * x.a;
    for (int i = 0; i < gW; ++i) r.g[i] = x.g[i] / h;
    return r;
}
// parameter with scalar, parameter with itself (FOV's omega)
P operator*(double c, const P& p) { return P{c * p.a, c * p.da, p.col}; }
P operator/(const P& p, double c) { return P{p.a / c, p.da / c, p.col}; }
P operator*(const P& x, const P& y) { return P{x.a * y.a, x.a * y.da + x.da * y.a, x.col}; }
P operator/(const P& x, const P& y) {
    const double a = x.a / y.a;
    return P{a, (x.da - a * y.da) / y.a, x.col};
}
P SinP(const P& p) { return P{Sin(p.a), Cos(p.a) * p.da, p.col}; }
P CosP(const P& p) { return P{Cos(p.a), -(Sin(p.a) * p.da), p.col}; }
// parameter with jet: the full rule in the parameter's own column, the constant-operand rule in the others
J operator*(const P& p, const J& x) {
    J r = JCst(p.a * x.a);
    for (int i = 0; i < gW; ++i) r.g[i] = i == p.col ? p.a * x.g[i] + p.da * x.a : p.a * x.g[i];
    return r;
}
J operator*(const J& x, const P& p) {
    J r = JCst(x.a * p.a);
    for (int i = 0; i < gW; ++i) r.g[i] = i == p.col ? x.a * p.da + x.g[i] * p.a : x.g[i] * p.a;
    return r;
}
J operator/(const J& x, const P& p) {
    J r = JCst(x.a / p.a);
    for (int i = 0; i < gW; ++i) r.g[i] = i == p.col ? (x.g[i] - r.a * p.da) / p.a : x.g[i] / p.a;
    return r;
}
J operator+(const J& x, const P& p) {
    J r = x;
    r.a = x.a + p.a;
    if (p.col >= 0) r.g[p.col] = x.g[p.col] + p.da;
    return r;
}
J operator-(const J& x, const P& p) {
    J r = x;
    r.a = x.a - p.a;
    if (p.col >= 0) r.g[p.col] = x.g[p.col] - p.da;
    return r;
}

// Camera::ImgFromCam with the camera's parameters active
void ImgFromCamJ(int model, const double* prm, const int* pcol, const J& pu, const J& pv, const J& pw, J* x, J* y) {
    J u = pu / pw, v = pv / pw;
    const int nf = NumFocal(model);
    auto par = [&](int i) { return P{prm[i], pcol[i] >= 0 ? 1.0 : 0.0, pcol[i]}; };
    const P f1 = par(0), f2 = par(nf - 1), c1 = par(nf), c2 = par(nf + 1);
    auto e = [&](int i) { return par(nf + 2 + i); };
    if (model <= 1) {
        *x = f1 * u + c1;
        *y = f2 * v + c2;
        return;
    }
    if (model == 7) {
        const P om = e(0), om2 = om * om;
        const J r2 = u * u + v * v;
        J f;
        if (om2.a < 1e-4) {
            f = (om2 * r2) / 3.0 - om2 / 12.0 + 1.0;
        } else {
            const P th = SinP(om / 2.0) / CosP(om / 2.0);
            if (r2.a < 1e-4) {
                f = (-2.0 * th * (4.0 * r2 * th * th - 3.0)) / (3.0 * om);
            } else {
                const J r = SqrtJ(r2);
                f = AtanJ(r * 2.0 * th) / (r * om);
            }
        }
        *x = f1 * (u * f) + c1;
        *y = f2 * (v * f) + c2;
        return;
    }
    if (model == 10) {
        const J r = SqrtJ(u * u + v * v);
        if (r.a > kEps) {
            const J th = AtanJ(r);
            u = th * u / r;
            v = th * v / r;
        }
    }
    J du, dv;
    if (model == 5 || model == 8 || model == 9) {
        const J r = SqrtJ(u * u + v * v);
        if (r.a > kEps) {
            const J th = AtanJ(r), t2 = th * th;
            J thd;
            if (model == 8) {
                thd = th * (1.0 + e(0) * t2);
            } else if (model == 9) {
                const J t4 = t2 * t2;
                thd = th * (1.0 + e(0) * t2 + e(1) * t4);
            } else {
                const J t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
                thd = th * (1.0 + e(0) * t2 + e(1) * t4 + e(2) * t6 + e(3) * t8);
            }
            du = u * thd / r - u;
            dv = v * thd / r - v;
        } else {
            du = u * 0.0;
            dv = v * 0.0;
        }
    } else if (model == 2 || model == 3) {
        const J r2 = u * u + v * v;
        const J rad = model == 2 ? e(0) * r2 : e(0) * r2 + e(1) * r2 * r2;
        du = u * rad;
        dv = v * rad;
    } else {  // 4, 6, 10
        const J u2 = u * u, uv = u * v, v2 = v * v, r2 = u2 + v2;
        if (model == 4) {
            const J rad = e(0) * r2 + e(1) * r2 * r2;
            du = u * rad + 2.0 * e(2) * uv + e(3) * (r2 + 2.0 * u2);
            dv = v * rad + 2.0 * e(3) * uv + e(2) * (r2 + 2.0 * v2);
        } else if (model == 6) {
            const J r4 = r2 * r2, r6 = r4 * r2;
            const J rad = (1.0 + e(0) * r2 + e(1) * r4 + e(4) * r6) / (1.0 + e(5) * r2 + e(6) * r4 + e(7) * r6);
            du = u * rad + 2.0 * e(2) * uv + e(3) * (r2 + 2.0 * u2) - u;
            dv = v * rad + 2.0 * e(3) * uv + e(2) * (r2 + 2.0 * v2) - v;
        } else {
            const J r4 = r2 * r2, r6 = r4 * r2, r8 = r6 * r2;
            const J rad = e(0) * r2 + e(1) * r4 + e(4) * r6 + e(5) * r8;
            du = u * rad + 2.0 * e(2) * uv + e(3) * (r2 + 2.0 * u2) + e(6) * r2;
            dv = v * rad + 2.0 * e(3) * uv + e(2) * (r2 + 2.0 * v2) + e(7) * r2;
        }
    }
    *x = f1 * (u + du) + c1;
    *y = f2 * (v + dv) + c2;
}

// the pixel of the world point Pw with d/d(qx, qy, qz, qw, tx, ty, tz, camera columns)
void ProjectJ(int model, const double* prm, const int* pcol, const double* q, const double* t, const double* Pw, J* rx,
              J* ry) {
    J qv[4], tv[3];
    for (int i = 0; i < 4; ++i) { qv[i] = JCst(q[i]); qv[i].g[i] = 1.0; }
    for (int i = 0; i < 3; ++i) { tv[i] = JCst(t[i]); tv[i].g[4 + i] = 1.0; }
    J w0 = qv[1] * Pw[2] - qv[2] * Pw[1], w1 = qv[2] * Pw[0] - qv[0] * Pw[2], w2 = qv[0] * Pw[1] - qv[1] * Pw[0];
    w0 = w0 + w0;
    w1 = w1 + w1;
    w2 = w2 + w2;
    const J p0 = (Pw[0] + qv[3] * w0) + (qv[1] * w2 - qv[2] * w1) + tv[0];
    const J p1 = (Pw[1] + qv[3] * w1) + (qv[2] * w0 - qv[0] * w2) + tv[1];
    const J p2 = (Pw[2] + qv[3] * w2) + (qv[0] * w1 - qv[1] * w0) + tv[2];
    ImgFromCamJ(model, prm, pcol, p0, p1, p2, rx, ry);
}

// D1's round-robin Jacobi for n <= 16 (the section-12 reference's stops at 12)
void Jacobi16(int n, double* a, double* v) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) v[i * n + j] = i == j ? 1.0 : 0.0;
    double total = 0.0;
    for (int i = 0; i < n * n; ++i) total += a[i] * a[i];
    const double tol = total * 1e-32;
    const int m = (n & 1) ? n : n - 1;
    for (int sweep = 0; sweep < 40; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) off += a[p * n + q] * a[p * n + q];
        if (!(off > tol)) break;
        for (int r = 0; r < m; ++r) {
            int pq[8][2], np = 0;
            for (int k = 1; k <= (m - 1) / 2; ++k) {
                const int x = (r + k) % m, y = (r - k + m) % m;
                pq[np][0] = std::min(x, y);
                pq[np][1] = std::max(x, y);
                ++np;
            }
            if (!(n & 1)) {
                pq[np][0] = r;
                pq[np][1] = n - 1;
                ++np;
            }
            double cs[8][2];
            bool act[8];
            for (int e = 0; e < np; ++e) {
                const int p = pq[e][0], q = pq[e][1];
                act[e] = a[p * n + q] != 0.0;
                if (!act[e]) continue;
                const double theta = (a[q * n + q] - a[p * n + p]) / (2.0 * a[p * n + q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                cs[e][0] = 1.0 / std::sqrt(t * t + 1.0);
                cs[e][1] = t * cs[e][0];
            }
            for (int e = 0; e < np; ++e) {
                if (!act[e]) continue;
                const int p = pq[e][0], q = pq[e][1];
                const double c = cs[e][0], s = cs[e][1];
                for (int k = 0; k < n; ++k) {
                    const double akp = a[k * n + p], akq = a[k * n + q];
                    a[k * n + p] = c * akp - s * akq;
                    a[k * n + q] = s * akp + c * akq;
                    const double vkp = v[k * n + p], vkq = v[k * n + q];
                    v[k * n + p] = c * vkp - s * vkq;
                    v[k * n + q] = s * vkp + c * vkq;
                }
            }
            for (int e = 0; e < np; ++e) {
                if (!act[e]) continue;
                const int p = pq[e][0], q = pq[e][1];
                const double c = cs[e][0], s = cs[e][1];
                for (int k = 0; k < n; ++k) {
                    const double apk = a[p * n + k], aqk = a[q * n + k];
                    a[p * n + k] = c * apk - s * aqk;
                    a[q * n + k] = s * apk + c * aqk;
                }
            }
        }
    }
}

// Gaussian elimination with partial pivoting (first largest |pivot|) on the n x n row-major A; false on a zero or
// non-finite pivot
bool GaussN(int n, double* A, double* b) {
    for (int k = 0; k < n; ++k) {
        int piv = k;
        double best = std::fabs(A[k * n + k]);
        for (int i = k + 1; i < n; ++i)
            if (std::fabs(A[i * n + k]) > best) {
                best = std::fabs(A[i * n + k]);
                piv = i;
            }
        if (!(best > 0.0) || !std::isfinite(best)) return false;
        if (piv != k) {
            for (int j = 0; j < n; ++j) std::swap(A[k * n + j], A[piv * n + j]);
            std::swap(b[k], b[piv]);
        }
        for (int i = k + 1; i < n; ++i) {
            const double f = A[i * n + k] / A[k * n + k];
            for (int j = k; j < n; ++j) A[i * n + j] = A[i * n + j] - f * A[k * n + j];
            b[i] = b[i] - f * b[k];
        }
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = b[i];
        for (int j = i + 1; j < n; ++j) s = s - A[i * n + j] * b[j];
        b[i] = s / A[i * n + i];
    }
    return true;
}

// ---- 25.2: the solver over K = 6 + nv columns ------------------------------------------------------------------------
struct Opts {
    int model;
    bool rf, re;
    double gtol, scale;
    int64_t iters;
    bool cov;
};
struct EvalK {
    double cost, H[kMaxK][kMaxK], g[kMaxK];
};
constexpr int kMaxSum = 1 + kMaxK * (kMaxK + 1) / 2 + kMaxK;

struct Solver {
    Opts o;
    int nv, K, idx[10], pcol[12];
    const double* xy;
    const double* X;
    const std::vector<char>* mask;

    EvalK Evaluate(const double* q, const double* t, const double* prm, bool jac) const {
        const double b = o.scale * o.scale, c = 1.0 / b;
        const double Jm[4][3] = {{q[3], q[2], -q[1]}, {-q[2], q[3], q[0]}, {q[1], -q[0], q[3]}, {-q[0], -q[1], -q[2]}};
        const int NH = K * (K + 1) / 2;
        const std::vector<double> s = Sum64<kMaxSum>(mask->size(), [&](size_t k, double* acc) {
            if (!(*mask)[k]) return;
            J rx, ry;
            ProjectJ(o.model, prm, pcol, q, t, X + 3 * k, &rx, &ry);
            rx = rx - xy[2 * k];
            ry = ry - xy[2 * k + 1];
            const double sq = rx.a * rx.a + ry.a * ry.a, sum = 1.0 + sq * c;
            acc[0] = acc[0] + 0.5 * (b * Log(sum));
            if (!jac) return;
            const double w = std::sqrt(1.0 / sum);
            double Jr[2][kMaxK];
            const J* rr[2] = {&rx, &ry};
            for (int r = 0; r < 2; ++r) {
                const double* g = rr[r]->g;
                for (int j = 0; j < 3; ++j) Jr[r][j] = w * (g[0] * Jm[0][j] + g[1] * Jm[1][j] + g[2] * Jm[2][j] + g[3] * Jm[3][j]);
                for (int j = 0; j < 3; ++j) Jr[r][3 + j] = w * g[4 + j];
                for (int j = 0; j < nv; ++j) Jr[r][6 + j] = w * g[7 + j];
            }
            const double f[2] = {w * rx.a, w * ry.a};
            int tt = 1;
            for (int i = 0; i < K; ++i)
                for (int j = i; j < K; ++j, ++tt) acc[tt] = acc[tt] + (Jr[0][i] * Jr[0][j] + Jr[1][i] * Jr[1][j]);
            for (int i = 0; i < K; ++i) acc[1 + NH + i] = acc[1 + NH + i] + (Jr[0][i] * f[0] + Jr[1][i] * f[1]);
        });
        EvalK e;
        e.cost = s[0];
        for (int i = 0, tt = 1; i < K; ++i)
            for (int j = i; j < K; ++j, ++tt) e.H[i][j] = e.H[j][i] = s[tt];
        for (int i = 0; i < K; ++i) e.g[i] = s[1 + NH + i];
        return e;
    }
    double GradNormK(const double* q, const double* t, const double* g) const {
        double m = GradNorm(q, t, g);
        for (int j = 0; j < nv; ++j) m = std::max(m, std::fabs(g[6 + j]));
        return m;
    }
};

// returns usable; q, t, prm (12) updated in place; cov (36) when asked
bool RefineK(const Opts& o, double* q, double* t, double* prm, const double* xy, const double* X,
             const std::vector<char>& mask, double* cov, Trace* tr) {
    Trace local;
    Trace& T = tr ? *tr : local;
    T = Trace();
    Solver S;
    S.o = o;
    S.nv = VariableParams(o.model, o.rf, o.re, S.idx);
    S.K = 6 + S.nv;
    for (int i = 0; i < 12; ++i) S.pcol[i] = -1;
    for (int j = 0; j < S.nv; ++j) S.pcol[S.idx[j]] = 7 + j;
    S.xy = xy;
    S.X = X;
    S.mask = &mask;
    gW = 7 + S.nv;
    const int K = S.K, nv = S.nv, np = NumParams(o.model);
    if (cov) std::fill(cov, cov + 36, 0.0);
    if (std::count(mask.begin(), mask.end(), 1) == 0) {  // A9
        T.exit = NOTHING_TO_REFINE;
        return true;
    }
    EvalK ev = S.Evaluate(q, t, prm, true);
    if (!std::isfinite(ev.cost)) {
        T.exit = NOT_FINITE_START;
        return false;
    }
    double sc[kMaxK];
    for (int i = 0; i < K; ++i) sc[i] = 1.0 / (1.0 + std::sqrt(ev.H[i][i]));
    double radius = 1e4, decrease = 2.0;
    int invalid = 0;
    if (!(S.GradNormK(q, t, ev.g) <= o.gtol)) {
        for (int64_t it = 1; it <= o.iters; ++it) {
            T.iterations = static_cast<int32_t>(it);
            double Hs[kMaxK * kMaxK], A[kMaxK * kMaxK], y[kMaxK];
            for (int i = 0; i < K; ++i) {
                for (int j = 0; j < K; ++j) Hs[K * i + j] = sc[i] * ev.H[i][j] * sc[j];
                y[i] = -(sc[i] * ev.g[i]);
            }
            for (int i = 0; i < K * K; ++i) A[i] = Hs[i];
            for (int i = 0; i < K; ++i)
                A[(K + 1) * i] = A[(K + 1) * i] + std::min(std::max(Hs[(K + 1) * i], 1e-6), 1e32) / radius;
            bool valid = GaussN(K, A, y);
            double mcc = 0.0;
            if (valid) {
                double gy = 0.0, yhy = 0.0;
                for (int i = 0; i < K; ++i) {
                    gy = gy + (sc[i] * ev.g[i]) * y[i];
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
            double d[kMaxK], qn[4], tn[3], pn[12];
            for (int i = 0; i < K; ++i) d[i] = sc[i] * y[i];
            QuatPlus(q, d, qn);
            for (int i = 0; i < 3; ++i) tn[i] = t[i] + d[3 + i];
            for (int i = 0; i < 12; ++i) pn[i] = prm[i];
            for (int j = 0; j < nv; ++j) pn[S.idx[j]] = prm[S.idx[j]] + d[6 + j];
            double sn = 0.0, xn = 0.0;
            for (int i = 0; i < 4; ++i) { sn = sn + (q[i] - qn[i]) * (q[i] - qn[i]); xn = xn + q[i] * q[i]; }
            for (int i = 0; i < 3; ++i) { sn = sn + (t[i] - tn[i]) * (t[i] - tn[i]); xn = xn + t[i] * t[i]; }
            if (nv > 0)  // the whole camera block is in the state vector once one of its coordinates varies
                for (int i = 0; i < np; ++i) { sn = sn + (prm[i] - pn[i]) * (prm[i] - pn[i]); xn = xn + prm[i] * prm[i]; }
            if (std::sqrt(sn) <= 1e-8 * (std::sqrt(xn) + 1e-8)) {
                T.exit = PARAMETER_TOLERANCE;
                break;
            }
            const double cand = S.Evaluate(qn, tn, pn, false).cost;
            const double change = ev.cost - (std::isfinite(cand) ? cand : DBL_MAX);
            if (std::fabs(change) <= 1e-6 * ev.cost) {
                T.exit = FUNCTION_TOLERANCE;
                break;
            }
            const double rel = change / mcc;
            if (rel > 1e-3) {
                std::memcpy(q, qn, sizeof qn);
                std::memcpy(t, tn, sizeof tn);
                std::memcpy(prm, pn, sizeof pn);
                ev = S.Evaluate(q, t, prm, true);
                const double z = 2.0 * rel - 1.0, f = 1.0 - z * z * z;
                radius = std::min(radius / std::max(f, 1.0 / 3.0), 1e16);
                decrease = 2.0;
                ++T.accepted;
                if (S.GradNormK(q, t, ev.g) <= o.gtol) {
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
    double H[kMaxK * kMaxK], V[kMaxK * kMaxK];
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) H[K * i + j] = ev.H[i][j];
    Jacobi16(K, H, V);
    double lmin = H[0], lmax = H[0];
    for (int i = 1; i < K; ++i) {
        lmin = std::min(lmin, H[(K + 1) * i]);
        lmax = std::max(lmax, H[(K + 1) * i]);
    }
    if (!(lmax > 0.0) || !(lmin > 1e-28 * lmax) || !std::isfinite(lmax)) {
        T.rank_failed = 1;
        return false;
    }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double s = 0.0;
            for (int k = 0; k < K; ++k) s = s + V[K * i + k] * (V[K * j + k] / H[(K + 1) * k]);
            cov[6 * i + j] = s;
        }
    return true;
}

}  // namespace

extern "C" {

// one correspondence's projection as the joint refinement evaluates it: the pixel and its derivatives by
// (qx, qy, qz, qw, tx, ty, tz, camera columns), row-major 2 x 17 (the first 7 + nv columns are set); returns nv
int absrefine_ref_project(int model, const double* params, int rf, int re, const double* q, const double* t,
                          const double* X, double* xy, double* Jout, int32_t* idx_out) {
    int idx[10], pcol[12];
    const int nv = VariableParams(model, rf != 0, re != 0, idx);
    for (int i = 0; i < 12; ++i) pcol[i] = -1;
    for (int j = 0; j < nv; ++j) pcol[idx[j]] = 7 + j;
    gW = 7 + nv;
    J rx, ry;
    ProjectJ(model, params, pcol, q, t, X, &rx, &ry);
    xy[0] = rx.a;
    xy[1] = ry.a;
    for (int i = 0; i < kMaxW; ++i) {
        Jout[i] = i < gW ? rx.g[i] : 0.0;
        Jout[kMaxW + i] = i < gW ? ry.g[i] : 0.0;
    }
    for (int j = 0; j < nv; ++j) idx_out[j] = idx[j];
    return nv;
}

// the pixels of n world points (no derivatives asked: the camera constant), n x 2
void absrefine_ref_project_points(int model, const double* params, const double* q, const double* t, const double* X,
                                  size_t n, double* xy) {
    int pcol[12];
    for (int i = 0; i < 12; ++i) pcol[i] = -1;
    gW = 7;
    for (size_t k = 0; k < n; ++k) {
        J rx, ry;
        ProjectJ(model, params, pcol, q, t, X + 3 * k, &rx, &ry);
        xy[2 * k] = rx.a;
        xy[2 * k + 1] = ry.a;
    }
}

// ref: gradient_tolerance, max_num_iterations, loss_function_scale, refine_focal_length, refine_extra_params (as
// doubles); prm_out: nq x 12 (the refined camera of a usable query, else the input); trace: 6 int32 per query, or null
int absrefine_ref_refine(const uint64_t* off, size_t nq, const int32_t* models, const double* cparams, const double* p2,
                         const double* p3, const double* q0, const double* t0, const uint8_t* mask, const double* ref,
                         int want_cov, uint8_t* success, double* qvec, double* tvec, double* prm_out, double* cov,
                         int32_t* trace) {
    for (size_t i = 0; i < nq; ++i) {
        if (models[i] < 0 || models[i] > 10) return 1;
        Opts o;
        o.model = models[i];
        o.gtol = ref[0];
        o.iters = static_cast<int64_t>(ref[1]);
        o.scale = ref[2];
        o.rf = ref[3] != 0.0;
        o.re = ref[4] != 0.0;
        o.cov = want_cov != 0;
        const size_t a = off[i], n = off[i + 1] - off[i];
        std::vector<char> m(n);
        for (size_t k = 0; k < n; ++k) m[k] = mask[a + k] ? 1 : 0;
        double q[4], t[3], prm[12], in[12], c36[36];
        for (int k = 0; k < 12; ++k) in[k] = prm[k] = k < NumParams(o.model) ? cparams[12 * i + k] : 0.0;
        std::memcpy(q, q0 + 4 * i, sizeof q);
        std::memcpy(t, t0 + 3 * i, sizeof t);
        Trace T;
        const bool ok = RefineK(o, q, t, prm, p2 + 2 * a, p3 + 3 * a, m, c36, &T);
        success[i] = ok ? 1 : 0;
        std::memcpy(qvec + 4 * i, q, sizeof q);
        std::memcpy(tvec + 3 * i, t, sizeof t);
        std::memcpy(prm_out + 12 * i, ok ? prm : in, sizeof prm);
        if (cov) std::memcpy(cov + 36 * i, c36, sizeof c36);
        if (trace) {
            const int32_t row[6] = {T.iterations, T.accepted, T.rejected, T.invalid, T.exit, T.rank_failed};
            std::memcpy(trace + 6 * i, row, sizeof row);
        }
    }
    return 0;
}

}  // extern "C"
