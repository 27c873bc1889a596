// abspose_ref.cc — CPU reference of absolute pose, written from DESIGN.md section 12 alone (it includes no product
// header: nothing of pycolmap_amd/csrc or include/): COLMAP 3.9.1's EstimateAbsolutePose (LORANSAC<P3P, EPnP> per
// focal-length factor, RandomSampler on std::mt19937 + std::uniform_int_distribution) and RefineAbsolutePose (Cauchy
// loss, Ceres' Levenberg-Marquardt on the quaternion manifold, covariance).  Plain sequential C++ with std::vector;
// the sums over correspondences are the 64-way order of 12.10 written as an explicit array of 64 partial sums.
// The round-robin Jacobi (D1), the real-root finder (D2), svd3, the camera lift and the quaternion follow
// oracle/tvg_oracle.cc's restatements.  -ffp-contract=off: the GPU kernel (csrc/abspose.hip) must match this bit for
// bit.
#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

namespace {

const double kEps = std::numeric_limits<double>::epsilon();

// ---- 12.9: fdlibm 5.3 in + - * / and bit operations ----------------------------------------------------------------
uint32_t hi32(double x) {
    uint64_t u;
    std::memcpy(&u, &x, 8);
    return static_cast<uint32_t>(u >> 32);
}
double from_bits(uint64_t u) {
    double x;
    std::memcpy(&x, &u, 8);
    return x;
}
uint64_t to_bits(double x) {
    uint64_t u;
    std::memcpy(&u, &x, 8);
    return u;
}

double Atan(double x) {  // s_atan.c
    static const double atanhi[] = {4.63647609000806093515e-01, 7.85398163397448278999e-01,
                                    9.82793723247329054082e-01, 1.57079632679489655800e+00};
    static const double atanlo[] = {2.26987774529616870924e-17, 3.06161699786838301793e-17,
                                    1.39033110312309984516e-17, 6.12323399573676603587e-17};
    static const double aT[] = {3.33333333333329318027e-01,  -1.99999999998764832476e-01, 1.42857142725034663711e-01,
                                -1.11111104054623557880e-01, 9.09088713343650656196e-02,  -7.69187620504482999495e-02,
                                6.66107313738753120669e-02,  -5.83357013379057348645e-02, 4.97687799461593236017e-02,
                                -3.65315727442169155270e-02, 1.62858201153657823623e-02};
    const uint32_t hx = hi32(x), ix = hx & 0x7fffffff;
    int id;
    if (ix >= 0x44100000) {
        if (std::isnan(x)) return x + x;
        return (hx >> 31) ? -atanhi[3] - atanlo[3] : atanhi[3] + atanlo[3];
    }
    if (ix < 0x3fdc0000) {
        if (ix < 0x3e200000) return x;
        id = -1;
    } else {
        x = std::fabs(x);
        if (ix < 0x3ff30000) {
            if (ix < 0x3fe60000) {
                id = 0;
                x = (2.0 * x - 1.0) / (2.0 + x);
            } else {
                id = 1;
                x = (x - 1.0) / (x + 1.0);
            }
        } else if (ix < 0x40038000) {
            id = 2;
            x = (x - 1.5) / (1.0 + 1.5 * x);
        } else {
            id = 3;
            x = -1.0 / x;
        }
    }
    const double z = x * x;
    const double w = z * z;
    const double s1 = z * (aT[0] + w * (aT[2] + w * (aT[4] + w * (aT[6] + w * (aT[8] + w * aT[10])))));
    const double s2 = w * (aT[1] + w * (aT[3] + w * (aT[5] + w * (aT[7] + w * aT[9]))));
    if (id < 0) return x - x * (s1 + s2);
    const double zz = atanhi[id] - ((x * (s1 + s2) - atanlo[id]) - x);
    return (hx >> 31) ? -zz : zz;
}

double KSin(double x, double y, int iy) {  // k_sin.c
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    if ((hi32(x) & 0x7fffffff) < 0x3e400000) return x;
    const double z = x * x, v = z * x;
    const double r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    return iy == 0 ? x + v * (S1 + z * r) : x - ((z * (0.5 * y - v * r) - y) - v * S1);
}
double KCos(double x, double y) {  // k_cos.c
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const uint32_t ix = hi32(x) & 0x7fffffff;
    if (ix < 0x3e400000) return 1.0;
    const double z = x * x;
    const double r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    if (ix < 0x3fd33333) return 1.0 - (0.5 * z - (z * r - x * y));
    const double qx = ix > 0x3fe90000 ? 0.28125 : from_bits(static_cast<uint64_t>(ix - 0x00200000) << 32);
    return (1.0 - qx) - ((0.5 * z - qx) - (z * r - x * y));
}
int RemPio2(double x, double* y) {  // e_rem_pio2.c, medium arguments (|x| <= 2^19 pi/2) only
    const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00,
                 pio2_1t = 6.07710050650619224932e-11, pio2_2 = 6.07710050630396597660e-11,
                 pio2_2t = 2.02226624879595063154e-21, pio2_3 = 2.02226624871116645580e-21,
                 pio2_3t = 8.47842766036889956997e-32;
    const uint32_t hx = hi32(x), ix = hx & 0x7fffffff;
    if (ix > 0x413921fb) return -1;
    const double t = std::fabs(x);
    const int n = static_cast<int>(t * invpio2 + 0.5);
    const double fn = n;
    double r = t - fn * pio2_1, w = fn * pio2_1t;
    const int j = static_cast<int>(ix >> 20);
    y[0] = r - w;
    if (j - static_cast<int>((hi32(y[0]) >> 20) & 0x7ff) > 16) {
        double tt = r;
        w = fn * pio2_2;
        r = tt - w;
        w = fn * pio2_2t - ((tt - r) - w);
        y[0] = r - w;
        if (j - static_cast<int>((hi32(y[0]) >> 20) & 0x7ff) > 49) {
            tt = r;
            w = fn * pio2_3;
            r = tt - w;
            w = fn * pio2_3t - ((tt - r) - w);
            y[0] = r - w;
        }
    }
    y[1] = (r - y[0]) - w;
    if (hx >> 31) {
        y[0] = -y[0];
        y[1] = -y[1];
        return (-n) & 3;
    }
    return n & 3;
}
double Sin(double x) {
    const uint32_t ix = hi32(x) & 0x7fffffff;
    if (ix <= 0x3fe921fb) return KSin(x, 0.0, 0);
    if (ix >= 0x7ff00000) return x - x;
    double y[2];
    switch (RemPio2(x, y)) {
        case 0: return KSin(y[0], y[1], 1);
        case 1: return KCos(y[0], y[1]);
        case 2: return -KSin(y[0], y[1], 1);
        case 3: return -KCos(y[0], y[1]);
    }
    return std::numeric_limits<double>::quiet_NaN();
}
double Cos(double x) {
    const uint32_t ix = hi32(x) & 0x7fffffff;
    if (ix <= 0x3fe921fb) return KCos(x, 0.0);
    if (ix >= 0x7ff00000) return x - x;
    double y[2];
    switch (RemPio2(x, y)) {
        case 0: return KCos(y[0], y[1]);
        case 1: return -KSin(y[0], y[1], 1);
        case 2: return -KCos(y[0], y[1]);
        case 3: return KSin(y[0], y[1], 1);
    }
    return std::numeric_limits<double>::quiet_NaN();
}
double Log(double x) {  // e_log.c
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, two54 = 1.8014398509481984e16,
                 Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
                 Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    int32_t hx = static_cast<int32_t>(hi32(x));
    const uint32_t lx = static_cast<uint32_t>(to_bits(x));
    int k = 0;
    if (hx < 0x00100000) {
        if (((hx & 0x7fffffff) | static_cast<int32_t>(lx)) == 0) return -std::numeric_limits<double>::infinity();
        if (hx < 0) return std::numeric_limits<double>::quiet_NaN();
        k -= 54;
        x *= two54;
        hx = static_cast<int32_t>(hi32(x));
    }
    if (hx >= 0x7ff00000) return x + x;
    k += (hx >> 20) - 1023;
    hx &= 0x000fffff;
    const int32_t i = (hx + 0x95f64) & 0x100000;
    x = from_bits((static_cast<uint64_t>(static_cast<uint32_t>(hx | (i ^ 0x3ff00000))) << 32) | (to_bits(x) & 0xffffffffu));
    k += i >> 20;
    const double f = x - 1.0, dk = k;
    if ((0x000fffff & (2 + hx)) < 3) {
        if (f == 0.0) return k == 0 ? 0.0 : dk * ln2_hi + dk * ln2_lo;
        const double R = f * f * (0.5 - 0.33333333333333333 * f);
        return k == 0 ? f - R : dk * ln2_hi - ((R - dk * ln2_lo) - f);
    }
    const double s = f / (2.0 + f), z = s * s, w = z * z;
    const int32_t sel = (hx - 0x6147a) | (0x6b851 - hx);
    const double R = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7))) + w * (Lg2 + w * (Lg4 + w * Lg6));
    if (sel > 0) {
        const double hfsq = 0.5 * f * f;
        return k == 0 ? f - (hfsq - s * (hfsq + R)) : dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
    }
    return k == 0 ? f - s * (f - R) : dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f);
}

// ---- 12.10: the 64-way order (D3) ----------------------------------------------------------------------------------
// term(k, out) adds correspondence k's terms to out (a partial of lane k & 63); then the xor butterfly 32 .. 1
template <int N, typename F>
std::vector<double> Sum64(size_t n, F term) {
    std::vector<double> p(64 * N, 0.0), q(64 * N);
    for (size_t k = 0; k < n; ++k) term(k, &p[(k & 63) * N]);
    for (int m = 32; m >= 1; m >>= 1) {
        for (int l = 0; l < 64; ++l)
            for (int i = 0; i < N; ++i) q[l * N + i] = p[l * N + i] + p[(l ^ m) * N + i];
        p.swap(q);
    }
    return std::vector<double>(p.begin(), p.begin() + N);
}

// ---- D1: round-robin Jacobi (n <= 12) --------------------------------------------------------------------------------
void Jacobi(int n, double* a, double* v) {
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
            int pq[6][2], np = 0;
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
            double cs[6][2];
            bool act[6];
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

// ---- D2: real roots, bottom-up over the derivative chain -------------------------------------------------------------
double PolyEval(const double* c, int deg, double x) {
    double v = c[deg];
    for (int i = deg - 1; i >= 0; --i) v = v * x + c[i];
    return v;
}
double BracketRoot(const double* c, const double* dc, int deg, double lo, double hi, double flo) {
    for (int it = 0; it < 200; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (mid == lo || mid == hi) break;
        const double fm = PolyEval(c, deg, mid);
        if (fm == 0.0) return mid;
        if ((fm < 0.0) == (flo < 0.0)) {
            lo = mid;
            flo = fm;
        } else {
            hi = mid;
        }
        if (hi - lo <= 1.4901161193847656e-08 * (std::fabs(lo) + std::fabs(hi))) break;
    }
    double r = 0.5 * (lo + hi);
    for (int it = 0; it < 3; ++it) {
        const double rn = r - PolyEval(c, deg, r) / PolyEval(dc, deg - 1, r);
        if (rn > lo && rn < hi) r = rn;
    }
    return r;
}
int RootsBetween(const double* c, const double* dc, int deg, const double* crit, int nc, double* roots) {
    if (deg == 1) {
        roots[0] = -c[0] / c[1];
        return 1;
    }
    double bound = 0.0;
    for (int i = 0; i < deg; ++i) bound = std::max(bound, std::fabs(c[i] / c[deg]));
    bound = 1.0 + bound;
    double edges[12];
    int ne = 0;
    edges[ne++] = -bound;
    for (int i = 0; i < nc; ++i)
        if (crit[i] > -bound && crit[i] < bound) edges[ne++] = crit[i];
    edges[ne++] = bound;
    int nr = 0;
    for (int i = 0; i + 1 < ne; ++i) {
        const double lo = edges[i], hi = edges[i + 1];
        const double flo = PolyEval(c, deg, lo), fhi = PolyEval(c, deg, hi);
        if (flo == 0.0) {
            if (nr == 0 || roots[nr - 1] != lo) roots[nr++] = lo;
            continue;
        }
        if (fhi == 0.0 || (flo < 0.0) == (fhi < 0.0)) continue;
        roots[nr++] = BracketRoot(c, dc, deg, lo, hi, flo);
    }
    if (PolyEval(c, deg, edges[ne - 1]) == 0.0 && (nr == 0 || roots[nr - 1] != edges[ne - 1])) roots[nr++] = edges[ne - 1];
    return nr;
}
int RealRoots(const double* cin, int deg, double* roots) {
    while (deg > 0 && cin[deg] == 0.0) --deg;
    if (deg == 0) return 0;
    double chain[5][5];
    for (int i = 0; i <= deg; ++i) chain[0][i] = cin[i];
    for (int j = 1; j < deg; ++j)
        for (int i = 1; i <= deg - j + 1; ++i) chain[j][i - 1] = chain[j - 1][i] * i;
    double crit[4], cur[4];
    int nc = 0;
    for (int j = deg - 1; j >= 0; --j) {
        nc = RootsBetween(chain[j], j + 1 < deg ? chain[j + 1] : nullptr, deg - j, crit, nc, cur);
        for (int i = 0; i < nc; ++i) crit[i] = cur[i];
    }
    for (int i = 0; i < nc; ++i) roots[i] = crit[i];
    return nc;
}

// ---- 3 x 3 helpers (row-major) ---------------------------------------------------------------------------------------
double Det3(const double* m) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
void Inv3(const double* m, double* r) {
    const double d = Det3(m);
    r[0] = (m[4] * m[8] - m[5] * m[7]) / d; r[1] = (m[2] * m[7] - m[1] * m[8]) / d; r[2] = (m[1] * m[5] - m[2] * m[4]) / d;
    r[3] = (m[5] * m[6] - m[3] * m[8]) / d; r[4] = (m[0] * m[8] - m[2] * m[6]) / d; r[5] = (m[2] * m[3] - m[0] * m[5]) / d;
    r[6] = (m[3] * m[7] - m[4] * m[6]) / d; r[7] = (m[1] * m[6] - m[0] * m[7]) / d; r[8] = (m[0] * m[4] - m[1] * m[3]) / d;
}
// A = U diag(S) V^T from Jacobi on A^T A (S descending), u_k = A v_k / s_k (e_k when s_k = 0), u_2 = u_0 x u_1
void Svd3(const double* A, double* U, double* S, double* V) {
    double ata[9], ev[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) ata[3 * i + j] = A[i] * A[j] + A[3 + i] * A[3 + j] + A[6 + i] * A[6 + j];
    Jacobi(3, ata, ev);
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (ata[4 * ord[j]] > ata[4 * ord[i]]) std::swap(ord[i], ord[j]);
    double vc[3][3], uc[3][3];
    for (int k = 0; k < 3; ++k) {
        const double lam = ata[4 * ord[k]];
        S[k] = std::sqrt(lam < 0.0 ? 0.0 : lam);
        for (int i = 0; i < 3; ++i) vc[k][i] = ev[3 * i + ord[k]];
    }
    for (int k = 0; k < 2; ++k) {
        if (S[k] == 0.0) {
            uc[k][0] = k == 0 ? 1.0 : 0.0; uc[k][1] = k == 1 ? 1.0 : 0.0; uc[k][2] = 0.0;
            continue;
        }
        const double inv = 1.0 / S[k];
        for (int i = 0; i < 3; ++i)
            uc[k][i] = (A[3 * i] * vc[k][0] + A[3 * i + 1] * vc[k][1] + A[3 * i + 2] * vc[k][2]) * inv;
    }
    uc[2][0] = uc[0][1] * uc[1][2] - uc[0][2] * uc[1][1];
    uc[2][1] = uc[0][2] * uc[1][0] - uc[0][0] * uc[1][2];
    uc[2][2] = uc[0][0] * uc[1][1] - uc[0][1] * uc[1][0];
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) { U[3 * i + k] = uc[k][i]; V[3 * i + k] = vc[k][i]; }
}
// proper rotation of the Procrustes problem: U diag(1, 1, sign(det U det V)) V^T (12.3, A4)
void Procrustes(const double* U, const double* V, double* R) {
    const double sgn = Det3(U) * Det3(V) < 0.0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1] + sgn * U[3 * r + 2] * V[3 * c + 2];
}

// ---- cameras: Camera::CamFromImg (host libm for the fisheye family and FOV), CamFromImgThreshold -----------------------
int NumFocal(int m) { return (m == 0 || m == 2 || m == 3 || m == 8 || m == 9) ? 1 : 2; }
int NumParams(int m) {
    static const int np[11] = {3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12};
    return np[m];
}
void Distortion(int model, const double* e, double u, double v, double* du, double* dv) {
    const double u2 = u * u, uv = u * v, v2 = v * v, r2 = u2 + v2;
    switch (model) {
        case 2: { const double rad = e[0] * r2; *du = u * rad; *dv = v * rad; return; }
        case 3: { const double rad = e[0] * r2 + e[1] * r2 * r2; *du = u * rad; *dv = v * rad; return; }
        case 4: {
            const double rad = e[0] * r2 + e[1] * r2 * r2;
            *du = u * rad + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2);
            *dv = v * rad + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2);
            return;
        }
        case 6: {
            const double r4 = r2 * r2, r6 = r4 * r2;
            const double rad = (1.0 + e[0] * r2 + e[1] * r4 + e[4] * r6) / (1.0 + e[5] * r2 + e[6] * r4 + e[7] * r6);
            *du = u * rad + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2) - u;
            *dv = v * rad + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2) - v;
            return;
        }
        case 10: {
            const double r4 = r2 * r2, r6 = r4 * r2, r8 = r6 * r2;
            const double rad = e[0] * r2 + e[1] * r4 + e[4] * r6 + e[5] * r8;
            *du = u * rad + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2) + e[6] * r2;
            *dv = v * rad + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2) + e[7] * r2;
            return;
        }
        case 5: case 8: case 9: {
            const double r = std::sqrt(u * u + v * v);
            if (!(r > kEps)) { *du = 0.0; *dv = 0.0; return; }
            const double th = std::atan(r), t2 = th * th;
            double thd;
            if (model == 8) thd = th * (1.0 + e[0] * t2);
            else if (model == 9) thd = th * (1.0 + e[0] * t2 + e[1] * (t2 * t2));
            else {
                const double t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
                thd = th * (1.0 + e[0] * t2 + e[1] * t4 + e[2] * t6 + e[3] * t8);
            }
            *du = u * thd / r - u;
            *dv = v * thd / r - v;
            return;
        }
    }
    *du = 0.0;
    *dv = 0.0;
}
void CamFromImg(int model, const double* p, double x, double y, double* uo, double* vo) {
    const int nf = NumFocal(model);
    double u = (x - p[nf]) / p[0], v = (y - p[nf + 1]) / p[nf - 1];
    const double* e = p + nf + 2;
    if (model <= 1) { *uo = u; *vo = v; return; }
    if (model == 7) {
        const double om = e[0], r2 = u * u + v * v, om2 = om * om;
        double f;
        if (om2 < 1e-4) f = (om2 * r2) / 3.0 - om2 / 12.0 + 1.0;
        else if (r2 < 1e-4) f = (om * (om * om * r2 + 3.0)) / (6.0 * std::tan(om / 2.0));
        else { const double r = std::sqrt(r2); f = std::tan(r * om) / (r * 2.0 * std::tan(om / 2.0)); }
        *uo = u * f; *vo = v * f;
        return;
    }
    const double x0 = u, y0 = v;
    for (int it = 0; it < 100; ++it) {  // IterativeUndistortion
        const double s0 = std::max(kEps, std::fabs(1e-6 * u)), s1 = std::max(kEps, std::fabs(1e-6 * v));
        double d[2], b0[2], f0[2], b1[2], f1[2];
        Distortion(model, e, u, v, &d[0], &d[1]);
        Distortion(model, e, u - s0, v, &b0[0], &b0[1]);
        Distortion(model, e, u + s0, v, &f0[0], &f0[1]);
        Distortion(model, e, u, v - s1, &b1[0], &b1[1]);
        Distortion(model, e, u, v + s1, &f1[0], &f1[1]);
        const double J00 = 1.0 + (f0[0] - b0[0]) / (2.0 * s0), J01 = (f1[0] - b1[0]) / (2.0 * s1);
        const double J10 = (f0[1] - b0[1]) / (2.0 * s0), J11 = 1.0 + (f1[1] - b1[1]) / (2.0 * s1);
        const double id = 1.0 / (J00 * J11 - J10 * J01);
        const double r0 = u + d[0] - x0, r1 = v + d[1] - y0;
        const double st0 = (J11 * id) * r0 + (-J01 * id) * r1, st1 = (-J10 * id) * r0 + (J00 * id) * r1;
        u -= st0;
        v -= st1;
        if (st0 * st0 + st1 * st1 < 1e-10) break;
    }
    if (model == 10) {
        const double th = std::sqrt(u * u + v * v);
        double sn, cs;
        ::sincos(th, &sn, &cs);
        if (th * cs > kEps) {
            const double sc = sn / (th * cs);
            u *= sc;
            v *= sc;
        }
    }
    *uo = u;
    *vo = v;
}

// ---- 12.7: forward-mode derivatives w.r.t. (qx, qy, qz, qw, tx, ty, tz) ---------------------------------------------
struct D {
    double a, g[7];
};
D Cst(double a) { D r{a, {0, 0, 0, 0, 0, 0, 0}}; return r; }
D operator+(const D& x, const D& y) { D r{x.a + y.a, {}}; for (int i = 0; i < 7; ++i) r.g[i] = x.g[i] + y.g[i]; return r; }
D operator-(const D& x, const D& y) { D r{x.a - y.a, {}}; for (int i = 0; i < 7; ++i) r.g[i] = x.g[i] - y.g[i]; return r; }
D operator*(const D& x, const D& y) {
    D r{x.a * y.a, {}};
    for (int i = 0; i < 7; ++i) r.g[i] = x.a * y.g[i] + x.g[i] * y.a;
    return r;
}
D operator/(const D& x, const D& y) {
    D r{x.a / y.a, {}};
    for (int i = 0; i < 7; ++i) r.g[i] = (x.g[i] - r.a * y.g[i]) / y.a;
    return r;
}
D operator+(const D& x, double c) { D r = x; r.a = x.a + c; return r; }
D operator+(double c, const D& x) { return x + c; }
D operator-(const D& x, double c) { D r = x; r.a = x.a - c; return r; }
D operator*(const D& x, double c) { D r{x.a * c, {}}; for (int i = 0; i < 7; ++i) r.g[i] = x.g[i] * c; return r; }
D operator*(double c, const D& x) { return x * c; }
D operator/(const D& x, double c) { D r{x.a / c, {}}; for (int i = 0; i < 7; ++i) r.g[i] = x.g[i] / c; return r; }
D Sqrt(const D& x) {
    D r{std::sqrt(x.a), {}};
    for (int i = 0; i < 7; ++i) r.g[i] = x.g[i] / (2.0 * r.a);
    return r;
}
D AtanD(const D& x) {
    D r{Atan(x.a), {}};
    for (int i = 0; i < 7; ++i) r.g[i] = x.g[i] / (1.0 + x.a * x.a);
    return r;
}

// Camera::ImgFromCam of the camera-frame point (pu, pv, pw)
void ImgFromCam(int model, const double* p, const D& pu, const D& pv, const D& pw, D* x, D* y) {
    D u = pu / pw, v = pv / pw;
    const int nf = NumFocal(model);
    const double f1 = p[0], f2 = p[nf - 1], c1 = p[nf], c2 = p[nf + 1];
    const double* e = p + nf + 2;
    if (model <= 1) {
        *x = f1 * u + c1;
        *y = f2 * v + c2;
        return;
    }
    if (model == 7) {
        const double om = e[0], om2 = om * om;
        const D r2 = u * u + v * v;
        D f;
        if (om2 < 1e-4) {
            f = (om2 * r2) / 3.0 - om2 / 12.0 + 1.0;
        } else {
            const double th = Sin(om / 2.0) / Cos(om / 2.0);
            if (r2.a < 1e-4) {
                f = (-2.0 * th * (4.0 * r2 * th * th - 3.0)) / (3.0 * om);
            } else {
                const D r = Sqrt(r2);
                f = AtanD(r * 2.0 * th) / (r * om);
            }
        }
        *x = f1 * (u * f) + c1;
        *y = f2 * (v * f) + c2;
        return;
    }
    if (model == 10) {
        const D r = Sqrt(u * u + v * v);
        if (r.a > kEps) {
            const D th = AtanD(r);
            u = th * u / r;
            v = th * v / r;
        }
    }
    D du, dv;
    if (model == 5 || model == 8 || model == 9) {
        const D r = Sqrt(u * u + v * v);
        if (r.a > kEps) {
            const D th = AtanD(r), t2 = th * th;
            D thd;
            if (model == 8) {
                thd = th * (1.0 + e[0] * t2);
            } else if (model == 9) {
                const D t4 = t2 * t2;
                thd = th * (1.0 + e[0] * t2 + e[1] * t4);
            } else {
                const D t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
                thd = th * (1.0 + e[0] * t2 + e[1] * t4 + e[2] * t6 + e[3] * t8);
            }
            du = u * thd / r - u;
            dv = v * thd / r - v;
        } else {
            du = u * 0.0;
            dv = v * 0.0;
        }
    } else if (model == 2 || model == 3) {
        const D r2 = u * u + v * v;
        const D rad = model == 2 ? e[0] * r2 : e[0] * r2 + e[1] * r2 * r2;
        du = u * rad;
        dv = v * rad;
    } else {  // 4, 6, 10
        const D u2 = u * u, uv = u * v, v2 = v * v, r2 = u2 + v2;
        if (model == 4) {
            const D rad = e[0] * r2 + e[1] * r2 * r2;
            du = u * rad + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2);
            dv = v * rad + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2);
        } else if (model == 6) {
            const D r4 = r2 * r2, r6 = r4 * r2;
            const D rad = (1.0 + e[0] * r2 + e[1] * r4 + e[4] * r6) / (1.0 + e[5] * r2 + e[6] * r4 + e[7] * r6);
            du = u * rad + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2) - u;
            dv = v * rad + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2) - v;
        } else {
            const D r4 = r2 * r2, r6 = r4 * r2, r8 = r6 * r2;
            const D rad = e[0] * r2 + e[1] * r4 + e[4] * r6 + e[5] * r8;
            du = u * rad + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2) + e[6] * r2;
            dv = v * rad + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2) + e[7] * r2;
        }
    }
    *x = f1 * (u + du) + c1;
    *y = f2 * (v + dv) + c2;
}

// ---- 12.5 / 12.3 / 12.4 ----------------------------------------------------------------------------------------------
struct Corr {
    size_t n;
    const double* uv;  // normalized
    const double* X;
};
typedef std::array<double, 12> Model;  // [R | t] row-major

double SqReproj(const Model& P, const double* X, double u, double v) {
    const double z = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
    if (!(z > kEps)) return DBL_MAX;
    const double x = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
    const double y = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
    const double du = x / z - u, dv = y / z - v;
    return du * du + dv * dv;
}

void PolyMul(const double* a, int na, const double* b, int nb, double* r) {
    for (int i = 0; i < na + nb - 1; ++i) r[i] = 0.0;
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j) r[i + j] = r[i + j] + a[i] * b[j];
}

std::vector<Model> P3P(const double* uv, const double* X) {
    std::vector<Model> out;
    double b[3][3];
    for (int i = 0; i < 3; ++i) {
        const double nn = std::sqrt(uv[2 * i] * uv[2 * i] + uv[2 * i + 1] * uv[2 * i + 1] + 1.0);
        b[i][0] = uv[2 * i] / nn;
        b[i][1] = uv[2 * i + 1] / nn;
        b[i][2] = 1.0 / nn;
    }
    auto dot = [&](int i, int j) { return b[i][0] * b[j][0] + b[i][1] * b[j][1] + b[i][2] * b[j][2]; };
    auto d2 = [&](int i, int j) {
        const double* A = X + 3 * i;
        const double* B = X + 3 * j;
        return (A[0] - B[0]) * (A[0] - B[0]) + (A[1] - B[1]) * (A[1] - B[1]) + (A[2] - B[2]) * (A[2] - B[2]);
    };
    const double cuv = dot(0, 1), cuw = dot(0, 2), cvw = dot(1, 2);
    const double AB2 = d2(0, 1), AC2 = d2(0, 2), BC2 = d2(1, 2);
    if (!(AB2 > 0.0) || !std::isfinite(AB2)) return out;
    const double AB = std::sqrt(AB2), a = BC2 / AB2, bb = AC2 / AB2;
    const double p = 2.0 * cvw, q = 2.0 * cuw, r = 2.0 * cuv;
    const double A1 = 1.0 - a, A2 = -bb;
    const double B1[2] = {-p, a * r}, B2[2] = {0.0, bb * r}, C1[3] = {1.0, 0.0, -a}, C2[3] = {1.0, -q, 1.0 - bb};
    double E[3], F[2], G[4], t1[4], t2[4], EE[5], FG[5], c[5];
    for (int i = 0; i < 3; ++i) E[i] = A1 * C2[i] - A2 * C1[i];
    for (int i = 0; i < 2; ++i) F[i] = A1 * B2[i] - A2 * B1[i];
    PolyMul(B1, 2, C2, 3, t1);
    PolyMul(B2, 2, C1, 3, t2);
    for (int i = 0; i < 4; ++i) G[i] = t1[i] - t2[i];
    PolyMul(E, 3, E, 3, EE);
    PolyMul(F, 2, G, 4, FG);
    for (int i = 0; i < 5; ++i) {
        c[i] = EE[i] - FG[i];
        if (!std::isfinite(c[i])) return out;
    }
    double roots[4];
    const int nr = RealRoots(c, 4, roots);
    for (int k = 0; k < nr; ++k) {
        const double x = roots[k];
        if (x < 0.0) continue;
        const double b1 = -(F[0] + F[1] * x);
        if (b1 == 0.0) continue;
        const double y = (E[0] + x * (E[1] + x * E[2])) / b1;
        const double nu = x * x + y * y - 2.0 * x * y * cuv;
        if (!(nu > 0.0)) continue;
        const double PC = AB / std::sqrt(nu), PB = y * PC, PA = x * PC;
        const double dist[3] = {PA, PB, PC};
        double cam[3][3], ms[3], md[3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) cam[i][j] = b[i][j] * dist[i];
        for (int j = 0; j < 3; ++j) {
            ms[j] = (X[j] + X[3 + j] + X[6 + j]) / 3.0;
            md[j] = (cam[0][j] + cam[1][j] + cam[2][j]) / 3.0;
        }
        double S[9], U[9], Sv[3], V[9], R[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double s = 0.0;
                for (int k2 = 0; k2 < 3; ++k2) s = s + (cam[k2][i] - md[i]) * (X[3 * k2 + j] - ms[j]);
                S[3 * i + j] = s / 3.0;
            }
        Svd3(S, U, Sv, V);
        Procrustes(U, V, R);
        Model P;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) P[4 * i + j] = R[3 * i + j];
            P[4 * i + 3] = md[i] - (R[3 * i] * ms[0] + R[3 * i + 1] * ms[1] + R[3 * i + 2] * ms[2]);
        }
        out.push_back(P);
    }
    return out;
}

template <int N>
bool Gauss(double* A, double* b) {  // partial pivoting (first largest |pivot|)
    for (int k = 0; k < N; ++k) {
        int piv = k;
        double best = std::fabs(A[k * N + k]);
        for (int i = k + 1; i < N; ++i)
            if (std::fabs(A[i * N + k]) > best) { best = std::fabs(A[i * N + k]); piv = i; }
        if (!(best > 0.0) || !std::isfinite(best)) return false;
        if (piv != k) {
            for (int j = 0; j < N; ++j) std::swap(A[k * N + j], A[piv * N + j]);
            std::swap(b[k], b[piv]);
        }
        for (int i = k + 1; i < N; ++i) {
            const double f = A[i * N + k] / A[k * N + k];
            for (int j = k; j < N; ++j) A[i * N + j] = A[i * N + j] - f * A[k * N + j];
            b[i] = b[i] - f * b[k];
        }
    }
    for (int i = N - 1; i >= 0; --i) {
        double s = b[i];
        for (int j = i + 1; j < N; ++j) s = s - A[i * N + j] * b[j];
        b[i] = s / A[i * N + i];
    }
    return true;
}
template <int N>
void LeastSquares6(const double (*A)[N], const double* y, double* x) {  // normal equations
    double M[N * N];
    for (int i = 0; i < N; ++i) {
        for (int j = 0; j < N; ++j) {
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s = s + A[k][i] * A[k][j];
            M[i * N + j] = s;
        }
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s = s + A[k][i] * y[k];
        x[i] = s;
    }
    if (!Gauss<N>(M, x))
        for (int i = 0; i < N; ++i) x[i] = std::numeric_limits<double>::quiet_NaN();
}

bool EPnP(const Corr& c, const std::vector<char>& set, Model* out) {
    const std::vector<double> s4 = Sum64<4>(c.n, [&](size_t k, double* o) {
        if (!set[k]) return;
        o[0] = o[0] + 1.0;
        for (int i = 0; i < 3; ++i) o[1 + i] = o[1 + i] + c.X[3 * k + i];
    });
    const double n = s4[0];
    if (!(n >= 4.0)) return false;
    const double pw0[3] = {s4[1] / n, s4[2] / n, s4[3] / n};
    size_t first = 0;
    while (!set[first]) ++first;
    const std::vector<double> s6 = Sum64<6>(c.n, [&](size_t k, double* o) {
        if (!set[k]) return;
        const double d0 = c.X[3 * k] - pw0[0], d1 = c.X[3 * k + 1] - pw0[1], d2 = c.X[3 * k + 2] - pw0[2];
        o[0] = o[0] + d0 * d0; o[1] = o[1] + d0 * d1; o[2] = o[2] + d0 * d2;
        o[3] = o[3] + d1 * d1; o[4] = o[4] + d1 * d2; o[5] = o[5] + d2 * d2;
    });
    const double Cm[9] = {s6[0], s6[1], s6[2], s6[1], s6[3], s6[4], s6[2], s6[4], s6[5]};
    double U[9], Sv[3], V[9], cw[4][3], CC[9], Ci[9];
    Svd3(Cm, U, Sv, V);
    for (int j = 0; j < 3; ++j) cw[0][j] = pw0[j];
    for (int i = 0; i < 3; ++i) {
        const double k = std::sqrt(Sv[i] / n);
        for (int j = 0; j < 3; ++j) cw[i + 1][j] = cw[0][j] + k * U[3 * j + i];
    }
    for (int r = 0; r < 3; ++r)
        for (int i = 0; i < 3; ++i) CC[3 * r + i] = cw[i + 1][r] - cw[0][r];
    const double det = Det3(CC);
    if (det == 0.0 || !std::isfinite(det)) return false;
    Inv3(CC, Ci);
    auto alphas = [&](size_t k, double* al) {
        const double d0 = c.X[3 * k] - cw[0][0], d1 = c.X[3 * k + 1] - cw[0][1], d2 = c.X[3 * k + 2] - cw[0][2];
        for (int i = 0; i < 3; ++i) al[1 + i] = Ci[3 * i] * d0 + Ci[3 * i + 1] * d1 + Ci[3 * i + 2] * d2;
        al[0] = 1.0 - al[1] - al[2] - al[3];
    };
    const std::vector<double> mtm = Sum64<78>(c.n, [&](size_t k, double* o) {
        if (!set[k]) return;
        double al[4], m1[12], m2[12];
        alphas(k, al);
        for (int j = 0; j < 4; ++j) {
            m1[3 * j] = al[j]; m1[3 * j + 1] = 0.0; m1[3 * j + 2] = -al[j] * c.uv[2 * k];
            m2[3 * j] = 0.0; m2[3 * j + 1] = al[j]; m2[3 * j + 2] = -al[j] * c.uv[2 * k + 1];
        }
        int t = 0;
        for (int i = 0; i < 12; ++i)
            for (int j = i; j < 12; ++j, ++t) o[t] = o[t] + (m1[i] * m1[j] + m2[i] * m2[j]);
    });
    double A[144], W[144];
    for (int i = 0, t = 0; i < 12; ++i)
        for (int j = i; j < 12; ++j, ++t) A[12 * i + j] = A[12 * j + i] = mtm[t];
    Jacobi(12, A, W);
    int idx[12];
    for (int i = 0; i < 12; ++i) idx[i] = i;
    std::stable_sort(idx, idx + 12, [&](int x, int y) { return A[13 * x] < A[13 * y]; });
    double nv[4][12];
    for (int s = 0; s < 4; ++s)
        for (int r = 0; r < 12; ++r) nv[s][r] = W[12 * r + idx[s]];
    static const int ea[6] = {0, 0, 0, 1, 1, 2}, eb[6] = {1, 2, 3, 2, 3, 3};
    double L[6][10], rho[6];
    for (int j = 0; j < 6; ++j) {
        double dv[4][3];
        for (int i = 0; i < 4; ++i)
            for (int k = 0; k < 3; ++k) dv[i][k] = nv[i][3 * ea[j] + k] - nv[i][3 * eb[j] + k];
        auto dt = [&](int x, int y) { return dv[x][0] * dv[y][0] + dv[x][1] * dv[y][1] + dv[x][2] * dv[y][2]; };
        const double row[10] = {dt(0, 0), 2.0 * dt(0, 1), dt(1, 1), 2.0 * dt(0, 2), 2.0 * dt(1, 2),
                                dt(2, 2), 2.0 * dt(0, 3), 2.0 * dt(1, 3), 2.0 * dt(2, 3), dt(3, 3)};
        for (int i = 0; i < 10; ++i) L[j][i] = row[i];
        const double* pa = cw[ea[j]];
        const double* pb = cw[eb[j]];
        rho[j] = (pa[0] - pb[0]) * (pa[0] - pb[0]) + (pa[1] - pb[1]) * (pa[1] - pb[1]) + (pa[2] - pb[2]) * (pa[2] - pb[2]);
    }
    double betas[3][4];
    {
        double A4[6][4], x[4];
        for (int j = 0; j < 6; ++j) { A4[j][0] = L[j][0]; A4[j][1] = L[j][1]; A4[j][2] = L[j][3]; A4[j][3] = L[j][6]; }
        LeastSquares6<4>(A4, rho, x);
        const double sg = x[0] < 0.0 ? -1.0 : 1.0, s = std::sqrt(sg * x[0]);
        betas[0][0] = s;
        for (int i = 1; i < 4; ++i) betas[0][i] = (sg < 0.0 ? -x[i] : x[i]) / s;
    }
    for (int v = 1; v < 3; ++v) {  // FindBetasApprox2 (columns 0 1 2) and 3 (0 .. 4)
        double A5[6][5], x[5];
        const int nc = v == 1 ? 3 : 5;
        for (int j = 0; j < 6; ++j)
            for (int i = 0; i < 5; ++i) A5[j][i] = L[j][i];
        if (nc == 3) {
            double A3[6][3];
            for (int j = 0; j < 6; ++j)
                for (int i = 0; i < 3; ++i) A3[j][i] = L[j][i];
            LeastSquares6<3>(A3, rho, x);
        } else {
            LeastSquares6<5>(A5, rho, x);
        }
        double b0, b1;
        if (x[0] < 0.0) { b0 = std::sqrt(-x[0]); b1 = x[2] < 0.0 ? std::sqrt(-x[2]) : 0.0; }
        else { b0 = std::sqrt(x[0]); b1 = x[2] > 0.0 ? std::sqrt(x[2]) : 0.0; }
        if (x[1] < 0.0) b0 = -b0;
        betas[v][0] = b0; betas[v][1] = b1; betas[v][2] = nc == 5 ? x[3] / b0 : 0.0; betas[v][3] = 0.0;
    }
    Model Ps[3];
    double err[3];
    for (int s = 0; s < 3; ++s) {
        double* bt = betas[s];
        for (int it = 0; it < 5; ++it) {  // Gauss-Newton
            double J[6][4], y[6], dx[4];
            for (int j = 0; j < 6; ++j) {
                const double* l = L[j];
                J[j][0] = 2.0 * l[0] * bt[0] + l[1] * bt[1] + l[3] * bt[2] + l[6] * bt[3];
                J[j][1] = l[1] * bt[0] + 2.0 * l[2] * bt[1] + l[4] * bt[2] + l[7] * bt[3];
                J[j][2] = l[3] * bt[0] + l[4] * bt[1] + 2.0 * l[5] * bt[2] + l[8] * bt[3];
                J[j][3] = l[6] * bt[0] + l[7] * bt[1] + l[8] * bt[2] + 2.0 * l[9] * bt[3];
                y[j] = rho[j] - (l[0] * bt[0] * bt[0] + l[1] * bt[0] * bt[1] + l[2] * bt[1] * bt[1] +
                                 l[3] * bt[0] * bt[2] + l[4] * bt[1] * bt[2] + l[5] * bt[2] * bt[2] +
                                 l[6] * bt[0] * bt[3] + l[7] * bt[1] * bt[3] + l[8] * bt[2] * bt[3] + l[9] * bt[3] * bt[3]);
            }
            LeastSquares6<4>(J, y, dx);
            for (int i = 0; i < 4; ++i) bt[i] = bt[i] + dx[i];
        }
        double cc[4][3];
        for (int j = 0; j < 4; ++j)
            for (int k = 0; k < 3; ++k) {
                double v = 0.0;
                for (int i = 0; i < 4; ++i) v = v + bt[i] * nv[i][3 * j + k];
                cc[j][k] = v;
            }
        auto pc_of = [&](size_t k, double* pc) {
            double al[4];
            alphas(k, al);
            for (int i = 0; i < 3; ++i) pc[i] = al[0] * cc[0][i] + al[1] * cc[1][i] + al[2] * cc[2][i] + al[3] * cc[3][i];
        };
        double pf[3];
        pc_of(first, pf);
        if (pf[2] < 0.0)
            for (int j = 0; j < 4; ++j)
                for (int k = 0; k < 3; ++k) cc[j][k] = -cc[j][k];
        const std::vector<double> s3 = Sum64<3>(c.n, [&](size_t k, double* o) {
            if (!set[k]) return;
            double pc[3];
            pc_of(k, pc);
            for (int i = 0; i < 3; ++i) o[i] = o[i] + pc[i];
        });
        const double pc0[3] = {s3[0] / n, s3[1] / n, s3[2] / n};
        const std::vector<double> abt = Sum64<9>(c.n, [&](size_t k, double* o) {
            if (!set[k]) return;
            double pc[3];
            pc_of(k, pc);
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) o[3 * i + j] = o[3 * i + j] + (pc[i] - pc0[i]) * (c.X[3 * k + j] - pw0[j]);
        });
        double Ua[9], Sa[3], Va[9], R[9];
        Svd3(abt.data(), Ua, Sa, Va);
        Procrustes(Ua, Va, R);
        Model& P = Ps[s];
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) P[4 * i + j] = R[3 * i + j];
            P[4 * i + 3] = pc0[i] - (R[3 * i] * pw0[0] + R[3 * i + 1] * pw0[1] + R[3 * i + 2] * pw0[2]);
        }
        const std::vector<double> e1 = Sum64<1>(c.n, [&](size_t k, double* o) {
            if (!set[k]) return;
            const double* X = c.X + 3 * k;
            const double xc = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
            const double yc = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
            const double zc = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
            const double du = c.uv[2 * k] - xc / zc, dv = c.uv[2 * k + 1] - yc / zc;
            o[0] = o[0] + std::sqrt(du * du + dv * dv);
        });
        err[s] = e1[0] / n;
    }
    int best = 0;
    if (err[1] < err[0]) best = 1;
    if (err[2] < err[best]) best = 2;
    *out = Ps[best];
    return true;
}

// ---- 12.6: LORANSAC<P3PEstimator, EPNPEstimator> ---------------------------------------------------------------------
struct Support {
    size_t cnt = 0;
    double sum = DBL_MAX;
};
bool Better(const Support& a, const Support& b) { return a.cnt > b.cnt || (a.cnt == b.cnt && a.sum < b.sum); }
Support Score(const Corr& c, const Model& P, double maxr, std::vector<char>* mask) {
    const std::vector<double> s = Sum64<2>(c.n, [&](size_t k, double* o) {
        const double r = SqReproj(P, c.X + 3 * k, c.uv[2 * k], c.uv[2 * k + 1]);
        if (r <= maxr) {
            o[0] = o[0] + 1.0;
            o[1] = o[1] + r;
        }
        if (mask) (*mask)[k] = r <= maxr;
    });
    Support sp;
    sp.cnt = static_cast<size_t>(s[0]);
    sp.sum = s[1];
    return sp;
}
uint64_t NumTrials(uint64_t inl, uint64_t n, double conf, double mult) {  // ComputeNumTrials, kMinNumSamples = 3
    const double ratio = inl / static_cast<double>(n), nom = 1 - conf;
    if (nom <= 0) return ~0ull;
    const double denom = 1 - std::pow(ratio, 3);
    if (denom <= 0) return 1;
    if (denom == 1.0) return ~0ull;
    return static_cast<uint64_t>(std::ceil(std::log(nom) / std::log(denom) * mult));
}
struct Ransac {
    bool success = false;
    size_t inliers = 0;
    uint64_t trials = 0;
    Model model{};
    std::vector<char> mask;
};
struct RansacOpts {
    double maxr, conf, mult;
    uint64_t min_trials, max_trials;
};
Ransac LoRansac(const Corr& c, const RansacOpts& o) {
    Ransac rep;
    rep.mask.assign(c.n, 0);
    if (c.n < 3) return rep;
    std::mt19937 gen(0);  // a fresh generator per RANSAC (12.2)
    std::vector<uint32_t> perm(c.n);
    for (size_t i = 0; i < c.n; ++i) perm[i] = static_cast<uint32_t>(i);
    Support best;
    Model best_model{};
    uint64_t dyn = o.max_trials;
    bool abort = false;
    std::vector<char> inl(c.n);
    uint64_t t;
    for (t = 0; t < o.max_trials; ++t) {
        if (abort) {
            t += 1;
            break;
        }
        double uv3[6], X3[9];
        for (uint32_t i = 0; i < 3; ++i) {
            std::uniform_int_distribution<uint32_t> d(i, static_cast<uint32_t>(c.n - 1));
            std::swap(perm[i], perm[d(gen)]);
        }
        for (int i = 0; i < 3; ++i) {
            uv3[2 * i] = c.uv[2 * perm[i]];
            uv3[2 * i + 1] = c.uv[2 * perm[i] + 1];
            for (int k = 0; k < 3; ++k) X3[3 * i + k] = c.X[3 * perm[i] + k];
        }
        for (const Model& m : P3P(uv3, X3)) {
            const Support s = Score(c, m, o.maxr, nullptr);
            if (Better(s, best)) {
                best = s;
                best_model = m;
                if (s.cnt > 3 && s.cnt >= 4) {
                    for (int lt = 0; lt < 10; ++lt) {
                        const size_t prev = best.cnt;
                        Score(c, best_model, o.maxr, &inl);
                        Model L;
                        if (EPnP(c, inl, &L)) {
                            const Support ls = Score(c, L, o.maxr, nullptr);
                            if (Better(ls, best)) {
                                best = ls;
                                best_model = L;
                            }
                        }
                        if (best.cnt <= prev) break;
                    }
                }
                dyn = o.max_trials > o.min_trials ? NumTrials(best.cnt, c.n, o.conf, o.mult) : o.max_trials;
            }
            if (t >= dyn && t >= o.min_trials) {
                abort = true;
                break;
            }
        }
    }
    rep.trials = t;
    rep.inliers = best.cnt;
    if (best.cnt < 3) return rep;
    rep.success = true;
    rep.model = best_model;
    Score(c, best_model, o.maxr, &rep.mask);
    return rep;
}

// ---- 12.7 / 12.8: RefineAbsolutePose -----------------------------------------------------------------------------------
void QuatPlus(const double* q, const double* d, double* o) {  // EigenQuaternionManifold::Plus
    const double nd = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (nd == 0.0) { std::memcpy(o, q, 4 * sizeof(double)); return; }
    const double s = Sin(nd) / nd;
    const double x = s * d[0], y = s * d[1], z = s * d[2], w = Cos(nd);
    o[3] = w * q[3] - x * q[0] - y * q[1] - z * q[2];
    o[0] = w * q[0] + x * q[3] + y * q[2] - z * q[1];
    o[1] = w * q[1] - x * q[2] + y * q[3] + z * q[0];
    o[2] = w * q[2] + x * q[1] - y * q[0] + z * q[3];
}
// the camera-frame point q * P + t with its derivatives by (qx, qy, qz, qw, tx, ty, tz)
void PosePoint(const double* q, const double* t, const double* P, D* pc) {
    D qv[4], tv[3];
    for (int i = 0; i < 4; ++i) { qv[i] = Cst(q[i]); qv[i].g[i] = 1.0; }
    for (int i = 0; i < 3; ++i) { tv[i] = Cst(t[i]); tv[i].g[4 + i] = 1.0; }
    D w0 = qv[1] * P[2] - qv[2] * P[1], w1 = qv[2] * P[0] - qv[0] * P[2], w2 = qv[0] * P[1] - qv[1] * P[0];
    w0 = w0 + w0;
    w1 = w1 + w1;
    w2 = w2 + w2;
    pc[0] = (P[0] + qv[3] * w0) + (qv[1] * w2 - qv[2] * w1) + tv[0];
    pc[1] = (P[1] + qv[3] * w1) + (qv[2] * w0 - qv[0] * w2) + tv[1];
    pc[2] = (P[2] + qv[3] * w2) + (qv[0] * w1 - qv[1] * w0) + tv[2];
}
struct RefOpts {
    int model;
    const double* params;
    double gtol, scale;
    int64_t iters;
    bool cov;
};
struct Eval {
    double cost, H[6][6], g[6];
};
Eval Evaluate(const RefOpts& o, const double* q, const double* t, const double* xy, const double* X,
              const std::vector<char>& mask, bool jac) {
    const double b = o.scale * o.scale, c = 1.0 / b;
    const double Jm[4][3] = {{q[3], q[2], -q[1]}, {-q[2], q[3], q[0]}, {q[1], -q[0], q[3]}, {-q[0], -q[1], -q[2]}};
    const std::vector<double> s = Sum64<28>(mask.size(), [&](size_t k, double* acc) {
        if (!mask[k]) return;
        D pc[3];
        PosePoint(q, t, X + 3 * k, pc);
        D rx, ry;
        ImgFromCam(o.model, o.params, pc[0], pc[1], pc[2], &rx, &ry);
        rx = rx - xy[2 * k];
        ry = ry - xy[2 * k + 1];
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
double GradNorm(const double* q, const double* t, const double* g) {
    const double mg[3] = {-g[0], -g[1], -g[2]};
    double qp[4], m = 0.0;
    QuatPlus(q, mg, qp);
    for (int i = 0; i < 4; ++i) m = std::max(m, std::fabs(q[i] - qp[i]));
    for (int i = 0; i < 3; ++i) m = std::max(m, std::fabs(t[i] - (t[i] + (-g[3 + i]))));
    return m;
}
// What a refinement did, for the tests alone (the product exports none of it): recorded, never read back.
enum Exit : int32_t {
    GRADIENT_AT_START, GRADIENT_AFTER_STEP, MAX_ITERATIONS, PARAMETER_TOLERANCE, FUNCTION_TOLERANCE, INVALID_STEPS,
    MIN_RADIUS, NOT_FINITE_START, NOTHING_TO_REFINE
};
struct Trace {
    int32_t iterations = 0;  // trips of the loop begun
    int32_t accepted = 0;    // steps taken
    int32_t rejected = 0;    // steps evaluated and not taken
    int32_t invalid = 0;     // steps without a positive model cost change
    int32_t exit = MAX_ITERATIONS;
    int32_t rank_failed = 0;  // the covariance's rank test
};
// returns usable; q, t updated in place; cov (36) when asked; tr filled when given
bool Refine(const RefOpts& o, double* q, double* t, const double* xy, const double* X, const std::vector<char>& mask,
            double* cov, Trace* tr = nullptr) {
    Trace local;
    Trace& T = tr ? *tr : local;
    T = Trace();
    if (cov) std::fill(cov, cov + 36, 0.0);
    if (std::count(mask.begin(), mask.end(), 1) == 0) {  // A9
        T.exit = NOTHING_TO_REFINE;
        return true;
    }
    Eval ev = Evaluate(o, q, t, xy, X, mask, true);
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
            const double cand = Evaluate(o, qn, tn, xy, X, mask, false).cost;
            const double change = ev.cost - (std::isfinite(cand) ? cand : DBL_MAX);
            if (std::fabs(change) <= 1e-6 * ev.cost) {
                T.exit = FUNCTION_TOLERANCE;
                break;
            }
            const double rel = change / mcc;
            if (rel > 1e-3) {
                std::memcpy(q, qn, sizeof qn);
                std::memcpy(t, tn, sizeof tn);
                ev = Evaluate(o, q, t, xy, X, mask, true);
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

// Eigen::Quaterniond(R) as (x, y, z, w); false on a NaN in the pose
bool ModelToPose(const Model& P, double* q, double* t) {
    const double m[9] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]};
    double w[4];
    double tr = m[0] + m[4] + m[8];
    if (tr > 0.0) {
        tr = std::sqrt(tr + 1.0);
        w[0] = 0.5 * tr;
        tr = 0.5 / tr;
        w[1] = (m[7] - m[5]) * tr; w[2] = (m[2] - m[6]) * tr; w[3] = (m[3] - m[1]) * tr;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        tr = std::sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
        w[1 + i] = 0.5 * tr;
        tr = 0.5 / tr;
        w[0] = (m[3 * k + j] - m[3 * j + k]) * tr;
        w[1 + j] = (m[3 * j + i] + m[3 * i + j]) * tr;
        w[1 + k] = (m[3 * k + i] + m[3 * i + k]) * tr;
    }
    q[0] = w[1]; q[1] = w[2]; q[2] = w[3]; q[3] = w[0];
    t[0] = P[3]; t[1] = P[7]; t[2] = P[11];
    for (int i = 0; i < 4; ++i) if (std::isnan(q[i])) return false;
    for (int i = 0; i < 3; ++i) if (std::isnan(t[i])) return false;
    return true;
}

std::vector<double> FocalFactors(int estimate, int k, double lo, double hi) {
    std::vector<double> f;
    if (!estimate) return {1.0};
    for (double x = 0; x <= 1.0; x += 1.0 / k) f.push_back(lo + (hi - lo) * x * x);
    return f;
}

}  // namespace

extern "C" {

double abspose_ref_atan(double x) { return Atan(x); }
double abspose_ref_sin(double x) { return Sin(x); }
double abspose_ref_cos(double x) { return Cos(x); }
double abspose_ref_log(double x) { return Log(x); }

// one correspondence's projection as the refinement evaluates it (12.7): the pixel and its derivatives by
// (qx, qy, qz, qw, tx, ty, tz), row-major 2 x 7
void abspose_ref_project(int model, const double* params, const double* q, const double* t, const double* X, double* xy,
                         double* J) {
    D pc[3], x, y;
    PosePoint(q, t, X, pc);
    ImgFromCam(model, params, pc[0], pc[1], pc[2], &x, &y);
    xy[0] = x.a;
    xy[1] = y.a;
    for (int i = 0; i < 7; ++i) {
        J[i] = x.g[i];
        J[7 + i] = y.g[i];
    }
}

int abspose_ref_p3p(const double* uv, const double* X, double* out) {
    const std::vector<Model> m = P3P(uv, X);
    for (size_t i = 0; i < m.size(); ++i) std::memcpy(out + 12 * i, m[i].data(), 12 * sizeof(double));
    return static_cast<int>(m.size());
}

int abspose_ref_epnp(uint32_t n, const double* uv, const double* X, double* out) {
    Model P;
    if (!EPnP(Corr{n, uv, X}, std::vector<char>(n, 1), &P)) return 0;
    std::memcpy(out, P.data(), sizeof(double) * 12);
    return 1;
}

size_t abspose_ref_focal_factors(int estimate, int k, double lo, double hi, double* out, size_t cap) {
    const std::vector<double> f = FocalFactors(estimate, k, lo, hi);
    for (size_t i = 0; i < f.size() && i < cap; ++i) out[i] = f[i];
    return f.size();
}

// est: estimate_focal_length, num_focal_length_samples, min ratio, max ratio, max_error, min_inlier_ratio, confidence,
// dyn_num_trials_multiplier, min_num_trials, max_num_trials; ref: gradient_tolerance, max_num_iterations,
// loss_function_scale (all as doubles)
int abspose_ref_estimate(const uint64_t* off, size_t nq, const int32_t* models, const double* cparams, const double* p2,
                         const double* p3, const double* est, const double* ref, int want_cov, uint8_t* success,
                         double* qvec, double* tvec, uint32_t* num_inliers, uint64_t* num_trials, double* focal,
                         double* covariance, uint8_t* mask) {
    const std::vector<double> factors = FocalFactors(est[0] != 0.0, static_cast<int>(est[1]), est[2], est[3]);
    const uint64_t min_t = static_cast<uint64_t>(est[8]);
    const uint64_t max_t = std::min(static_cast<uint64_t>(est[9]),
                                    NumTrials(static_cast<uint64_t>(est[5] * 100000), 100000, est[6], est[7]));
    for (size_t qi = 0; qi < nq; ++qi) {
        const size_t c0 = off[qi], n = off[qi + 1] - off[qi];
        const int model = models[qi];
        const int nf = NumFocal(model);
        double* cv = covariance ? covariance + 36 * qi : nullptr;
        if (cv) std::fill(cv, cv + 36, 0.0);
        int best = -1;
        Ransac chosen;
        uint64_t first_trials = 0;
        double best_prm[12] = {};
        for (size_t f = 0; f < factors.size(); ++f) {
            double prm[12] = {};
            for (int i = 0; i < NumParams(model); ++i) prm[i] = cparams[12 * qi + i];
            for (int i = 0; i < nf; ++i) prm[i] *= factors[f];
            double mf = 0.0;
            for (int i = 0; i < nf; ++i) mf += prm[i];
            const double thr = est[4] / (mf / nf);
            std::vector<double> uv(2 * n);
            for (size_t k = 0; k < n; ++k) CamFromImg(model, prm, p2[2 * (c0 + k)], p2[2 * (c0 + k) + 1], &uv[2 * k], &uv[2 * k + 1]);
            Ransac r = LoRansac(Corr{n, uv.data(), p3 + 3 * c0}, RansacOpts{thr * thr, est[6], est[7], min_t, max_t});
            if (f == 0) first_trials = r.trials;
            if (r.success && r.inliers > (best < 0 ? 0 : chosen.inliers)) {
                best = static_cast<int>(f);
                chosen = r;
                std::memcpy(best_prm, prm, sizeof prm);
            }
        }
        success[qi] = 0;
        std::fill(qvec + 4 * qi, qvec + 4 * qi + 4, 0.0);
        std::fill(tvec + 3 * qi, tvec + 3 * qi + 3, 0.0);
        if (best < 0) {
            num_inliers[qi] = 0;
            num_trials[qi] = first_trials;
            focal[qi] = 0.0;
            std::fill(mask + c0, mask + c0 + n, 0);
            continue;
        }
        num_inliers[qi] = static_cast<uint32_t>(chosen.inliers);
        num_trials[qi] = chosen.trials;
        focal[qi] = factors[best];
        for (size_t k = 0; k < n; ++k) mask[c0 + k] = chosen.mask[k];
        double* q = qvec + 4 * qi;
        double* t = tvec + 3 * qi;
        if (!ModelToPose(chosen.model, q, t)) continue;
        const RefOpts ro{model, best_prm, ref[0], ref[2], static_cast<int64_t>(ref[1]), want_cov != 0};
        success[qi] = Refine(ro, q, t, p2 + 2 * c0, p3 + 3 * c0, chosen.mask, cv) ? 1 : 0;
    }
    return 0;
}

// trace: 6 int32 per query (iterations, accepted, rejected, invalid, exit, rank test failed), or null
int abspose_ref_refine_trace(const uint64_t* off, size_t nq, const int32_t* models, const double* cparams,
                             const double* p2, const double* p3, const double* init_q, const double* init_t,
                             const uint8_t* in_mask, const double* ref, int want_cov, uint8_t* success, double* qvec,
                             double* tvec, double* covariance, int32_t* trace) {
    for (size_t qi = 0; qi < nq; ++qi) {
        const size_t c0 = off[qi], n = off[qi + 1] - off[qi];
        double prm[12] = {};
        for (int i = 0; i < NumParams(models[qi]); ++i) prm[i] = cparams[12 * qi + i];
        std::vector<char> m(n);
        for (size_t k = 0; k < n; ++k) m[k] = in_mask[c0 + k] ? 1 : 0;
        std::memcpy(qvec + 4 * qi, init_q + 4 * qi, 4 * sizeof(double));
        std::memcpy(tvec + 3 * qi, init_t + 3 * qi, 3 * sizeof(double));
        const RefOpts ro{models[qi], prm, ref[0], ref[2], static_cast<int64_t>(ref[1]), want_cov != 0};
        Trace tr;
        success[qi] = Refine(ro, qvec + 4 * qi, tvec + 3 * qi, p2 + 2 * c0, p3 + 3 * c0, m,
                             covariance ? covariance + 36 * qi : nullptr, &tr) ? 1 : 0;
        if (trace) {
            const int32_t row[6] = {tr.iterations, tr.accepted, tr.rejected, tr.invalid, tr.exit, tr.rank_failed};
            std::memcpy(trace + 6 * qi, row, sizeof row);
        }
    }
    return 0;
}

int abspose_ref_refine(const uint64_t* off, size_t nq, const int32_t* models, const double* cparams, const double* p2,
                       const double* p3, const double* init_q, const double* init_t, const uint8_t* in_mask,
                       const double* ref, int want_cov, uint8_t* success, double* qvec, double* tvec,
                       double* covariance) {
    return abspose_ref_refine_trace(off, nq, models, cparams, p2, p3, init_q, init_t, in_mask, ref, want_cov, success,
                                    qvec, tvec, covariance, nullptr);
}

}  // extern "C"
