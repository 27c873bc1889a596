// abspose_core.h — absolute pose (include/amc_abspose.h): COLMAP 3.9.1's EstimateAbsolutePose (LO-RANSAC of P3P
// with EPnP local optimisation) and RefineAbsolutePose (Levenberg-Marquardt on the Cauchy-robustified reprojection
// error), restated in DESIGN.md section 12.  One 64-lane wave runs one problem.
//
// Everything that is not a sum over correspondences is wave-uniform scalar code that every lane computes alike (the
// sampler, the minimal solver, the Jacobi eigen solves, the trust-region bookkeeping).  Every sum over correspondences
// has one order (12.10): lane l adds the terms of correspondences l, l + 64, l + 128, ... in that order, then the 64
// partials are combined by the xor butterfly m = 32, 16, ..., 1 (the order of DESIGN.md D3).  wave_sum below is that
// order: on the device each lane is itself, on the host the 64 lanes run one after another (the header compiles for
// both).  FP contraction is off and every transcendental is the project's own (+ - * / and sqrt), so
// the kernel's bits equal those of the CPU reference written from DESIGN.md section 12 (tests/abspose_ref).
#pragma once

#include <float.h>
#include <stdint.h>

#include "camera_math.h"
#include "pose_math.h"

namespace amc {
namespace ap {

using tvg::dabs;
using tvg::dsqrt;

constexpr int kLanes = 64;
constexpr double kDblMax = DBL_MAX;
constexpr double kDblEps = DBL_EPSILON;

// ---- 12.10: the reduction order -------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ int ap_lane() { return (int)(threadIdx.x & 63u); }
#define AP_SYNC() __syncthreads()
#define AP_IS_LANE0 (ap_lane() == 0)
template <int N, class F>
__device__ __forceinline__ void wave_sum(F f, double (&out)[N]) {
    double v[N];
    f(ap_lane(), v);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = v[i] + __shfl_xor(v[i], m);
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = v[i];
}
#else
#define AP_SYNC() ((void)0)
#define AP_IS_LANE0 true
template <int N, class F>
inline void wave_sum(F f, double (&out)[N]) {
    static thread_local double p[kLanes][N], q[kLanes][N];
    for (int l = 0; l < kLanes; ++l) f(l, p[l]);
    for (int m = 32; m >= 1; m >>= 1) {
        for (int l = 0; l < kLanes; ++l)
            for (int i = 0; i < N; ++i) q[l][i] = p[l][i] + p[l ^ m][i];
        for (int l = 0; l < kLanes; ++l)
            for (int i = 0; i < N; ++i) p[l][i] = q[l][i];
    }
    for (int i = 0; i < N; ++i) out[i] = p[0][i];
}
#endif

// ---- 12.9: transcendentals from + - * / and sqrt (fdlibm 5.3: s_atan.c, k_sin.c, k_cos.c, e_rem_pio2.c, e_log.c) ------
AMC_HD uint64_t dbits(double x) {
    union { double d; uint64_t u; } b;
    b.d = x;
    return b.u;
}
AMC_HD double bitsd(uint64_t u) {
    union { double d; uint64_t u; } b;
    b.u = u;
    return b.d;
}
AMC_HD uint32_t hiword(double x) { return (uint32_t)(dbits(x) >> 32); }

AMC_HD double ap_atan(double x) {
    const double atanhi[4] = {4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01,
                              1.57079632679489655800e+00};
    const double atanlo[4] = {2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17,
                              6.12323399573676603587e-17};
    const double aT0 = 3.33333333333329318027e-01, aT1 = -1.99999999998764832476e-01, aT2 = 1.42857142725034663711e-01,
                 aT3 = -1.11111104054623557880e-01, aT4 = 9.09088713343650656196e-02, aT5 = -7.69187620504482999495e-02,
                 aT6 = 6.66107313738753120669e-02, aT7 = -5.83357013379057348645e-02, aT8 = 4.97687799461593236017e-02,
                 aT9 = -3.65315727442169155270e-02, aT10 = 1.62858201153657823623e-02;
    const uint32_t hx = hiword(x), ix = hx & 0x7fffffffu;
    const bool neg = (hx >> 31) != 0;
    int id;
    if (ix >= 0x44100000u) {  // |x| >= 2^66 or NaN
        if (x != x) return x + x;
        return neg ? -atanhi[3] - atanlo[3] : atanhi[3] + atanlo[3];
    }
    if (ix < 0x3fdc0000u) {  // |x| < 0.4375
        if (ix < 0x3e200000u) return x;  // |x| < 2^-29
        id = -1;
    } else {
        x = dabs(x);
        if (ix < 0x3ff30000u) {
            if (ix < 0x3fe60000u) {
                id = 0;
                x = (2.0 * x - 1.0) / (2.0 + x);
            } else {
                id = 1;
                x = (x - 1.0) / (x + 1.0);
            }
        } else if (ix < 0x40038000u) {
            id = 2;
            x = (x - 1.5) / (1.0 + 1.5 * x);
        } else {
            id = 3;
            x = -1.0 / x;
        }
    }
    const double z = x * x;
    const double w = z * z;
    const double s1 = z * (aT0 + w * (aT2 + w * (aT4 + w * (aT6 + w * (aT8 + w * aT10)))));
    const double s2 = w * (aT1 + w * (aT3 + w * (aT5 + w * (aT7 + w * aT9))));
    if (id < 0) return x - x * (s1 + s2);
    const double hi = id == 0 ? atanhi[0] : id == 1 ? atanhi[1] : id == 2 ? atanhi[2] : atanhi[3];
    const double lo = id == 0 ? atanlo[0] : id == 1 ? atanlo[1] : id == 2 ? atanlo[2] : atanlo[3];
    const double r = hi - ((x * (s1 + s2) - lo) - x);
    return neg ? -r : r;
}

AMC_HD double ap_ksin(double x, double y, int iy) {
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    if ((hiword(x) & 0x7fffffffu) < 0x3e400000u) return x;  // |x| < 2^-27
    const double z = x * x;
    const double v = z * x;
    const double r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    if (iy == 0) return x + v * (S1 + z * r);
    return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}
AMC_HD double ap_kcos(double x, double y) {
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const uint32_t ix = hiword(x) & 0x7fffffffu;
    if (ix < 0x3e400000u) return 1.0;  // |x| < 2^-27
    const double z = x * x;
    const double r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    if (ix < 0x3fd33333u) return 1.0 - (0.5 * z - (z * r - x * y));
    const double qx = ix > 0x3fe90000u ? 0.28125 : bitsd((uint64_t)(ix - 0x00200000u) << 32);
    const double hz = 0.5 * z - qx;
    const double a = 1.0 - qx;
    return a - (hz - (z * r - x * y));
}
// x = n pi/2 + y0 + y1 for |x| <= 2^19 pi/2 (the medium-size path of e_rem_pio2.c, its cancellation test by exponents);
// larger arguments return n = -1 (the callers' angles are far smaller: 12.9)
AMC_HD int ap_rem_pio2(double x, double& y0, double& y1) {
    const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00,
                 pio2_1t = 6.07710050650619224932e-11, pio2_2 = 6.07710050630396597660e-11,
                 pio2_2t = 2.02226624879595063154e-21, pio2_3 = 2.02226624871116645580e-21,
                 pio2_3t = 8.47842766036889956997e-32;
    const uint32_t hx = hiword(x), ix = hx & 0x7fffffffu;
    if (ix > 0x413921fbu) return -1;
    const double t0 = dabs(x);
    const int n = (int)(t0 * invpio2 + 0.5);
    const double fn = (double)n;
    double r = t0 - fn * pio2_1;
    double w = fn * pio2_1t;
    const int j = (int)(ix >> 20);
    y0 = r - w;
    int i = j - (int)((hiword(y0) >> 20) & 0x7ffu);
    if (i > 16) {
        double t = r;
        w = fn * pio2_2;
        r = t - w;
        w = fn * pio2_2t - ((t - r) - w);
        y0 = r - w;
        i = j - (int)((hiword(y0) >> 20) & 0x7ffu);
        if (i > 49) {
            t = r;
            w = fn * pio2_3;
            r = t - w;
            w = fn * pio2_3t - ((t - r) - w);
            y0 = r - w;
        }
    }
    y1 = (r - y0) - w;
    if (hx >> 31) {
        y0 = -y0;
        y1 = -y1;
        return (-n) & 3;
    }
    return n & 3;
}
AMC_HD double ap_sin(double x) {
    const uint32_t ix = hiword(x) & 0x7fffffffu;
    if (ix <= 0x3fe921fbu) return ap_ksin(x, 0.0, 0);
    if (ix >= 0x7ff00000u) return x - x;
    double y0, y1;
    const int n = ap_rem_pio2(x, y0, y1);
    switch (n) {
        case 0: return ap_ksin(y0, y1, 1);
        case 1: return ap_kcos(y0, y1);
        case 2: return -ap_ksin(y0, y1, 1);
        case 3: return -ap_kcos(y0, y1);
    }
    return __builtin_nan("");
}
AMC_HD double ap_cos(double x) {
    const uint32_t ix = hiword(x) & 0x7fffffffu;
    if (ix <= 0x3fe921fbu) return ap_kcos(x, 0.0);
    if (ix >= 0x7ff00000u) return x - x;
    double y0, y1;
    const int n = ap_rem_pio2(x, y0, y1);
    switch (n) {
        case 0: return ap_kcos(y0, y1);
        case 1: return -ap_ksin(y0, y1, 1);
        case 2: return -ap_kcos(y0, y1);
        case 3: return ap_ksin(y0, y1, 1);
    }
    return __builtin_nan("");
}
AMC_HD double ap_log(double x) {
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10,
                 two54 = 1.80143985094819840000e+16, Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01,
                 Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01,
                 Lg6 = 1.531383769920937332e-01, Lg7 = 1.479819860511658591e-01;
    uint64_t b = dbits(x);
    int32_t hx = (int32_t)(b >> 32);
    const uint32_t lx = (uint32_t)b;
    int k = 0;
    if (hx < 0x00100000) {
        if (((hx & 0x7fffffff) | (int32_t)lx) == 0) return -__builtin_inf();
        if (hx < 0) return __builtin_nan("");
        k -= 54;
        x *= two54;
        b = dbits(x);
        hx = (int32_t)(b >> 32);
    }
    if (hx >= 0x7ff00000) return x + x;
    k += (hx >> 20) - 1023;
    hx &= 0x000fffff;
    const int32_t i0 = (hx + 0x95f64) & 0x100000;
    x = bitsd(((uint64_t)(uint32_t)(hx | (i0 ^ 0x3ff00000)) << 32) | (dbits(x) & 0xffffffffu));
    k += (i0 >> 20);
    const double f = x - 1.0;
    const double dk = (double)k;
    if ((0x000fffff & (2 + hx)) < 3) {  // |f| < 2^-20
        if (f == 0.0) return k == 0 ? 0.0 : dk * ln2_hi + dk * ln2_lo;
        const double R = f * f * (0.5 - 0.33333333333333333 * f);
        if (k == 0) return f - R;
        return dk * ln2_hi - ((R - dk * ln2_lo) - f);
    }
    const double s = f / (2.0 + f);
    const double z = s * s;
    int32_t i = hx - 0x6147a;
    const double w = z * z;
    const int32_t j = 0x6b851 - hx;
    const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
    const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
    i |= j;
    const double R = t2 + t1;
    if (i > 0) {
        const double hfsq = 0.5 * f * f;
        if (k == 0) return f - (hfsq - s * (hfsq + R));
        return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
    }
    if (k == 0) return f - s * (f - R);
    return dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f);
}

// ---- forward-mode derivatives for the refinement (12.7): value + d/d(qx, qy, qz, qw, tx, ty, tz) ----------------------
constexpr int kJ = 7;
struct Jet {
    double a;
    double d[kJ];
};
AMC_HD Jet jconst(double a) {
    Jet r;
    r.a = a;
    for (int i = 0; i < kJ; ++i) r.d[i] = 0.0;
    return r;
}
AMC_HD Jet operator+(const Jet& x, const Jet& y) {
    Jet r;
    r.a = x.a + y.a;
    for (int i = 0; i < kJ; ++i) r.d[i] = x.d[i] + y.d[i];
    return r;
}
AMC_HD Jet operator-(const Jet& x, const Jet& y) {
    Jet r;
    r.a = x.a - y.a;
    for (int i = 0; i < kJ; ++i) r.d[i] = x.d[i] - y.d[i];
    return r;
}
AMC_HD Jet operator-(const Jet& x) {
    Jet r;
    r.a = -x.a;
    for (int i = 0; i < kJ; ++i) r.d[i] = -x.d[i];
    return r;
}
AMC_HD Jet operator*(const Jet& x, const Jet& y) {
    Jet r;
    r.a = x.a * y.a;
    for (int i = 0; i < kJ; ++i) r.d[i] = x.a * y.d[i] + x.d[i] * y.a;
    return r;
}
AMC_HD Jet operator/(const Jet& x, const Jet& y) {  // (x' - (x / y) y') / y
    Jet r;
    r.a = x.a / y.a;
    for (int i = 0; i < kJ; ++i) r.d[i] = (x.d[i] - r.a * y.d[i]) / y.a;
    return r;
}
AMC_HD Jet operator+(const Jet& x, double c) { Jet r = x; r.a = x.a + c; return r; }
AMC_HD Jet operator+(double c, const Jet& x) { Jet r = x; r.a = c + x.a; return r; }
AMC_HD Jet operator-(const Jet& x, double c) { Jet r = x; r.a = x.a - c; return r; }
AMC_HD Jet operator-(double c, const Jet& x) {
    Jet r;
    r.a = c - x.a;
    for (int i = 0; i < kJ; ++i) r.d[i] = -x.d[i];
    return r;
}
AMC_HD Jet operator*(const Jet& x, double c) {
    Jet r;
    r.a = x.a * c;
    for (int i = 0; i < kJ; ++i) r.d[i] = x.d[i] * c;
    return r;
}
AMC_HD Jet operator*(double c, const Jet& x) {
    Jet r;
    r.a = c * x.a;
    for (int i = 0; i < kJ; ++i) r.d[i] = c * x.d[i];
    return r;
}
AMC_HD Jet operator/(const Jet& x, double c) {
    Jet r;
    r.a = x.a / c;
    for (int i = 0; i < kJ; ++i) r.d[i] = x.d[i] / c;
    return r;
}
AMC_HD double val(double x) { return x; }
AMC_HD double val(const Jet& x) { return x.a; }
AMC_HD double tsqrt(double x) { return dsqrt(x); }
AMC_HD Jet tsqrt(const Jet& x) {
    Jet r;
    r.a = dsqrt(x.a);
    const double h = 2.0 * r.a;
    for (int i = 0; i < kJ; ++i) r.d[i] = x.d[i] / h;
    return r;
}
AMC_HD double tatan(double x) { return ap_atan(x); }
AMC_HD Jet tatan(const Jet& x) {
    Jet r;
    r.a = ap_atan(x.a);
    const double h = 1.0 + x.a * x.a;
    for (int i = 0; i < kJ; ++i) r.d[i] = x.d[i] / h;
    return r;
}

// Camera::ImgFromCam of the camera-frame point (u, v, w) for the eleven models (colmap/sensor/models.h: projection to
// the normalized plane u / w, v / w, then the model's distortion and the affine map), any scalar type
template <class T>
AMC_HD void img_from_cam_t(int model, const double* p, const T& pu, const T& pv, const T& pw, T& x, T& y) {
    using namespace cam;
    T u = pu / pw, v = pv / pw;
    const int nf = num_focal(model);
    const double f1 = p[0], f2 = p[nf - 1], c1 = p[nf], c2 = p[nf + 1];
    const double* e = p + nf + 2;
    if (model == FOV) {
        const double omega = e[0];
        const double kEpsilon = 1e-4;
        const T radius2 = u * u + v * v;
        const double omega2 = omega * omega;
        T factor;
        if (omega2 < kEpsilon) {
            factor = (omega2 * radius2) / 3.0 - omega2 / 12.0 + 1.0;
        } else {
            const double tan_half_omega = ap_sin(omega / 2.0) / ap_cos(omega / 2.0);
            if (val(radius2) < kEpsilon) {
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
        if (val(r) > kDblEps) {
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
            const T r = tsqrt(u * u + v * v);
            if (val(r) > kDblEps) {
                const T theta = tatan(r);
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

// ---- 12.5: ComputeSquaredReprojectionError in normalized coordinates -------------------------------------------------
AMC_HD double sq_reproj(const double* P, const double* X, double u, double v) {
    const double z = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
    if (!(z > kDblEps)) return kDblMax;
    const double x = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
    const double y = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
    const double du = x / z - u, dv = y / z - v;
    return du * du + dv * dv;
}

// ---- 12.3: P3P (Gao et al.'s quartic, obtained as the resultant of the two law-of-cosines quadratics) ----------------
// Coefficients low -> high.
AMC_HD void pmul(const double* a, int na, const double* b, int nb, double* r) {
    for (int i = 0; i < na + nb - 1; ++i) r[i] = 0.0;
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j) r[i + j] = r[i + j] + a[i] * b[j];
}
AMC_HD bool finite(double x) { return x - x == 0.0; }

// Eigen::umeyama(src, dst, false) for three points (world -> camera) as [R | t]
AMC_HD void umeyama3(const double (&src)[3][3], const double (&dst)[3][3], double* P) {
    double ms[3], md[3];
    for (int c = 0; c < 3; ++c) {
        ms[c] = (src[0][c] + src[1][c] + src[2][c]) / 3.0;
        md[c] = (dst[0][c] + dst[1][c] + dst[2][c]) / 3.0;
    }
    double S[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s = s + (dst[k][r] - md[r]) * (src[k][c] - ms[c]);
            S[3 * r + c] = s / 3.0;
        }
    double U[9], D[3], V[9];
    tvg::svd3(S, U, D, V);
    const double sgn = tvg::mat3_det(U) * tvg::mat3_det(V) < 0.0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            P[4 * r + c] = U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1] + sgn * U[3 * r + 2] * V[3 * c + 2];
    for (int r = 0; r < 3; ++r)
        P[4 * r + 3] = md[r] - (P[4 * r] * ms[0] + P[4 * r + 1] * ms[1] + P[4 * r + 2] * ms[2]);
}

// uv: 3 x 2 normalized image points, X: 3 x 3 world points; models ascending by the quartic's root; returns the count
AMC_HD int p3p(const double* uv, const double* X, double (*models)[12]) {
    double b[3][3];
    for (int i = 0; i < 3; ++i) {
        const double x = uv[2 * i], y = uv[2 * i + 1];
        const double nn = dsqrt(x * x + y * y + 1.0);
        b[i][0] = x / nn;
        b[i][1] = y / nn;
        b[i][2] = 1.0 / nn;
    }
    const double cos_uv = b[0][0] * b[1][0] + b[0][1] * b[1][1] + b[0][2] * b[1][2];
    const double cos_uw = b[0][0] * b[2][0] + b[0][1] * b[2][1] + b[0][2] * b[2][2];
    const double cos_vw = b[1][0] * b[2][0] + b[1][1] * b[2][1] + b[1][2] * b[2][2];
    double d[3];
    const int pa[3] = {0, 0, 1}, pb[3] = {1, 2, 2};  // AB, AC, BC
    for (int k = 0; k < 3; ++k) {
        const double* A = X + 3 * pa[k];
        const double* B = X + 3 * pb[k];
        d[k] = (A[0] - B[0]) * (A[0] - B[0]) + (A[1] - B[1]) * (A[1] - B[1]) + (A[2] - B[2]) * (A[2] - B[2]);
    }
    if (!(d[0] > 0.0) || !finite(d[0])) return 0;
    const double dist_AB = dsqrt(d[0]);
    const double a = d[2] / d[0], bb = d[1] / d[0];
    const double p = 2.0 * cos_vw, q = 2.0 * cos_uw, r = 2.0 * cos_uv;
    // (1 - a) y^2 + (a r x - p) y + (1 - a x^2) = 0 and -b y^2 + b r x y + ((1 - b) x^2 - q x + 1) = 0
    const double A1 = 1.0 - a, A2 = -bb;
    const double B1[2] = {-p, a * r}, B2[2] = {0.0, bb * r};
    const double C1[3] = {1.0, 0.0, -a}, C2[3] = {1.0, -q, 1.0 - bb};
    double E[3], F[2], G[4];
    for (int i = 0; i < 3; ++i) E[i] = A1 * C2[i] - A2 * C1[i];
    for (int i = 0; i < 2; ++i) F[i] = A1 * B2[i] - A2 * B1[i];
    double t1[4], t2[4];
    pmul(B1, 2, C2, 3, t1);
    pmul(B2, 2, C1, 3, t2);
    for (int i = 0; i < 4; ++i) G[i] = t1[i] - t2[i];
    double EE[5], FG[5];
    pmul(E, 3, E, 3, EE);
    pmul(F, 2, G, 4, FG);
    double c[5];
    bool ok = true;
    for (int i = 0; i < 5; ++i) {
        c[i] = EE[i] - FG[i];
        ok = ok && finite(c[i]);
    }
    if (!ok) return 0;
    double roots[4];
    const int nr = tvg::real_roots_t<4>(c, roots);
    int nm = 0;
    for (int k = 0; k < nr; ++k) {
        const double x = roots[k];
        if (x < 0.0) continue;
        const double b1 = -(F[0] + F[1] * x);                  // A2 B1(x) - A1 B2(x)
        if (b1 == 0.0) continue;
        const double y = (E[0] + x * (E[1] + x * E[2])) / b1;  // E(x) / b1
        const double nu = x * x + y * y - 2.0 * x * y * cos_uv;
        if (!(nu > 0.0)) continue;
        const double dist_PC = dist_AB / dsqrt(nu);
        const double dist_PB = y * dist_PC;
        const double dist_PA = x * dist_PC;
        double src[3][3], dst[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) src[i][j] = X[3 * i + j];
        for (int j = 0; j < 3; ++j) {
            dst[0][j] = b[0][j] * dist_PA;
            dst[1][j] = b[1][j] * dist_PB;
            dst[2][j] = b[2][j] * dist_PC;
        }
        umeyama3(src, dst, models[nm]);
        ++nm;
    }
    return nm;
}

// ---- small dense solves ---------------------------------------------------------------------------------------------
// Gaussian elimination with partial pivoting (first largest |pivot|) on the n x n row-major A (destroyed); false on a
// zero or non-finite pivot
template <int N>
AMC_HD bool solve_gauss(double (&A)[N * N], double (&b)[N]) {
    for (int k = 0; k < N; ++k) {
        int piv = k;
        double best = dabs(A[k * N + k]);
        for (int i = k + 1; i < N; ++i)
            if (dabs(A[i * N + k]) > best) {
                best = dabs(A[i * N + k]);
                piv = i;
            }
        if (!(best > 0.0) || !finite(best)) return false;
        if (piv != k) {
            for (int j = 0; j < N; ++j) {
                const double t = A[k * N + j];
                A[k * N + j] = A[piv * N + j];
                A[piv * N + j] = t;
            }
            const double t = b[k];
            b[k] = b[piv];
            b[piv] = t;
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
// least squares min |A x - y| (6 x N) through the normal equations A^T A x = A^T y
template <int N>
AMC_HD void lstsq6(const double (&A)[6][N], const double (&y)[6], double (&x)[N]) {
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
    if (!solve_gauss<N>(M, x))
        for (int i = 0; i < N; ++i) x[i] = __builtin_nan("");
}

// ---- the problem a wave works on ------------------------------------------------------------------------------------
struct Problem {
    uint32_t n;
    const double* uv;  // n x 2: normalized image points (CamFromImg of the scaled camera)
    const double* X;   // n x 3
};

// ---- 12.4: EPnP on the correspondences marked in `set` (n_set of them, >= 4) ------------------------------------------
struct EpnpFrame {
    double cw[4][3];  // control points (world)
    double ci[9];     // inverse of [cw1 - cw0, cw2 - cw0, cw3 - cw0]
    double nv[4][12]; // the null vectors, smallest eigenvalue first
    double cnt;
    double pw0[3];    // centroid
    uint32_t first;   // the first member
};
AMC_HD void epnp_alphas(const EpnpFrame& F, const double* X, double (&al)[4]) {
    const double d0 = X[0] - F.cw[0][0], d1 = X[1] - F.cw[0][1], d2 = X[2] - F.cw[0][2];
    al[1] = F.ci[0] * d0 + F.ci[1] * d1 + F.ci[2] * d2;
    al[2] = F.ci[3] * d0 + F.ci[4] * d1 + F.ci[5] * d2;
    al[3] = F.ci[6] * d0 + F.ci[7] * d1 + F.ci[8] * d2;
    al[0] = 1.0 - al[1] - al[2] - al[3];
}
// camera-frame control points of `betas`, R and t, and the mean reprojection error (NaN propagates)
AMC_HD double epnp_rt(const Problem& pr, const uint8_t* set, const EpnpFrame& F, const double (&betas)[4], double* P) {
    double cc[4][3];
    for (int j = 0; j < 4; ++j)
        for (int c = 0; c < 3; ++c) {
            double s = 0.0;
            for (int i = 0; i < 4; ++i) s = s + betas[i] * F.nv[i][3 * j + c];
            cc[j][c] = s;
        }
    // SolveForSign: the first member's camera-frame z
    {
        double al[4];
        epnp_alphas(F, pr.X + 3 * F.first, al);
        const double z = al[0] * cc[0][2] + al[1] * cc[1][2] + al[2] * cc[2][2] + al[3] * cc[3][2];
        if (z < 0.0)
            for (int j = 0; j < 4; ++j)
                for (int c = 0; c < 3; ++c) cc[j][c] = -cc[j][c];
    }
    auto pc_of = [&](uint32_t k, double* pc) {
        double al[4];
        epnp_alphas(F, pr.X + 3 * k, al);
        for (int c = 0; c < 3; ++c) pc[c] = al[0] * cc[0][c] + al[1] * cc[1][c] + al[2] * cc[2][c] + al[3] * cc[3][c];
    };
    double s3[3];
    wave_sum<3>(
        [&](int l, double (&o)[3]) {
            o[0] = o[1] = o[2] = 0.0;
            for (uint32_t k = (uint32_t)l; k < pr.n; k += kLanes) {
                if (!set[k]) continue;
                double pc[3];
                pc_of(k, pc);
                o[0] = o[0] + pc[0];
                o[1] = o[1] + pc[1];
                o[2] = o[2] + pc[2];
            }
        },
        s3);
    const double pc0[3] = {s3[0] / F.cnt, s3[1] / F.cnt, s3[2] / F.cnt};
    double abt[9];
    wave_sum<9>(
        [&](int l, double (&o)[9]) {
            for (int i = 0; i < 9; ++i) o[i] = 0.0;
            for (uint32_t k = (uint32_t)l; k < pr.n; k += kLanes) {
                if (!set[k]) continue;
                double pc[3];
                pc_of(k, pc);
                const double* X = pr.X + 3 * k;
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) o[3 * r + c] = o[3 * r + c] + (pc[r] - pc0[r]) * (X[c] - F.pw0[c]);
            }
        },
        abt);
    // R = U diag(1, 1, det U det V) V^T: svd3's third left vector is u0 x u1 (D1), whatever sign A v2 / s2 has, so
    // the original's "negate R's last row when det(U V^T) < 0" would also fire on a proper rotation (A4)
    double U[9], D[3], V[9], R[9];
    tvg::svd3(abt, U, D, V);
    const double sgn = tvg::mat3_det(U) * tvg::mat3_det(V) < 0.0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            R[3 * r + c] = U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1] + sgn * U[3 * r + 2] * V[3 * c + 2];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) P[4 * r + c] = R[3 * r + c];
        P[4 * r + 3] = pc0[r] - (R[3 * r] * F.pw0[0] + R[3 * r + 1] * F.pw0[1] + R[3 * r + 2] * F.pw0[2]);
    }
    double e1[1];
    wave_sum<1>(
        [&](int l, double (&o)[1]) {
            o[0] = 0.0;
            for (uint32_t k = (uint32_t)l; k < pr.n; k += kLanes) {
                if (!set[k]) continue;
                const double* X = pr.X + 3 * k;
                const double xc = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
                const double yc = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
                const double zc = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
                const double du = pr.uv[2 * k] - xc / zc, dv = pr.uv[2 * k + 1] - yc / zc;
                o[0] = o[0] + dsqrt(du * du + dv * dv);
            }
        },
        e1);
    return e1[0] / F.cnt;
}

AMC_HD void epnp_gauss_newton(const double (&L)[6][10], const double (&rho)[6], double (&b)[4]) {
    for (int it = 0; it < 5; ++it) {
        double A[6][4], y[6];
        for (int j = 0; j < 6; ++j) {
            const double* l = L[j];
            A[j][0] = 2.0 * l[0] * b[0] + l[1] * b[1] + l[3] * b[2] + l[6] * b[3];
            A[j][1] = l[1] * b[0] + 2.0 * l[2] * b[1] + l[4] * b[2] + l[7] * b[3];
            A[j][2] = l[3] * b[0] + l[4] * b[1] + 2.0 * l[5] * b[2] + l[8] * b[3];
            A[j][3] = l[6] * b[0] + l[7] * b[1] + l[8] * b[2] + 2.0 * l[9] * b[3];
            y[j] = rho[j] - (l[0] * b[0] * b[0] + l[1] * b[0] * b[1] + l[2] * b[1] * b[1] + l[3] * b[0] * b[2] +
                             l[4] * b[1] * b[2] + l[5] * b[2] * b[2] + l[6] * b[0] * b[3] + l[7] * b[1] * b[3] +
                             l[8] * b[2] * b[3] + l[9] * b[3] * b[3]);
        }
        double x[4];
        lstsq6<4>(A, y, x);
        for (int i = 0; i < 4; ++i) b[i] = b[i] + x[i];
    }
}

AMC_HD bool epnp(const Problem& pr, const uint8_t* set, double* P) {
    EpnpFrame F;
    double s4[4];
    wave_sum<4>(
        [&](int l, double (&o)[4]) {
            o[0] = o[1] = o[2] = o[3] = 0.0;
            for (uint32_t k = (uint32_t)l; k < pr.n; k += kLanes) {
                if (!set[k]) continue;
                o[0] = o[0] + 1.0;
                o[1] = o[1] + pr.X[3 * k];
                o[2] = o[2] + pr.X[3 * k + 1];
                o[3] = o[3] + pr.X[3 * k + 2];
            }
        },
        s4);
    F.cnt = s4[0];
    if (!(F.cnt >= 4.0)) return false;
    for (int c = 0; c < 3; ++c) F.pw0[c] = s4[1 + c] / F.cnt;
    F.first = 0;
    while (!set[F.first]) ++F.first;
    // ChooseControlPoints: the centroid and the principal axes scaled by sqrt(singular value / n)
    double cov6[6];
    wave_sum<6>(
        [&](int l, double (&o)[6]) {
            for (int i = 0; i < 6; ++i) o[i] = 0.0;
            for (uint32_t k = (uint32_t)l; k < pr.n; k += kLanes) {
                if (!set[k]) continue;
                const double d0 = pr.X[3 * k] - F.pw0[0], d1 = pr.X[3 * k + 1] - F.pw0[1], d2 = pr.X[3 * k + 2] - F.pw0[2];
                o[0] = o[0] + d0 * d0;
                o[1] = o[1] + d0 * d1;
                o[2] = o[2] + d0 * d2;
                o[3] = o[3] + d1 * d1;
                o[4] = o[4] + d1 * d2;
                o[5] = o[5] + d2 * d2;
            }
        },
        cov6);
    const double C[9] = {cov6[0], cov6[1], cov6[2], cov6[1], cov6[3], cov6[4], cov6[2], cov6[4], cov6[5]};
    double U[9], D[3], V[9];
    tvg::svd3(C, U, D, V);
    for (int c = 0; c < 3; ++c) F.cw[0][c] = F.pw0[c];
    for (int i = 0; i < 3; ++i) {
        const double k = dsqrt(D[i] / F.cnt);
        for (int c = 0; c < 3; ++c) F.cw[i + 1][c] = F.cw[0][c] + k * U[3 * c + i];
    }
    // ComputeBarycentricCoordinates
    double CC[9];
    for (int r = 0; r < 3; ++r)
        for (int i = 0; i < 3; ++i) CC[3 * r + i] = F.cw[i + 1][r] - F.cw[0][r];
    const double det = tvg::mat3_det(CC);
    if (det == 0.0 || !finite(det)) return false;
    tvg::mat3_inv(CC, F.ci);
    // M^T M over the members, upper triangle row by row
    double mtm[78];
    wave_sum<78>(
        [&](int l, double (&o)[78]) {
            for (int i = 0; i < 78; ++i) o[i] = 0.0;
            for (uint32_t k = (uint32_t)l; k < pr.n; k += kLanes) {
                if (!set[k]) continue;
                double al[4];
                epnp_alphas(F, pr.X + 3 * k, al);
                const double u = pr.uv[2 * k], v = pr.uv[2 * k + 1];
                double m1[12], m2[12];
                for (int j = 0; j < 4; ++j) {
                    m1[3 * j] = al[j];
                    m1[3 * j + 1] = 0.0;
                    m1[3 * j + 2] = -al[j] * u;
                    m2[3 * j] = 0.0;
                    m2[3 * j + 1] = al[j];
                    m2[3 * j + 2] = -al[j] * v;
                }
                int t = 0;
                for (int i = 0; i < 12; ++i)
                    for (int j = i; j < 12; ++j, ++t) o[t] = o[t] + (m1[i] * m1[j] + m2[i] * m2[j]);
            }
        },
        mtm);
    double A[144], W[144];
    {
        int t = 0;
        for (int i = 0; i < 12; ++i)
            for (int j = i; j < 12; ++j, ++t) {
                A[12 * i + j] = mtm[t];
                A[12 * j + i] = mtm[t];
            }
    }
    tvg::jacobi_eigen_t<12>(A, W);
    // the four smallest eigenvalues, ascending (a tie keeps the lower index)
    bool used[12];
    for (int i = 0; i < 12; ++i) used[i] = false;
    for (int s = 0; s < 4; ++s) {
        int best = -1;
        for (int i = 0; i < 12; ++i)
            if (!used[i] && (best < 0 || A[13 * i] < A[13 * best])) best = i;
        used[best] = true;
        for (int r = 0; r < 12; ++r) F.nv[s][r] = W[12 * r + best];
    }
    // L (6 x 10) and rho over the control-point pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
    const int ea[6] = {0, 0, 0, 1, 1, 2}, eb[6] = {1, 2, 3, 2, 3, 3};
    double L[6][10], rho[6];
    for (int j = 0; j < 6; ++j) {
        double dv[4][3];
        for (int i = 0; i < 4; ++i)
            for (int c = 0; c < 3; ++c) dv[i][c] = F.nv[i][3 * ea[j] + c] - F.nv[i][3 * eb[j] + c];
        auto dot = [&](int a, int b) { return dv[a][0] * dv[b][0] + dv[a][1] * dv[b][1] + dv[a][2] * dv[b][2]; };
        L[j][0] = dot(0, 0);
        L[j][1] = 2.0 * dot(0, 1);
        L[j][2] = dot(1, 1);
        L[j][3] = 2.0 * dot(0, 2);
        L[j][4] = 2.0 * dot(1, 2);
        L[j][5] = dot(2, 2);
        L[j][6] = 2.0 * dot(0, 3);
        L[j][7] = 2.0 * dot(1, 3);
        L[j][8] = 2.0 * dot(2, 3);
        L[j][9] = dot(3, 3);
        const double* a = F.cw[ea[j]];
        const double* b = F.cw[eb[j]];
        rho[j] = (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
    }
    double betas[3][4], Ps[3][12], err[3];
    {  // FindBetasApprox1: columns 0 1 3 6
        double A4[6][4], x[4];
        for (int j = 0; j < 6; ++j) {
            A4[j][0] = L[j][0]; A4[j][1] = L[j][1]; A4[j][2] = L[j][3]; A4[j][3] = L[j][6];
        }
        lstsq6<4>(A4, rho, x);
        if (x[0] < 0.0) {
            const double s = dsqrt(-x[0]);
            betas[0][0] = s; betas[0][1] = -x[1] / s; betas[0][2] = -x[2] / s; betas[0][3] = -x[3] / s;
        } else {
            const double s = dsqrt(x[0]);
            betas[0][0] = s; betas[0][1] = x[1] / s; betas[0][2] = x[2] / s; betas[0][3] = x[3] / s;
        }
    }
    {  // FindBetasApprox2: columns 0 1 2
        double A3[6][3], x[3];
        for (int j = 0; j < 6; ++j) {
            A3[j][0] = L[j][0]; A3[j][1] = L[j][1]; A3[j][2] = L[j][2];
        }
        lstsq6<3>(A3, rho, x);
        double b0, b1;
        if (x[0] < 0.0) {
            b0 = dsqrt(-x[0]);
            b1 = x[2] < 0.0 ? dsqrt(-x[2]) : 0.0;
        } else {
            b0 = dsqrt(x[0]);
            b1 = x[2] > 0.0 ? dsqrt(x[2]) : 0.0;
        }
        if (x[1] < 0.0) b0 = -b0;
        betas[1][0] = b0; betas[1][1] = b1; betas[1][2] = 0.0; betas[1][3] = 0.0;
    }
    {  // FindBetasApprox3: columns 0 1 2 3 4
        double A5[6][5], x[5];
        for (int j = 0; j < 6; ++j)
            for (int c = 0; c < 5; ++c) A5[j][c] = L[j][c];
        lstsq6<5>(A5, rho, x);
        double b0, b1;
        if (x[0] < 0.0) {
            b0 = dsqrt(-x[0]);
            b1 = x[2] < 0.0 ? dsqrt(-x[2]) : 0.0;
        } else {
            b0 = dsqrt(x[0]);
            b1 = x[2] > 0.0 ? dsqrt(x[2]) : 0.0;
        }
        if (x[1] < 0.0) b0 = -b0;
        betas[2][0] = b0; betas[2][1] = b1; betas[2][2] = x[3] / b0; betas[2][3] = 0.0;
    }
    for (int s = 0; s < 3; ++s) {
        epnp_gauss_newton(L, rho, betas[s]);
        err[s] = epnp_rt(pr, set, F, betas[s], Ps[s]);
    }
    int best = 0;
    if (err[1] < err[0]) best = 1;
    if (err[2] < err[best]) best = 2;
    for (int i = 0; i < 12; ++i) P[i] = Ps[best][i];
    return true;
}

// ---- 12.6: LORANSAC<P3PEstimator, EPNPEstimator> --------------------------------------------------------------------
struct Support {
    uint32_t cnt;
    double sum;
};
AMC_HD bool better(const Support& a, const Support& b) { return a.cnt > b.cnt || (a.cnt == b.cnt && a.sum < b.sum); }

// InlierSupportMeasurer::Evaluate of the model P; mark: also write the inlier flags to mask
AMC_HD Support score(const Problem& pr, const double* P, double max_residual, uint8_t* mask, bool mark) {
    double s[2];
    wave_sum<2>(
        [&](int l, double (&o)[2]) {
            o[0] = o[1] = 0.0;
            for (uint32_t k = (uint32_t)l; k < pr.n; k += kLanes) {
                const double r = sq_reproj(P, pr.X + 3 * k, pr.uv[2 * k], pr.uv[2 * k + 1]);
                const bool in = r <= max_residual;
                if (in) {
                    o[0] = o[0] + 1.0;
                    o[1] = o[1] + r;
                }
                if (mark) mask[k] = in ? 1 : 0;
            }
        },
        s);
    AP_SYNC();
    return Support{(uint32_t)s[0], s[1]};
}

struct RansacParams {
    double max_residual;       // max_error^2 (normalized units)
    uint64_t min_trials;
    uint64_t max_trials;       // after the RANSAC constructor's clamp
    const uint64_t* dyn_row;   // ComputeNumTrials(c, n) for c = 0 .. n, or null (never earlier than max_trials)
    const uint32_t* stream;    // tempered mt19937(0) words
    uint64_t stream_len;
};
struct RansacOut {
    bool success;
    bool overrun;              // the sample stream ran out: the caller reruns on a longer table
    uint32_t num_inliers;
    uint64_t num_trials;
    double model[12];
};

// perm (n entries, the sampler's persistent permutation) and mask (n bytes) are the problem's scratch; on return mask
// holds the final inlier mask (all 0 on failure)
AMC_HD RansacOut lo_ransac(const Problem& pr, const RansacParams& rp, uint32_t* perm, uint8_t* mask) {
    RansacOut out;
    out.success = false;
    out.overrun = false;
    out.num_inliers = 0;
    out.num_trials = 0;
    for (int i = 0; i < 12; ++i) out.model[i] = 0.0;
    const uint32_t n = pr.n;
    if (n < 3) {
        for (uint32_t k = (uint32_t)0; k < n; ++k)
            if (AP_IS_LANE0) mask[k] = 0;
        AP_SYNC();
        return out;
    }
    if (AP_IS_LANE0)
        for (uint32_t k = 0; k < n; ++k) perm[k] = k;
    AP_SYNC();
    Support best{0u, kDblMax};
    double best_model[12];
    for (int i = 0; i < 12; ++i) best_model[i] = 0.0;
    uint64_t pos = 0;  // stream words consumed
    uint64_t dyn_max = rp.max_trials;
    bool abort = false;
    uint64_t trial;
    for (trial = 0; trial < rp.max_trials; ++trial) {
        if (abort) {
            trial += 1;
            break;
        }
        // RandomSampler::Sample: j = uniform_int(i, n - 1) (libstdc++'s Lemire reduction), swap(perm[i], perm[j])
        uint32_t sidx[3];
        for (uint32_t i = 0; i < 3; ++i) {
            const uint32_t range = n - i;
            uint64_t prod = 0;
            uint32_t low = 0;
            bool first = true;
            const uint32_t threshold = (uint32_t)(-range) % range;
            while (first || low < threshold) {
                if (pos >= rp.stream_len) {
                    out.overrun = true;
                    break;
                }
                prod = (uint64_t)rp.stream[pos++] * (uint64_t)range;
                low = (uint32_t)prod;
                if (first && low >= range) break;
                first = false;
            }
            if (out.overrun) break;
            const uint32_t j = i + (uint32_t)(prod >> 32);
            const uint32_t a = perm[i], b = perm[j];
            AP_SYNC();
            if (AP_IS_LANE0) {
                perm[i] = b;
                perm[j] = a;
            }
            AP_SYNC();
            sidx[i] = b;
        }
        if (out.overrun) break;
        double uv3[6], X3[9];
        for (int i = 0; i < 3; ++i) {
            uv3[2 * i] = pr.uv[2 * sidx[i]];
            uv3[2 * i + 1] = pr.uv[2 * sidx[i] + 1];
            for (int c = 0; c < 3; ++c) X3[3 * i + c] = pr.X[3 * sidx[i] + c];
        }
        double models[4][12];
        const int nm = p3p(uv3, X3, models);
        for (int mi = 0; mi < nm; ++mi) {
            const Support s = score(pr, models[mi], rp.max_residual, mask, false);
            if (better(s, best)) {
                best = s;
                for (int i = 0; i < 12; ++i) best_model[i] = models[mi][i];
                if (s.cnt > 3 && s.cnt >= 4) {
                    for (int lt = 0; lt < 10; ++lt) {
                        const uint32_t prev = best.cnt;
                        score(pr, best_model, rp.max_residual, mask, true);  // the current best's inliers
                        double L[12];
                        if (epnp(pr, mask, L)) {
                            const Support ls = score(pr, L, rp.max_residual, mask, false);
                            if (better(ls, best)) {
                                best = ls;
                                for (int i = 0; i < 12; ++i) best_model[i] = L[i];
                            }
                        }
                        if (best.cnt <= prev) break;
                    }
                }
                dyn_max = rp.dyn_row ? rp.dyn_row[best.cnt] : rp.max_trials;
            }
            if (trial >= dyn_max && trial >= rp.min_trials) {
                abort = true;
                break;
            }
        }
    }
    out.num_trials = trial;
    out.num_inliers = best.cnt;
    if (best.cnt < 3 || out.overrun) {
        for (uint32_t k = 0; k < n; ++k)
            if (AP_IS_LANE0) mask[k] = 0;
        AP_SYNC();
        return out;
    }
    out.success = true;
    for (int i = 0; i < 12; ++i) out.model[i] = best_model[i];
    score(pr, best_model, rp.max_residual, mask, true);
    return out;
}

// ---- 12.7 / 12.8: RefineAbsolutePose --------------------------------------------------------------------------------
struct RefineParams {
    int model;
    const double* params;     // the (scaled) camera
    double gradient_tolerance;
    int64_t max_num_iterations;
    double loss_scale;        // CauchyLoss(loss_function_scale)
    bool covariance;
};
struct RefineOut {
    bool success;             // Summary::IsSolutionUsable (and, when asked, a covariance)
    double q[4];              // x y z w
    double t[3];
    double cov[36];
    int iterations;
};

// EigenQuaternionManifold::Plus(x, delta)
AMC_HD void quat_plus(const double* q, const double* d, double* out) {
    const double nd = dsqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (nd == 0.0) {
        for (int i = 0; i < 4; ++i) out[i] = q[i];
        return;
    }
    const double sd = ap_sin(nd) / nd;
    const double a[4] = {sd * d[0], sd * d[1], sd * d[2], ap_cos(nd)};  // x y z w
    out[3] = a[3] * q[3] - a[0] * q[0] - a[1] * q[1] - a[2] * q[2];
    out[0] = a[3] * q[0] + a[0] * q[3] + a[1] * q[2] - a[2] * q[1];
    out[1] = a[3] * q[1] - a[0] * q[2] + a[1] * q[3] + a[2] * q[0];
    out[2] = a[3] * q[2] + a[0] * q[1] - a[1] * q[0] + a[2] * q[3];
}
// EigenQuaternionManifold::PlusJacobian (4 x 3, row-major) at q
AMC_HD void quat_plus_jacobian(const double* q, double* J) {
    J[0] = q[3];  J[1] = q[2];   J[2] = -q[1];
    J[3] = -q[2]; J[4] = q[3];   J[5] = q[0];
    J[6] = q[1];  J[7] = -q[0];  J[8] = q[3];
    J[9] = -q[0]; J[10] = -q[1]; J[11] = -q[2];
}

// residual of one correspondence (pixels) with d/d(q, t); Eigen's q * X (v + w uv + q.vec x uv, uv = 2 q.vec x X) + t
AMC_HD void pixel_residual(const RefineParams& rp, const double* q, const double* t, const double* X, double ox,
                           double oy, Jet& rx, Jet& ry) {
    Jet qv[4], tv[3];
    for (int i = 0; i < 4; ++i) {
        qv[i] = jconst(q[i]);
        qv[i].d[i] = 1.0;
    }
    for (int i = 0; i < 3; ++i) {
        tv[i] = jconst(t[i]);
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
    const Jet p0 = (X[0] + qv[3] * uv0) + c0 + tv[0];
    const Jet p1 = (X[1] + qv[3] * uv1) + c1 + tv[1];
    const Jet p2 = (X[2] + qv[3] * uv2) + c2 + tv[2];
    img_from_cam_t<Jet>(rp.model, rp.params, p0, p1, p2, rx, ry);
    rx = rx - ox;
    ry = ry - oy;
}

// one evaluation over the inliers: cost = 1/2 sum rho(s); with jac, also H = J^T J (21, upper) and g = J^T f (6) in the
// tangent space, J and f Ceres' loss-corrected ones (CauchyLoss: rho'' < 0, so J and f are scaled by sqrt(rho'))
struct Eval {
    double cost;
    double H[21];
    double g[6];
};
// res(k, q, t, rx, ry): the residual of correspondence k with d/d(q, t) (the rig refinement of rigpose_core.h passes its own)
template <class Res>
AMC_HD Eval evaluate_t(const Res& res, double loss_scale, const double* q, const double* t, const uint8_t* mask,
                       uint32_t n, bool jac) {
    const double b = loss_scale * loss_scale, c = 1.0 / b;
    double Jm[12];
    quat_plus_jacobian(q, Jm);
    Eval ev;
    double s[28];
    wave_sum<28>(
        [&](int l, double (&o)[28]) {
            for (int i = 0; i < 28; ++i) o[i] = 0.0;
            for (uint32_t k = (uint32_t)l; k < n; k += kLanes) {
                if (!mask[k]) continue;
                Jet rx, ry;
                res(k, q, t, rx, ry);
                const double sq = rx.a * rx.a + ry.a * ry.a;
                const double sum = 1.0 + sq * c;
                const double inv = 1.0 / sum;
                o[0] = o[0] + 0.5 * (b * ap_log(sum));
                if (!jac) continue;
                const double w = dsqrt(inv);
                double J[2][6];
                const Jet* rr[2] = {&rx, &ry};
                for (int r = 0; r < 2; ++r) {
                    for (int j = 0; j < 3; ++j)
                        J[r][j] = w * (rr[r]->d[0] * Jm[j] + rr[r]->d[1] * Jm[3 + j] + rr[r]->d[2] * Jm[6 + j] +
                                       rr[r]->d[3] * Jm[9 + j]);
                    for (int j = 0; j < 3; ++j) J[r][3 + j] = w * rr[r]->d[4 + j];
                }
                const double f[2] = {w * rx.a, w * ry.a};
                int tt = 1;
                for (int i = 0; i < 6; ++i)
                    for (int j = i; j < 6; ++j, ++tt) o[tt] = o[tt] + (J[0][i] * J[0][j] + J[1][i] * J[1][j]);
                for (int i = 0; i < 6; ++i) o[22 + i] = o[22 + i] + (J[0][i] * f[0] + J[1][i] * f[1]);
            }
        },
        s);
    ev.cost = s[0];
    for (int i = 0; i < 21; ++i) ev.H[i] = s[1 + i];
    for (int i = 0; i < 6; ++i) ev.g[i] = s[22 + i];
    return ev;
}
AMC_HD double sym6(const double* H, int i, int j) {
    if (i > j) {
        const int t = i;
        i = j;
        j = t;
    }
    return H[i * 6 - i * (i - 1) / 2 + (j - i)];
}
// ‖x − Plus(x, −g)‖∞ over the seven ambient coordinates
AMC_HD double gradient_max_norm(const double* q, const double* t, const double* g) {
    const double mg[3] = {-g[0], -g[1], -g[2]};
    double qp[4];
    quat_plus(q, mg, qp);
    double m = 0.0;
    for (int i = 0; i < 4; ++i) m = tvg::dmax(m, dabs(q[i] - qp[i]));
    for (int i = 0; i < 3; ++i) m = tvg::dmax(m, dabs(t[i] - (t[i] + (-g[3 + i]))));
    return m;
}

// the solver's settings without the camera (12.7)
struct LmParams {
    double gradient_tolerance;
    int64_t max_num_iterations;
    double loss_scale;
    bool covariance;
};
template <class Res>
AMC_HD RefineOut refine_t(const Res& res, const LmParams& rp, const double* q0, const double* t0, const uint8_t* mask,
                          uint32_t n) {
    RefineOut out;
    out.success = false;
    out.iterations = 0;
    double q[4] = {q0[0], q0[1], q0[2], q0[3]}, t[3] = {t0[0], t0[1], t0[2]};
    for (int i = 0; i < 36; ++i) out.cov[i] = 0.0;
    double cnt[1];
    wave_sum<1>(
        [&](int l, double (&o)[1]) {
            o[0] = 0.0;
            for (uint32_t k = (uint32_t)l; k < n; k += kLanes) o[0] = o[0] + (mask[k] ? 1.0 : 0.0);
        },
        cnt);
    bool usable = true;
    if (cnt[0] > 0.0) {
        Eval ev = evaluate_t(res, rp.loss_scale, q, t, mask, n, true);
        if (!finite(ev.cost)) usable = false;
        double scale[6];
        for (int i = 0; i < 6; ++i) scale[i] = 1.0 / (1.0 + dsqrt(sym6(ev.H, i, i)));
        double radius = 1e4, decrease = 2.0;
        int invalid_run = 0;
        bool done = !usable || gradient_max_norm(q, t, ev.g) <= rp.gradient_tolerance;
        for (int64_t it = 1; !done && it <= rp.max_num_iterations; ++it) {
            out.iterations = (int)it;
            // the LM step in Jacobi-scaled variables: (Js^T Js + diag(clamp(diag(Js^T Js)) / radius)) y = -Js^T f
            double A[36], y[6], Hs[36];
            for (int i = 0; i < 6; ++i) {
                for (int j = 0; j < 6; ++j) Hs[6 * i + j] = scale[i] * sym6(ev.H, i, j) * scale[j];
                y[i] = -(scale[i] * ev.g[i]);
            }
            for (int i = 0; i < 36; ++i) A[i] = Hs[i];
            for (int i = 0; i < 6; ++i) {
                double dgl = Hs[7 * i];
                dgl = dgl < 1e-6 ? 1e-6 : dgl > 1e32 ? 1e32 : dgl;
                A[7 * i] = A[7 * i] + dgl / radius;
            }
            bool valid = solve_gauss<6>(A, y);
            double mcc = 0.0;
            if (valid) {
                double gy = 0.0, yhy = 0.0;
                for (int i = 0; i < 6; ++i) {
                    gy = gy + (scale[i] * ev.g[i]) * y[i];
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
                if (++invalid_run >= 5) {
                    usable = false;
                    break;
                }
                if (radius < 1e-32) break;
                continue;
            }
            invalid_run = 0;
            double delta[6], qn[4], tn[3];
            for (int i = 0; i < 6; ++i) delta[i] = scale[i] * y[i];
            quat_plus(q, delta, qn);
            for (int i = 0; i < 3; ++i) tn[i] = t[i] + delta[3 + i];
            // parameter tolerance: |x - x_new| <= 1e-8 (|x| + 1e-8)
            double sn = 0.0, xn = 0.0;
            for (int i = 0; i < 4; ++i) {
                sn = sn + (q[i] - qn[i]) * (q[i] - qn[i]);
                xn = xn + q[i] * q[i];
            }
            for (int i = 0; i < 3; ++i) {
                sn = sn + (t[i] - tn[i]) * (t[i] - tn[i]);
                xn = xn + t[i] * t[i];
            }
            if (dsqrt(sn) <= 1e-8 * (dsqrt(xn) + 1e-8)) break;
            const Eval cand = evaluate_t(res, rp.loss_scale, qn, tn, mask, n, false);
            const double new_cost = finite(cand.cost) ? cand.cost : kDblMax;
            const double cost_change = ev.cost - new_cost;
            if (dabs(cost_change) <= 1e-6 * ev.cost) break;  // function tolerance
            const double rel = cost_change / mcc;
            if (rel > 1e-3) {
                for (int i = 0; i < 4; ++i) q[i] = qn[i];
                for (int i = 0; i < 3; ++i) t[i] = tn[i];
                ev = evaluate_t(res, rp.loss_scale, q, t, mask, n, true);
                const double z = 2.0 * rel - 1.0;
                const double f = 1.0 - z * z * z;
                radius = radius / (f > 1.0 / 3.0 ? f : 1.0 / 3.0);
                radius = radius < 1e16 ? radius : 1e16;
                decrease = 2.0;
                if (gradient_max_norm(q, t, ev.g) <= rp.gradient_tolerance) break;
            } else {
                radius = radius / decrease;
                decrease = 2.0 * decrease;
                if (radius < 1e-32) break;
            }
        }
        if (usable && rp.covariance) {
            // (J^T J)^-1 in the tangent space by Jacobi; rank test: lambda_min > 1e-28 lambda_max (12.8)
            double H[36], V[36];
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 6; ++j) H[6 * i + j] = sym6(ev.H, i, j);
            tvg::jacobi_eigen_t<6>(H, V);
            double lmin = H[0], lmax = H[0];
            for (int i = 1; i < 6; ++i) {
                lmin = H[7 * i] < lmin ? H[7 * i] : lmin;
                lmax = H[7 * i] > lmax ? H[7 * i] : lmax;
            }
            if (!(lmax > 0.0) || !(lmin > 1e-28 * lmax) || !finite(lmax)) {
                usable = false;
            } else {
                for (int i = 0; i < 6; ++i)
                    for (int j = 0; j < 6; ++j) {
                        double s2 = 0.0;
                        for (int k = 0; k < 6; ++k) s2 = s2 + V[6 * i + k] * (V[6 * j + k] / H[7 * k]);
                        out.cov[6 * i + j] = s2;
                    }
            }
        }
    }
    out.success = usable;
    for (int i = 0; i < 4; ++i) out.q[i] = q[i];
    for (int i = 0; i < 3; ++i) out.t[i] = t[i];
    return out;
}
AMC_HD RefineOut refine(const RefineParams& rp, const double* q0, const double* t0, const double* xy, const double* X,
                        const uint8_t* mask, uint32_t n) {
    const LmParams lm{rp.gradient_tolerance, rp.max_num_iterations, rp.loss_scale, rp.covariance};
    return refine_t(
        [&](uint32_t k, const double* qq, const double* tt, Jet& rx, Jet& ry) {
            pixel_residual(rp, qq, tt, X + 3 * k, xy[2 * k], xy[2 * k + 1], rx, ry);
        },
        lm, q0, t0, mask, n);
}

// ---- 12.1: the model -> quaternion step and the NaN test --------------------------------------------------------------
AMC_HD bool model_to_pose(const double* P, double* qxyzw, double* t) {
    const double m[9] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]};
    double wxyz[4];
    tvg::rotation_to_quaternion(m, wxyz);
    qxyzw[0] = wxyz[1];
    qxyzw[1] = wxyz[2];
    qxyzw[2] = wxyz[3];
    qxyzw[3] = wxyz[0];
    t[0] = P[3];
    t[1] = P[7];
    t[2] = P[11];
    for (int i = 0; i < 4; ++i)
        if (qxyzw[i] != qxyzw[i]) return false;
    for (int i = 0; i < 3; ++i)
        if (t[i] != t[i]) return false;
    return true;
}

}  // namespace ap
}  // namespace amc
