// tri_angle.h — DESIGN.md 11.4's acos and CalculateTriangulationAngle for the kernels: track triangulation (tri.hip)
// and the point filter (filter.hip) take the same bits from them.  Only + - * / and the correctly rounded sqrt; FP
// contraction is off for every translation unit that includes this header.  Device functions only: the CPU references
// restate them.
#pragma once

#include "tvg_math.h"  // dsqrt

#define AMC_TRI_FN __device__ __forceinline__

namespace amc {
namespace tri {

constexpr double kTriPi = 3.14159265358979311600e+00;  // M_PI

// acos of fdlibm's e_acos.c (the rational approximation of asin on [0, 0.5] and its two reductions), written in
// + - * / and sqrt; NaN outside [-1, 1]
AMC_TRI_FN double tri_acos_r(double z) {
    const double p = z * (1.66666666666666657415e-01 +
                          z * (-3.25565818622400915405e-01 +
                               z * (2.01212532134862925881e-01 +
                                    z * (-4.00555345006794114027e-02 +
                                         z * (7.91534994289814532176e-04 + z * 3.47933107596021167570e-05)))));
    const double q = 1.0 + z * (-2.40339491173441421878e+00 +
                                z * (2.02094576023350569471e+00 +
                                     z * (-6.88283971605453293030e-01 + z * 7.70381505559019352791e-02)));
    return p / q;
}
AMC_TRI_FN double tri_acos(double x) {
    const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17;
    const double ax = x < 0.0 ? -x : x;
    if (!(ax <= 1.0)) return __builtin_nan("");
    if (x == 1.0) return 0.0;
    if (x == -1.0) return kTriPi;
    if (ax < 0.5) return pio2_hi - (x - (pio2_lo - x * tri_acos_r(x * x)));
    if (x < 0.0) {
        const double z = (1.0 + x) * 0.5;
        const double s = tvg::dsqrt(z);
        const double w = tri_acos_r(z) * s - pio2_lo;
        return kTriPi - 2.0 * (s + w);
    }
    const double z = (1.0 - x) * 0.5;
    const double s = tvg::dsqrt(z);
    return 2.0 * (s + s * tri_acos_r(z));
}

// CalculateTriangulationAngle: law of cosines, min(angle, pi - angle); 0 for a zero denominator, NaN when the ratio
// rounds outside [-1, 1]
AMC_TRI_FN double tri_angle(const double* c1, const double* c2, const double* X) {
    const double b0 = c1[0] - c2[0], b1 = c1[1] - c2[1], b2 = c1[2] - c2[2];
    const double baseline2 = b0 * b0 + b1 * b1 + b2 * b2;
    const double r0 = X[0] - c1[0], r1 = X[1] - c1[1], r2 = X[2] - c1[2];
    const double ray1 = r0 * r0 + r1 * r1 + r2 * r2;
    const double s0 = X[0] - c2[0], s1 = X[1] - c2[1], s2 = X[2] - c2[2];
    const double ray2 = s0 * s0 + s1 * s1 + s2 * s2;
    const double den = 2.0 * tvg::dsqrt(ray1 * ray2);
    if (den == 0.0) return 0.0;
    const double nom = ray1 + ray2 - baseline2;
    const double a = tri_acos(nom / den);
    const double angle = a < 0.0 ? -a : a;
    const double other = kTriPi - angle;
    return other < angle ? other : angle;  // std::min(angle, pi - angle)
}

}  // namespace tri
}  // namespace amc
