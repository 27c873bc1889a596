// filter_core.h — the point filter (include/amc_filter.h): the per-observation and per-pair arithmetic of DESIGN.md
// section 16.  The world-to-camera map and the camera models are bundle adjustment's (ba_core.h: quat_rotate,
// img_from_cam_p<double>), so a filter after an adjustment sees the bits the adjustment minimised; the angle is
// triangulation's (tri_angle.h).  FP contraction is off and every transcendental is the project's own (12.9), so the
// bits equal tests/filter_ref.  The functions carry AMC_HD like ba_core.h's, which they call, but only filter.hip's
// kernels use them: no host code includes this header (there is no CPU path, and the CPU reference restates the
// arithmetic on purpose), so their host side is compiled and never run.
#pragma once

#include <cfloat>

#include "ba_core.h"
#include "tri_angle.h"

namespace amc {
namespace filt {

// 16.4: a selected track of at least this many elements gets a wave of its own, a shorter one a lane
constexpr uint32_t kWaveClassMin = 64;
// DegToRad's factor, as COLMAP writes it
constexpr double kDegToRad = 0.0174532925199432954743716805978692718781530857086181640625;

// Image::ProjectionCenter (16.2): rotation.inverse() * -translation for q = (x, y, z, w), not normalised.  Eigen's
// inverse is the conjugate over the squared norm, and the zero quaternion where that norm is not positive.
AMC_HD void projection_centre(const double* q, const double* t, double* C) {
    const double n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
    double qi[4] = {0.0, 0.0, 0.0, 0.0};
    if (n2 > 0.0) {
        qi[0] = -q[0] / n2;
        qi[1] = -q[1] / n2;
        qi[2] = -q[2] / n2;
        qi[3] = q[3] / n2;
    }
    const double nt[3] = {-t[0], -t[1], -t[2]};
    ba::quat_rotate(qi, nt, C);
}

// CalculateSquaredReprojectionError (16.1): DBL_MAX for a depth below DBL_EPSILON; a NaN depth goes through
AMC_HD double squared_reprojection_error(int model, const double* prm, const double* q, const double* t, const double* X,
                                         const double* xy) {
    double Xc[3];
    ba::quat_rotate(q, X, Xc);
    for (int i = 0; i < 3; ++i) Xc[i] = Xc[i] + t[i];
    if (Xc[2] < DBL_EPSILON) return DBL_MAX;
    double p[ba::kMaxParams], x, y;
    for (int i = 0; i < ba::kMaxParams; ++i) p[i] = prm[i];
    ba::img_from_cam_p<double>(model, p, Xc[0], Xc[1], Xc[2], x, y);
    const double dx = x - xy[0], dy = y - xy[1];
    return dx * dx + dy * dy;
}

}  // namespace filt
}  // namespace amc
