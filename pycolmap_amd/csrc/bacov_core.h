// bacov_core.h — bundle-adjustment covariance (include/amc_bacov.h): the small arithmetic of DESIGN.md section 24 that
// the kernels and the host share.  The observation, the loss corrector and sym3_inverse are ba_core.h's.
#pragma once

#include "ba_core.h"

namespace amc {
namespace bacov {

constexpr int kTile = 64;                // the dense passes' tile edge: a panel is one tile wide (24.4)
constexpr int kLocal = 6 + ba::kMaxParams;           // an observation's columns: its pose, then its camera
constexpr int kLocalPairs = kLocal * (kLocal + 1) / 2;  // 171 entries (u >= v) of J_c^T J_c
constexpr int kCamPairs = ba::kMaxParams * (ba::kMaxParams + 1) / 2;  // 78 of them lie in the camera block

// entry e = u (u + 1) / 2 + v of a lower triangle, u >= v
AMC_HD void tri_decode(int e, int& u, int& v) {
    u = 0;
    while ((u + 1) * (u + 2) / 2 <= e) ++u;
    v = e - u * (u + 1) / 2;
}

// the full symmetric 3 x 3 of ba_core.h's packing
AMC_HD void sym3_full(const double* s, double (&m)[3][3]) {
    m[0][0] = s[0]; m[0][1] = s[1]; m[0][2] = s[2];
    m[1][0] = s[1]; m[1][1] = s[3]; m[1][2] = s[4];
    m[2][0] = s[2]; m[2][1] = s[4]; m[2][2] = s[5];
}

// 24.6: V^-1 + V^-1 M V^-1 with each product entry a three-term sum left to right
AMC_HD void point_cov_finish(const double* vinv, const double* M, double* out) {
    double Vi[3][3], P[3][3];
    sym3_full(vinv, Vi);
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) P[a][b] = Vi[a][0] * M[b] + Vi[a][1] * M[3 + b] + Vi[a][2] * M[6 + b];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            out[3 * a + b] = Vi[a][b] + (P[a][0] * Vi[0][b] + P[a][1] * Vi[1][b] + P[a][2] * Vi[2][b]);
}

}  // namespace bacov
}  // namespace amc
