// tri_core.h — DESIGN.md section 11's estimator and LO-RANSAC as device functions, shared by track triangulation
// (tri.hip) and the incremental triangulator's observation kernel (triobs.hip): both take the same bits from them.
// Every FP64 operation is written in the order of that section, the order tests/tri_ref/tri_ref.cc follows too.  acos
// and the triangulation angle are tri_angle.h's; both eigen problems use the round-robin Jacobi of D1 (pose_math.h).
//
// The functions are templates over a view V of one problem's observations.  V provides
//   double x(o), y(o)            the normalised image point of observation o
//   const TriPose& pose(o)       its pose
//   uint8_t* mask                one byte per observation: the inlier set of a local optimisation, then the final mask
//   double max_residual          max_error^2
//   double min_tri_angle
// where o counts the view's observations; a RANSAC runs on the n observations o0 .. o0 + n.  No atomics, no LDS, no
// scratch: the lane's state is a few dozen registers.
#pragma once

#include <cfloat>
#include <cstdint>

#include "pose_math.h"
#include "tri_angle.h"

namespace amc {
namespace tri {

constexpr uint64_t kNoTable = ~(uint64_t)0;

// one pose: cam_from_world [R | t] row-major, the projection centre -R^T t, padding to 128 bytes
struct TriPose {
    double P[12];
    double C[3];
    double pad;
};

// ---- numerics (acos and the triangulation angle: tri_angle.h) -----------------------------------------
// P.row(2) . [X; 1]
AMC_TRI_FN double tri_depth(const double* P, const double* X) {
    return P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
}

// angular error of observation (x, y) under pose P for the point X: acos of the cosine between [x, y, 1] and P [X; 1]
AMC_TRI_FN double tri_angular_error(double x, double y, const double* P, const double* X) {
    const double na = tvg::dsqrt(x * x + y * y + 1.0);
    const double a0 = x / na, a1 = y / na, a2 = 1.0 / na;
    const double q0 = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
    const double q1 = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
    const double q2 = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
    const double nb = tvg::dsqrt(q0 * q0 + q1 * q1 + q2 * q2);
    const double c = a0 * (q0 / nb) + a1 * (q1 / nb) + a2 * (q2 / nb);
    return tri_acos(c);
}

// squared angular error
AMC_TRI_FN double tri_residual(double x, double y, const double* P, const double* X) {
    const double e = tri_angular_error(x, y, P, X);
    return e * e;
}

// eigenvector of the smallest eigenvalue of the symmetric 4 x 4 `a` (first minimum of the Jacobi diagonal), dehomogenised
AMC_TRI_FN void tri_smallest_dehom(double (&a)[16], double* X) {
    double v[16];
    tvg::jacobi_eigen_t<4>(a, v);
    double dmin = a[0];
    double e0 = v[0], e1 = v[4], e2 = v[8], w = v[12];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (a[5 * i] < dmin) { dmin = a[5 * i]; e0 = v[i]; e1 = v[4 + i]; e2 = v[8 + i]; w = v[12 + i]; }
    X[0] = e0 / w; X[1] = e1 / w; X[2] = e2 / w;
}

// ---- the estimator ------------------------------------------------------------------------------------
// two observations: DLT rows x P2 - P0, y P2 - P1 of both views, A^T A, smallest eigenvector; then both depths and the
// angle
template <class V>
AMC_TRI_FN bool tri_estimate_two(const V& p, uint64_t i, uint64_t j, double* X) {
    const double xi = p.x(i), yi = p.y(i), xj = p.x(j), yj = p.y(j);
    const TriPose& Pi = p.pose(i);
    const TriPose& Pj = p.pose(j);
    double A[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        A[0][c] = xi * Pi.P[8 + c] - Pi.P[c];
        A[1][c] = yi * Pi.P[8 + c] - Pi.P[4 + c];
        A[2][c] = xj * Pj.P[8 + c] - Pj.P[c];
        A[3][c] = yj * Pj.P[8 + c] - Pj.P[4 + c];
    }
    double ata[16];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += A[k][r] * A[k][c];
            ata[4 * r + c] = s;
        }
    tri_smallest_dehom(ata, X);
    return tri_depth(Pi.P, X) >= DBL_EPSILON && tri_depth(Pj.P, X) >= DBL_EPSILON &&
           tri_angle(Pi.C, Pj.C, X) >= p.min_tri_angle;
}

// the local estimator on the inlier set marked in mask[o0 .. o0 + n) (cnt >= 2 members): two members -> the two-view
// estimator; more -> A = sum term^T term, term = P - p p^T P, p = normalized([x, y, 1]); every depth, then any pair
// (i, j < i) with the angle
template <class V>
AMC_TRI_FN bool tri_estimate_set(const V& p, uint64_t o0, uint64_t n, uint32_t cnt, double* X) {
    const uint8_t* set = p.mask + o0;
    if (cnt == 2) {
        uint64_t i = 0;
        while (!set[i]) ++i;
        uint64_t j = i + 1;
        while (!set[j]) ++j;
        return tri_estimate_two(p, o0 + i, o0 + j, X);
    }
    double A[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) A[k] = 0.0;
    for (uint64_t k = 0; k < n; ++k) {
        if (!set[k]) continue;
        const uint64_t o = o0 + k;
        const double x = p.x(o), y = p.y(o);
        const double* P = p.pose(o).P;
        const double nrm = tvg::dsqrt(x * x + y * y + 1.0);
        const double h[3] = {x / nrm, y / nrm, 1.0 / nrm};
        double T[3][4];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double m = h[r] * h[0] * P[c] + h[r] * h[1] * P[4 + c] + h[r] * h[2] * P[8 + c];
                T[r][c] = P[4 * r + c] - m;
            }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) A[4 * r + c] = A[4 * r + c] + (T[0][r] * T[0][c] + T[1][r] * T[1][c] + T[2][r] * T[2][c]);
    }
    tri_smallest_dehom(A, X);
    for (uint64_t k = 0; k < n; ++k)
        if (set[k] && !(tri_depth(p.pose(o0 + k).P, X) >= DBL_EPSILON)) return false;
    for (uint64_t i = 1; i < n; ++i) {
        if (!set[i]) continue;
        const double* ci = p.pose(o0 + i).C;
        for (uint64_t j = 0; j < i; ++j) {
            if (!set[j]) continue;
            if (tri_angle(ci, p.pose(o0 + j).C, X) >= p.min_tri_angle) return true;
        }
    }
    return false;
}

// InlierSupportMeasurer::Evaluate: inliers have residual <= max_residual (NaN is an outlier); the residual sum adds
// the inliers' residuals in observation order.  mark: also write the inlier flags to the mask bytes.
struct TriSupport {
    uint32_t cnt;
    double sum;
};
template <class V>
AMC_TRI_FN TriSupport tri_score(const V& p, uint64_t o0, uint64_t n, const double* X, bool mark) {
    TriSupport s{0u, 0.0};
    uint8_t* m = p.mask + o0;
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t o = o0 + k;
        const double r = tri_residual(p.x(o), p.y(o), p.pose(o).P, X);
        const bool in = r <= p.max_residual;
        if (in) {
            s.cnt += 1;
            s.sum += r;
        }
        if (mark) m[k] = in ? 1 : 0;
    }
    return s;
}
AMC_TRI_FN bool tri_better(const TriSupport a, const TriSupport b) {
    return a.cnt > b.cnt || (a.cnt == b.cnt && a.sum < b.sum);
}

// ---- LORANSAC<TriangulationEstimator x 2, InlierSupportMeasurer, CombinationSampler> -----------------
// on the observations o0 .. o0 + n (n >= 2).  max_trials: RANSACOptions::max_num_trials after the RANSAC constructor's
// clamp; dyn_row: the dyn_max_num_trials row of length n (ComputeNumTrials(num_inliers, n) for num_inliers = 0 .. n),
// or nullptr for a RANSAC that cannot stop early.  best / best_xyz: the best support and model (best.cnt < 2: failure);
// returns LORANSAC's num_trials.  The mask bytes hold a local optimisation's inlier set afterwards, not the final mask.
template <class V>
AMC_TRI_FN uint64_t tri_lo_ransac(const V& p, uint64_t o0, uint64_t n, uint64_t max_trials_cfg, uint64_t min_trials,
                                  const uint64_t* dyn_row, double* best_xyz, TriSupport& best) {
    best_xyz[0] = 0.0; best_xyz[1] = 0.0; best_xyz[2] = 0.0;
    best = TriSupport{0u, DBL_MAX};
    const uint64_t combos = n * (n - 1) / 2;
    const uint64_t max_trials = max_trials_cfg < combos ? max_trials_cfg : combos;
    uint64_t dyn_max = max_trials;
    uint64_t a = 0, b = 1;  // the next pair of the lexicographic combination order
    bool abort = false;
    uint64_t trial;
    for (trial = 0; trial < max_trials; ++trial) {
        if (abort) {
            trial += 1;
            break;
        }
        const uint64_t i = a, j = b;
        if (++b == n) {
            ++a;
            b = a + 1;
            if (b == n) { a = 0; b = 1; }
        }
        double X[3];
        if (!tri_estimate_two(p, o0 + i, o0 + j, X)) continue;
        const TriSupport s = tri_score(p, o0, n, X, false);
        if (tri_better(s, best)) {
            best = s;
            best_xyz[0] = X[0]; best_xyz[1] = X[1]; best_xyz[2] = X[2];
            if (s.cnt > 2) {
                for (int lt = 0; lt < 10; ++lt) {
                    const uint32_t prev = best.cnt;
                    // the inlier set of the current best model, in the mask bytes
                    const TriSupport cur = tri_score(p, o0, n, best_xyz, true);
                    double L[3];
                    if (tri_estimate_set(p, o0, n, cur.cnt, L)) {
                        const TriSupport ls = tri_score(p, o0, n, L, false);
                        if (tri_better(ls, best)) {
                            best = ls;
                            best_xyz[0] = L[0]; best_xyz[1] = L[1]; best_xyz[2] = L[2];
                        }
                    }
                    if (best.cnt <= prev) break;
                }
            }
            dyn_max = dyn_row ? dyn_row[best.cnt] : kNoTable;
        }
        if (trial >= dyn_max && trial >= min_trials) abort = true;
    }
    return trial;
}

}  // namespace tri
}  // namespace amc
