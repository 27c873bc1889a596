// tri_ref.cc — CPU reference of track triangulation, written from DESIGN.md section 11 alone (it includes none of
// pycolmap_amd/csrc): COLMAP 3.9.1's EstimateTriangulation with the angular residual, LORANSAC's control flow as
// colmap/optim/loransac.h has it (residual vectors swapped, not recomputed), the combination sampler, the estimator of
// colmap/estimators/triangulation.cc.  Plain scalar C++, -ffp-contract=off: the GPU kernel must match it bit for bit.
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

namespace {

const double kPi = 3.14159265358979311600e+00;

// 11.4: acos from + - * / and sqrt (fdlibm's e_acos.c reductions and rational approximation)
double R(double z) {
    const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
                 pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05;
    const double qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
                 qS4 = 7.70381505559019352791e-02;
    const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    return p / q;
}

double Acos(double x) {
    const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17;
    if (!(std::fabs(x) <= 1.0)) return std::numeric_limits<double>::quiet_NaN();
    if (x == 1.0) return 0.0;
    if (x == -1.0) return kPi;
    if (std::fabs(x) < 0.5) return pio2_hi - (x - (pio2_lo - x * R(x * x)));
    if (x < 0.0) {
        const double z = (1.0 + x) * 0.5;
        const double s = std::sqrt(z);
        const double w = R(z) * s - pio2_lo;
        return kPi - 2.0 * (s + w);
    }
    const double z = (1.0 - x) * 0.5;
    const double s = std::sqrt(z);
    return 2.0 * (s + s * R(z));
}

struct Pose {
    double P[3][4];
    double C[3];
};
struct Obs {
    double x, y;
    const Pose* pose;
};
struct Vec3 {
    double v[3];
};

// 11.2: law of cosines
double TriAngle(const double* c1, const double* c2, const Vec3& X) {
    double b[3], r[3], s[3];
    for (int i = 0; i < 3; ++i) {
        b[i] = c1[i] - c2[i];
        r[i] = X.v[i] - c1[i];
        s[i] = X.v[i] - c2[i];
    }
    const double baseline2 = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
    const double ray1 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    const double ray2 = s[0] * s[0] + s[1] * s[1] + s[2] * s[2];
    const double den = 2.0 * std::sqrt(ray1 * ray2);
    if (den == 0.0) return 0.0;
    const double nom = ray1 + ray2 - baseline2;
    const double angle = std::fabs(Acos(nom / den));
    const double other = kPi - angle;
    return other < angle ? other : angle;
}

double Depth(const Pose& p, const Vec3& X) {
    return p.P[2][0] * X.v[0] + p.P[2][1] * X.v[1] + p.P[2][2] * X.v[2] + p.P[2][3];
}

double Residual(const Obs& o, const Vec3& X) {
    const double na = std::sqrt(o.x * o.x + o.y * o.y + 1.0);
    const double a[3] = {o.x / na, o.y / na, 1.0 / na};
    double q[3];
    for (int r = 0; r < 3; ++r)
        q[r] = o.pose->P[r][0] * X.v[0] + o.pose->P[r][1] * X.v[1] + o.pose->P[r][2] * X.v[2] + o.pose->P[r][3];
    const double nb = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    const double c = a[0] * (q[0] / nb) + a[1] * (q[1] / nb) + a[2] * (q[2] / nb);
    const double e = Acos(c);
    return e * e;
}

// D1: cyclic-by-rounds Jacobi on a symmetric 4 x 4 (pairs of round r: (r+1, r-1 mod 3) and (r, 3)), rotations of a
// round computed first, then applied to the columns of a and v, then to the rows of a; at most 40 sweeps, ending
// when the squared off-diagonal upper triangle is no longer above 1e-32 times the squared Frobenius norm
void Jacobi4(double a[4][4], double v[4][4]) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    double total = 0.0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) total += a[i][j] * a[i][j];
    const double tol = total * 1e-32;
    for (int sweep = 0; sweep < 40; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) off += a[p][q] * a[p][q];
        if (!(off > tol)) break;
        for (int r = 0; r < 3; ++r) {
            int pp[2], qq[2];
            bool act[2];
            double c[2], s[2];
            {
                const int x = (r + 1) % 3, y = (r - 1 + 3) % 3;
                pp[0] = x < y ? x : y;
                qq[0] = x < y ? y : x;
                pp[1] = r;
                qq[1] = 3;
            }
            for (int e = 0; e < 2; ++e) {
                const double app = a[pp[e]][pp[e]], aqq = a[qq[e]][qq[e]], apq = a[pp[e]][qq[e]];
                act[e] = apq != 0.0;
                if (!act[e]) continue;
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                c[e] = 1.0 / std::sqrt(t * t + 1.0);
                s[e] = t * c[e];
            }
            for (int e = 0; e < 2; ++e) {
                if (!act[e]) continue;
                const int p = pp[e], q = qq[e];
                for (int k = 0; k < 4; ++k) {
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c[e] * akp - s[e] * akq;
                    a[k][q] = s[e] * akp + c[e] * akq;
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c[e] * vkp - s[e] * vkq;
                    v[k][q] = s[e] * vkp + c[e] * vkq;
                }
            }
            for (int e = 0; e < 2; ++e) {
                if (!act[e]) continue;
                const int p = pp[e], q = qq[e];
                for (int k = 0; k < 4; ++k) {
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c[e] * apk - s[e] * aqk;
                    a[q][k] = s[e] * apk + c[e] * aqk;
                }
            }
        }
    }
}

// eigenvector of the first smallest diagonal entry after Jacobi, dehomogenised
Vec3 SmallestDehom(double a[4][4]) {
    double v[4][4];
    Jacobi4(a, v);
    int m = 0;
    for (int i = 1; i < 4; ++i)
        if (a[i][i] < a[m][m]) m = i;
    return Vec3{{v[0][m] / v[3][m], v[1][m] / v[3][m], v[2][m] / v[3][m]}};
}

// What tri_ref_triangulate_trace reports of one track's RANSAC (the tests prove with it that an edge case is of the
// kind its name says).  Filling it changes no arithmetic.
struct Trace {
    int64_t dyn_row = 0;         // 1: min(max_num_trials', n(n-1)/2) > min_num_trials, the RANSAC can stop early (11.3)
    int64_t abort_trial = -1;    // the trial at which abort was set, or -1
    int64_t depth_rejects = 0;   // two-view samples refused by a depth
    int64_t angle_rejects = 0;   // two-view samples refused by the angle
    int64_t lo_rounds = 0;       // local optimisations entered
    int64_t lo_max_iters = 0;    // most iterations of one of them
    int64_t lo_max_growing = 0;  // most iterations of one of them after which the inlier count had grown
    int64_t lo_iters = 0;        // iterations of all of them
    int64_t lo_replaced = 0;     // local models that replaced the best
    int64_t lo_refused = 0;      // local estimates without a model
    int64_t nan = 0;             // 1: a residual or an angle was NaN
    double angle = std::numeric_limits<double>::quiet_NaN();  // the angle that admitted the final model; without a
                                                              // model, the last angle that refused one
    double last_angle = std::numeric_limits<double>::quiet_NaN();
    int why = 0;                 // the last Estimate: 0 a model, 1 refused by a depth, 2 by the angle
};
constexpr int kTraceInts = 11;

struct Estimator {
    double min_tri_angle;
    Trace* tr = nullptr;
    bool Admit(double angle) const {
        if (tr) {
            tr->last_angle = angle;
            if (angle != angle) tr->nan = 1;
        }
        return angle >= min_tri_angle;
    }
    void Why(int w) const {
        if (tr) tr->why = w;
    }
    // TriangulationEstimator::Estimate: empty or one model
    std::vector<Vec3> Estimate(const std::vector<Obs>& obs) const {
        if (obs.size() == 2) {
            double A[4][4];
            for (int c = 0; c < 4; ++c) {
                A[0][c] = obs[0].x * obs[0].pose->P[2][c] - obs[0].pose->P[0][c];
                A[1][c] = obs[0].y * obs[0].pose->P[2][c] - obs[0].pose->P[1][c];
                A[2][c] = obs[1].x * obs[1].pose->P[2][c] - obs[1].pose->P[0][c];
                A[3][c] = obs[1].y * obs[1].pose->P[2][c] - obs[1].pose->P[1][c];
            }
            double ata[4][4];
            for (int r = 0; r < 4; ++r)
                for (int c = 0; c < 4; ++c) {
                    double s = 0.0;
                    for (int k = 0; k < 4; ++k) s += A[k][r] * A[k][c];
                    ata[r][c] = s;
                }
            const Vec3 X = SmallestDehom(ata);
            Why(1);
            if (!(Depth(*obs[0].pose, X) >= DBL_EPSILON && Depth(*obs[1].pose, X) >= DBL_EPSILON)) return {};
            Why(2);
            if (!Admit(TriAngle(obs[0].pose->C, obs[1].pose->C, X))) return {};
            Why(0);
            return {X};
        }
        double A[4][4] = {};
        for (const Obs& o : obs) {
            const double nrm = std::sqrt(o.x * o.x + o.y * o.y + 1.0);
            const double h[3] = {o.x / nrm, o.y / nrm, 1.0 / nrm};
            double T[3][4];
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 4; ++c) {
                    const double m = h[r] * h[0] * o.pose->P[0][c] + h[r] * h[1] * o.pose->P[1][c] +
                                     h[r] * h[2] * o.pose->P[2][c];
                    T[r][c] = o.pose->P[r][c] - m;
                }
            for (int r = 0; r < 4; ++r)
                for (int c = 0; c < 4; ++c) A[r][c] = A[r][c] + (T[0][r] * T[0][c] + T[1][r] * T[1][c] + T[2][r] * T[2][c]);
        }
        const Vec3 X = SmallestDehom(A);
        Why(1);
        for (const Obs& o : obs)
            if (!(Depth(*o.pose, X) >= DBL_EPSILON)) return {};
        Why(2);
        for (size_t i = 0; i < obs.size(); ++i)
            for (size_t j = 0; j < i; ++j)
                if (Admit(TriAngle(obs[i].pose->C, obs[j].pose->C, X))) {
                    Why(0);
                    return {X};
                }
        return {};
    }
    void Residuals(const std::vector<Obs>& obs, const Vec3& X, std::vector<double>* res) const {
        res->resize(obs.size());
        for (size_t i = 0; i < obs.size(); ++i) {
            (*res)[i] = Residual(obs[i], X);
            if (tr && (*res)[i] != (*res)[i]) tr->nan = 1;
        }
    }
};

struct Support {
    size_t num_inliers = 0;
    double residual_sum = std::numeric_limits<double>::max();
};
Support Evaluate(const std::vector<double>& res, double max_residual) {
    Support s;
    s.num_inliers = 0;
    s.residual_sum = 0.0;
    for (double r : res)
        if (r <= max_residual) {
            s.num_inliers += 1;
            s.residual_sum += r;
        }
    return s;
}
bool Better(const Support& a, const Support& b) {
    return a.num_inliers > b.num_inliers || (a.num_inliers == b.num_inliers && a.residual_sum < b.residual_sum);
}

// colmap/optim/ransac.h ComputeNumTrials, kMinNumSamples = 2
size_t ComputeNumTrials(size_t num_inliers, size_t num_samples, double confidence, double multiplier) {
    const double inlier_ratio = num_inliers / static_cast<double>(num_samples);
    const double nom = 1 - confidence;
    if (nom <= 0) return std::numeric_limits<size_t>::max();
    const double denom = 1 - std::pow(inlier_ratio, 2);
    if (denom <= 0) return 1;
    if (denom == 1.0) return std::numeric_limits<size_t>::max();
    return static_cast<size_t>(std::ceil(std::log(nom) / std::log(denom) * multiplier));
}

struct Options {
    double min_tri_angle, max_error, min_inlier_ratio, confidence, multiplier;
    int64_t min_num_trials, max_num_trials;
};

struct Report {
    bool success = false;
    size_t num_trials = 0;
    Support support;
    Vec3 model{{0, 0, 0}};
    std::vector<char> mask;
};

// LORANSAC<TriangulationEstimator, TriangulationEstimator, InlierSupportMeasurer, CombinationSampler>::Estimate
// (tr, final_res: the trace, filled when given)
Report LoRansac(const Options& o, const std::vector<Obs>& obs, Trace* tr = nullptr,
                std::vector<double>* final_res = nullptr) {
    const Estimator est{o.min_tri_angle, tr};
    Report report;
    const size_t n = obs.size();
    report.mask.assign(n, 0);
    if (n < 2) return report;
    const size_t kNumSamples = 100000;
    const size_t max_cfg = std::min<size_t>(static_cast<size_t>(o.max_num_trials),
                                            ComputeNumTrials(static_cast<size_t>(o.min_inlier_ratio * kNumSamples),
                                                             kNumSamples, o.confidence, o.multiplier));
    const size_t max_num_trials = std::min<size_t>(max_cfg, n * (n - 1) / 2);  // CombinationSampler::MaxNumSamples
    size_t dyn_max_num_trials = max_num_trials;
    if (tr) tr->dyn_row = max_num_trials > static_cast<size_t>(o.min_num_trials) ? 1 : 0;
    const double max_residual = o.max_error * o.max_error;
    Support best_support;
    Vec3 best_model{{0, 0, 0}};
    bool abort = false, have_model = false;
    std::vector<double> res, best_local_res;
    std::vector<Obs> sample(2), inl;
    std::vector<size_t> comb(n);  // CombinationSampler: the first two entries are the sample, next_combination order
    for (size_t i = 0; i < n; ++i) comb[i] = i;
    for (report.num_trials = 0; report.num_trials < max_num_trials; ++report.num_trials) {
        if (abort) {
            report.num_trials += 1;
            break;
        }
        sample[0] = obs[comb[0]];
        sample[1] = obs[comb[1]];
        // next combination of 2 out of n in lexicographic order; after the last one, back to (0, 1)
        if (comb[1] + 1 < n) {
            comb[1] += 1;
        } else if (comb[0] + 2 < n) {
            comb[0] += 1;
            comb[1] = comb[0] + 1;
        } else {
            comb[0] = 0;
            comb[1] = 1;
        }
        const std::vector<Vec3> models = est.Estimate(sample);
        if (tr && models.empty()) (tr->why == 1 ? tr->depth_rejects : tr->angle_rejects) += 1;
        for (const Vec3& m : models) {
            est.Residuals(obs, m, &res);
            const Support support = Evaluate(res, max_residual);
            if (Better(support, best_support)) {
                best_support = support;
                best_model = m;
                if (tr) {
                    tr->angle = tr->last_angle;
                    have_model = true;
                }
                if (support.num_inliers > 2) {
                    if (tr) tr->lo_rounds += 1;
                    int64_t iters = 0, growing = 0;
                    for (size_t lt = 0; lt < 10; ++lt) {
                        iters += 1;
                        inl.clear();
                        for (size_t i = 0; i < n; ++i)
                            if (res[i] <= max_residual) inl.push_back(obs[i]);
                        const size_t prev = best_support.num_inliers;
                        const std::vector<Vec3> local_models = est.Estimate(inl);
                        if (tr && local_models.empty()) tr->lo_refused += 1;
                        for (const Vec3& lm : local_models) {
                            est.Residuals(obs, lm, &res);
                            const Support ls = Evaluate(res, max_residual);
                            if (Better(ls, best_support)) {
                                best_support = ls;
                                best_model = lm;
                                std::swap(res, best_local_res);
                                if (tr) {
                                    tr->lo_replaced += 1;
                                    tr->angle = tr->last_angle;
                                }
                            }
                        }
                        if (tr) {
                            tr->lo_iters += 1;
                            tr->lo_max_iters = std::max(tr->lo_max_iters, iters);
                        }
                        if (best_support.num_inliers <= prev) break;
                        growing += 1;
                        if (tr) tr->lo_max_growing = std::max(tr->lo_max_growing, growing);
                        std::swap(res, best_local_res);
                    }
                }
                dyn_max_num_trials = ComputeNumTrials(best_support.num_inliers, n, o.confidence, o.multiplier);
            }
            if (report.num_trials >= dyn_max_num_trials && report.num_trials >= static_cast<size_t>(o.min_num_trials)) {
                abort = true;
                if (tr) tr->abort_trial = static_cast<int64_t>(report.num_trials);
                break;
            }
        }
    }
    report.support = best_support;
    if (best_support.num_inliers < 2) {
        if (tr && !have_model) tr->angle = tr->last_angle;
        return report;
    }
    report.success = true;
    report.model = best_model;
    est.Residuals(obs, best_model, &res);
    if (final_res) *final_res = res;
    for (size_t i = 0; i < n; ++i) report.mask[i] = res[i] <= max_residual;
    return report;
}

int Run(const double* poses, size_t nposes, const uint64_t* offsets, size_t ntracks, const uint32_t* obs_pose,
        const double* obs_xy, const Options& o, double* xyz, uint8_t* success, uint32_t* num_inliers,
        uint64_t* num_trials, uint8_t* mask, int64_t* trace, double* trace_angle, double* trace_residuals) {
    if (offsets[0] != 0) return -1;
    std::vector<Pose> ps(nposes);
    for (size_t i = 0; i < nposes; ++i) {
        Pose& p = ps[i];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) p.P[r][c] = poses[12 * i + 4 * r + c];
        // 11.1: C = -R^T t
        for (int c = 0; c < 3; ++c) p.C[c] = -(p.P[0][c] * p.P[0][3] + p.P[1][c] * p.P[1][3] + p.P[2][c] * p.P[2][3]);
    }
    std::vector<Obs> obs;
    std::vector<double> final_res;
    for (size_t t = 0; t < ntracks; ++t) {
        if (offsets[t + 1] < offsets[t]) return -1;
        obs.clear();
        for (uint64_t k = offsets[t]; k < offsets[t + 1]; ++k) {
            if (obs_pose[k] >= nposes) return -1;
            obs.push_back(Obs{obs_xy[2 * k], obs_xy[2 * k + 1], &ps[obs_pose[k]]});
        }
        Trace tr;
        final_res.assign(obs.size(), std::numeric_limits<double>::quiet_NaN());
        const Report r = trace ? LoRansac(o, obs, &tr, &final_res) : LoRansac(o, obs);
        for (int c = 0; c < 3; ++c) xyz[3 * t + c] = r.success ? r.model.v[c] : 0.0;
        success[t] = r.success ? 1 : 0;
        num_inliers[t] = static_cast<uint32_t>(r.support.num_inliers);
        num_trials[t] = r.num_trials;
        for (size_t k = 0; k < obs.size(); ++k) mask[offsets[t] + k] = r.mask[k];
        if (trace) {
            const int64_t v[kTraceInts] = {tr.dyn_row,        tr.abort_trial, tr.depth_rejects, tr.angle_rejects,
                                           tr.lo_rounds,      tr.lo_max_iters, tr.lo_max_growing, tr.lo_iters,
                                           tr.lo_replaced,    tr.lo_refused,  tr.nan};
            for (int c = 0; c < kTraceInts; ++c) trace[kTraceInts * t + c] = v[c];
            trace_angle[t] = tr.angle;
            for (size_t k = 0; k < obs.size(); ++k) trace_residuals[offsets[t] + k] = final_res[k];
        }
    }
    return 0;
}

}  // namespace

extern "C" {

double tri_ref_acos(double x) { return Acos(x); }

double tri_ref_angle(const double* c1, const double* c2, const double* X) {
    return TriAngle(c1, c2, Vec3{{X[0], X[1], X[2]}});
}

// poses: nposes x 12 ([R | t] row-major).  Outputs as amc_triangulate_tracks has them.  Returns 0, or -1 for invalid
// input.
int tri_ref_triangulate(const double* poses, size_t nposes, const uint64_t* offsets, size_t ntracks,
                        const uint32_t* obs_pose, const double* obs_xy, double min_tri_angle, double max_error,
                        double min_inlier_ratio, double confidence, double multiplier, int64_t min_num_trials,
                        int64_t max_num_trials, double* xyz, uint8_t* success, uint32_t* num_inliers,
                        uint64_t* num_trials, uint8_t* mask) {
    const Options o{min_tri_angle, max_error, min_inlier_ratio, confidence, multiplier, min_num_trials, max_num_trials};
    return Run(poses, nposes, offsets, ntracks, obs_pose, obs_xy, o, xyz, success, num_inliers, num_trials, mask,
               nullptr, nullptr, nullptr);
}

// The same, and what each track's RANSAC went through: trace, ntracks x 11 (struct Trace's integers in its order);
// trace_angle, one per track (Trace::angle); trace_residuals, one per observation: the final model's residuals (NaN in
// a track without one).
int tri_ref_triangulate_trace(const double* poses, size_t nposes, const uint64_t* offsets, size_t ntracks,
                              const uint32_t* obs_pose, const double* obs_xy, double min_tri_angle, double max_error,
                              double min_inlier_ratio, double confidence, double multiplier, int64_t min_num_trials,
                              int64_t max_num_trials, double* xyz, uint8_t* success, uint32_t* num_inliers,
                              uint64_t* num_trials, uint8_t* mask, int64_t* trace, double* trace_angle,
                              double* trace_residuals) {
    const Options o{min_tri_angle, max_error, min_inlier_ratio, confidence, multiplier, min_num_trials, max_num_trials};
    return Run(poses, nposes, offsets, ntracks, obs_pose, obs_xy, o, xyz, success, num_inliers, num_trials, mask, trace,
               trace_angle, trace_residuals);
}

}  // extern "C"
