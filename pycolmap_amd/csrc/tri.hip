// tri.hip — track triangulation on gfx950 (include/amc_tri.h): COLMAP 3.9.1's EstimateTriangulation with the angular
// residual, one LO-RANSAC per track, restated in DESIGN.md section 11.  Every FP64 operation below is written in the
// order of that section, the order tests/tri_ref/tri_ref.cc follows too: the two are bit-identical.  acos is the
// project's own (+ - * /, correctly rounded sqrt), both eigen problems use the round-robin Jacobi solver of D1
// (pose_math.h), and the dynamic trial count comes from a host-built table (host libm), as in verification.
//
// Work split: one lane runs one track's whole RANSAC.  The host orders each batch's tracks by length, longest first
// (a counting sort, "binning"), so that the 64 tracks of a wave have the same length and finish together; a track's
// result depends on its own observations only, never on its neighbours, the batch or the order.  No atomics, no LDS,
// no scratch: the lane's state is a few dozen registers, and the inlier set of a local optimisation is kept in the
// track's own bytes of the output mask until the final mask overwrites them.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "amc_internal.h"
#include "pose_math.h"
#include "tri_angle.h"
#include "../../include/amc_tri.h"

using namespace amc;

namespace {

using tvg::dsqrt;
using tri::tri_acos;
using tri::tri_angle;

constexpr uint64_t kNoTable = ~(uint64_t)0;
constexpr int kBlock = 256;
// device batch bounds: a call with more observations or tracks is split into several launches on the same buffers
constexpr uint64_t kMaxBatchObs = (uint64_t)1 << 23;
constexpr uint64_t kMaxBatchTracks = (uint64_t)1 << 20;

// one pose: cam_from_world [R | t] row-major, the projection centre -R^T t, padding to 128 bytes
struct TriPose {
    double P[12];
    double C[3];
    double pad;
};

struct TriParams {
    const uint64_t* off;      // batch tracks + 1: the caller's observation offsets (obs_base = the batch's first)
    const uint32_t* order;    // batch tracks: batch-local track index, longest tracks first
    const uint32_t* pose;     // the batch's observations, batch-local index
    const double* xy;         // 2 per observation
    const TriPose* poses;
    const uint64_t* dyn_off;  // by track length (< dyn_n): start of its dyn_max_num_trials row in dyn_tab, or kNoTable
    const uint64_t* dyn_tab;  // row of length n: ComputeNumTrials(num_inliers, n) for num_inliers = 0 .. n
    uint64_t dyn_n;
    uint64_t obs_base;
    uint32_t ntracks;
    double max_residual;      // max_error^2
    double min_tri_angle;
    uint64_t min_trials;
    uint64_t max_trials;      // RANSACOptions::max_num_trials after the RANSAC constructor's clamp
    double* xyz;              // batch tracks x 3
    uint32_t* num_inliers;
    uint64_t* num_trials;
    uint8_t* success;
    uint8_t* mask;            // the batch's observations
};

// ---- numerics (acos and the triangulation angle: tri_angle.h) -----------------------------------------
// P.row(2) . [X; 1]
__device__ __forceinline__ double tri_depth(const double* P, const double* X) {
    return P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
}

// squared angular error of observation (x, y) under pose P for the point X
__device__ __forceinline__ double tri_residual(double x, double y, const double* P, const double* X) {
    const double na = dsqrt(x * x + y * y + 1.0);
    const double a0 = x / na, a1 = y / na, a2 = 1.0 / na;
    const double q0 = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
    const double q1 = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
    const double q2 = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
    const double nb = dsqrt(q0 * q0 + q1 * q1 + q2 * q2);
    const double c = a0 * (q0 / nb) + a1 * (q1 / nb) + a2 * (q2 / nb);
    const double e = tri_acos(c);
    return e * e;
}

// eigenvector of the smallest eigenvalue of the symmetric 4 x 4 `a` (first minimum of the Jacobi diagonal), dehomogenised
__device__ __forceinline__ void tri_smallest_dehom(double (&a)[16], double* X) {
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
__device__ __forceinline__ bool tri_estimate_two(const TriParams& p, uint64_t i, uint64_t j, double* X) {
    const double xi = p.xy[2 * i], yi = p.xy[2 * i + 1], xj = p.xy[2 * j], yj = p.xy[2 * j + 1];
    const TriPose& Pi = p.poses[p.pose[i]];
    const TriPose& Pj = p.poses[p.pose[j]];
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

// (observation indices below are batch-local)
// the local estimator on the inlier set marked in mask[o0 .. o0 + n) (cnt >= 2 members): two members -> the two-view
// estimator; more -> A = sum term^T term, term = P - p p^T P, p = normalized([x, y, 1]); every depth, then any pair
// (i, j < i) with the angle
__device__ __forceinline__ bool tri_estimate_set(const TriParams& p, uint64_t o0, uint64_t n, uint32_t cnt, double* X) {
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
        const double x = p.xy[2 * o], y = p.xy[2 * o + 1];
        const double* P = p.poses[p.pose[o]].P;
        const double nrm = dsqrt(x * x + y * y + 1.0);
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
        if (set[k] && !(tri_depth(p.poses[p.pose[o0 + k]].P, X) >= DBL_EPSILON)) return false;
    for (uint64_t i = 1; i < n; ++i) {
        if (!set[i]) continue;
        const double* ci = p.poses[p.pose[o0 + i]].C;
        for (uint64_t j = 0; j < i; ++j) {
            if (!set[j]) continue;
            if (tri_angle(ci, p.poses[p.pose[o0 + j]].C, X) >= p.min_tri_angle) return true;
        }
    }
    return false;
}

// InlierSupportMeasurer::Evaluate: inliers have residual <= max_residual (NaN is an outlier); the residual sum adds
// the inliers' residuals in observation order.  mark: also write the inlier flags to the track's mask bytes.
struct TriSupport {
    uint32_t cnt;
    double sum;
};
__device__ __forceinline__ TriSupport tri_score(const TriParams& p, uint64_t o0, uint64_t n, const double* X, bool mark) {
    TriSupport s{0u, 0.0};
    uint8_t* m = p.mask + o0;
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t o = o0 + k;
        const double r = tri_residual(p.xy[2 * o], p.xy[2 * o + 1], p.poses[p.pose[o]].P, X);
        const bool in = r <= p.max_residual;
        if (in) {
            s.cnt += 1;
            s.sum += r;
        }
        if (mark) m[k] = in ? 1 : 0;
    }
    return s;
}
__device__ __forceinline__ bool tri_better(const TriSupport a, const TriSupport b) {
    return a.cnt > b.cnt || (a.cnt == b.cnt && a.sum < b.sum);
}

// ---- LORANSAC<TriangulationEstimator x 2, InlierSupportMeasurer, CombinationSampler> -----------------
__global__ __launch_bounds__(kBlock) void tri_kernel(TriParams p) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= p.ntracks) return;
    const uint32_t t = p.order[g];
    const uint64_t o0 = p.off[t] - p.obs_base, n = p.off[t + 1] - p.off[t];
    uint8_t* mask = p.mask + o0;
    double best_xyz[3] = {0.0, 0.0, 0.0};
    TriSupport best{0u, DBL_MAX};
    uint64_t trial = 0;
    if (n >= 2) {
        const uint64_t combos = n * (n - 1) / 2;
        const uint64_t max_trials = p.max_trials < combos ? p.max_trials : combos;
        const uint64_t tab = n < p.dyn_n ? p.dyn_off[n] : kNoTable;
        uint64_t dyn_max = max_trials;
        uint64_t a = 0, b = 1;  // the next pair of the lexicographic combination order
        bool abort = false;
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
                dyn_max = tab == kNoTable ? kNoTable : p.dyn_tab[tab + best.cnt];
            }
            if (trial >= dyn_max && trial >= p.min_trials) abort = true;
        }
    }
    const bool ok = best.cnt >= 2;
    if (ok) {
        tri_score(p, o0, n, best_xyz, true);
    } else {
        for (uint64_t k = 0; k < n; ++k) mask[k] = 0;
    }
    p.xyz[3 * t] = ok ? best_xyz[0] : 0.0;
    p.xyz[3 * t + 1] = ok ? best_xyz[1] : 0.0;
    p.xyz[3 * t + 2] = ok ? best_xyz[2] : 0.0;
    p.num_inliers[t] = best.cnt;
    p.num_trials[t] = trial;
    p.success[t] = ok ? 1 : 0;
}

// ---- host side ------------------------------------------------------------------------------------------------------
constexpr int kMinSamples = 2;  // two views: ComputeNumTrials' kMinNumSamples (tvg_math.h)

}  // namespace

extern "C" {

void amc_tri_opts_default(amc_tri_opts* o) {
    if (!o) return;
    o->min_tri_angle = 0.0;  // EstimateTriangulationOptions() with pycolmap's RANSACOptions()
    o->max_error = 4.0;
    o->min_inlier_ratio = 0.01;
    o->confidence = 0.9999;
    o->dyn_num_trials_multiplier = 3.0;
    o->min_num_trials = 1000;
    o->max_num_trials = 100000;
}

void amc_tri_result_free(amc_tri_result* r) {
    if (!r) return;
    std::free(r->xyz);
    std::free(r->success);
    std::free(r->num_inliers);
    std::free(r->num_trials);
    std::free(r->inlier_mask);
    std::memset(r, 0, sizeof *r);
}

static int triangulate_impl(amc_ctx* ctx, const double* poses, size_t nposes, const uint64_t* track_offsets,
                            size_t ntracks, const uint32_t* obs_pose, const double* obs_xy, const amc_tri_opts* opts,
                            amc_tri_result* result) {
    const char* const hipchk_who = "amc_triangulate_tracks";
    if (!ctx || !opts || !result || !track_offsets || (nposes && !poses))
        return api_fail(AMC_E_INVALID, "amc_triangulate_tracks: NULL argument");
    std::memset(result, 0, sizeof *result);
    const amc_tri_opts op = *opts;
    // EstimateTriangulationOptions::Check and RANSACOptions::Check
    if (!(op.min_tri_angle >= 0.0) || !(op.max_error > 0.0) || !(op.min_inlier_ratio >= 0.0) ||
        !(op.min_inlier_ratio <= 1.0) || !(op.confidence >= 0.0) || !(op.confidence <= 1.0) || op.min_num_trials < 0 ||
        op.max_num_trials < 0 || op.min_num_trials > op.max_num_trials)
        return api_fail(AMC_E_INVALID, "amc_triangulate_tracks: invalid options (min_tri_angle %g, max_error %g, "
                        "min_inlier_ratio %g, confidence %g, min_num_trials %lld, max_num_trials %lld)",
                        op.min_tri_angle, op.max_error, op.min_inlier_ratio, op.confidence,
                        (long long)op.min_num_trials, (long long)op.max_num_trials);
    if (track_offsets[0] != 0) return api_fail(AMC_E_INVALID, "amc_triangulate_tracks: track_offsets[0] != 0");
    for (size_t i = 0; i < ntracks; ++i)
        if (track_offsets[i + 1] < track_offsets[i])
            return api_fail(AMC_E_INVALID, "amc_triangulate_tracks: track_offsets decrease at track %zu", i);
    const uint64_t nobs = track_offsets[ntracks];
    if (nobs && (!obs_pose || !obs_xy)) return api_fail(AMC_E_INVALID, "amc_triangulate_tracks: NULL observations");
    for (uint64_t k = 0; k < nobs; ++k)
        if (obs_pose[k] >= nposes)
            return api_fail(AMC_E_INVALID, "amc_triangulate_tracks: observation %llu names pose %u of %zu",
                            (unsigned long long)k, obs_pose[k], nposes);

    result->ntracks = ntracks;
    result->nobs = nobs;
    result->xyz = static_cast<double*>(std::malloc(std::max<size_t>(ntracks, 1) * 3 * sizeof(double)));
    result->success = static_cast<uint8_t*>(std::malloc(std::max<size_t>(ntracks, 1)));
    result->num_inliers = static_cast<uint32_t*>(std::malloc(std::max<size_t>(ntracks, 1) * sizeof(uint32_t)));
    result->num_trials = static_cast<uint64_t*>(std::malloc(std::max<size_t>(ntracks, 1) * sizeof(uint64_t)));
    result->inlier_mask = static_cast<uint8_t*>(std::malloc(std::max<uint64_t>(nobs, 1)));
    if (!result->xyz || !result->success || !result->num_inliers || !result->num_trials || !result->inlier_mask) {
        amc_tri_result_free(result);
        return api_fail(AMC_E_NOMEM, "amc_triangulate_tracks: out of host memory for %zu tracks", ntracks);
    }
    if (ntracks == 0) return AMC_OK;

    // the pose table with its centres
    std::vector<TriPose> tab(std::max<size_t>(nposes, 1));
    for (size_t i = 0; i < nposes; ++i) {
        TriPose& q = tab[i];
        std::memcpy(q.P, poses + 12 * i, sizeof q.P);
        for (int c = 0; c < 3; ++c) q.C[c] = -(q.P[c] * q.P[3] + q.P[4 + c] * q.P[7] + q.P[8 + c] * q.P[11]);
        q.pad = 0.0;
    }
    const uint64_t max_trials = tvg::ransac_max_trials(op.max_num_trials, op.min_inlier_ratio, op.confidence,
                                                       op.dyn_num_trials_multiplier, kMinSamples);
    const uint64_t min_trials = (uint64_t)op.min_num_trials;

    // dyn_max_num_trials rows for the track lengths whose RANSAC can stop early (more trials than min_num_trials)
    uint64_t nmax = 0;
    for (size_t i = 0; i < ntracks; ++i) nmax = std::max<uint64_t>(nmax, track_offsets[i + 1] - track_offsets[i]);
    std::vector<uint64_t> dyn_off(nmax + 1, kNoTable), dyn_tab;
    for (size_t i = 0; i < ntracks; ++i) {
        const uint64_t n = track_offsets[i + 1] - track_offsets[i];
        if (n < 2 || dyn_off[n] != kNoTable) continue;
        const uint64_t combos = n * (n - 1) / 2;
        if (std::min(max_trials, combos) <= min_trials) continue;
        dyn_off[n] = dyn_tab.size();
        for (uint64_t c = 0; c <= n; ++c)
            dyn_tab.push_back(tvg::compute_num_trials(c, n, op.confidence, op.dyn_num_trials_multiplier, kMinSamples));
    }
    if (dyn_tab.empty()) dyn_tab.push_back(0);

    // batches: contiguous track ranges of at most kMaxBatchTracks tracks and kMaxBatchObs observations (a longer track
    // is a batch of its own)
    const Batches batches = split_batches(track_offsets, ntracks, kMaxBatchTracks, kMaxBatchObs);
    const std::vector<size_t>& bstart = batches.start;
    const size_t nbatch = batches.count();
    const uint64_t max_bt = batches.most_items, max_bo = std::max<uint64_t>(batches.most_elems, 1);

    const CtxView cv = ctx_view(ctx);
    HIPCHK(hipSetDevice(cv.device));
    hipStream_t st = cv.stream;
    StreamTimer timer(st);
    HIPCHK(timer.start());
    // one device allocation: constants, then the batch buffers
    TriPose* d_pose;
    uint64_t *d_doff, *d_dtab, *d_off, *d_ntr;
    uint32_t *d_ord, *d_opose, *d_ninl;
    double *d_xy, *d_xyz;
    uint8_t *d_succ, *d_mask;
    DevBuf<void> mem;
    HIPCHK(DevParts()
               .part(&d_pose, tab.size())
               .part(&d_doff, dyn_off.size())
               .part(&d_dtab, dyn_tab.size())
               .part(&d_off, max_bt + 1)
               .part(&d_ord, max_bt)
               .part(&d_opose, max_bo)
               .part(&d_xy, 2 * max_bo)
               .part(&d_xyz, 3 * max_bt)
               .part(&d_ninl, max_bt)
               .part(&d_ntr, max_bt)
               .part(&d_succ, max_bt)
               .part(&d_mask, max_bo)
               .carve(mem));
    HIPCHK(hipMemcpyAsync(d_pose, tab.data(), tab.size() * sizeof(TriPose), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_doff, dyn_off.data(), dyn_off.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_dtab, dyn_tab.data(), dyn_tab.size() * 8, hipMemcpyHostToDevice, st));

    std::vector<std::vector<uint32_t>> orders(nbatch);  // host copies stay alive until the stream is drained
    for (size_t bi = 0; bi < nbatch; ++bi) {
        const size_t t0 = bstart[bi], t1 = bstart[bi + 1], nt = t1 - t0;
        const uint64_t ob = track_offsets[t0], no = track_offsets[t1] - ob;
        // counting sort by length, longest first (lengths above 64 share the first bin, in track order)
        constexpr int kBins = 66;
        size_t cnt[kBins + 1] = {};
        auto bin_of = [&](size_t t) {
            const uint64_t n = track_offsets[t + 1] - track_offsets[t];
            return n > 64 ? 0 : (int)(65 - n);
        };
        for (size_t t = t0; t < t1; ++t) cnt[bin_of(t) + 1] += 1;
        for (int b = 0; b < kBins; ++b) cnt[b + 1] += cnt[b];
        std::vector<uint32_t>& ord = orders[bi];
        ord.resize(nt);
        for (size_t t = t0; t < t1; ++t) ord[cnt[bin_of(t)]++] = (uint32_t)(t - t0);

        HIPCHK(hipMemcpyAsync(d_off, track_offsets + t0, (nt + 1) * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_ord, ord.data(), nt * 4, hipMemcpyHostToDevice, st));
        if (no) {
            HIPCHK(hipMemcpyAsync(d_opose, obs_pose + ob, no * 4, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_xy, obs_xy + 2 * ob, no * 16, hipMemcpyHostToDevice, st));
        }
        TriParams p{};
        p.off = d_off;
        p.order = d_ord;
        p.pose = d_opose;
        p.xy = d_xy;
        p.poses = d_pose;
        p.dyn_off = d_doff;
        p.dyn_tab = d_dtab;
        p.dyn_n = dyn_off.size();
        p.obs_base = ob;
        p.ntracks = (uint32_t)nt;
        p.max_residual = op.max_error * op.max_error;
        p.min_tri_angle = op.min_tri_angle;
        p.min_trials = min_trials;
        p.max_trials = max_trials;
        p.xyz = d_xyz;
        p.num_inliers = d_ninl;
        p.num_trials = d_ntr;
        p.success = d_succ;
        p.mask = d_mask;
        HIPCHK(timer.span_begin());
        hipLaunchKernelGGL(tri_kernel, dim3((unsigned)((nt + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, p);
        HIPCHK(hipGetLastError());
        HIPCHK(timer.span_end());
        HIPCHK(hipMemcpyAsync(result->xyz + 3 * t0, d_xyz, nt * 24, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(result->num_inliers + t0, d_ninl, nt * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(result->num_trials + t0, d_ntr, nt * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(result->success + t0, d_succ, nt, hipMemcpyDeviceToHost, st));
        if (no) HIPCHK(hipMemcpyAsync(result->inlier_mask + ob, d_mask, no, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(timer.stop(result->device_ms));  // (result was zeroed on entry)
    HIPCHK(timer.spans(result->kernel_ms));
    result->num_batches = (uint32_t)nbatch;
    return AMC_OK;
}

int amc_triangulate_tracks(amc_ctx* ctx, const double* poses, size_t nposes, const uint64_t* track_offsets,
                           size_t ntracks, const uint32_t* obs_pose, const double* obs_xy, const amc_tri_opts* opts,
                           amc_tri_result* result) {
    const int rc = triangulate_impl(ctx, poses, nposes, track_offsets, ntracks, obs_pose, obs_xy, opts, result);
    if (rc != AMC_OK && result) amc_tri_result_free(result);  // no partial results
    return rc;
}

}  // extern "C"
