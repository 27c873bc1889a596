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
// track's own bytes of the output mask until the final mask overwrites them.  The device functions live in tri_core.h,
// which the incremental triangulator's kernel (triobs.hip) includes too.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "amc_internal.h"
#include "pose_math.h"
#include "tri_core.h"
#include "../../include/amc_tri.h"

using namespace amc;

namespace {

using tri::kNoTable;
using tri::TriPose;
using tri::TriSupport;

constexpr int kBlock = 256;
// device batch bounds: a call with more observations or tracks is split into several launches on the same buffers
constexpr uint64_t kMaxBatchObs = (uint64_t)1 << 23;
constexpr uint64_t kMaxBatchTracks = (uint64_t)1 << 20;

struct TriParams {
    const uint64_t* off;      // batch tracks + 1: the caller's observation offsets (obs_base = the batch's first)
    const uint32_t* order;    // batch tracks: batch-local track index, longest tracks first
    const uint32_t* pose_idx; // the batch's observations, batch-local index
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
    // tri_core.h's view of the batch's observations
    __device__ __forceinline__ double x(uint64_t o) const { return xy[2 * o]; }
    __device__ __forceinline__ double y(uint64_t o) const { return xy[2 * o + 1]; }
    __device__ __forceinline__ const TriPose& pose(uint64_t o) const { return poses[this->pose_idx[o]]; }
};

// ---- the estimator and the LO-RANSAC are tri_core.h's ---------------------------------------------
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
        const uint64_t tab = n < p.dyn_n ? p.dyn_off[n] : kNoTable;
        trial = tri::tri_lo_ransac(p, o0, n, p.max_trials, p.min_trials, tab == kNoTable ? nullptr : p.dyn_tab + tab,
                                   best_xyz, best);
    }
    const bool ok = best.cnt >= 2;
    if (ok) {
        tri::tri_score(p, o0, n, best_xyz, true);
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
    // (the test hooks are read before anything can fail, once per call: smaller batch bounds, the same results)
    const uint64_t max_batch_tracks = (uint64_t)env_int("AMC_TRI_BATCH_TRACKS", (long long)kMaxBatchTracks, 1, (long long)kMaxBatchTracks);
    const uint64_t max_batch_obs = (uint64_t)env_int("AMC_TRI_BATCH_OBS", (long long)kMaxBatchObs, 1, (long long)kMaxBatchObs);
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
    // is a batch of its own); AMC_TRI_BATCH_TRACKS and AMC_TRI_BATCH_OBS lower the bounds
    const Batches batches = split_batches(track_offsets, ntracks, max_batch_tracks, max_batch_obs);
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
        p.pose_idx = d_opose;
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
