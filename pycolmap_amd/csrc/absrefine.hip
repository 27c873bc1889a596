// absrefine.hip — absolute pose with a variable camera on gfx950 (include/amc_absrefine.h): COLMAP 3.9.1's
// RefineAbsolutePose with refine_focal_length / refine_extra_params honoured, restated in DESIGN.md section 25.  The
// numerics are absrefine_core.h's, the host planning absrefine_plan.h's; this file is the kernel and the C entry points.
//
// Work split (25.4).  One 64-lane wave refines one query, the lanes over its inliers.  The kernel is a template on NV,
// the number of variable camera columns, so that the solver's loops over its 6 + NV columns are compile-time; a batch's
// queries are grouped by NV on the host and each group gets one launch.  A query's result depends on its own inputs
// only.  No atomics.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "amc_internal.h"
#include "absrefine_core.h"
#include "absrefine_plan.h"
#include "abspose_plan.h"
#include "../../include/amc_absrefine.h"

using namespace amc;

namespace {

constexpr int kWave = 64;

struct Launch {
    const uint32_t* order;   // this launch's batch-local query indices
    const uint64_t* qcorr0;  // batch-local first correspondence of each query
    const uint32_t* qn;
    const double* xy;
    const double* X;
    const uint8_t* mask;
    const int32_t* qmodel;
    const double* qparams;   // nq x kMaxParams
    const double* init_q;
    const double* init_t;
    double gradient_tolerance;
    int64_t max_num_iterations;
    double loss_scale;
    int covariance;
    int refine_focal;
    int refine_extra;
    uint8_t* o_success;
    double* o_q;
    double* o_t;
    double* o_prm;
    double* o_cov;           // nq x 36, or null
};

template <int NV>
__global__ __launch_bounds__(kWave) void absrefine_kernel(Launch p) {
    const uint32_t qi = p.order[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const uint64_t c0 = p.qcorr0[qi];
    apr::Query Q;
    Q.model = p.qmodel[qi];
    for (int i = 0; i < 10; ++i) Q.idx[i] = -1;
    apr::variable_params(Q.model, p.refine_focal != 0, p.refine_extra != 0, Q.idx);  // NV of them (the host's grouping)
    Q.xy = p.xy + 2 * c0;
    Q.X = p.X + 3 * c0;
    Q.mask = p.mask + c0;
    Q.n = p.qn[qi];
    double q[4], t[3], prm[cam::kMaxParams];
    for (int i = 0; i < 4; ++i) q[i] = p.init_q[4 * qi + i];
    for (int i = 0; i < 3; ++i) t[i] = p.init_t[3 * qi + i];
    for (int i = 0; i < cam::kMaxParams; ++i) prm[i] = p.qparams[cam::kMaxParams * qi + i];
    const apr::LmOpts lm{p.gradient_tolerance, p.max_num_iterations, p.loss_scale, p.covariance != 0};
    apr::Out r;
    apr::refine_k<NV>(Q, lm, q, t, prm, r);
    if (lane == 0) {
        p.o_success[qi] = r.success ? 1 : 0;
        for (int i = 0; i < 4; ++i) p.o_q[4 * qi + i] = r.q[i];
        for (int i = 0; i < 3; ++i) p.o_t[3 * qi + i] = r.t[i];
        for (int i = 0; i < cam::kMaxParams; ++i) p.o_prm[cam::kMaxParams * qi + i] = r.success ? r.prm[i] : prm[i];
        if (p.o_cov)
            for (int i = 0; i < 36; ++i) p.o_cov[36 * qi + i] = r.cov[i];
    }
}

void launch_class(int nv, unsigned nblocks, hipStream_t st, const Launch& p) {
    switch (nv) {
#define AMC_ABSREFINE_CASE(N)                                                                   \
    case N:                                                                                     \
        hipLaunchKernelGGL(absrefine_kernel<N>, dim3(nblocks), dim3(kWave), 0, st, p);          \
        break;
        AMC_ABSREFINE_CASE(0)
        AMC_ABSREFINE_CASE(1)
        AMC_ABSREFINE_CASE(2)
        AMC_ABSREFINE_CASE(3)
        AMC_ABSREFINE_CASE(4)
        AMC_ABSREFINE_CASE(6)
        AMC_ABSREFINE_CASE(8)
        AMC_ABSREFINE_CASE(10)
#undef AMC_ABSREFINE_CASE
        default: break;  // 5, 7, 9: no model has that many variable parameters
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
void result_alloc(amc_absrefine_result* r, size_t nq, uint64_t ncorr, bool cov) {
    const size_t q = std::max<size_t>(nq, 1);
    r->nqueries = nq;
    r->ncorr = ncorr;
    r->success = static_cast<uint8_t*>(std::calloc(q, 1));
    r->qvec = static_cast<double*>(std::calloc(q * 4, sizeof(double)));
    r->tvec = static_cast<double*>(std::calloc(q * 3, sizeof(double)));
    r->num_inliers = static_cast<uint32_t*>(std::calloc(q, sizeof(uint32_t)));
    r->num_trials = static_cast<uint64_t*>(std::calloc(q, sizeof(uint64_t)));
    r->focal_factor = static_cast<double*>(std::calloc(q, sizeof(double)));
    r->covariance = cov ? static_cast<double*>(std::calloc(q * 36, sizeof(double))) : nullptr;
    r->inlier_mask = static_cast<uint8_t*>(std::calloc(std::max<uint64_t>(ncorr, 1), 1));
    r->camera_params = static_cast<double*>(std::calloc(q * cam::kMaxParams, sizeof(double)));
}
bool result_ok(const amc_absrefine_result* r, bool cov) {
    return r->success && r->qvec && r->tvec && r->num_inliers && r->num_trials && r->focal_factor && r->inlier_mask &&
           r->camera_params && (!cov || r->covariance);
}

// the joint refinement of checked input on the device: success, qvec, tvec, camera_params and covariance of `result`.
// cparams holds kMaxParams doubles per query, zero past the model's own.
int refine_run(const char* fn, amc_ctx* ctx, const uint64_t* offsets, size_t nq, const int32_t* models,
               const double* cparams, const double* points2D, const double* points3D, const double* init_q,
               const double* init_t, const uint8_t* mask, const amc_abspose_refine_opts& ro, bool cov,
               amc_absrefine_result* result) {
    const char* const hipchk_who = fn;
    const uint64_t max_q = (uint64_t)env_int("AMC_ABSREFINE_BATCH_QUERIES", (long long)apr::kMaxBatchQueries, 1,
                                             (long long)apr::kMaxBatchQueries);
    const std::vector<size_t> bstart = apr::plan_batches(offsets, nq, max_q, apr::kMaxBatchCorr);
    const size_t nbatch = bstart.size() - 1;
    uint64_t max_bq = 1, max_bc = 1;
    for (size_t bi = 0; bi < nbatch; ++bi) {
        max_bq = std::max<uint64_t>(max_bq, bstart[bi + 1] - bstart[bi]);
        max_bc = std::max<uint64_t>(max_bc, offsets[bstart[bi + 1]] - offsets[bstart[bi]]);
    }
    const CtxView cv = ctx_view(ctx);
    HIPCHK(hipSetDevice(cv.device));
    hipStream_t st = cv.stream;
    StreamTimer timer(st);
    HIPCHK(timer.start());
    uint32_t *d_qn, *d_qord;
    double *d_xy, *d_X, *d_qprm, *d_iq, *d_it, *d_oq, *d_ot, *d_oprm, *d_ocov;
    uint8_t *d_mask, *d_osucc;
    uint64_t* d_qc0;
    int32_t* d_qmod;
    DevBuf<void> mem;
    HIPCHK(DevParts()
               .part(&d_xy, 2 * max_bc)
               .part(&d_X, 3 * max_bc)
               .part(&d_mask, max_bc)
               .part(&d_qc0, max_bq)
               .part(&d_qn, max_bq)
               .part(&d_qord, max_bq)
               .part(&d_qmod, max_bq)
               .part(&d_qprm, max_bq * cam::kMaxParams)
               .part(&d_iq, 4 * max_bq)
               .part(&d_it, 3 * max_bq)
               .part(&d_osucc, max_bq)
               .part(&d_oq, 4 * max_bq)
               .part(&d_ot, 3 * max_bq)
               .part(&d_oprm, max_bq * cam::kMaxParams)
               .part(&d_ocov, 36 * max_bq)
               .carve(mem));
    // host copies stay alive until the stream is drained
    struct BatchHost {
        std::vector<uint64_t> qc0;
        std::vector<uint32_t> qn;
        apr::BatchClasses cls;
    };
    std::vector<BatchHost> hb(nbatch);
    for (size_t bi = 0; bi < nbatch; ++bi) {
        BatchHost& H = hb[bi];
        const size_t q0 = bstart[bi], q1 = bstart[bi + 1], bq = q1 - q0;
        const uint64_t ob = offsets[q0], bc = offsets[q1] - ob;
        H.qc0.resize(bq);
        H.qn.resize(bq);
        for (size_t i = 0; i < bq; ++i) {
            H.qc0[i] = offsets[q0 + i] - ob;
            H.qn[i] = (uint32_t)(offsets[q0 + i + 1] - offsets[q0 + i]);
        }
        H.cls = apr::plan_classes(offsets, models, q0, q1, ro.refine_focal_length != 0, ro.refine_extra_params != 0);
        HIPCHK(hipMemcpyAsync(d_qc0, H.qc0.data(), bq * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_qn, H.qn.data(), bq * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_qord, H.cls.order.data(), bq * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_qmod, models + q0, bq * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_qprm, cparams + cam::kMaxParams * q0, bq * 8 * cam::kMaxParams, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_iq, init_q + 4 * q0, bq * 32, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_it, init_t + 3 * q0, bq * 24, hipMemcpyHostToDevice, st));
        if (bc) {
            HIPCHK(hipMemcpyAsync(d_xy, points2D + 2 * ob, bc * 16, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_X, points3D + 3 * ob, bc * 24, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_mask, mask + ob, bc, hipMemcpyHostToDevice, st));
        }
        Launch p{};
        p.qcorr0 = d_qc0;
        p.qn = d_qn;
        p.xy = d_xy;
        p.X = d_X;
        p.mask = d_mask;
        p.qmodel = d_qmod;
        p.qparams = d_qprm;
        p.init_q = d_iq;
        p.init_t = d_it;
        p.gradient_tolerance = ro.gradient_tolerance;
        p.max_num_iterations = ro.max_num_iterations;
        p.loss_scale = ro.loss_function_scale;
        p.covariance = cov ? 1 : 0;
        p.refine_focal = ro.refine_focal_length != 0;
        p.refine_extra = ro.refine_extra_params != 0;
        p.o_success = d_osucc;
        p.o_q = d_oq;
        p.o_t = d_ot;
        p.o_prm = d_oprm;
        p.o_cov = cov ? d_ocov : nullptr;
        HIPCHK(timer.span_begin());
        for (int nv = 0; nv <= apr::kMaxNV; ++nv) {
            const uint32_t b = H.cls.begin[nv], e = H.cls.begin[nv + 1];
            if (e == b) continue;
            p.order = d_qord + b;
            launch_class(nv, e - b, st, p);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(timer.span_end());
        HIPCHK(hipMemcpyAsync(result->success + q0, d_osucc, bq, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(result->qvec + 4 * q0, d_oq, bq * 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(result->tvec + 3 * q0, d_ot, bq * 24, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(result->camera_params + cam::kMaxParams * q0, d_oprm, bq * 8 * cam::kMaxParams,
                              hipMemcpyDeviceToHost, st));
        if (cov) HIPCHK(hipMemcpyAsync(result->covariance + 36 * q0, d_ocov, bq * 288, hipMemcpyDeviceToHost, st));
        if (nbatch > 1) HIPCHK(hipStreamSynchronize(st));  // the next batch reuses the buffers the copies read
    }
    HIPCHK(timer.stop(result->device_ms));
    HIPCHK(timer.spans(result->kernel_ms));
    result->num_batches = (uint32_t)nbatch;
    return AMC_OK;
}

int run_impl(const char* fn, amc_ctx* ctx, bool estimate, const uint64_t* offsets, size_t nq, const int32_t* models,
             const double* cparams, const double* points2D, const double* points3D, const double* init_q,
             const double* init_t, const uint8_t* in_mask, const amc_abspose_opts* eo,
             const amc_abspose_refine_opts* ro_in, int want_cov, amc_absrefine_result* result) {
    if (result) std::memset(result, 0, sizeof *result);
    if (!ctx || !result || !offsets || !ro_in || (estimate && !eo)) return api_fail(AMC_E_INVALID, "%s: NULL argument", fn);
    const amc_abspose_refine_opts ro = *ro_in;
    std::string bad = estimate ? ap::check_estimation(*eo) : std::string();
    if (bad.empty()) bad = apr::check_refinement(ro);
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: invalid options: %s", fn, bad.c_str());
    bad = apr::check_input(estimate, offsets, nq, models, cparams, points2D, points3D, init_q, init_t, in_mask);
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: %s", fn, bad.c_str());
    const uint64_t ncorr = offsets[nq];
    const bool cov = want_cov != 0;
    result_alloc(result, nq, ncorr, cov);
    if (!result_ok(result, cov)) return api_fail(AMC_E_NOMEM, "%s: out of host memory for %zu queries", fn, nq);
    if (nq == 0) return AMC_OK;

    std::vector<double> prm(nq * cam::kMaxParams);
    if (!estimate) {
        for (size_t i = 0; i < nq; ++i)
            ap::scaled_params(models[i], cparams + cam::kMaxParams * i, 1.0, &prm[cam::kMaxParams * i]);
        const int rc = refine_run(fn, ctx, offsets, nq, models, prm.data(), points2D, points3D, init_q, init_t, in_mask,
                                  ro, cov, result);
        if (rc != AMC_OK) return rc;
        for (size_t i = 0; i < nq; ++i) {  // the input mask and its count
            uint32_t c = 0;
            for (uint64_t k = offsets[i]; k < offsets[i + 1]; ++k) c += in_mask[k] ? 1 : 0;
            result->num_inliers[i] = c;
            result->focal_factor[i] = 1.0;
        }
        if (ncorr) std::memcpy(result->inlier_mask, in_mask, ncorr);
        return AMC_OK;
    }
    // COLMAP's flow (25.3): the LO-RANSAC of 12.6 per focal factor, whose pose amc_estimate_absolute_poses returns
    // unchanged when its refinement has no iterations; then one joint refinement with the camera scaled by the factor
    amc_abspose_refine_opts r0 = ro;
    r0.max_num_iterations = 0;
    r0.refine_focal_length = 0;
    r0.refine_extra_params = 0;
    amc_abspose_result est;
    int rc = amc_estimate_absolute_poses(ctx, offsets, nq, models, cparams, points2D, points3D, eo, &r0, 0, &est);
    if (rc != AMC_OK) return rc;
    for (size_t i = 0; i < nq; ++i) {
        const double f = est.focal_factor[i];
        ap::scaled_params(models[i], cparams + cam::kMaxParams * i, f != 0.0 ? f : 1.0, &prm[cam::kMaxParams * i]);
        result->num_inliers[i] = est.num_inliers[i];
        result->num_trials[i] = est.num_trials[i];
        result->focal_factor[i] = f;
    }
    if (ncorr) std::memcpy(result->inlier_mask, est.inlier_mask, ncorr);
    // a query whose estimation failed is refined over no correspondence (nothing changes) and stays failed
    std::vector<uint8_t> mask(std::max<uint64_t>(ncorr, 1), 0);
    for (size_t i = 0; i < nq; ++i)
        if (est.success[i])
            for (uint64_t k = offsets[i]; k < offsets[i + 1]; ++k) mask[k] = est.inlier_mask[k];
    rc = refine_run(fn, ctx, offsets, nq, models, prm.data(), points2D, points3D, est.qvec, est.tvec, mask.data(), ro,
                    cov, result);
    if (rc == AMC_OK) {
        for (size_t i = 0; i < nq; ++i)
            if (!est.success[i]) {
                result->success[i] = 0;
                if (cov)
                    for (int k = 0; k < 36; ++k) result->covariance[36 * i + k] = 0.0;
            }
        result->device_ms += est.device_ms;
        result->kernel_ms += est.kernel_ms;
    }
    amc_abspose_result_free(&est);
    return rc;
}

}  // namespace

extern "C" {

void amc_absrefine_result_free(amc_absrefine_result* r) {
    if (!r) return;
    std::free(r->success);
    std::free(r->qvec);
    std::free(r->tvec);
    std::free(r->num_inliers);
    std::free(r->num_trials);
    std::free(r->focal_factor);
    std::free(r->covariance);
    std::free(r->inlier_mask);
    std::free(r->camera_params);
    std::memset(r, 0, sizeof *r);
}

int amc_refine_poses_and_cameras(amc_ctx* ctx, const uint64_t* offsets, size_t nqueries, const int32_t* camera_models,
                                 const double* camera_params, const double* points2D, const double* points3D,
                                 const double* init_qvec, const double* init_tvec, const uint8_t* inlier_mask,
                                 const amc_abspose_refine_opts* refinement_options, int return_covariance,
                                 amc_absrefine_result* result) {
    const int rc = run_impl("amc_refine_poses_and_cameras", ctx, false, offsets, nqueries, camera_models, camera_params,
                            points2D, points3D, init_qvec, init_tvec, inlier_mask, nullptr, refinement_options,
                            return_covariance, result);
    if (rc != AMC_OK && result) amc_absrefine_result_free(result);  // no partial results
    return rc;
}

int amc_estimate_poses_and_cameras(amc_ctx* ctx, const uint64_t* offsets, size_t nqueries,
                                   const int32_t* camera_models, const double* camera_params, const double* points2D,
                                   const double* points3D, const amc_abspose_opts* estimation_options,
                                   const amc_abspose_refine_opts* refinement_options, int return_covariance,
                                   amc_absrefine_result* result) {
    const int rc = run_impl("amc_estimate_poses_and_cameras", ctx, true, offsets, nqueries, camera_models,
                            camera_params, points2D, points3D, nullptr, nullptr, nullptr, estimation_options,
                            refinement_options, return_covariance, result);
    if (rc != AMC_OK && result) amc_absrefine_result_free(result);
    return rc;
}

}  // extern "C"
