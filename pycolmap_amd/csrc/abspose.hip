// abspose.hip — absolute pose on gfx950 (include/amc_abspose.h): COLMAP 3.9.1's EstimateAbsolutePose and
// RefineAbsolutePose, restated in DESIGN.md section 12.  The numerics and the control flow are abspose_core.h's, the
// host planning abspose_plan.h's; this file is the two kernels and the C entry points.
//
// Work split (12.11).  Kernel 1 runs one 64-lane wave per (query, focal-length factor): the wave lifts the query's
// pixels with the scaled camera (the polynomial models; the fisheye family and FOV are lifted with host libm, as
// camera_math.h has it), then runs the LO-RANSAC with every sum over correspondences split across the lanes in the
// order of 12.10.  Kernel 2 runs one wave per query: it picks the factor, converts the model to a pose and refines it
// with the lanes over the inliers.  The host orders each batch's waves by correspondence count, largest first, so that
// long problems start early; a query's result depends on its own inputs only.  No atomics.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "amc_internal.h"
#include "abspose_core.h"
#include "abspose_plan.h"
#include "../../include/amc_abspose.h"

using namespace amc;

namespace {

constexpr int kWave = 64;
// device batch bounds: (query, factor) correspondences and queries per launch; a larger call is split into several
// launches on the same buffers
constexpr uint64_t kMaxBatchSlotCorr = (uint64_t)1 << 22;
constexpr uint64_t kMaxBatchQueries = (uint64_t)1 << 16;
constexpr size_t kMaxStreamWords = (size_t)1 << 28;

// one (query, factor) problem of a batch
struct SlotDesc {
    uint64_t corr0;        // batch-local first correspondence
    uint64_t scratch0;     // first entry of the slot's lifted points, permutation and mask
    uint32_t n;
    int32_t model;
    uint32_t lift_on_device;
    uint32_t pad;
    double max_residual;   // CamFromImgThreshold(max_error)^2 of the scaled camera
    double factor;
    double params[cam::kMaxParams];  // the scaled camera
};

struct RansacLaunch {
    const SlotDesc* slots;
    const uint32_t* order;
    uint32_t nslots;
    const double* xy;
    const double* X;
    double* uv;
    uint32_t* perm;
    uint8_t* smask;
    const uint64_t* dyn_off;  // by n (< dyn_n): start of its row in dyn_tab, or kNoRow
    const uint64_t* dyn_tab;
    uint64_t dyn_n;
    const uint32_t* stream;
    uint64_t stream_len;
    uint64_t min_trials;
    uint64_t max_trials;
    uint8_t* s_success;
    uint8_t* s_overrun;
    uint32_t* s_ninl;
    uint64_t* s_ntr;
    double* s_model;
};

__global__ __launch_bounds__(kWave) void abspose_ransac_kernel(RansacLaunch p) {
    const uint32_t s = p.order[blockIdx.x];
    const SlotDesc& d = p.slots[s];
    const int lane = (int)threadIdx.x;
    double* uv = p.uv + 2 * d.scratch0;
    const double* xy = p.xy + 2 * d.corr0;
    if (d.lift_on_device) {
        double prm[cam::kMaxParams];
#pragma unroll
        for (int i = 0; i < cam::kMaxParams; ++i) prm[i] = d.params[i];
        for (uint32_t k = (uint32_t)lane; k < d.n; k += kWave)
            cam::cam_from_img(d.model, prm, xy[2 * k], xy[2 * k + 1], uv[2 * k], uv[2 * k + 1]);
    }
    __syncthreads();
    ap::Problem pr{d.n, uv, p.X + 3 * d.corr0};
    ap::RansacParams rp;
    rp.max_residual = d.max_residual;
    rp.min_trials = p.min_trials;
    rp.max_trials = p.max_trials;
    const uint64_t row = d.n < p.dyn_n ? p.dyn_off[d.n] : ap::kNoRow;
    rp.dyn_row = row == ap::kNoRow ? nullptr : p.dyn_tab + row;
    rp.stream = p.stream;
    rp.stream_len = p.stream_len;
    const ap::RansacOut o = ap::lo_ransac(pr, rp, p.perm + d.scratch0, p.smask + d.scratch0);
    if (lane == 0) {
        p.s_success[s] = o.success ? 1 : 0;
        p.s_overrun[s] = o.overrun ? 1 : 0;
        p.s_ninl[s] = o.num_inliers;
        p.s_ntr[s] = o.num_trials;
        for (int i = 0; i < 12; ++i) p.s_model[12 * s + i] = o.model[i];
    }
}

struct RefineLaunch {
    uint32_t nq;
    int estimate;
    const uint32_t* order;
    const uint64_t* qcorr0;      // batch-local first correspondence of each query
    const uint32_t* qn;
    const double* xy;
    const double* X;
    uint8_t* mask;               // batch correspondences: written (estimation) or read (refinement)
    // estimation
    const uint32_t* slot_begin;  // nq + 1
    const SlotDesc* slots;
    const uint8_t* smask;
    const uint8_t* s_success;
    const uint32_t* s_ninl;
    const uint64_t* s_ntr;
    const double* s_model;
    // refinement
    const int32_t* qmodel;
    const double* qparams;       // nq x kMaxParams
    const double* init_q;
    const double* init_t;
    double gradient_tolerance;
    int64_t max_num_iterations;
    double loss_scale;
    int covariance;
    uint8_t* o_success;
    double* o_q;
    double* o_t;
    uint32_t* o_ninl;
    uint64_t* o_ntr;
    double* o_factor;
    double* o_cov;               // nq x 36, or null
};

__global__ __launch_bounds__(kWave) void abspose_refine_kernel(RefineLaunch p) {
    const uint32_t qi = p.order[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const uint64_t c0 = p.qcorr0[qi];
    const uint32_t n = p.qn[qi];
    double q[4], t[3];
    int model;
    const double* params;
    bool ok = true;
    uint32_t ninl = 0;
    uint64_t ntr = 0;
    double factor = 1.0;
    if (p.estimate) {
        // the first factor with the strictly largest successful inlier count
        int best = -1;
        uint32_t best_cnt = 0;
        for (uint32_t s = p.slot_begin[qi]; s < p.slot_begin[qi + 1]; ++s)
            if (p.s_success[s] && p.s_ninl[s] > best_cnt) {
                best_cnt = p.s_ninl[s];
                best = (int)s;
            }
        const uint32_t pick = best >= 0 ? (uint32_t)best : p.slot_begin[qi];
        const SlotDesc& d = p.slots[pick];
        model = d.model;
        params = d.params;
        ntr = p.s_ntr[pick];
        if (best < 0) {
            ok = false;
            factor = 0.0;
            for (uint32_t k = (uint32_t)lane; k < n; k += kWave) p.mask[c0 + k] = 0;
            for (int i = 0; i < 4; ++i) q[i] = 0.0;
            for (int i = 0; i < 3; ++i) t[i] = 0.0;
        } else {
            ninl = best_cnt;
            factor = d.factor;
            for (uint32_t k = (uint32_t)lane; k < n; k += kWave) p.mask[c0 + k] = p.smask[d.scratch0 + k];
            ok = ap::model_to_pose(p.s_model + 12 * pick, q, t);
        }
    } else {
        model = p.qmodel[qi];
        params = p.qparams + cam::kMaxParams * qi;
        for (int i = 0; i < 4; ++i) q[i] = p.init_q[4 * qi + i];
        for (int i = 0; i < 3; ++i) t[i] = p.init_t[3 * qi + i];
    }
    __syncthreads();
    double cov[36];
    for (int i = 0; i < 36; ++i) cov[i] = 0.0;
    if (ok) {
        double prm[cam::kMaxParams];
        for (int i = 0; i < cam::kMaxParams; ++i) prm[i] = params[i];
        ap::RefineParams rp{model, prm, p.gradient_tolerance, p.max_num_iterations, p.loss_scale, p.covariance != 0};
        const ap::RefineOut r = ap::refine(rp, q, t, p.xy + 2 * c0, p.X + 3 * c0, p.mask + c0, n);
        ok = r.success;
        for (int i = 0; i < 4; ++i) q[i] = r.q[i];
        for (int i = 0; i < 3; ++i) t[i] = r.t[i];
        for (int i = 0; i < 36; ++i) cov[i] = r.cov[i];
    }
    if (lane == 0) {
        p.o_success[qi] = ok ? 1 : 0;
        for (int i = 0; i < 4; ++i) p.o_q[4 * qi + i] = q[i];
        for (int i = 0; i < 3; ++i) p.o_t[3 * qi + i] = t[i];
        p.o_ninl[qi] = ninl;
        p.o_ntr[qi] = ntr;
        p.o_factor[qi] = factor;
        if (p.o_cov)
            for (int i = 0; i < 36; ++i) p.o_cov[36 * qi + i] = cov[i];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
void result_alloc(amc_abspose_result* r, size_t nq, uint64_t ncorr, bool cov) {
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
}
bool result_ok(const amc_abspose_result* r, bool cov) {
    return r->success && r->qvec && r->tvec && r->num_inliers && r->num_trials && r->focal_factor && r->inlier_mask &&
           (!cov || r->covariance);
}

int run_impl(const char* fn, amc_ctx* ctx, bool estimate, const uint64_t* offsets, size_t nq, const int32_t* models,
             const double* cparams, const double* points2D, const double* points3D, const double* init_q,
             const double* init_t, const uint8_t* in_mask, const amc_abspose_opts* eo_in,
             const amc_abspose_refine_opts* ro_in, int want_cov, amc_abspose_result* result) {
    const char* const hipchk_who = fn;
    if (!ctx || !result || !offsets || !ro_in || (estimate && !eo_in))
        return api_fail(AMC_E_INVALID, "%s: NULL argument", fn);
    std::memset(result, 0, sizeof *result);
    const amc_abspose_refine_opts ro = *ro_in;
    amc_abspose_opts eo;
    amc_abspose_opts_default(&eo);
    if (estimate) eo = *eo_in;
    std::string bad = estimate ? ap::check_estimation(eo) : std::string();
    if (bad.empty()) bad = ap::check_refinement(ro);
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: invalid options: %s", fn, bad.c_str());
    if (offsets[0] != 0) return api_fail(AMC_E_INVALID, "%s: offsets[0] != 0", fn);
    for (size_t i = 0; i < nq; ++i) {
        if (offsets[i + 1] < offsets[i]) return api_fail(AMC_E_INVALID, "%s: offsets decrease at query %zu", fn, i);
        if (offsets[i + 1] - offsets[i] > 0xffffffffull)
            return api_fail(AMC_E_INVALID, "%s: query %zu has more than 2^32 - 1 correspondences", fn, i);
    }
    const uint64_t ncorr = offsets[nq];
    if (nq && (!models || !cparams)) return api_fail(AMC_E_INVALID, "%s: NULL cameras", fn);
    if (ncorr && (!points2D || !points3D)) return api_fail(AMC_E_INVALID, "%s: NULL points", fn);
    if (!estimate && nq && (!init_q || !init_t)) return api_fail(AMC_E_INVALID, "%s: NULL initial poses", fn);
    if (!estimate && ncorr && !in_mask) return api_fail(AMC_E_INVALID, "%s: NULL inlier mask", fn);
    for (size_t i = 0; i < nq; ++i)
        if (models[i] < 0 || models[i] >= cam::kNumModels)
            return api_fail(AMC_E_INVALID, "%s: query %zu has camera model %d", fn, i, (int)models[i]);

    const bool cov = want_cov != 0;
    result_alloc(result, nq, ncorr, cov);
    if (!result_ok(result, cov)) return api_fail(AMC_E_NOMEM, "%s: out of host memory for %zu queries", fn, nq);
    if (nq == 0) return AMC_OK;

    const std::vector<double> factors = estimate ? ap::focal_factors(eo) : std::vector<double>{1.0};
    const uint64_t F = estimate ? factors.size() : 0;
    const uint64_t max_trials = tvg::ransac_max_trials(eo.max_num_trials, eo.min_inlier_ratio, eo.confidence,
                                                       eo.dyn_num_trials_multiplier, ap::kMinSamples);
    const uint64_t min_trials = (uint64_t)eo.min_num_trials;

    // batches: contiguous query ranges
    const uint64_t per = estimate ? F : 1;
    const Batches batches = split_batches(offsets, nq, kMaxBatchQueries, kMaxBatchSlotCorr, per);
    const std::vector<size_t>& bstart = batches.start;
    const size_t nbatch = batches.count();
    const uint64_t max_bq = batches.most_items, max_bc = std::max<uint64_t>(batches.most_elems, 1);
    const uint64_t max_bs = estimate ? max_bq * F : 1;
    const uint64_t max_bsc = estimate ? std::max<uint64_t>(batches.most_elems * per, 1) : 1;

    const CtxView cv = ctx_view(ctx);
    HIPCHK(hipSetDevice(cv.device));
    hipStream_t st = cv.stream;
    StreamTimer timer(st);
    HIPCHK(timer.start());
    SlotDesc* d_slots;
    uint32_t *d_sord, *d_perm, *d_sninl, *d_qn, *d_qord, *d_sbeg, *d_oninl;
    double *d_xy, *d_X, *d_uv, *d_smod, *d_qprm, *d_iq, *d_oq, *d_it, *d_ot, *d_ocov, *d_ofac;
    uint8_t *d_smask, *d_ssucc, *d_sover, *d_osucc, *d_mask;
    uint64_t *d_sntr, *d_doff, *d_dtab, *d_qc0, *d_ontr;
    int32_t* d_qmod;
    DevBuf<void> mem;
    HIPCHK(DevParts()
               .part(&d_slots, max_bs)
               .part(&d_sord, max_bs)
               .part(&d_xy, 2 * max_bc)
               .part(&d_X, 3 * max_bc)
               .part(&d_uv, 2 * max_bsc)
               .part(&d_perm, max_bsc)
               .part(&d_smask, max_bsc)
               .part(&d_ssucc, max_bs)
               .part(&d_sover, max_bs)
               .part(&d_sninl, max_bs)
               .part(&d_sntr, max_bs)
               .part(&d_smod, 12 * max_bs)
               .part(&d_doff, max_bc + 2)
               .part(&d_dtab, max_bc + max_bq + 1)
               .part(&d_qc0, max_bq)
               .part(&d_qn, max_bq)
               .part(&d_qord, max_bq)
               .part(&d_qmod, max_bq)
               .part(&d_sbeg, max_bq + 1)
               .part(&d_osucc, max_bq)
               .part(&d_qprm, max_bq * cam::kMaxParams)
               .part(&d_iq, 4 * max_bq)
               .part(&d_oq, 4 * max_bq)
               .part(&d_it, 3 * max_bq)
               .part(&d_ot, 3 * max_bq)
               .part(&d_ocov, 36 * max_bq)
               .part(&d_ontr, max_bq)
               .part(&d_ofac, max_bq)
               .part(&d_mask, max_bc)
               .part(&d_oninl, max_bq)
               .carve(mem));

    // the sample stream (estimation only)
    DevBuf<uint32_t> smem;
    size_t stream_len = 0;
    std::vector<uint32_t> words;
    auto upload_stream = [&](size_t len) -> int {
        HIPCHK(hipStreamSynchronize(st));
        words = ap::sample_stream_words(len);
        HIPCHK(smem.ensure(len));
        HIPCHK(hipMemcpyAsync(smem.p, words.data(), len * 4, hipMemcpyHostToDevice, st));
        stream_len = len;
        return AMC_OK;
    };
    if (estimate) {
        const int rc = upload_stream(ap::initial_stream_len(min_trials, max_trials));
        if (rc != AMC_OK) return rc;
    }

    // host copies stay alive until the stream is drained
    struct BatchHost {
        std::vector<SlotDesc> slots;
        std::vector<uint32_t> sord, qord, qn, sbeg;
        std::vector<uint64_t> qc0, dyn_off, dyn_tab;
        std::vector<double> uv, qprm;
        std::vector<uint8_t> over;
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
        // largest queries first (a stable sort of the batch-local indices)
        H.qord.resize(bq);
        for (size_t i = 0; i < bq; ++i) H.qord[i] = (uint32_t)i;
        std::stable_sort(H.qord.begin(), H.qord.end(), [&](uint32_t a, uint32_t b) { return H.qn[a] > H.qn[b]; });
        H.qprm.assign(bq * cam::kMaxParams, 0.0);
        std::vector<int32_t> qmod(bq);
        for (size_t i = 0; i < bq; ++i) {
            qmod[i] = models[q0 + i];
            ap::scaled_params(qmod[i], cparams + cam::kMaxParams * (q0 + i), 1.0, &H.qprm[cam::kMaxParams * i]);
        }
        HIPCHK(hipMemcpyAsync(d_qc0, H.qc0.data(), bq * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_qn, H.qn.data(), bq * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_qord, H.qord.data(), bq * 4, hipMemcpyHostToDevice, st));
        if (bc) {
            HIPCHK(hipMemcpyAsync(d_xy, points2D + 2 * ob, bc * 16, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_X, points3D + 3 * ob, bc * 24, hipMemcpyHostToDevice, st));
        }
        RefineLaunch rl{};
        if (estimate) {
            const uint64_t ns = bq * F;
            H.slots.resize(ns);
            H.sbeg.resize(bq + 1);
            uint64_t sc = 0;
            bool host_lift = false;
            for (size_t i = 0; i < bq; ++i) {
                H.sbeg[i] = (uint32_t)(i * F);
                for (uint64_t f = 0; f < F; ++f) {
                    SlotDesc& d = H.slots[i * F + f];
                    std::memset(&d, 0, sizeof d);
                    d.corr0 = H.qc0[i];
                    d.scratch0 = sc;
                    d.n = H.qn[i];
                    d.model = qmod[i];
                    d.factor = factors[f];
                    ap::scaled_params(d.model, &H.qprm[cam::kMaxParams * i], factors[f], d.params);
                    const double thr = cam::cam_from_img_threshold(d.model, d.params, eo.max_error);
                    d.max_residual = thr * thr;
                    d.lift_on_device = cam::needs_libm(d.model) ? 0u : 1u;
                    host_lift = host_lift || !d.lift_on_device;
                    sc += d.n;
                }
            }
            H.sbeg[bq] = (uint32_t)ns;
            if (host_lift) {
                H.uv.assign(2 * std::max<uint64_t>(sc, 1), 0.0);
                for (const SlotDesc& d : H.slots) {
                    if (d.lift_on_device) continue;
                    const double* xy = points2D + 2 * (ob + d.corr0);
                    for (uint32_t k = 0; k < d.n; ++k)
                        cam::cam_from_img(d.model, d.params, xy[2 * k], xy[2 * k + 1], H.uv[2 * (d.scratch0 + k)],
                                          H.uv[2 * (d.scratch0 + k) + 1]);
                }
                HIPCHK(hipMemcpyAsync(d_uv, H.uv.data(), sc * 16, hipMemcpyHostToDevice, st));
            }
            H.sord.resize(ns);
            for (size_t i = 0; i < bq; ++i)
                for (uint64_t f = 0; f < F; ++f) H.sord[i * F + f] = (uint32_t)(H.qord[i] * F + f);
            HIPCHK(hipMemcpyAsync(d_slots, H.slots.data(), ns * sizeof(SlotDesc), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_sord, H.sord.data(), ns * 4, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_sbeg, H.sbeg.data(), (bq + 1) * 4, hipMemcpyHostToDevice, st));
            // dynamic trial-count rows (ComputeNumTrials(c, n), c = 0 .. n) for the batch's sizes whose RANSAC can stop
            // before max_trials: at most (batch correspondences + 1) offsets and (batch correspondences + queries) rows
            H.dyn_off.assign(1, ap::kNoRow);
            if (max_trials > min_trials) {
                uint64_t nmax = 0;
                for (size_t i = 0; i < bq; ++i) nmax = std::max<uint64_t>(nmax, H.qn[i]);
                H.dyn_off.assign(nmax + 1, ap::kNoRow);
                for (size_t i = 0; i < bq; ++i) {
                    const uint64_t n = H.qn[i];
                    if (n < 3 || H.dyn_off[n] != ap::kNoRow) continue;
                    H.dyn_off[n] = H.dyn_tab.size();
                    for (uint64_t c = 0; c <= n; ++c)
                        H.dyn_tab.push_back(tvg::compute_num_trials(c, n, eo.confidence, eo.dyn_num_trials_multiplier,
                                                                    ap::kMinSamples));
                }
            }
            if (H.dyn_tab.empty()) H.dyn_tab.push_back(0);
            HIPCHK(hipMemcpyAsync(d_doff, H.dyn_off.data(), H.dyn_off.size() * 8, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_dtab, H.dyn_tab.data(), H.dyn_tab.size() * 8, hipMemcpyHostToDevice, st));
            H.over.assign(ns, 0);
            for (;;) {
                RansacLaunch p{};
                p.slots = d_slots;
                p.order = d_sord;
                p.nslots = (uint32_t)ns;
                p.xy = d_xy;
                p.X = d_X;
                p.uv = d_uv;
                p.perm = d_perm;
                p.smask = d_smask;
                p.dyn_off = d_doff;
                p.dyn_tab = d_dtab;
                p.dyn_n = H.dyn_off.size();
                p.stream = static_cast<const uint32_t*>(smem.p);
                p.stream_len = stream_len;
                p.min_trials = min_trials;
                p.max_trials = max_trials;
                p.s_success = d_ssucc;
                p.s_overrun = d_sover;
                p.s_ninl = d_sninl;
                p.s_ntr = d_sntr;
                p.s_model = d_smod;
                HIPCHK(timer.span_begin());
                hipLaunchKernelGGL(abspose_ransac_kernel, dim3((unsigned)ns), dim3(kWave), 0, st, p);
                HIPCHK(hipGetLastError());
                HIPCHK(timer.span_end());
                HIPCHK(hipMemcpyAsync(H.over.data(), d_sover, ns, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                bool any = false;
                for (uint8_t v : H.over) any = any || v;
                if (!any) break;
                // a RANSAC ran past the end of the sample stream: rerun the batch on a table twice as long
                if (stream_len * 2 > kMaxStreamWords)
                    return api_fail(AMC_E_INVALID, "%s: the sample stream would exceed %zu words", fn, kMaxStreamWords);
                const int rc = upload_stream(stream_len * 2);
                if (rc != AMC_OK) return rc;
            }
            rl.slot_begin = d_sbeg;
            rl.slots = d_slots;
            rl.smask = d_smask;
            rl.s_success = d_ssucc;
            rl.s_ninl = d_sninl;
            rl.s_ntr = d_sntr;
            rl.s_model = d_smod;
        } else {
            HIPCHK(hipMemcpyAsync(d_qmod, qmod.data(), bq * 4, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_qprm, H.qprm.data(), bq * 8 * cam::kMaxParams, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_iq, init_q + 4 * q0, bq * 32, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_it, init_t + 3 * q0, bq * 24, hipMemcpyHostToDevice, st));
            if (bc) HIPCHK(hipMemcpyAsync(d_mask, in_mask + ob, bc, hipMemcpyHostToDevice, st));
        }
        rl.nq = (uint32_t)bq;
        rl.estimate = estimate ? 1 : 0;
        rl.order = d_qord;
        rl.qcorr0 = d_qc0;
        rl.qn = d_qn;
        rl.xy = d_xy;
        rl.X = d_X;
        rl.mask = d_mask;
        rl.qmodel = d_qmod;
        rl.qparams = d_qprm;
        rl.init_q = d_iq;
        rl.init_t = d_it;
        rl.gradient_tolerance = ro.gradient_tolerance;
        rl.max_num_iterations = ro.max_num_iterations;
        rl.loss_scale = ro.loss_function_scale;
        rl.covariance = cov ? 1 : 0;
        rl.o_success = d_osucc;
        rl.o_q = d_oq;
        rl.o_t = d_ot;
        rl.o_ninl = d_oninl;
        rl.o_ntr = d_ontr;
        rl.o_factor = d_ofac;
        rl.o_cov = cov ? d_ocov : nullptr;
        HIPCHK(timer.span_begin());
        hipLaunchKernelGGL(abspose_refine_kernel, dim3((unsigned)bq), dim3(kWave), 0, st, rl);
        HIPCHK(hipGetLastError());
        HIPCHK(timer.span_end());
        HIPCHK(hipMemcpyAsync(result->success + q0, d_osucc, bq, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(result->qvec + 4 * q0, d_oq, bq * 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(result->tvec + 3 * q0, d_ot, bq * 24, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(result->num_inliers + q0, d_oninl, bq * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(result->num_trials + q0, d_ontr, bq * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(result->focal_factor + q0, d_ofac, bq * 8, hipMemcpyDeviceToHost, st));
        if (cov) HIPCHK(hipMemcpyAsync(result->covariance + 36 * q0, d_ocov, bq * 288, hipMemcpyDeviceToHost, st));
        if (bc) HIPCHK(hipMemcpyAsync(result->inlier_mask + ob, d_mask, bc, hipMemcpyDeviceToHost, st));
        if (nbatch > 1) HIPCHK(hipStreamSynchronize(st));  // the next batch reuses the buffers the copies read
    }
    HIPCHK(timer.stop(result->device_ms));  // (result was zeroed on entry)
    HIPCHK(timer.spans(result->kernel_ms));
    result->num_batches = (uint32_t)nbatch;
    if (!estimate)  // refinement: the input mask and its count
        for (size_t i = 0; i < nq; ++i) {
            uint32_t c = 0;
            for (uint64_t k = offsets[i]; k < offsets[i + 1]; ++k) c += in_mask[k] ? 1 : 0;
            result->num_inliers[i] = c;
            result->focal_factor[i] = 1.0;
        }
    return AMC_OK;
}

}  // namespace

extern "C" {

void amc_abspose_opts_default(amc_abspose_opts* o) {
    if (!o) return;
    o->estimate_focal_length = 0;  // AbsolutePoseEstimationOptions() as the binding builds it
    o->num_focal_length_samples = 30;
    o->min_focal_length_ratio = 0.1;
    o->max_focal_length_ratio = 10.0;
    o->max_error = 12.0;
    o->min_inlier_ratio = 0.01;
    o->confidence = 0.9999;
    o->dyn_num_trials_multiplier = 3.0;
    o->min_num_trials = 1000;
    o->max_num_trials = 100000;
}

void amc_abspose_refine_opts_default(amc_abspose_refine_opts* o) {
    if (!o) return;
    o->gradient_tolerance = 1.0;
    o->max_num_iterations = 100;
    o->loss_function_scale = 1.0;
    o->refine_focal_length = 0;
    o->refine_extra_params = 0;
    o->print_summary = 0;
}

void amc_abspose_result_free(amc_abspose_result* r) {
    if (!r) return;
    std::free(r->success);
    std::free(r->qvec);
    std::free(r->tvec);
    std::free(r->num_inliers);
    std::free(r->num_trials);
    std::free(r->focal_factor);
    std::free(r->covariance);
    std::free(r->inlier_mask);
    std::memset(r, 0, sizeof *r);
}

int amc_estimate_absolute_poses(amc_ctx* ctx, const uint64_t* offsets, size_t nqueries, const int32_t* camera_models,
                                const double* camera_params, const double* points2D, const double* points3D,
                                const amc_abspose_opts* estimation_options,
                                const amc_abspose_refine_opts* refinement_options, int return_covariance,
                                amc_abspose_result* result) {
    const int rc = run_impl("amc_estimate_absolute_poses", ctx, true, offsets, nqueries, camera_models, camera_params,
                            points2D, points3D, nullptr, nullptr, nullptr, estimation_options, refinement_options,
                            return_covariance, result);
    if (rc != AMC_OK && result) amc_abspose_result_free(result);  // no partial results
    return rc;
}

int amc_refine_absolute_poses(amc_ctx* ctx, const uint64_t* offsets, size_t nqueries, const int32_t* camera_models,
                              const double* camera_params, const double* points2D, const double* points3D,
                              const double* init_qvec, const double* init_tvec, const uint8_t* inlier_mask,
                              const amc_abspose_refine_opts* refinement_options, int return_covariance,
                              amc_abspose_result* result) {
    const int rc = run_impl("amc_refine_absolute_poses", ctx, false, offsets, nqueries, camera_models, camera_params,
                            points2D, points3D, init_qvec, init_tvec, inlier_mask, nullptr, refinement_options,
                            return_covariance, result);
    if (rc != AMC_OK && result) amc_abspose_result_free(result);
    return rc;
}

}  // extern "C"
