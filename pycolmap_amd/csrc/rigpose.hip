// rigpose.hip — absolute pose of a multi-camera rig on gfx950 (include/amc_rigpose.h): COLMAP 3.9.1's
// EstimateGeneralizedAbsolutePose and RefineGeneralizedAbsolutePose, restated in DESIGN.md section 13.  The numerics are
// rigpose_core.h's and abspose_core.h's; this file is the two kernels, the host preparation (13.2) and the C entry point.
//
// Work split.  Kernel 1 runs one 64-lane wave per query, lanes as trials: lane 0 draws the next round's samples in trial
// order (the stream is data-independent), lane l solves trial l's GP3P completely and leaves its models in the block's
// workspace, then the wave walks the models in (trial, root) order with the lanes over the correspondences, exactly as
// the sequential statement of 13.6 does; trials solved beyond the abort are discarded.  The grid is persistent (a block
// takes every gridDim.x-th query of the batch's order), so the model workspace is per block, not per query.  Kernel 2
// runs one wave per query and refines rig_from_world with the lanes over the inliers.  A query's result depends on its
// own inputs only.  No atomics.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "amc_internal.h"
#include "rigpose_core.h"
#include "abspose_plan.h"
#include "../../include/amc_rigpose.h"

using namespace amc;

namespace {

constexpr int kWave = 64;
constexpr int kMaxModels = 8;                                // GP3P solutions per trial
constexpr size_t kWsDoubles = (size_t)kWave * kMaxModels * 12;  // one block's model workspace
constexpr uint32_t kMaxBlocks = 2048;                        // persistent grid: 8 waves on each of 256 CUs
constexpr uint64_t kMaxBatchCorr = (uint64_t)1 << 22;
constexpr uint64_t kMaxBatchQueries = (uint64_t)1 << 16;
constexpr size_t kMaxStreamWords = (size_t)1 << 28;

struct QueryDesc {
    uint64_t corr0;       // batch-local first correspondence
    uint32_t n;
    uint32_t cam0;        // batch-local first camera
    uint32_t has_dup;     // some 3D point occurs more than once
    uint32_t pad;
    double max_residual;  // (mean CamFromImgThreshold(max_error))^2
};

struct RansacLaunch {
    const QueryDesc* q;
    const uint32_t* order;
    uint32_t nq;
    uint32_t round;           // trials per round, 1 .. 64 (the result does not depend on it)
    const rp::RigCam* cams;
    const uint32_t* cidx;     // per correspondence: its camera, query-local
    const uint32_t* prev_same;  // per correspondence: the previous one (query-local) with the same 3D point, or kNoPrev
    const double* xy;
    const double* X;
    double* uv;
    uint32_t* perm;
    uint8_t* mask;
    double* ws;               // gridDim.x x kWsDoubles
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
    uint32_t* s_nuniq;
    uint64_t* s_ntr;
    double* s_model;
};

// one query's view of the batch
struct QueryView {
    uint32_t n;
    uint32_t has_dup;
    double max_residual;
    const rp::RigCam* cams;
    const uint32_t* cidx;
    const uint32_t* prev_same;
    const double* uv;
    const double* X;
    uint8_t* mask;
};

// 13.4 / 13.5: the support of rig_from_world P; the inlier flags go to v.mask when the unique count or the caller needs
// them
AMC_HD rp::Support rig_score(const QueryView& v, const double* P, bool mark) {
    const bool flags = mark || v.has_dup != 0;
    double s[2];
    ap::wave_sum<2>(
        [&](int lane, double (&o)[2]) {
            o[0] = o[1] = 0.0;
            for (uint32_t k = (uint32_t)lane; k < v.n; k += kWave) {
                const double r = rp::sq_reproj_rig(P, v.cams[v.cidx[k]].Rt, v.X + 3 * k, v.uv[2 * k], v.uv[2 * k + 1]);
                const bool in = r <= v.max_residual;
                if (in) {
                    o[0] = o[0] + 1.0;
                    o[1] = o[1] + r;
                }
                if (flags) v.mask[k] = in ? 1 : 0;
            }
        },
        s);
    rp::Support sp{(uint32_t)s[0], (uint32_t)s[0], s[1]};
    if (v.has_dup) {
        AP_SYNC();
        double u[1];
        ap::wave_sum<1>(
            [&](int lane, double (&o)[1]) {
                o[0] = 0.0;
                for (uint32_t k = (uint32_t)lane; k < v.n; k += kWave)
                    if (v.mask[k] && rp::first_flagged_of_its_point(v.mask, v.prev_same, k)) o[0] = o[0] + 1.0;
            },
            u);
        sp.uniq = (uint32_t)u[0];
    }
    AP_SYNC();
    return sp;
}

__global__ __launch_bounds__(kWave) void rigpose_ransac_kernel(RansacLaunch p) {
    __shared__ uint32_t s_idx[kWave][3];
    __shared__ int s_nm[kWave];
    __shared__ uint32_t s_nvalid;
    const int lane = (int)threadIdx.x;
    double* ws = p.ws + (size_t)blockIdx.x * kWsDoubles;
    for (uint32_t bi = blockIdx.x; bi < p.nq; bi += gridDim.x) {
        const uint32_t qi = p.order[bi];
        const QueryDesc d = p.q[qi];
        const uint32_t n = d.n;
        const rp::RigCam* cams = p.cams + d.cam0;
        const uint32_t* cidx = p.cidx + d.corr0;
        double* uv = p.uv + 2 * d.corr0;
        const double* xy = p.xy + 2 * d.corr0;
        const double* X = p.X + 3 * d.corr0;
        uint32_t* perm = p.perm + d.corr0;
        uint8_t* mask = p.mask + d.corr0;
        for (uint32_t k = (uint32_t)lane; k < n; k += kWave) {
            const rp::RigCam& cm = cams[cidx[k]];
            if (cm.lift_on_device) cam::cam_from_img(cm.model, cm.params, xy[2 * k], xy[2 * k + 1], uv[2 * k], uv[2 * k + 1]);
            perm[k] = k;
            mask[k] = 0;
        }
        __syncthreads();
        const QueryView v{n, d.has_dup, d.max_residual, cams, cidx, p.prev_same + d.corr0, uv, X, mask};
        const uint64_t row = n < p.dyn_n ? p.dyn_off[n] : ap::kNoRow;
        const uint64_t* dyn_row = row == ap::kNoRow ? nullptr : p.dyn_tab + row;
        rp::Support best{0u, 0u, ap::kDblMax};
        double best_model[12];
        for (int i = 0; i < 12; ++i) best_model[i] = 0.0;
        uint64_t pos = 0;  // stream words consumed (lane 0)
        uint64_t dyn_max = p.max_trials;
        uint64_t ntr = n < 3 ? 0 : p.max_trials;
        bool overrun = false, done = n < 3;
        for (uint64_t t0 = 0; t0 < p.max_trials && !done;) {
            const uint32_t R = (uint32_t)(p.max_trials - t0 < p.round ? p.max_trials - t0 : p.round);
            if (lane == 0) {
                // RandomSampler::Sample per trial, in trial order: j = uniform_int(i, n - 1) (libstdc++'s Lemire
                // reduction), swap(perm[i], perm[j])
                uint32_t l = 0;
                bool out_of_words = false;
                for (; l < R; ++l) {
                    for (uint32_t i = 0; i < 3 && !out_of_words; ++i) {
                        const uint32_t range = n - i;
                        uint64_t prod = 0;
                        uint32_t low = 0;
                        bool first = true;
                        const uint32_t threshold = (uint32_t)(-range) % range;
                        while (first || low < threshold) {
                            if (pos >= p.stream_len) {
                                out_of_words = true;
                                break;
                            }
                            prod = (uint64_t)p.stream[pos++] * (uint64_t)range;
                            low = (uint32_t)prod;
                            if (first && low >= range) break;
                            first = false;
                        }
                        if (out_of_words) break;
                        const uint32_t j = i + (uint32_t)(prod >> 32);
                        const uint32_t a = perm[i], b = perm[j];
                        perm[i] = b;
                        perm[j] = a;
                        s_idx[l][i] = b;
                    }
                    if (out_of_words) break;
                }
                s_nvalid = l;
            }
            __syncthreads();
            const uint32_t nvalid = s_nvalid;
            int nm = 0;
            if ((uint32_t)lane < nvalid) {
                double c[3][3], dd[3][3], X3[3][3];
                for (int i = 0; i < 3; ++i) {
                    const uint32_t k = s_idx[lane][i];
                    const rp::RigCam& cm = cams[cidx[k]];
                    rp::rig_ray(cm.Rt, uv[2 * k], uv[2 * k + 1], dd[i]);
                    for (int j = 0; j < 3; ++j) {
                        c[i][j] = cm.origin[j];
                        X3[i][j] = X[3 * k + j];
                    }
                }
                nm = rp::gp3p(c, dd, X3, reinterpret_cast<double(*)[12]>(ws + (size_t)lane * kMaxModels * 12));
            }
            s_nm[lane] = nm;
            __syncthreads();
            // the models in (trial, root) order, as the sequential RANSAC meets them
            for (uint32_t l = 0; l < R && !done; ++l) {
                const uint64_t trial = t0 + l;
                if (l >= nvalid) {  // the sample stream ran out before this trial: the host reruns on a longer table
                    overrun = true;
                    done = true;
                    break;
                }
                const int nml = s_nm[l];
                for (int mi = 0; mi < nml; ++mi) {
                    double P[12];
                    const double* src = ws + ((size_t)l * kMaxModels + mi) * 12;
                    for (int i = 0; i < 12; ++i) P[i] = src[i];
                    const rp::Support s = rig_score(v, P, false);
                    if (rp::better(s, best)) {
                        best = s;
                        for (int i = 0; i < 12; ++i) best_model[i] = P[i];
                        dyn_max = dyn_row ? dyn_row[best.cnt] : p.max_trials;
                    }
                    if (trial >= dyn_max && trial >= p.min_trials) {
                        // the sequential loop leaves through its abort test at the top of the next trial
                        ntr = trial + 1 < p.max_trials ? trial + 2 : trial + 1;
                        done = true;
                        break;
                    }
                }
            }
            t0 += R;
            __syncthreads();
        }
        const bool success = best.cnt >= 3 && !overrun;
        if (success) {
            rig_score(v, best_model, true);
        } else {
            for (uint32_t k = (uint32_t)lane; k < n; k += kWave) mask[k] = 0;
        }
        if (lane == 0) {
            p.s_success[qi] = success ? 1 : 0;
            p.s_overrun[qi] = overrun ? 1 : 0;
            p.s_ninl[qi] = success ? best.cnt : 0u;  // a failed RANSAC's best support is not a result
            p.s_nuniq[qi] = success ? best.uniq : 0u;
            p.s_ntr[qi] = ntr;
            for (int i = 0; i < 12; ++i) p.s_model[12 * qi + i] = best_model[i];
        }
        __syncthreads();
    }
}

struct RefineLaunch {
    const QueryDesc* q;
    const uint32_t* order;
    const rp::RigCam* cams;
    const uint32_t* cidx;
    const double* xy;
    const double* X;
    const uint8_t* mask;
    const uint8_t* s_success;
    const double* s_model;
    double gradient_tolerance;
    int64_t max_num_iterations;
    double loss_scale;
    int covariance;
    uint8_t* o_success;
    double* o_q;
    double* o_t;
    double* o_cov;  // nq x 36, or null
};

__global__ __launch_bounds__(kWave) void rigpose_refine_kernel(RefineLaunch p) {
    const uint32_t qi = p.order[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const QueryDesc d = p.q[qi];
    double q[4] = {0.0, 0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0};
    double cov[36];
    for (int i = 0; i < 36; ++i) cov[i] = 0.0;
    bool ok = p.s_success[qi] != 0;
    if (ok) ok = ap::model_to_pose(p.s_model + 12 * qi, q, t);
    if (ok) {
        const rp::RigCam* cams = p.cams + d.cam0;
        const uint32_t* cidx = p.cidx + d.corr0;
        const double* xy = p.xy + 2 * d.corr0;
        const double* X = p.X + 3 * d.corr0;
        const ap::LmParams lm{p.gradient_tolerance, p.max_num_iterations, p.loss_scale, p.covariance != 0};
        const ap::RefineOut r = ap::refine_t(
            [&](uint32_t k, const double* qq, const double* tt, ap::Jet& rx, ap::Jet& ry) {
                rp::rig_pixel_residual(cams[cidx[k]], qq, tt, X + 3 * k, xy[2 * k], xy[2 * k + 1], rx, ry);
            },
            lm, q, t, p.mask + d.corr0, d.n);
        ok = r.success;
        for (int i = 0; i < 4; ++i) q[i] = r.q[i];
        for (int i = 0; i < 3; ++i) t[i] = r.t[i];
        for (int i = 0; i < 36; ++i) cov[i] = r.cov[i];
    }
    if (lane == 0) {
        p.o_success[qi] = ok ? 1 : 0;
        for (int i = 0; i < 4; ++i) p.o_q[4 * qi + i] = q[i];
        for (int i = 0; i < 3; ++i) p.o_t[3 * qi + i] = t[i];
        if (p.o_cov)
            for (int i = 0; i < 36; ++i) p.o_cov[36 * qi + i] = cov[i];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
// RANSACOptions::Check; empty string = valid
std::string check_ransac(const amc_ransac_opts& o) {
    if (!(o.max_error > 0)) return "max_error > 0";
    if (!(o.min_inlier_ratio >= 0) || !(o.min_inlier_ratio <= 1)) return "0 <= min_inlier_ratio <= 1";
    if (!(o.confidence >= 0) || !(o.confidence <= 1)) return "0 <= confidence <= 1";
    if (o.min_num_trials < 0 || o.max_num_trials < 0 || o.min_num_trials > o.max_num_trials)
        return "0 <= min_num_trials <= max_num_trials";
    return std::string();
}

// 13.2: one camera of the rig (cam_from_rig: x y z w tx ty tz), Eigen::Quaterniond::toRotationMatrix's arithmetic
rp::RigCam make_rig_cam(int model, const double* params, const double* g) {
    rp::RigCam c;
    std::memset(&c, 0, sizeof c);
    c.model = model;
    c.lift_on_device = cam::needs_libm(model) ? 0u : 1u;
    ap::scaled_params(model, params, 1.0, c.params);
    const double x = g[0], y = g[1], z = g[2], w = g[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double R[9] = {1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx,
                         txz - twy, tyz + twx, 1.0 - (txx + tyy)};
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) c.Rt[4 * r + k] = R[3 * r + k];
        c.Rt[4 * r + 3] = g[4 + r];
    }
    for (int j = 0; j < 3; ++j) c.origin[j] = -((R[j] * g[4] + R[3 + j] * g[5]) + R[6 + j] * g[6]);
    for (int i = 0; i < 4; ++i) c.q[i] = g[i];
    return c;
}

void result_alloc(amc_rigpose_result* r, size_t nq, uint64_t ncorr, bool cov) {
    const size_t q = std::max<size_t>(nq, 1);
    r->nqueries = nq;
    r->ncorr = ncorr;
    r->success = static_cast<uint8_t*>(std::calloc(q, 1));
    r->qvec = static_cast<double*>(std::calloc(q * 4, sizeof(double)));
    r->tvec = static_cast<double*>(std::calloc(q * 3, sizeof(double)));
    r->num_inliers = static_cast<uint32_t*>(std::calloc(q, sizeof(uint32_t)));
    r->num_all_inliers = static_cast<uint32_t*>(std::calloc(q, sizeof(uint32_t)));
    r->num_trials = static_cast<uint64_t*>(std::calloc(q, sizeof(uint64_t)));
    r->covariance = cov ? static_cast<double*>(std::calloc(q * 36, sizeof(double))) : nullptr;
    r->inlier_mask = static_cast<uint8_t*>(std::calloc(std::max<uint64_t>(ncorr, 1), 1));
}
bool result_ok(const amc_rigpose_result* r, bool cov) {
    return r->success && r->qvec && r->tvec && r->num_inliers && r->num_all_inliers && r->num_trials && r->inlier_mask &&
           (!cov || r->covariance);
}

int run_impl(const char* fn, amc_ctx* ctx, const uint64_t* offsets, size_t nq, const uint64_t* cam_offsets,
             const int32_t* models, const double* cparams, const double* rigs, const int32_t* cam_idxs,
             const double* points2D, const double* points3D, const amc_ransac_opts* eo_in,
             const amc_abspose_refine_opts* ro_in, int want_cov, amc_rigpose_result* result) {
    const char* const hipchk_who = fn;
    if (!ctx || !result || !offsets || !cam_offsets || !ro_in || !eo_in)
        return api_fail(AMC_E_INVALID, "%s: NULL argument", fn);
    std::memset(result, 0, sizeof *result);
    const amc_abspose_refine_opts ro = *ro_in;
    const amc_ransac_opts eo = *eo_in;
    std::string bad = check_ransac(eo);
    if (bad.empty()) bad = ap::check_refinement(ro);
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: invalid options: %s", fn, bad.c_str());
    if (offsets[0] != 0 || cam_offsets[0] != 0) return api_fail(AMC_E_INVALID, "%s: offsets[0] != 0", fn);
    for (size_t i = 0; i < nq; ++i) {
        if (offsets[i + 1] < offsets[i] || cam_offsets[i + 1] < cam_offsets[i])
            return api_fail(AMC_E_INVALID, "%s: offsets decrease at query %zu", fn, i);
        if (offsets[i + 1] - offsets[i] > 0xfffffffeull)
            return api_fail(AMC_E_INVALID, "%s: query %zu has more than 2^32 - 2 correspondences", fn, i);
        if (cam_offsets[i + 1] - cam_offsets[i] > 0xffffffffull)
            return api_fail(AMC_E_INVALID, "%s: query %zu has more than 2^32 - 1 cameras", fn, i);
    }
    const uint64_t ncorr = offsets[nq], ncam = cam_offsets[nq];
    if (ncam && (!models || !cparams || !rigs)) return api_fail(AMC_E_INVALID, "%s: NULL cameras", fn);
    if (ncorr && (!points2D || !points3D || !cam_idxs)) return api_fail(AMC_E_INVALID, "%s: NULL points", fn);
    for (uint64_t i = 0; i < ncam; ++i)
        if (models[i] < 0 || models[i] >= cam::kNumModels)
            return api_fail(AMC_E_INVALID, "%s: camera %llu has camera model %d", fn, (unsigned long long)i, (int)models[i]);
    for (size_t i = 0; i < nq; ++i) {
        const uint64_t nc = cam_offsets[i + 1] - cam_offsets[i];
        for (uint64_t k = offsets[i]; k < offsets[i + 1]; ++k)
            if (cam_idxs[k] < 0 || (uint64_t)cam_idxs[k] >= nc)
                return api_fail(AMC_E_INVALID, "%s: query %zu: camera index %d of correspondence %llu is not in [0, %llu)",
                                fn, i, (int)cam_idxs[k], (unsigned long long)(k - offsets[i]), (unsigned long long)nc);
    }

    const bool cov = want_cov != 0;
    result_alloc(result, nq, ncorr, cov);
    if (!result_ok(result, cov)) return api_fail(AMC_E_NOMEM, "%s: out of host memory for %zu queries", fn, nq);
    if (nq == 0) return AMC_OK;

    const uint64_t max_trials = tvg::ransac_max_trials(eo.max_num_trials, eo.min_inlier_ratio, eo.confidence,
                                                       eo.dyn_num_trials_multiplier, ap::kMinSamples);
    const uint64_t min_trials = (uint64_t)eo.min_num_trials;
    const uint32_t round = (uint32_t)env_int("AMC_RIGPOSE_ROUND", kWave, 1, kWave);  // test hook: trials per round

    const Batches batches = split_batches(offsets, nq, kMaxBatchQueries, kMaxBatchCorr);
    const std::vector<size_t>& bstart = batches.start;
    const size_t nbatch = batches.count();
    const uint64_t max_bq = batches.most_items, max_bc = std::max<uint64_t>(batches.most_elems, 1);
    uint64_t max_bcam = 1;
    for (size_t bi = 0; bi < nbatch; ++bi)
        max_bcam = std::max<uint64_t>(max_bcam, cam_offsets[bstart[bi + 1]] - cam_offsets[bstart[bi]]);
    const uint32_t max_blocks = (uint32_t)std::min<uint64_t>(max_bq, kMaxBlocks);

    const CtxView cv = ctx_view(ctx);
    HIPCHK(hipSetDevice(cv.device));
    hipStream_t st = cv.stream;
    StreamTimer timer(st);
    HIPCHK(timer.start());
    QueryDesc* d_q;
    rp::RigCam* d_cams;
    uint32_t *d_ord, *d_cidx, *d_prev, *d_perm, *d_sninl, *d_snuniq;
    double *d_xy, *d_X, *d_uv, *d_ws, *d_smod, *d_oq, *d_ot, *d_ocov;
    uint8_t *d_mask, *d_ssucc, *d_sover, *d_osucc;
    uint64_t *d_sntr, *d_doff, *d_dtab;
    DevBuf<void> mem;
    HIPCHK(DevParts()
               .part(&d_q, max_bq)
               .part(&d_ord, max_bq)
               .part(&d_cams, max_bcam)
               .part(&d_cidx, max_bc)
               .part(&d_prev, max_bc)
               .part(&d_xy, 2 * max_bc)
               .part(&d_X, 3 * max_bc)
               .part(&d_uv, 2 * max_bc)
               .part(&d_perm, max_bc)
               .part(&d_mask, max_bc)
               .part(&d_ws, (size_t)max_blocks * kWsDoubles)
               .part(&d_ssucc, max_bq)
               .part(&d_sover, max_bq)
               .part(&d_sninl, max_bq)
               .part(&d_snuniq, max_bq)
               .part(&d_sntr, max_bq)
               .part(&d_smod, 12 * max_bq)
               .part(&d_doff, max_bc + 2)
               .part(&d_dtab, max_bc + max_bq + 1)
               .part(&d_osucc, max_bq)
               .part(&d_oq, 4 * max_bq)
               .part(&d_ot, 3 * max_bq)
               .part(&d_ocov, 36 * max_bq)
               .carve(mem));

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
    {
        const int rc = upload_stream(ap::initial_stream_len(min_trials, max_trials));
        if (rc != AMC_OK) return rc;
    }

    // host copies stay alive until the stream is drained
    struct BatchHost {
        std::vector<QueryDesc> q;
        std::vector<uint32_t> ord, cidx, prev;
        std::vector<rp::RigCam> cams;
        std::vector<uint64_t> dyn_off, dyn_tab;
        std::vector<double> uv;
        std::vector<uint8_t> over;
    };
    std::vector<BatchHost> hb(nbatch);
    for (size_t bi = 0; bi < nbatch; ++bi) {
        BatchHost& H = hb[bi];
        const size_t q0 = bstart[bi], q1 = bstart[bi + 1], bq = q1 - q0;
        const uint64_t ob = offsets[q0], bc = offsets[q1] - ob;
        const uint64_t cb = cam_offsets[q0], bcam = cam_offsets[q1] - cb;
        H.cams.resize(std::max<uint64_t>(bcam, 1));
        for (uint64_t i = 0; i < bcam; ++i)
            H.cams[i] = make_rig_cam(models[cb + i], cparams + cam::kMaxParams * (cb + i), rigs + 7 * (cb + i));
        H.q.resize(bq);
        H.cidx.resize(std::max<uint64_t>(bc, 1));
        H.prev.assign(std::max<uint64_t>(bc, 1), rp::kNoPrev);
        bool host_lift = false;
        for (size_t i = 0; i < bq; ++i) {
            QueryDesc& d = H.q[i];
            std::memset(&d, 0, sizeof d);
            d.corr0 = offsets[q0 + i] - ob;
            d.n = (uint32_t)(offsets[q0 + i + 1] - offsets[q0 + i]);
            d.cam0 = (uint32_t)(cam_offsets[q0 + i] - cb);
            const rp::RigCam* qc = H.cams.data() + d.cam0;
            const double* p3 = points3D + 3 * (ob + d.corr0);
            // the threshold: the mean over the correspondences, in their order; the cameras that need host libm
            double sum = 0.0;
            for (uint32_t k = 0; k < d.n; ++k) {
                const uint32_t c = (uint32_t)cam_idxs[ob + d.corr0 + k];
                H.cidx[d.corr0 + k] = c;
                sum += cam::cam_from_img_threshold(qc[c].model, qc[c].params, eo.max_error);
                host_lift = host_lift || !qc[c].lift_on_device;
            }
            const double thr = d.n ? sum / (double)d.n : 0.0;
            d.max_residual = thr * thr;
            // point ids: the previous correspondence whose three doubles compare equal (first match by value; NaN never
            // equals), through a sort of the indices by the doubles' bits with an == check inside each run
            std::vector<uint32_t> idx(d.n);
            for (uint32_t k = 0; k < d.n; ++k) idx[k] = k;
            auto key = [&](uint32_t k, int c) {
                const double x = p3[3 * k + c] == 0.0 ? 0.0 : p3[3 * k + c];  // -0 == +0
                return ap::dbits(x);
            };
            std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
                for (int c = 0; c < 3; ++c)
                    if (key(a, c) != key(b, c)) return key(a, c) < key(b, c);
                return false;
            });
            uint32_t* prev = H.prev.data() + d.corr0;
            for (uint32_t s = 1; s < d.n; ++s) {
                const uint32_t a = idx[s - 1], b = idx[s];
                if (p3[3 * a] == p3[3 * b] && p3[3 * a + 1] == p3[3 * b + 1] && p3[3 * a + 2] == p3[3 * b + 2]) {
                    prev[b] = a;  // a < b: the sort is stable
                    d.has_dup = 1;
                }
            }
        }
        // largest queries first (a stable sort of the batch-local indices)
        H.ord.resize(bq);
        for (size_t i = 0; i < bq; ++i) H.ord[i] = (uint32_t)i;
        std::stable_sort(H.ord.begin(), H.ord.end(), [&](uint32_t a, uint32_t b) { return H.q[a].n > H.q[b].n; });
        HIPCHK(hipMemcpyAsync(d_q, H.q.data(), bq * sizeof(QueryDesc), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_ord, H.ord.data(), bq * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_cams, H.cams.data(), H.cams.size() * sizeof(rp::RigCam), hipMemcpyHostToDevice, st));
        if (bc) {
            HIPCHK(hipMemcpyAsync(d_cidx, H.cidx.data(), bc * 4, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_prev, H.prev.data(), bc * 4, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_xy, points2D + 2 * ob, bc * 16, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_X, points3D + 3 * ob, bc * 24, hipMemcpyHostToDevice, st));
        }
        if (host_lift) {
            H.uv.assign(2 * bc, 0.0);
            for (const QueryDesc& d : H.q)
                for (uint32_t k = 0; k < d.n; ++k) {
                    const rp::RigCam& cm = H.cams[d.cam0 + H.cidx[d.corr0 + k]];
                    if (cm.lift_on_device) continue;
                    const double* xy = points2D + 2 * (ob + d.corr0 + k);
                    cam::cam_from_img(cm.model, cm.params, xy[0], xy[1], H.uv[2 * (d.corr0 + k)],
                                      H.uv[2 * (d.corr0 + k) + 1]);
                }
            HIPCHK(hipMemcpyAsync(d_uv, H.uv.data(), bc * 16, hipMemcpyHostToDevice, st));
        }
        // dynamic trial-count rows (ComputeNumTrials(c, n), c = 0 .. n) for the batch's sizes whose RANSAC can stop
        // before max_trials
        H.dyn_off.assign(1, ap::kNoRow);
        if (max_trials > min_trials) {
            uint64_t nmax = 0;
            for (size_t i = 0; i < bq; ++i) nmax = std::max<uint64_t>(nmax, H.q[i].n);
            H.dyn_off.assign(nmax + 1, ap::kNoRow);
            for (size_t i = 0; i < bq; ++i) {
                const uint64_t n = H.q[i].n;
                if (n < 3 || H.dyn_off[n] != ap::kNoRow) continue;
                H.dyn_off[n] = H.dyn_tab.size();
                for (uint64_t c = 0; c <= n; ++c)
                    H.dyn_tab.push_back(
                        tvg::compute_num_trials(c, n, eo.confidence, eo.dyn_num_trials_multiplier, ap::kMinSamples));
            }
        }
        if (H.dyn_tab.empty()) H.dyn_tab.push_back(0);
        HIPCHK(hipMemcpyAsync(d_doff, H.dyn_off.data(), H.dyn_off.size() * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_dtab, H.dyn_tab.data(), H.dyn_tab.size() * 8, hipMemcpyHostToDevice, st));
        H.over.assign(bq, 0);
        const uint32_t blocks = (uint32_t)std::min<uint64_t>(bq, kMaxBlocks);
        for (;;) {
            RansacLaunch p{};
            p.q = d_q;
            p.order = d_ord;
            p.nq = (uint32_t)bq;
            p.round = round;
            p.cams = d_cams;
            p.cidx = d_cidx;
            p.prev_same = d_prev;
            p.xy = d_xy;
            p.X = d_X;
            p.uv = d_uv;
            p.perm = d_perm;
            p.mask = d_mask;
            p.ws = d_ws;
            p.dyn_off = d_doff;
            p.dyn_tab = d_dtab;
            p.dyn_n = H.dyn_off.size();
            p.stream = smem.p;
            p.stream_len = stream_len;
            p.min_trials = min_trials;
            p.max_trials = max_trials;
            p.s_success = d_ssucc;
            p.s_overrun = d_sover;
            p.s_ninl = d_sninl;
            p.s_nuniq = d_snuniq;
            p.s_ntr = d_sntr;
            p.s_model = d_smod;
            HIPCHK(timer.span_begin());
            hipLaunchKernelGGL(rigpose_ransac_kernel, dim3(blocks), dim3(kWave), 0, st, p);
            HIPCHK(hipGetLastError());
            HIPCHK(timer.span_end());
            HIPCHK(hipMemcpyAsync(H.over.data(), d_sover, bq, hipMemcpyDeviceToHost, st));
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
        RefineLaunch rl{};
        rl.q = d_q;
        rl.order = d_ord;
        rl.cams = d_cams;
        rl.cidx = d_cidx;
        rl.xy = d_xy;
        rl.X = d_X;
        rl.mask = d_mask;
        rl.s_success = d_ssucc;
        rl.s_model = d_smod;
        rl.gradient_tolerance = ro.gradient_tolerance;
        rl.max_num_iterations = ro.max_num_iterations;
        rl.loss_scale = ro.loss_function_scale;
        rl.covariance = cov ? 1 : 0;
        rl.o_success = d_osucc;
        rl.o_q = d_oq;
        rl.o_t = d_ot;
        rl.o_cov = cov ? d_ocov : nullptr;
        HIPCHK(timer.span_begin());
        hipLaunchKernelGGL(rigpose_refine_kernel, dim3((unsigned)bq), dim3(kWave), 0, st, rl);
        HIPCHK(hipGetLastError());
        HIPCHK(timer.span_end());
        HIPCHK(hipMemcpyAsync(result->success + q0, d_osucc, bq, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(result->qvec + 4 * q0, d_oq, bq * 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(result->tvec + 3 * q0, d_ot, bq * 24, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(result->num_inliers + q0, d_snuniq, bq * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(result->num_all_inliers + q0, d_sninl, bq * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(result->num_trials + q0, d_sntr, bq * 8, hipMemcpyDeviceToHost, st));
        if (cov) HIPCHK(hipMemcpyAsync(result->covariance + 36 * q0, d_ocov, bq * 288, hipMemcpyDeviceToHost, st));
        if (bc) HIPCHK(hipMemcpyAsync(result->inlier_mask + ob, d_mask, bc, hipMemcpyDeviceToHost, st));
        if (nbatch > 1) HIPCHK(hipStreamSynchronize(st));  // the next batch reuses the buffers the copies read
    }
    HIPCHK(timer.stop(result->device_ms));  // (result was zeroed on entry)
    HIPCHK(timer.spans(result->kernel_ms));
    result->num_batches = (uint32_t)nbatch;
    return AMC_OK;
}

}  // namespace

extern "C" {

void amc_rigpose_result_free(amc_rigpose_result* r) {
    if (!r) return;
    std::free(r->success);
    std::free(r->qvec);
    std::free(r->tvec);
    std::free(r->num_inliers);
    std::free(r->num_all_inliers);
    std::free(r->num_trials);
    std::free(r->covariance);
    std::free(r->inlier_mask);
    std::memset(r, 0, sizeof *r);
}

int amc_estimate_rig_absolute_poses(amc_ctx* ctx, const uint64_t* offsets, size_t nqueries,
                                    const uint64_t* camera_offsets, const int32_t* camera_models,
                                    const double* camera_params, const double* cams_from_rig,
                                    const int32_t* camera_idxs, const double* points2D, const double* points3D,
                                    const amc_ransac_opts* ransac_options,
                                    const amc_abspose_refine_opts* refinement_options, int return_covariance,
                                    amc_rigpose_result* result) {
    const int rc = run_impl("amc_estimate_rig_absolute_poses", ctx, offsets, nqueries, camera_offsets, camera_models,
                            camera_params, cams_from_rig, camera_idxs, points2D, points3D, ransac_options,
                            refinement_options, return_covariance, result);
    if (rc != AMC_OK && result) amc_rigpose_result_free(result);  // no partial results
    return rc;
}

}  // extern "C"
