// retri.hip — the pair retriangulator on gfx950 (include/amc_retri.h): the arithmetic of COLMAP 3.9.1's
// IncrementalTriangulator::Retriangulate restated in DESIGN.md section 19.  Every FP64 operation is tri_core.h's, in
// the order of sections 11 and 17: a correspondence's outcome has the bits triobs.hip gives its two-candidate item.
//
// Work split (19.4).  The whole state of a call lives on the device: per observation its image, its lifted pixel and
// the slot of the point it carries, and the positions of the existing points followed by one slot per correspondence
// for the point it may create.  One lane per image builds the pose and one lane per observation lifts its pixel, once.
// Then every round queues two kernels and the host does not wait between rounds:
//   retri_ratio_kernel  a wave per pair counts the correspondences whose observations carry one point and writes the
//                       pair's ran byte (19.2's ratio test);
//   retri_corr_kernel   a lane per correspondence of the pairs that ran classifies it, runs Continue or the
//                       two-observation Create and writes the outcome into the state itself.
// The pairs of a round share no image and a pair's list is one-to-one, so no two lanes of a round touch one
// observation (19.3); a created point's slot is num_points + the correspondence's index.  No atomics, no LDS.
#include <cfloat>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "amc_internal.h"
#include "camera_math.h"
#include "retri_plan.h"
#include "tri_core.h"
#include "triobs_plan.h"
#include "../../include/amc_retri.h"

using namespace amc;

namespace {

using tri::TriPose;
using tri::TriSupport;

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kKC = cam::kMaxParams;

struct Dev {
    uint32_t nimg, nobs, npoints;
    double max_residual;   // DegToRad(create_max_angle_error)^2
    double min_tri_angle;  // DegToRad(min_angle)
    double re_max;         // DegToRad(re_max_angle_error)
    double re_min_ratio;
    uint64_t max_trials;   // 10000 after the RANSAC constructor's clamp
    const int32_t* cmodel;
    const double* cparams;
    const uint32_t* icam;
    const double *q, *t;
    TriPose* poses;
    const uint32_t* oimg;   // per observation
    const double* oxy;
    double* nxy;            // 2 per observation: the normalised image point
    int32_t* opoint;        // per observation: the slot of its point, or -1 (the state)
    double* xyz;            // 3 per slot: the existing points, then one slot per correspondence (the state)
    const uint64_t* poff;   // pairs + 1
    const uint32_t* cobs;   // 2 per correspondence
    const uint32_t* cpair;  // per correspondence
    const uint8_t* two_view;  // nullptr: all zero
    uint8_t* ran;           // per pair
    uint32_t* ntri;         // per pair
    uint8_t* action;        // per correspondence, zeroed before the kernels
    uint8_t* mask;          // 2 per correspondence: tri_core.h's inlier bytes
    // the launch
    uint32_t pair_first, pair_last;
    uint64_t corr_first, corr_last;
};

unsigned blocks_for(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// 11.1: [R | t] with the Rigid3d binding's quaternion -> matrix arithmetic, the centre -(R^T t) (as in triobs.hip)
__global__ __launch_bounds__(kBlock) void retri_pose_kernel(Dev d) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= d.nimg) return;
    const double x = d.q[4 * i], y = d.q[4 * i + 1], z = d.q[4 * i + 2], w = d.q[4 * i + 3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double R[9] = {1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy,
                         tyz + twx, 1.0 - (txx + tyy)};
    TriPose& p = d.poses[i];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) p.P[4 * r + c] = R[3 * r + c];
        p.P[4 * r + 3] = d.t[3 * i + r];
    }
    for (int c = 0; c < 3; ++c) p.C[c] = -(p.P[c] * p.P[3] + p.P[4 + c] * p.P[7] + p.P[8 + c] * p.P[11]);
    p.pad = 0.0;
}

__global__ __launch_bounds__(kBlock) void retri_lift_kernel(Dev d) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    if (o >= d.nobs) return;
    const uint32_t c = d.icam[d.oimg[o]];
    const int model = d.cmodel[c];
    if (cam::needs_libm(model)) return;  // the host's value is already there
    double prm[kKC], u, v;
    for (int i = 0; i < kKC; ++i) prm[i] = d.cparams[kKC * c + i];
    cam::cam_from_img(model, prm, d.oxy[2 * (size_t)o], d.oxy[2 * (size_t)o + 1], u, v);
    d.nxy[2 * (size_t)o] = u;
    d.nxy[2 * (size_t)o + 1] = v;
}

// 19.2's under-reconstruction test: a wave per pair of the launch
__global__ __launch_bounds__(kBlock) void retri_ratio_kernel(Dev d) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t p = (uint64_t)d.pair_first + ((uint64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;
    if (p >= d.pair_last) return;  // (the whole wave)
    const uint64_t k0 = d.poff[p], k1 = d.poff[p + 1];
    uint32_t n = 0;
    for (uint64_t k = k0 + lane; k < k1; k += kWave) {
        const int32_t a = d.opoint[d.cobs[2 * k]], b = d.opoint[d.cobs[2 * k + 1]];
        n += (a >= 0 && a == b) ? 1u : 0u;
    }
    for (int m = kWave / 2; m >= 1; m >>= 1) n += __shfl_xor(n, m);  // an integer sum: its order is free
    if (lane == 0) {
        const double tri_ratio = (double)n / (double)(k1 - k0);
        d.ntri[p] = n;
        d.ran[p] = tri_ratio >= d.re_min_ratio ? 0 : 1;  // 0 / 0 is NaN: a pair without correspondences runs, on nothing
    }
}

// tri_core.h's view of one correspondence: observation 0 and observation 1
struct PairView {
    double x0, y0, x1, y1;
    const TriPose *p0, *p1;
    uint8_t* mask;
    double max_residual, min_tri_angle;
    __device__ __forceinline__ double x(uint64_t o) const { return o ? x1 : x0; }
    __device__ __forceinline__ double y(uint64_t o) const { return o ? y1 : y0; }
    __device__ __forceinline__ const TriPose& pose(uint64_t o) const { return o ? *p1 : *p0; }
};

// 19.2's per-correspondence cases: a lane per correspondence of the launch
__global__ __launch_bounds__(kBlock) void retri_corr_kernel(Dev d) {
    const uint64_t k = d.corr_first + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= d.corr_last) return;
    if (!d.ran[d.cpair[k]]) return;
    const uint32_t o1 = d.cobs[2 * k], o2 = d.cobs[2 * k + 1];
    const int32_t s1 = d.opoint[o1], s2 = d.opoint[o2];
    if (s1 >= 0 && s2 >= 0) return;
    if (s1 >= 0 || s2 >= 0) {
        // Continue: the reference observation is the one without a point, the single candidate the other
        const uint32_t ref = s1 >= 0 ? o2 : o1;
        const int32_t slot = s1 >= 0 ? s1 : s2;
        const double e = tri::tri_angular_error(d.nxy[2 * (size_t)ref], d.nxy[2 * (size_t)ref + 1], d.poses[d.oimg[ref]].P,
                                                d.xyz + 3 * (size_t)slot);
        if (e < DBL_MAX && e <= d.re_max) {  // (17.2: the best candidate starts at DBL_MAX; NaN is never the best)
            d.opoint[ref] = slot;
            d.action[k] = s1 >= 0 ? AMC_RETRI_CONTINUE_1TO2 : AMC_RETRI_CONTINUE_2TO1;
        }
        return;
    }
    // Create on [obs1, obs2]
    if (d.two_view && d.two_view[k]) return;
    PairView v;
    v.x0 = d.nxy[2 * (size_t)o1];
    v.y0 = d.nxy[2 * (size_t)o1 + 1];
    v.x1 = d.nxy[2 * (size_t)o2];
    v.y1 = d.nxy[2 * (size_t)o2 + 1];
    v.p0 = d.poses + d.oimg[o1];
    v.p1 = d.poses + d.oimg[o2];
    v.mask = d.mask + 2 * k;
    v.max_residual = d.max_residual;
    v.min_tri_angle = d.min_tri_angle;
    double X[3];
    TriSupport best;
    tri::tri_lo_ransac(v, 0, 2, d.max_trials, 1, nullptr, X, best);  // two observations: min_trials = 2 * 1 / 2
    if (best.cnt < 2) return;
    tri::tri_score(v, 0, 2, X, true);  // the final mask
    if (!(v.mask[0] && v.mask[1])) return;  // (cannot happen: the mask repeats best's count on the same model)
    const uint32_t slot = d.npoints + (uint32_t)k;
    for (int c = 0; c < 3; ++c) d.xyz[3 * (size_t)slot + c] = X[c];
    d.opoint[o1] = (int32_t)slot;
    d.opoint[o2] = (int32_t)slot;
    d.action[k] = AMC_RETRI_CREATED;
}

void free_arrays(amc_retri_result* r) {
    std::free(r->pair_ran);
    std::free(r->pair_num_tri);
    std::free(r->corr_action);
    std::free(r->created_offsets);
    std::free(r->created_xyz);
    r->pair_ran = nullptr;
    r->pair_num_tri = nullptr;
    r->corr_action = nullptr;
    r->created_offsets = nullptr;
    r->created_xyz = nullptr;
}

// new_xyz: 3 per correspondence, the slots behind the existing points as the device left them
int run_device(amc_ctx* ctx, const amc_retri_problem& pb, const amc_retri_opts& op, const std::vector<retri::Launch>& launches,
               amc_retri_result* result, std::vector<double>* new_xyz) {
    static const char* const hipchk_who = "amc_retriangulate_pairs";
    const size_t ncam = pb.num_cameras, nimg = pb.num_images, nobs = pb.num_obs, npt = pb.num_points, np = pb.num_pairs;
    const uint64_t nc = pb.pair_offsets[np];
    // the whole call's plan first, so that the device clock below holds copies and kernels only
    std::vector<uint32_t> cpair(std::max<uint64_t>(nc, 1), 0);
    for (size_t p = 0; p < np; ++p)
        for (uint64_t k = pb.pair_offsets[p]; k < pb.pair_offsets[p + 1]; ++k) cpair[k] = (uint32_t)p;
    std::vector<double> nxy_host;
    const bool host_lift = retri::lift_libm_observations(pb, &nxy_host);
    new_xyz->assign(std::max<uint64_t>(3 * nc, 1), 0.0);
    const uint64_t max_trials = tvg::ransac_max_trials(triobs::kMaxNumTrials, triobs::kMinInlierRatio, triobs::kConfidence,
                                                       triobs::kDynMultiplier, triobs::kMinSamples);

    const CtxView cv = ctx_view(ctx);
    HIPCHK(hipSetDevice(cv.device));
    hipStream_t st = cv.stream;
    Dev d{};
    int32_t* d_cmodel;
    uint32_t *d_icam, *d_oimg, *d_cobs, *d_cpair;
    double *d_cparams, *d_q, *d_t, *d_oxy;
    uint64_t* d_poff;
    uint8_t* d_two;
    DevBuf<void> mem;  // the call's working set: allocated here, freed on return
    DevParts parts;
    parts.part(&d_cmodel, ncam).part(&d_cparams, kKC * ncam).part(&d_icam, nimg).part(&d_q, 4 * nimg).part(&d_t, 3 * nimg)
        .part(&d.poses, nimg).part(&d_oimg, nobs).part(&d_oxy, 2 * nobs).part(&d.nxy, 2 * nobs).part(&d.opoint, nobs)
        .part(&d.xyz, 3 * (npt + nc)).part(&d_poff, np + 1).part(&d_cobs, 2 * nc).part(&d_cpair, nc).part(&d_two, nc)
        .part(&d.ran, np).part(&d.ntri, np).part(&d.action, nc).part(&d.mask, 2 * nc);
    {
        const auto t0 = std::chrono::steady_clock::now();
        const hipError_t e = parts.carve(mem);
        if (e == hipErrorOutOfMemory) return api_fail(AMC_E_NOMEM, "%s: out of device memory", hipchk_who);
        HIPCHK(e);
        result->alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    // an early return must not leave copies in flight that read the plan above or write the result's arrays
    struct Drain {
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{st};
    StreamTimer timer(st), copies(st);  // timer: the device clock and the kernels' span; copies: the copies' spans
    HIPCHK(timer.start());
    d.nimg = (uint32_t)nimg;
    d.nobs = (uint32_t)nobs;
    d.npoints = (uint32_t)npt;
    const double max_error = triobs::kDegToRad * op.create_max_angle_error;
    d.max_residual = max_error * max_error;
    d.min_tri_angle = triobs::kDegToRad * op.min_angle;
    d.re_max = triobs::kDegToRad * op.re_max_angle_error;
    d.re_min_ratio = op.re_min_ratio;
    d.max_trials = max_trials;
    d.cmodel = d_cmodel;
    d.cparams = d_cparams;
    d.icam = d_icam;
    d.q = d_q;
    d.t = d_t;
    d.oimg = d_oimg;
    d.oxy = d_oxy;
    d.poff = d_poff;
    d.cobs = d_cobs;
    d.cpair = d_cpair;
    d.two_view = pb.corr_two_view ? d_two : nullptr;
    auto up = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    auto down = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
#define RETRI_LAUNCH(kernel, grid)                                        \
    do {                                                                  \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, st, d);   \
        HIPCHK(hipGetLastError());                                        \
    } while (0)
    HIPCHK(copies.span_begin());
    HIPCHK(up(d_cmodel, pb.camera_models, ncam * 4));
    HIPCHK(up(d_cparams, pb.camera_params, ncam * kKC * 8));
    HIPCHK(up(d_icam, pb.image_cameras, nimg * 4));
    HIPCHK(up(d_q, pb.qvec, nimg * 32));
    HIPCHK(up(d_t, pb.tvec, nimg * 24));
    HIPCHK(up(d_oimg, pb.obs_image, nobs * 4));
    HIPCHK(up(d_oxy, pb.obs_xy, nobs * 16));
    HIPCHK(up(d.opoint, pb.obs_point, nobs * 4));
    if (host_lift) HIPCHK(up(d.nxy, nxy_host.data(), nobs * 16));
    HIPCHK(up(d.xyz, pb.point_xyz, npt * 24));
    HIPCHK(up(d_poff, pb.pair_offsets, (np + 1) * 8));
    HIPCHK(up(d_cobs, pb.corr_obs, nc * 8));
    HIPCHK(up(d_cpair, cpair.data(), nc * 4));
    if (pb.corr_two_view) HIPCHK(up(d_two, pb.corr_two_view, nc));
    if (nc) HIPCHK(hipMemsetAsync(d.action, 0, nc, st));
    if (nc) HIPCHK(hipMemsetAsync(d.xyz + 3 * npt, 0, nc * 24, st));
    if (np) HIPCHK(hipMemsetAsync(d.ran, 0, np, st));
    if (np) HIPCHK(hipMemsetAsync(d.ntri, 0, np * 4, st));
    HIPCHK(copies.span_end());
    HIPCHK(timer.span_begin());
    if (nimg) RETRI_LAUNCH(retri_pose_kernel, blocks_for(nimg));
    if (nobs) RETRI_LAUNCH(retri_lift_kernel, blocks_for(nobs));
    // the rounds follow one another on the stream: a kernel sees what every earlier one wrote
    for (const retri::Launch& l : launches) {
        d.pair_first = (uint32_t)l.first;
        d.pair_last = (uint32_t)l.last;
        d.corr_first = pb.pair_offsets[l.first];
        d.corr_last = pb.pair_offsets[l.last];
        RETRI_LAUNCH(retri_ratio_kernel, blocks_for((l.last - l.first) * kWave));
        if (d.corr_last > d.corr_first) RETRI_LAUNCH(retri_corr_kernel, blocks_for(d.corr_last - d.corr_first));
    }
    HIPCHK(timer.span_end());
#undef RETRI_LAUNCH
    HIPCHK(copies.span_begin());
    HIPCHK(down(result->pair_ran, d.ran, np));
    HIPCHK(down(result->pair_num_tri, d.ntri, np * 4));
    HIPCHK(down(result->corr_action, d.action, nc));
    HIPCHK(down(new_xyz->data(), d.xyz + 3 * npt, nc * 24));
    HIPCHK(copies.span_end());
    result->num_launches = (uint32_t)launches.size();
    HIPCHK(timer.stop(result->device_ms));
    HIPCHK(timer.spans(result->kernel_ms));
    HIPCHK(copies.spans(result->copy_ms));
    return AMC_OK;
}

int run(amc_ctx* ctx, const amc_retri_problem* pb, const amc_retri_opts* options, amc_retri_result* result) {
    const char* fn = "amc_retriangulate_pairs";
    const auto host_t0 = std::chrono::steady_clock::now();
    if (result) std::memset(result, 0, sizeof *result);
    if (!ctx || !pb || !result) return api_fail(AMC_E_INVALID, "%s: NULL argument", fn);
    amc_retri_opts op;
    amc_retri_opts_default(&op);
    if (options) op = *options;
    // (the test hook is read before anything can fail, once per call)
    const uint64_t max_corrs = (uint64_t)env_int("AMC_RETRI_BATCH_CORRS", (long long)retri::kMaxLaunchCorrs, 1, (long long)retri::kMaxLaunchCorrs);
    std::string bad = retri::check_options(op);
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: invalid options (%s)", fn, bad.c_str());
    try {
        bad = retri::check_problem(*pb);
    } catch (const std::bad_alloc&) {
        return api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: %s", fn, bad.c_str());
    const size_t np = pb->num_pairs;
    const uint64_t nc = pb->pair_offsets[np];
    result->num_pairs = np;
    result->num_corrs = nc;
    result->pair_ran = (uint8_t*)std::calloc(std::max<size_t>(np, 1), 1);
    result->pair_num_tri = (uint32_t*)std::calloc(std::max<size_t>(np, 1), 4);
    result->corr_action = (uint8_t*)std::calloc(std::max<uint64_t>(nc, 1), 1);
    result->created_offsets = (uint64_t*)std::calloc(np + 1, 8);
    if (!result->pair_ran || !result->pair_num_tri || !result->corr_action || !result->created_offsets) {
        free_arrays(result);
        return api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    int rc = AMC_OK;
    try {
        std::vector<double> new_xyz;
        const std::vector<retri::Launch> launches = retri::plan_launches(*pb, max_corrs);
        rc = np ? run_device(ctx, *pb, op, launches, result, &new_xyz) : AMC_OK;
        if (rc == AMC_OK) {
            // the created points, compacted in correspondence order
            for (size_t p = 0; p < np; ++p) {
                uint64_t made = 0;
                for (uint64_t k = pb->pair_offsets[p]; k < pb->pair_offsets[p + 1]; ++k) {
                    const uint8_t a = result->corr_action[k];
                    made += a == AMC_RETRI_CREATED;
                    result->num_continued += a == AMC_RETRI_CONTINUE_1TO2 || a == AMC_RETRI_CONTINUE_2TO1;
                }
                result->created_offsets[p + 1] = result->created_offsets[p] + made;
                result->num_pairs_run += result->pair_ran[p] != 0;
            }
            result->num_created = result->created_offsets[np];
            result->created_xyz = (double*)std::calloc(std::max<uint64_t>(result->num_created, 1) * 3, 8);
            if (!result->created_xyz) {
                rc = api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
            } else {
                uint64_t at = 0;
                for (uint64_t k = 0; k < nc; ++k)
                    if (result->corr_action[k] == AMC_RETRI_CREATED) std::memcpy(result->created_xyz + 3 * at++, new_xyz.data() + 3 * k, 24);
            }
        }
    } catch (const std::bad_alloc&) {
        rc = api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    if (rc != AMC_OK) {
        free_arrays(result);
        return rc;
    }
    result->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count() - result->device_ms;
    return AMC_OK;
}

}  // namespace

extern "C" {

void amc_retri_opts_default(amc_retri_opts* o) {
    if (!o) return;
    o->create_max_angle_error = 2.0;  // IncrementalTriangulator::Options
    o->re_max_angle_error = 5.0;
    o->min_angle = 1.5;
    o->re_min_ratio = 0.2;
}

int amc_retriangulate_pairs(amc_ctx* ctx, const amc_retri_problem* problem, const amc_retri_opts* options,
                            amc_retri_result* result) {
    return run(ctx, problem, options, result);
}

void amc_retri_result_free(amc_retri_result* r) {
    if (!r) return;
    free_arrays(r);
}

}  // extern "C"
