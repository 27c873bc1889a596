// filter.hip — the point filter on gfx950 (include/amc_filter.h): COLMAP 3.9.1's FilterPoints3D restated in DESIGN.md
// section 16.  Every FP64 operation is written in the order of that section, the order tests/filter_ref/filter_ref.cc
// follows too: the two are bit-identical.
//
// Work split (16.4).  One lane per image for the projection centres, one lane per observation for the squared errors.
// The points come in two classes, decided on the host (filter_plan.h): a selected track of kWaveClassMin elements or
// more gets a wave, whose lanes share the pairs of one element with all earlier ones and vote; every other point gets
// a lane.  A point's error sum runs in track order in both classes (in the wave class every lane runs the same sum).
// A point's result depends on its own observations only, never on its neighbours, the batch or the order.  No atomics,
// no LDS: the vote is a ballot.
#include <cfloat>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "amc_internal.h"
#include "filter_core.h"
#include "filter_plan.h"
#include "../../include/amc_filter.h"

using namespace amc;

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kKC = ba::kMaxParams;
// device batch bounds: a call with more points or observations is split on point boundaries
constexpr uint64_t kMaxBatchPoints = (uint64_t)1 << 22;
constexpr uint64_t kMaxBatchObs = (uint64_t)1 << 24;

struct Dev {
    uint32_t nimg, npts, nobs, nwave;
    int32_t errors_only;
    double max2, min_angle;
    // the model (the whole call's)
    const int32_t* cmodel;
    const double* cparams;
    const uint32_t* icam;
    const double *q, *t;
    double* centre;
    // the batch
    const double* X;
    const uint32_t* off;   // npts + 1, batch-local
    const uint32_t* oimg;
    const uint32_t* opt;   // batch-local point of each observation
    const double* oxy;
    const uint8_t* sel;    // nullptr: every point
    const uint32_t* wave_points;
    double* e2;
    uint8_t* del;          // zeroed before the kernels
    uint8_t* verdict;
    double* perr;
};

unsigned blocks_for(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

__global__ __launch_bounds__(kBlock) void filter_centre_kernel(Dev d) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= d.nimg) return;
    double C[3];
    filt::projection_centre(d.q + 4 * i, d.t + 3 * i, C);
    for (int k = 0; k < 3; ++k) d.centre[3 * i + k] = C[k];
}

__global__ __launch_bounds__(kBlock) void filter_error_kernel(Dev d) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    if (o >= d.nobs) return;
    const uint32_t i = d.oimg[o], j = d.opt[o], c = d.icam[i];
    d.e2[o] = filt::squared_reprojection_error(d.cmodel[c], d.cparams + kKC * c, d.q + 4 * i, d.t + 3 * i, d.X + 3 * j,
                                               d.oxy + 2 * o);
}

// 16.3 for one point per lane: every point that is not the wave kernel's
__global__ __launch_bounds__(kBlock) void filter_point_lane_kernel(Dev d) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= d.npts) return;
    if (d.sel && !d.sel[j]) {
        d.verdict[j] = AMC_FILTER_NOT_SELECTED;
        d.perr[j] = 0.0;
        return;
    }
    const uint32_t o0 = d.off[j], L = d.off[j + 1] - o0;
    if (L >= filt::kWaveClassMin) return;
    if (d.errors_only) {
        double sum = 0.0;
        for (uint32_t k = 0; k < L; ++k) sum = sum + ba::dsqrt(d.e2[o0 + k]);
        d.verdict[j] = AMC_FILTER_KEPT;
        d.perr[j] = L ? sum / (double)L : 0.0;
        return;
    }
    d.perr[j] = 0.0;
    if (L < 2) {
        d.verdict[j] = AMC_FILTER_SHORT_TRACK;
        return;
    }
    uint32_t marked = 0;
    double sum = 0.0;
    for (uint32_t k = 0; k < L; ++k) {
        const double e = d.e2[o0 + k];
        if (e > d.max2) {
            d.del[o0 + k] = 1;
            ++marked;
        } else {
            sum = sum + ba::dsqrt(e);
        }
    }
    if (marked >= L - 1) {
        d.verdict[j] = AMC_FILTER_REPROJECTION;
        return;
    }
    d.perr[j] = sum / (double)(L - marked);
    const double* X = d.X + 3 * j;
    bool found = false;
    for (uint32_t i1 = 1; i1 < L && !found; ++i1) {
        if (d.e2[o0 + i1] > d.max2) continue;
        const double* c1 = d.centre + 3 * d.oimg[o0 + i1];
        for (uint32_t i2 = 0; i2 < i1; ++i2) {
            if (d.e2[o0 + i2] > d.max2) continue;
            if (tri::tri_angle(c1, d.centre + 3 * d.oimg[o0 + i2], X) >= d.min_angle) {
                found = true;
                break;
            }
        }
    }
    d.verdict[j] = found ? AMC_FILTER_KEPT : AMC_FILTER_ANGLE;
}

// 16.3 for one listed point per wave
__global__ __launch_bounds__(kBlock) void filter_point_wave_kernel(Dev d) {
    const uint32_t w = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (w >= d.nwave) return;  // the whole wave leaves
    const uint32_t j = d.wave_points[w];
    const uint32_t o0 = d.off[j], L = d.off[j + 1] - o0;
    const bool thresholds = !d.errors_only;
    // the marks and the sum in track order: the same in every lane
    uint32_t marked = 0;
    double sum = 0.0;
    for (uint32_t k = 0; k < L; ++k) {
        const double e = d.e2[o0 + k];
        if (thresholds && e > d.max2)
            ++marked;
        else
            sum = sum + ba::dsqrt(e);
    }
    if (!thresholds) {
        if (lane == 0) {
            d.verdict[j] = AMC_FILTER_KEPT;
            d.perr[j] = L ? sum / (double)L : 0.0;
        }
        return;
    }
    for (uint32_t k = lane; k < L; k += kWave)
        if (d.e2[o0 + k] > d.max2) d.del[o0 + k] = 1;
    if (marked >= L - 1) {  // (a listed track has kWaveClassMin elements or more: never a short one)
        if (lane == 0) {
            d.verdict[j] = AMC_FILTER_REPROJECTION;
            d.perr[j] = 0.0;
        }
        return;
    }
    const double* X = d.X + 3 * j;
    bool found = false;
    for (uint32_t i1 = 1; i1 < L && !found; ++i1) {
        if (d.e2[o0 + i1] > d.max2) continue;  // wave-uniform
        const double* c1 = d.centre + 3 * d.oimg[o0 + i1];
        for (uint32_t base = 0; base < i1; base += kWave) {
            const uint32_t i2 = base + lane;
            bool hit = false;
            if (i2 < i1 && !(d.e2[o0 + i2] > d.max2))
                hit = tri::tri_angle(c1, d.centre + 3 * d.oimg[o0 + i2], X) >= d.min_angle;
            if (__ballot(hit) != 0ull) {
                found = true;
                break;
            }
        }
    }
    if (lane == 0) {
        d.verdict[j] = found ? AMC_FILTER_KEPT : AMC_FILTER_ANGLE;
        d.perr[j] = sum / (double)(L - marked);
    }
}

void free_arrays(amc_filter_result* r) {
    std::free(r->obs_sq_error);
    std::free(r->obs_deleted);
    std::free(r->point_verdict);
    std::free(r->point_error);
    r->obs_sq_error = nullptr;
    r->obs_deleted = nullptr;
    r->point_verdict = nullptr;
    r->point_error = nullptr;
}

int run_batches(amc_ctx* ctx, const amc_filter_problem& pb, const amc_filter_opts& op, const Batches& batches,
                amc_filter_result* result) {
    static const char* const hipchk_who = "amc_filter_points3d";
    const size_t ncam = pb.num_cameras, nimg = pb.num_images, nb = batches.count();
    // the whole call's plan first, so that the device clock below holds copies and kernels only
    std::vector<uint32_t> off, opt, wave;
    std::vector<size_t> off_at(nb + 1, 0), opt_at(nb + 1, 0), wave_at(nb + 1, 0);
    off.reserve(pb.num_points + nb);
    opt.reserve((size_t)pb.track_offsets[pb.num_points]);
    for (size_t b = 0; b < nb; ++b) {
        filt::plan_batch(pb, batches.start[b], batches.start[b + 1], filt::kWaveClassMin, &off, &opt, &wave);
        off_at[b + 1] = off.size();
        opt_at[b + 1] = opt.size();
        wave_at[b + 1] = wave.size();
    }
    const CtxView cv = ctx_view(ctx);
    HIPCHK(hipSetDevice(cv.device));
    hipStream_t st = cv.stream;
    const size_t mp = batches.most_items, mo = batches.most_elems;
    Dev d{};
    int32_t* d_cmodel;
    uint32_t *d_icam, *d_off, *d_oimg, *d_opt, *d_wave;
    double *d_cparams, *d_q, *d_t, *d_X, *d_oxy;
    uint8_t* d_sel;
    DevBuf<void> mem;  // the call's working set: allocated here, freed on return
    DevParts parts;
    parts.part(&d_cmodel, ncam).part(&d_cparams, kKC * ncam).part(&d_icam, nimg).part(&d_q, 4 * nimg).part(&d_t, 3 * nimg)
        .part(&d.centre, 3 * nimg).part(&d_X, 3 * mp).part(&d_off, mp + 1).part(&d_oimg, mo).part(&d_opt, mo)
        .part(&d_oxy, 2 * mo).part(&d_sel, mp).part(&d_wave, mp).part(&d.e2, mo).part(&d.del, mo).part(&d.verdict, mp)
        .part(&d.perr, mp);
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
    StreamTimer timer(st), copies(st);  // timer: the device clock and the kernels' spans; copies: the copies' spans
    HIPCHK(timer.start());
    d.nimg = (uint32_t)nimg;
    d.errors_only = op.errors_only ? 1 : 0;
    d.max2 = op.max_reproj_error * op.max_reproj_error;
    d.min_angle = filt::kDegToRad * op.min_tri_angle;
    d.cmodel = d_cmodel;
    d.cparams = d_cparams;
    d.icam = d_icam;
    d.q = d_q;
    d.t = d_t;
    d.X = d_X;
    d.off = d_off;
    d.oimg = d_oimg;
    d.opt = d_opt;
    d.oxy = d_oxy;
    d.sel = pb.selected ? d_sel : nullptr;
    d.wave_points = d_wave;
    auto up = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    auto down = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
#define FILTER_LAUNCH(kernel, grid, block)                               \
    do {                                                                 \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, d);   \
        HIPCHK(hipGetLastError());                                       \
    } while (0)
    HIPCHK(copies.span_begin());
    HIPCHK(up(d_cmodel, pb.camera_models, ncam * 4));
    HIPCHK(up(d_cparams, pb.camera_params, ncam * kKC * 8));
    HIPCHK(up(d_icam, pb.image_cameras, nimg * 4));
    HIPCHK(up(d_q, pb.qvec, nimg * 32));
    HIPCHK(up(d_t, pb.tvec, nimg * 24));
    HIPCHK(copies.span_end());
    if (nimg) {
        HIPCHK(timer.span_begin());
        FILTER_LAUNCH(filter_centre_kernel, blocks_for(nimg), kBlock);
        HIPCHK(timer.span_end());
    }
    // The batches follow one another on the stream and reuse the device buffers; every host array a copy reads or
    // writes (the caller's, the plan's, the result's) lives until timer.stop() below has waited for the stream.
    for (size_t b = 0; b < nb; ++b) {
        const size_t first = batches.start[b], last = batches.start[b + 1], np = last - first;
        const uint64_t obase = pb.track_offsets[first], no = pb.track_offsets[last] - obase;
        d.npts = (uint32_t)np;
        d.nobs = (uint32_t)no;
        d.nwave = (uint32_t)(wave_at[b + 1] - wave_at[b]);
        HIPCHK(copies.span_begin());
        HIPCHK(up(d_X, pb.xyz + 3 * first, np * 24));
        HIPCHK(up(d_off, off.data() + off_at[b], (np + 1) * 4));
        HIPCHK(up(d_oimg, pb.obs_image + obase, no * 4));
        HIPCHK(up(d_opt, opt.data() + opt_at[b], no * 4));
        HIPCHK(up(d_oxy, pb.obs_xy + 2 * obase, no * 16));
        if (pb.selected) HIPCHK(up(d_sel, pb.selected + first, np));
        HIPCHK(up(d_wave, wave.data() + wave_at[b], (size_t)d.nwave * 4));
        if (no) HIPCHK(hipMemsetAsync(d.del, 0, no, st));
        HIPCHK(copies.span_end());
        HIPCHK(timer.span_begin());
        if (no) FILTER_LAUNCH(filter_error_kernel, blocks_for(no), kBlock);
        FILTER_LAUNCH(filter_point_lane_kernel, blocks_for(np), kBlock);
        if (d.nwave) FILTER_LAUNCH(filter_point_wave_kernel, blocks_for((size_t)d.nwave * kWave), kBlock);
        HIPCHK(timer.span_end());
        HIPCHK(copies.span_begin());
        HIPCHK(down(result->obs_sq_error + obase, d.e2, no * 8));
        HIPCHK(down(result->obs_deleted + obase, d.del, no));
        HIPCHK(down(result->point_verdict + first, d.verdict, np));
        HIPCHK(down(result->point_error + first, d.perr, np * 8));
        HIPCHK(copies.span_end());
    }
#undef FILTER_LAUNCH
    result->num_batches = (uint32_t)nb;
    HIPCHK(timer.stop(result->device_ms));
    HIPCHK(timer.spans(result->kernel_ms));
    HIPCHK(copies.spans(result->copy_ms));
    return AMC_OK;
}

int run(amc_ctx* ctx, const amc_filter_problem* pb, const amc_filter_opts* options, amc_filter_result* result) {
    const char* fn = "amc_filter_points3d";
    const auto host_t0 = std::chrono::steady_clock::now();
    if (result) std::memset(result, 0, sizeof *result);
    if (!ctx || !pb || !result) return api_fail(AMC_E_INVALID, "%s: NULL argument", fn);
    amc_filter_opts op;
    amc_filter_opts_default(&op);
    if (options) op = *options;
    // (the test hook is read before anything can fail, once per call)
    const uint64_t max_points = (uint64_t)env_int("AMC_FILTER_BATCH_POINTS", (long long)kMaxBatchPoints, 1, (long long)kMaxBatchPoints);
    std::string bad = filt::check_options(op);
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: invalid options (%s)", fn, bad.c_str());
    try {
        bad = filt::check_problem(*pb);
    } catch (const std::bad_alloc&) {
        return api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: %s", fn, bad.c_str());
    const size_t npts = pb->num_points;
    const uint64_t nobs = pb->track_offsets[npts];
    result->num_points = npts;
    result->num_observations = nobs;
    result->obs_sq_error = (double*)std::calloc(std::max<uint64_t>(nobs, 1), 8);
    result->obs_deleted = (uint8_t*)std::calloc(std::max<uint64_t>(nobs, 1), 1);
    result->point_verdict = (uint8_t*)std::calloc(std::max<size_t>(npts, 1), 1);
    result->point_error = (double*)std::calloc(std::max<size_t>(npts, 1), 8);
    if (!result->obs_sq_error || !result->obs_deleted || !result->point_verdict || !result->point_error) {
        free_arrays(result);
        return api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    int rc = AMC_OK;
    try {
        const Batches batches = split_batches(pb->track_offsets, npts, max_points, kMaxBatchObs);
        rc = run_batches(ctx, *pb, op, batches, result);
    } catch (const std::bad_alloc&) {
        rc = api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    if (rc != AMC_OK) {
        free_arrays(result);
        return rc;
    }
    result->num_filtered = op.errors_only ? 0 : filt::count_filtered(pb->track_offsets, npts, result->point_verdict, result->obs_deleted);
    result->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count() - result->device_ms;
    return AMC_OK;
}

}  // namespace

extern "C" {

void amc_filter_opts_default(amc_filter_opts* o) {
    if (!o) return;
    o->max_reproj_error = 4.0;  // IncrementalMapperOptions' filter_max_reproj_error and filter_min_tri_angle
    o->min_tri_angle = 1.5;
    o->errors_only = 0;
    o->reserved = 0;
}

int amc_filter_points3d(amc_ctx* ctx, const amc_filter_problem* problem, const amc_filter_opts* options,
                        amc_filter_result* result) {
    return run(ctx, problem, options, result);
}

void amc_filter_result_free(amc_filter_result* r) {
    if (!r) return;
    free_arrays(r);
}

}  // extern "C"
