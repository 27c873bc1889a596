// triobs.hip — the observation triangulator on gfx950 (include/amc_triobs.h): the arithmetic of COLMAP 3.9.1's
// IncrementalTriangulator::TriangulateImage restated in DESIGN.md section 17.  Every FP64 operation is written in the
// order of that section and of section 11, the order tests/triangulator_ref follows too: the two are bit-identical.
//
// Work split (17.5).  One lane per image builds [R | t] and the projection centre as 11.1 does; one lane per candidate
// lifts its pixel with cam::cam_from_img (the models that need libm are lifted on the host, as everywhere in this
// library); then one lane per item runs Continue and every Create round without returning to the host: the LO-RANSAC
// is tri_core.h's, the one tri.hip runs per track.  A round's observations are the entries of the item's slice of a
// work list of candidate indices, which the lane compacts to the left-over observations after each round.  The host
// orders a batch's items by length, longest first, as in 11.5.  An item's result depends on its own candidates only,
// never on its neighbours, the batch or the order.  No atomics, no LDS.
#include <cfloat>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "amc_internal.h"
#include "camera_math.h"
#include "tri_core.h"
#include "triobs_plan.h"
#include "../../include/amc_triobs.h"

using namespace amc;

namespace {

using tri::TriPose;
using tri::TriSupport;

constexpr int kBlock = 256;
constexpr int kKC = cam::kMaxParams;
// device batch bounds: a call with more items or candidates is split on item boundaries
constexpr uint64_t kMaxBatchItems = (uint64_t)1 << 20;
constexpr uint64_t kMaxBatchCands = (uint64_t)1 << 23;

struct Dev {
    uint32_t nimg, nitems, ncand;
    double max_residual;   // DegToRad(create_max_angle_error)^2
    double min_tri_angle;  // DegToRad(min_angle)
    double continue_max;   // DegToRad(continue_max_angle_error)
    uint64_t max_trials;   // 10000 after the RANSAC constructor's clamp
    // the model (the whole call's)
    const int32_t* cmodel;
    const double* cparams;
    const uint32_t* icam;
    const double *q, *t;
    TriPose* poses;
    const uint64_t* dyn_off;  // by round length (< dyn_n): start of its dyn_max_num_trials row in dyn_tab, or kNoTable
    const uint64_t* dyn_tab;
    uint64_t dyn_n;
    // the batch
    const uint32_t* off;    // nitems + 1, batch-local
    const uint32_t* order;  // nitems: batch-local item index, longest items first
    const uint32_t* slots;  // nitems + 1: the items' round slots
    const uint32_t* cimg;
    const double* cxy;
    const uint8_t* chas;
    const double* cxyz;
    const uint8_t* two_view;  // nullptr: all zero
    double* nxy;      // 2 per candidate: the normalised image point
    uint32_t* work;   // per candidate: the item's round list
    uint8_t* mask;    // per work entry
    int32_t* cont;    // per item
    uint32_t* cround; // per candidate, zeroed before the kernels
    uint32_t* nround; // per item
    double* rxyz;     // 3 per round slot
    // tri_core.h's view: observation o is work entry o
    __device__ __forceinline__ double x(uint64_t o) const { return nxy[2 * (uint64_t)work[o]]; }
    __device__ __forceinline__ double y(uint64_t o) const { return nxy[2 * (uint64_t)work[o] + 1]; }
    __device__ __forceinline__ const TriPose& pose(uint64_t o) const { return poses[cimg[work[o]]]; }
};

unsigned blocks_for(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// 11.1: [R | t] with the Rigid3d binding's quaternion -> matrix arithmetic, the centre -(R^T t)
__global__ __launch_bounds__(kBlock) void triobs_pose_kernel(Dev d) {
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

__global__ __launch_bounds__(kBlock) void triobs_lift_kernel(Dev d) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= d.ncand) return;
    const uint32_t c = d.icam[d.cimg[k]];
    const int model = d.cmodel[c];
    if (cam::needs_libm(model)) return;  // the host's value is already there
    double prm[kKC], u, v;
    for (int i = 0; i < kKC; ++i) prm[i] = d.cparams[kKC * c + i];
    cam::cam_from_img(model, prm, d.cxy[2 * (size_t)k], d.cxy[2 * (size_t)k + 1], u, v);
    d.nxy[2 * (size_t)k] = u;
    d.nxy[2 * (size_t)k + 1] = v;
}

// 17.2 and 17.3 for one item per lane
__global__ __launch_bounds__(kBlock) void triobs_item_kernel(Dev d) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= d.nitems) return;
    const uint32_t it = d.order[g];
    const uint32_t c0 = d.off[it], n = d.off[it + 1] - c0;  // n >= 1: the reference observation is the last candidate
    const uint32_t ref = c0 + n - 1;
    bool ref_has = d.chas[ref] != 0;
    // Continue
    int32_t cont = -1;
    if (!ref_has) {
        const double rx = d.nxy[2 * (size_t)ref], ry = d.nxy[2 * (size_t)ref + 1];
        const double* P = d.poses[d.cimg[ref]].P;
        double best = DBL_MAX;
        for (uint32_t k = 0; k + 1 < n; ++k) {
            if (!d.chas[c0 + k]) continue;
            const double e = tri::tri_angular_error(rx, ry, P, d.cxyz + 3 * (size_t)(c0 + k));
            if (e < best) {
                best = e;
                cont = (int32_t)k;
            }
        }
        if (cont >= 0 && best <= d.continue_max)
            ref_has = true;
        else
            cont = -1;
    }
    d.cont[it] = cont;
    // Create: the observations without a point
    uint32_t m = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const bool has = k + 1 == n ? ref_has : d.chas[c0 + k] != 0;
        if (!has) d.work[c0 + m++] = c0 + k;
    }
    const uint32_t s0 = d.slots[it], cap = d.slots[it + 1] - s0;
    uint32_t round = 0;
    while (m >= 2 && round < cap) {
        if (round == 0 && m == 2 && d.two_view && d.two_view[it]) break;
        const uint64_t min_trials = m <= triobs::kAllTrialsUpTo ? (uint64_t)m * (m - 1) / 2 : 0;
        const uint64_t tab = m < d.dyn_n ? d.dyn_off[m] : tri::kNoTable;
        double X[3];
        TriSupport best;
        tri::tri_lo_ransac(d, c0, m, d.max_trials, min_trials, tab == tri::kNoTable ? nullptr : d.dyn_tab + tab, X, best);
        if (best.cnt < 2) break;
        tri::tri_score(d, c0, m, X, true);  // the final mask
        round += 1;
        for (int c = 0; c < 3; ++c) d.rxyz[3 * (size_t)(s0 + round - 1) + c] = X[c];
        uint32_t left = 0;
        for (uint32_t k = 0; k < m; ++k) {
            const uint32_t cand = d.work[c0 + k];
            if (d.mask[c0 + k])
                d.cround[cand] = round;
            else
                d.work[c0 + left++] = cand;
        }
        if (left < 3) break;  // kMinRecursiveTrackLength
        m = left;
    }
    d.nround[it] = round;
}

void free_arrays(amc_triobs_result* r) {
    std::free(r->continued);
    std::free(r->cand_round);
    std::free(r->round_offsets);
    std::free(r->round_xyz);
    r->continued = nullptr;
    r->cand_round = nullptr;
    r->round_offsets = nullptr;
    r->round_xyz = nullptr;
}

// what the batches leave on the host before the result's round arrays are built
struct Raw {
    std::vector<uint32_t> slots;   // per batch: items + 1
    std::vector<size_t> slots_at;  // per batch: start in slots
    std::vector<uint32_t> nround;  // per item
    std::vector<double> rxyz;      // per batch: 3 per round slot
    std::vector<size_t> rxyz_at;
};

int run_batches(amc_ctx* ctx, const amc_triobs_problem& pb, const amc_triobs_opts& op, const Batches& batches,
                amc_triobs_result* result, Raw* raw) {
    static const char* const hipchk_who = "amc_triangulate_observations";
    const size_t ncam = pb.num_cameras, nimg = pb.num_images, nit = pb.num_items, nb = batches.count();
    // the whole call's plan first, so that the device clock below holds copies and kernels only
    std::vector<uint32_t> off, order;
    std::vector<size_t> order_at(nb + 1, 0), off_at(nb + 1, 0);
    raw->slots_at.assign(nb + 1, 0);
    raw->rxyz_at.assign(nb + 1, 0);
    raw->nround.assign(std::max<size_t>(nit, 1), 0);
    size_t most_slots = 0;
    for (size_t b = 0; b < nb; ++b) {
        const size_t first = batches.start[b], last = batches.start[b + 1];
        triobs::plan_batch(pb.item_offsets, first, last, &order, &raw->slots);
        for (size_t i = first; i <= last; ++i) off.push_back((uint32_t)(pb.item_offsets[i] - pb.item_offsets[first]));
        order_at[b + 1] = order.size();
        off_at[b + 1] = off.size();
        raw->slots_at[b + 1] = raw->slots.size();
        raw->rxyz_at[b + 1] = raw->rxyz_at[b] + 3 * (size_t)raw->slots.back();
        most_slots = std::max<size_t>(most_slots, raw->slots.back());
    }
    raw->rxyz.assign(std::max<size_t>(raw->rxyz_at[nb], 1), 0.0);
    std::vector<double> nxy_host;
    const bool host_lift = triobs::lift_libm_candidates(pb, &nxy_host);
    // the trial table: a row for every round length that can stop early (more than kAllTrialsUpTo observations)
    const uint64_t max_trials = tvg::ransac_max_trials(triobs::kMaxNumTrials, triobs::kMinInlierRatio, triobs::kConfidence,
                                                       triobs::kDynMultiplier, triobs::kMinSamples);
    uint64_t nmax = 0;
    for (size_t i = 0; i < nit; ++i) nmax = std::max<uint64_t>(nmax, pb.item_offsets[i + 1] - pb.item_offsets[i]);
    std::vector<uint64_t> dyn_off(nmax + 1, tri::kNoTable), dyn_tab;
    for (uint64_t n = triobs::kAllTrialsUpTo + 1; n <= nmax; ++n) {
        dyn_off[n] = dyn_tab.size();
        for (uint64_t c = 0; c <= n; ++c)
            dyn_tab.push_back(tvg::compute_num_trials(c, n, triobs::kConfidence, triobs::kDynMultiplier, triobs::kMinSamples));
    }
    if (dyn_tab.empty()) dyn_tab.push_back(0);

    const CtxView cv = ctx_view(ctx);
    HIPCHK(hipSetDevice(cv.device));
    hipStream_t st = cv.stream;
    const size_t mi = batches.most_items, mc = batches.most_elems;
    Dev d{};
    int32_t* d_cmodel;
    uint32_t *d_icam, *d_off, *d_order, *d_slots, *d_cimg;
    double *d_cparams, *d_q, *d_t, *d_cxy, *d_cxyz;
    uint8_t *d_chas, *d_two;
    uint64_t *d_doff, *d_dtab;
    DevBuf<void> mem;  // the call's working set: allocated here, freed on return
    DevParts parts;
    parts.part(&d_cmodel, ncam).part(&d_cparams, kKC * ncam).part(&d_icam, nimg).part(&d_q, 4 * nimg).part(&d_t, 3 * nimg)
        .part(&d.poses, nimg).part(&d_doff, dyn_off.size()).part(&d_dtab, dyn_tab.size()).part(&d_off, mi + 1)
        .part(&d_order, mi).part(&d_slots, mi + 1).part(&d_cimg, mc).part(&d_cxy, 2 * mc).part(&d_chas, mc)
        .part(&d_cxyz, 3 * mc).part(&d_two, mi).part(&d.nxy, 2 * mc).part(&d.work, mc).part(&d.mask, mc)
        .part(&d.cont, mi).part(&d.cround, mc).part(&d.nround, mi).part(&d.rxyz, 3 * most_slots);
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
    const double max_error = triobs::kDegToRad * op.create_max_angle_error;
    d.max_residual = max_error * max_error;
    d.min_tri_angle = triobs::kDegToRad * op.min_angle;
    d.continue_max = triobs::kDegToRad * op.continue_max_angle_error;
    d.max_trials = max_trials;
    d.cmodel = d_cmodel;
    d.cparams = d_cparams;
    d.icam = d_icam;
    d.q = d_q;
    d.t = d_t;
    d.dyn_off = d_doff;
    d.dyn_tab = d_dtab;
    d.dyn_n = dyn_off.size();
    d.off = d_off;
    d.order = d_order;
    d.slots = d_slots;
    d.cimg = d_cimg;
    d.cxy = d_cxy;
    d.chas = d_chas;
    d.cxyz = d_cxyz;
    d.two_view = pb.no_create_two_view ? d_two : nullptr;
    auto up = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    auto down = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
#define TRIOBS_LAUNCH(kernel, grid)                                       \
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
    HIPCHK(up(d_doff, dyn_off.data(), dyn_off.size() * 8));
    HIPCHK(up(d_dtab, dyn_tab.data(), dyn_tab.size() * 8));
    HIPCHK(copies.span_end());
    if (nimg) {
        HIPCHK(timer.span_begin());
        TRIOBS_LAUNCH(triobs_pose_kernel, blocks_for(nimg));
        HIPCHK(timer.span_end());
    }
    // The batches follow one another on the stream and reuse the device buffers; every host array a copy reads or
    // writes (the caller's, the plan's, the result's) lives until timer.stop() below has waited for the stream.
    for (size_t b = 0; b < nb; ++b) {
        const size_t first = batches.start[b], last = batches.start[b + 1], ni = last - first;
        const uint64_t cbase = pb.item_offsets[first], nc = pb.item_offsets[last] - cbase;
        const uint32_t nslots = raw->slots[raw->slots_at[b + 1] - 1];
        d.nitems = (uint32_t)ni;
        d.ncand = (uint32_t)nc;
        HIPCHK(copies.span_begin());
        HIPCHK(up(d_off, off.data() + off_at[b], (ni + 1) * 4));
        HIPCHK(up(d_order, order.data() + order_at[b], ni * 4));
        HIPCHK(up(d_slots, raw->slots.data() + raw->slots_at[b], (ni + 1) * 4));
        HIPCHK(up(d_cimg, pb.cand_image + cbase, nc * 4));
        HIPCHK(up(d_cxy, pb.cand_xy + 2 * cbase, nc * 16));
        HIPCHK(up(d_chas, pb.cand_has_point + cbase, nc));
        HIPCHK(up(d_cxyz, pb.cand_xyz + 3 * cbase, nc * 24));
        if (pb.no_create_two_view) HIPCHK(up(d_two, pb.no_create_two_view + first, ni));
        if (host_lift) HIPCHK(up(d.nxy, nxy_host.data() + 2 * cbase, nc * 16));
        HIPCHK(hipMemsetAsync(d.cround, 0, nc * 4, st));
        HIPCHK(copies.span_end());
        HIPCHK(timer.span_begin());
        TRIOBS_LAUNCH(triobs_lift_kernel, blocks_for(nc));
        TRIOBS_LAUNCH(triobs_item_kernel, blocks_for(ni));
        HIPCHK(timer.span_end());
        HIPCHK(copies.span_begin());
        HIPCHK(down(result->continued + first, d.cont, ni * 4));
        HIPCHK(down(result->cand_round + cbase, d.cround, nc * 4));
        HIPCHK(down(raw->nround.data() + first, d.nround, ni * 4));
        HIPCHK(down(raw->rxyz.data() + raw->rxyz_at[b], d.rxyz, (size_t)nslots * 24));
        HIPCHK(copies.span_end());
    }
#undef TRIOBS_LAUNCH
    result->num_batches = (uint32_t)nb;
    HIPCHK(timer.stop(result->device_ms));
    HIPCHK(timer.spans(result->kernel_ms));
    HIPCHK(copies.spans(result->copy_ms));
    return AMC_OK;
}

int run(amc_ctx* ctx, const amc_triobs_problem* pb, const amc_triobs_opts* options, amc_triobs_result* result) {
    const char* fn = "amc_triangulate_observations";
    const auto host_t0 = std::chrono::steady_clock::now();
    if (result) std::memset(result, 0, sizeof *result);
    if (!ctx || !pb || !result) return api_fail(AMC_E_INVALID, "%s: NULL argument", fn);
    amc_triobs_opts op;
    amc_triobs_opts_default(&op);
    if (options) op = *options;
    // (the test hook is read before anything can fail, once per call)
    const uint64_t max_items = (uint64_t)env_int("AMC_TRIOBS_BATCH_ITEMS", (long long)kMaxBatchItems, 1, (long long)kMaxBatchItems);
    std::string bad = triobs::check_options(op);
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: invalid options (%s)", fn, bad.c_str());
    try {
        bad = triobs::check_problem(*pb);
    } catch (const std::bad_alloc&) {
        return api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: %s", fn, bad.c_str());
    const size_t nit = pb->num_items;
    const uint64_t ncand = pb->item_offsets[nit];
    result->num_items = nit;
    result->num_candidates = ncand;
    result->continued = (int32_t*)std::calloc(std::max<size_t>(nit, 1), 4);
    result->cand_round = (uint32_t*)std::calloc(std::max<uint64_t>(ncand, 1), 4);
    result->round_offsets = (uint64_t*)std::calloc(nit + 1, 8);
    if (!result->continued || !result->cand_round || !result->round_offsets) {
        free_arrays(result);
        return api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    int rc = AMC_OK;
    try {
        Raw raw;
        const Batches batches = split_batches(pb->item_offsets, nit, max_items, kMaxBatchCands);
        rc = nit ? run_batches(ctx, *pb, op, batches, result, &raw) : AMC_OK;
        if (rc == AMC_OK) {
            // the created tracks, compacted in item order
            for (size_t i = 0; i < nit; ++i) {
                result->round_offsets[i + 1] = result->round_offsets[i] + raw.nround[i];
                result->num_continued += result->continued[i] >= 0;
            }
            result->num_created = result->round_offsets[nit];
            result->round_xyz = (double*)std::calloc(std::max<uint64_t>(result->num_created, 1) * 3, 8);
            if (!result->round_xyz) {
                rc = api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
            } else {
                for (size_t b = 0; b < batches.count() && nit; ++b) {
                    const size_t first = batches.start[b], last = batches.start[b + 1];
                    const uint32_t* slots = raw.slots.data() + raw.slots_at[b];
                    for (size_t i = first; i < last; ++i)
                        std::memcpy(result->round_xyz + 3 * result->round_offsets[i],
                                    raw.rxyz.data() + raw.rxyz_at[b] + 3 * (size_t)slots[i - first], (size_t)raw.nround[i] * 24);
                }
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

void amc_triobs_opts_default(amc_triobs_opts* o) {
    if (!o) return;
    o->create_max_angle_error = 2.0;  // IncrementalTriangulator::Options
    o->continue_max_angle_error = 2.0;
    o->min_angle = 1.5;
    o->reserved = 0.0;
}

int amc_triangulate_observations(amc_ctx* ctx, const amc_triobs_problem* problem, const amc_triobs_opts* options,
                                 amc_triobs_result* result) {
    return run(ctx, problem, options, result);
}

void amc_triobs_result_free(amc_triobs_result* r) {
    if (!r) return;
    free_arrays(r);
}

}  // extern "C"
