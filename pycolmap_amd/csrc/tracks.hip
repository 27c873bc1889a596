// tracks.hip — the device calls of track completion and track merging on gfx950 (include/amc_tracks.h).  Completion:
// the squared reprojection error of DESIGN.md 16.1 for every candidate observation of a completion walk against its
// point's position, and the pass byte of 18.1.  Merging: 18.2 for the roots of every connected component.  The
// arithmetic is filter_core.h's, the one the point filter and tests/filter_ref use: the bits equal tests/tracks_ref.
//
// Work split.  Completion (18.3): one lane per candidate.  A candidate's result depends on its own pixel, its image and
// its item's position only, never on its neighbours, the batch or the order: the sequential part of 18.1 (which
// observation is already taken when its turn comes) stays on the host.  Merging (18.4): one lane per component, which
// runs the component's roots one after the other; a lane reads and writes its own component's part of every array only,
// so components do not see each other, the batch or the order.  No atomics, no LDS.
#include <cfloat>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "amc_internal.h"
#include "filter_core.h"
#include "tracks_plan.h"
#include "../../include/amc_tracks.h"

using namespace amc;

namespace {

constexpr int kBlock = 256;
constexpr int kKC = ba::kMaxParams;
// merge batch bounds: a call with more components or observations is split on component boundaries
constexpr uint64_t kMaxBatchComponents = (uint64_t)1 << 20;
constexpr uint64_t kMaxBatchMergeObs = (uint64_t)1 << 23;

struct Dev {
    uint32_t ncand;  // the batch's
    double max2;
    // the model and the items (the whole call's)
    const int32_t* cmodel;
    const double* cparams;
    const uint32_t* icam;
    const double *q, *t;
    const double* X;
    // the batch
    const uint32_t* citem;
    const uint32_t* cimg;
    const double* cxy;
    double* e2;
    uint8_t* pass;
};

__global__ __launch_bounds__(kBlock) void complete_error_kernel(Dev d) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= d.ncand) return;
    const uint32_t i = d.cimg[k], c = d.icam[i];
    const double e = filt::squared_reprojection_error(d.cmodel[c], d.cparams + kKC * c, d.q + 4 * i, d.t + 3 * i,
                                                      d.X + 3 * (size_t)d.citem[k], d.cxy + 2 * (size_t)k);
    d.e2[k] = e;
    d.pass[k] = e > d.max2 ? 0 : 1;  // a NaN error is not above the threshold (18.1 H2)
}

// ---- merging ------------------------------------------------------------------------------------------------------------
// All offsets and indices count from the batch's first point, root, observation and correspondence (tracks_plan.h).  A
// component whose points start at p0 has its slots at 2 * p0 (k points use at most 2k - 1) and its log at p0 (at most
// k - 1 merges).
struct MergeDev {
    uint32_t ncomp;
    double max2;
    const int32_t* cmodel;
    const double* cparams;
    const uint32_t* icam;
    const double *q, *t;
    const uint32_t *comp_point, *comp_root, *roots, *point_obs, *obs_corr, *corr_obs;
    const double* pxyz;
    const uint32_t* oimg;
    const double* oxy;
    // work: per slot the track as a linked list over the observations, the position and the stamp "tried against slot
    // stamp - 1"; per observation its successor in its track and its slot
    uint32_t *head, *tail, *len, *stamp;
    double* sxyz;
    uint32_t *next, *oslot;
    // out
    uint32_t *root_ret, *root_nmerge, *log_cur, *log_other, *comp_tried;
    double* log_xyz;
};

// 18.2's test of one track at X: false at the first observation whose squared error is above the threshold
__device__ bool merge_track_fits(const MergeDev& d, uint32_t o, uint32_t n, const uint32_t* next, const double* X) {
    for (uint32_t i = 0; i < n; ++i, o = next[o]) {
        const uint32_t im = d.oimg[o], c = d.icam[im];
        const double e = filt::squared_reprojection_error(d.cmodel[c], d.cparams + kKC * c, d.q + 4 * im, d.t + 3 * im, X,
                                                          d.oxy + 2 * (size_t)o);
        if (e > d.max2) return false;
    }
    return true;
}

__global__ __launch_bounds__(kBlock) void merge_component_kernel(MergeDev d) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= d.ncomp) return;
    const uint32_t p0 = d.comp_point[c], k = d.comp_point[c + 1] - p0;
    uint32_t *head = d.head + 2 * (size_t)p0, *tail = d.tail + 2 * (size_t)p0, *len = d.len + 2 * (size_t)p0,
             *stamp = d.stamp + 2 * (size_t)p0;
    double* sxyz = d.sxyz + 6 * (size_t)p0;
    uint32_t* next = d.next;    // indexed by the batch's observation: a component's observations are its own
    uint32_t* oslot = d.oslot;
    for (uint32_t j = 0; j < k; ++j) {
        const uint32_t o0 = d.point_obs[p0 + j], o1 = d.point_obs[p0 + j + 1];
        head[j] = o0;
        tail[j] = o1 - 1;
        len[j] = o1 - o0;
        stamp[j] = 0;
        for (int a = 0; a < 3; ++a) sxyz[3 * j + a] = d.pxyz[3 * (size_t)(p0 + j) + a];
        for (uint32_t o = o0; o < o1; ++o) {
            next[o] = o + 1 < o1 ? o + 1 : o;
            oslot[o] = j;
        }
    }
    uint32_t nmerge = 0, tried = 0;
    for (uint32_t r = d.comp_root[c]; r < d.comp_root[c + 1]; ++r) {
        uint32_t cur = d.roots[r] - p0, ret = 0;
        const uint32_t first = nmerge;
        bool merged = len[cur] != 0;  // a root an earlier root merged away returns 0
        while (merged) {
            merged = false;
            const uint32_t n1 = len[cur];
            uint32_t o = head[cur];
            for (uint32_t i = 0; i < n1 && !merged; ++i) {
                for (uint32_t e = d.obs_corr[o]; e < d.obs_corr[o + 1]; ++e) {
                    const uint32_t other = oslot[d.corr_obs[e]];
                    if (other == cur || stamp[other] == cur + 1) continue;
                    stamp[other] = cur + 1;
                    ++tried;
                    if (nmerge + 1 >= k) continue;  // (k points merge at most k - 1 times: never taken)
                    const uint32_t n2 = len[other];
                    const double w1 = (double)n1, w2 = (double)n2, ws = (double)(n1 + n2);
                    double X[3];
                    for (int a = 0; a < 3; ++a) X[a] = (w1 * sxyz[3 * cur + a] + w2 * sxyz[3 * other + a]) / ws;
                    if (!merge_track_fits(d, head[cur], n1, next, X) || !merge_track_fits(d, head[other], n2, next, X)) continue;
                    const uint32_t M = k + nmerge;
                    head[M] = head[cur];
                    next[tail[cur]] = head[other];
                    tail[M] = tail[other];
                    len[M] = n1 + n2;
                    stamp[M] = 0;
                    for (int a = 0; a < 3; ++a) sxyz[3 * M + a] = X[a];
                    uint32_t w = head[M];
                    for (uint32_t i2 = 0; i2 < n1 + n2; ++i2, w = next[w]) oslot[w] = M;
                    len[cur] = 0;
                    len[other] = 0;
                    d.log_cur[p0 + nmerge] = cur;
                    d.log_other[p0 + nmerge] = other;
                    for (int a = 0; a < 3; ++a) d.log_xyz[3 * (size_t)(p0 + nmerge) + a] = X[a];
                    ++nmerge;
                    ret = n1 + n2;
                    cur = M;
                    merged = true;  // the walk starts again on M
                    break;
                }
                if (!merged) o = next[o];
            }
        }
        d.root_ret[r] = ret;
        d.root_nmerge[r] = nmerge - first;
    }
    d.comp_tried[c] = tried;
}

void free_arrays(amc_merge_result* r) {
    std::free(r->root_return);
    std::free(r->root_merge_offsets);
    std::free(r->merge_current);
    std::free(r->merge_other);
    std::free(r->merge_xyz);
    r->root_return = nullptr;
    r->root_merge_offsets = nullptr;
    r->merge_current = nullptr;
    r->merge_other = nullptr;
    r->merge_xyz = nullptr;
}

// what the batches bring back, by the call's roots, points (the logs) and components
struct MergeRaw {
    std::vector<uint32_t> root_ret, root_nmerge, log_cur, log_other, comp_tried;
    std::vector<double> log_xyz;
};

int run_merge_batches(amc_ctx* ctx, const amc_merge_problem& pb, const amc_merge_opts& op, const Batches& batches,
                      const std::vector<uint64_t>& comp_obs, MergeRaw* raw, amc_merge_result* result) {
    static const char* const hipchk_who = "amc_merge_tracks";
    const size_t ncam = pb.num_cameras, nimg = pb.num_images, nb = batches.count();
    // the whole call's plan first, so that the device clock below holds copies and kernels only
    std::vector<trk::MergeBatchPlan> plan;
    size_t mp = 0, mo = 0, mk = 0, mr = 0;
    for (size_t b = 0; b < nb; ++b) {
        plan.push_back(trk::plan_merge_batch(pb, batches.start[b], batches.start[b + 1]));
        mp = std::max(mp, plan[b].point_obs.size() - 1);
        mo = std::max(mo, plan[b].obs_corr.size() - 1);
        mk = std::max(mk, plan[b].corr_obs.size());
        mr = std::max(mr, plan[b].roots.size());
    }
    const size_t mc = batches.most_items;
    const CtxView cv = ctx_view(ctx);
    HIPCHK(hipSetDevice(cv.device));
    hipStream_t st = cv.stream;
    MergeDev d{};
    int32_t* d_cmodel;
    uint32_t *d_icam, *d_comp_point, *d_comp_root, *d_roots, *d_point_obs, *d_obs_corr, *d_corr_obs, *d_oimg;
    double *d_cparams, *d_q, *d_t, *d_pxyz, *d_oxy;
    DevBuf<void> mem;  // the call's working set: allocated here, freed on return
    DevParts parts;
    parts.part(&d_cmodel, ncam).part(&d_cparams, kKC * ncam).part(&d_icam, nimg).part(&d_q, 4 * nimg).part(&d_t, 3 * nimg)
        .part(&d_comp_point, mc + 1).part(&d_comp_root, mc + 1).part(&d_roots, mr).part(&d_point_obs, mp + 1)
        .part(&d_obs_corr, mo + 1).part(&d_corr_obs, mk).part(&d_pxyz, 3 * mp).part(&d_oimg, mo).part(&d_oxy, 2 * mo)
        .part(&d.head, 2 * mp).part(&d.tail, 2 * mp).part(&d.len, 2 * mp).part(&d.stamp, 2 * mp).part(&d.sxyz, 6 * mp)
        .part(&d.next, mo).part(&d.oslot, mo).part(&d.root_ret, mr).part(&d.root_nmerge, mr).part(&d.log_cur, mp)
        .part(&d.log_other, mp).part(&d.log_xyz, 3 * mp).part(&d.comp_tried, mc);
    {
        const auto t0 = std::chrono::steady_clock::now();
        const hipError_t e = parts.carve(mem);
        if (e == hipErrorOutOfMemory) return api_fail(AMC_E_NOMEM, "%s: out of device memory", hipchk_who);
        HIPCHK(e);
        result->alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    struct Drain {
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{st};
    StreamTimer timer(st), copies(st);
    HIPCHK(timer.start());
    d.max2 = op.merge_max_reproj_error * op.merge_max_reproj_error;
    d.cmodel = d_cmodel;
    d.cparams = d_cparams;
    d.icam = d_icam;
    d.q = d_q;
    d.t = d_t;
    d.comp_point = d_comp_point;
    d.comp_root = d_comp_root;
    d.roots = d_roots;
    d.point_obs = d_point_obs;
    d.obs_corr = d_obs_corr;
    d.corr_obs = d_corr_obs;
    d.pxyz = d_pxyz;
    d.oimg = d_oimg;
    d.oxy = d_oxy;
    auto up = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    auto down = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
    HIPCHK(copies.span_begin());
    HIPCHK(up(d_cmodel, pb.camera_models, ncam * 4));
    HIPCHK(up(d_cparams, pb.camera_params, ncam * kKC * 8));
    HIPCHK(up(d_icam, pb.image_cameras, nimg * 4));
    HIPCHK(up(d_q, pb.qvec, nimg * 32));
    HIPCHK(up(d_t, pb.tvec, nimg * 24));
    HIPCHK(copies.span_end());
    // The batches follow one another on the stream and reuse the device buffers; every host array a copy reads or
    // writes (the caller's, the plan's, raw's) lives until timer.stop() below has waited for the stream.
    for (size_t b = 0; b < nb; ++b) {
        const trk::MergeBatchPlan& B = plan[b];
        const size_t c0 = batches.start[b], nc = batches.start[b + 1] - c0;
        const uint64_t p0 = pb.comp_point_offsets[c0], r0 = pb.comp_root_offsets[c0], o0 = comp_obs[c0];
        const size_t np = B.point_obs.size() - 1, no = B.obs_corr.size() - 1, nr = B.roots.size();
        d.ncomp = (uint32_t)nc;
        HIPCHK(copies.span_begin());
        HIPCHK(up(d_comp_point, B.comp_point.data(), (nc + 1) * 4));
        HIPCHK(up(d_comp_root, B.comp_root.data(), (nc + 1) * 4));
        HIPCHK(up(d_roots, B.roots.data(), nr * 4));
        HIPCHK(up(d_point_obs, B.point_obs.data(), (np + 1) * 4));
        HIPCHK(up(d_obs_corr, B.obs_corr.data(), (no + 1) * 4));
        HIPCHK(up(d_corr_obs, B.corr_obs.data(), B.corr_obs.size() * 4));
        HIPCHK(up(d_pxyz, pb.point_xyz + 3 * p0, np * 24));
        HIPCHK(up(d_oimg, pb.obs_image + o0, no * 4));
        HIPCHK(up(d_oxy, pb.obs_xy + 2 * o0, no * 16));
        HIPCHK(copies.span_end());
        HIPCHK(timer.span_begin());
        hipLaunchKernelGGL(merge_component_kernel, dim3((unsigned)((nc + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, d);
        HIPCHK(hipGetLastError());
        HIPCHK(timer.span_end());
        HIPCHK(copies.span_begin());
        HIPCHK(down(raw->root_ret.data() + r0, d.root_ret, nr * 4));
        HIPCHK(down(raw->root_nmerge.data() + r0, d.root_nmerge, nr * 4));
        HIPCHK(down(raw->log_cur.data() + p0, d.log_cur, np * 4));
        HIPCHK(down(raw->log_other.data() + p0, d.log_other, np * 4));
        HIPCHK(down(raw->log_xyz.data() + 3 * p0, d.log_xyz, np * 24));
        HIPCHK(down(raw->comp_tried.data() + c0, d.comp_tried, nc * 4));
        HIPCHK(copies.span_end());
    }
    result->num_batches = (uint32_t)nb;
    HIPCHK(timer.stop(result->device_ms));
    HIPCHK(timer.spans(result->kernel_ms));
    HIPCHK(copies.spans(result->copy_ms));
    return AMC_OK;
}

int run_merge(amc_ctx* ctx, const amc_merge_problem* pb, const amc_merge_opts* options, amc_merge_result* result) {
    const char* fn = "amc_merge_tracks";
    const auto host_t0 = std::chrono::steady_clock::now();
    if (result) std::memset(result, 0, sizeof *result);
    if (!ctx || !pb || !result) return api_fail(AMC_E_INVALID, "%s: NULL argument", fn);
    amc_merge_opts op;
    amc_merge_opts_default(&op);
    if (options) op = *options;
    // (the test hook is read before anything can fail, once per call)
    const uint64_t max_comps = (uint64_t)env_int("AMC_TRACKS_BATCH_COMPONENTS", (long long)kMaxBatchComponents, 1, (long long)kMaxBatchComponents);
    std::string bad = trk::check_merge_options(op);
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: invalid options (%s)", fn, bad.c_str());
    bad = trk::check_merge_problem(*pb);
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: %s", fn, bad.c_str());
    const size_t nc = pb->num_components;
    const uint64_t npts = pb->comp_point_offsets[nc], nroots = pb->comp_root_offsets[nc];
    result->num_components = nc;
    result->num_points = npts;
    result->num_observations = pb->point_obs_offsets[npts];
    result->num_roots = nroots;
    int rc = AMC_OK;
    try {
        MergeRaw raw;
        raw.root_ret.assign(nroots, 0);
        raw.root_nmerge.assign(nroots, 0);
        raw.log_cur.assign(npts, 0);
        raw.log_other.assign(npts, 0);
        raw.log_xyz.assign(3 * npts, 0.0);
        raw.comp_tried.assign(nc, 0);
        if (nc) {  // nothing to merge: no device call
            const std::vector<uint64_t> comp_obs = trk::component_obs_offsets(*pb);
            const Batches batches = split_batches(comp_obs.data(), nc, max_comps, kMaxBatchMergeObs);
            rc = run_merge_batches(ctx, *pb, op, batches, comp_obs, &raw, result);
        }
        if (rc == AMC_OK) {
            // a component's log is its roots' logs one after the other: at most one merge less than it has points
            uint64_t nmerges = 0;
            for (size_t c = 0; c < nc && rc == AMC_OK; ++c) {
                uint64_t in_comp = 0;
                for (uint64_t r = pb->comp_root_offsets[c]; r < pb->comp_root_offsets[c + 1]; ++r) in_comp += raw.root_nmerge[r];
                if (in_comp + 1 > pb->comp_point_offsets[c + 1] - pb->comp_point_offsets[c])
                    rc = api_fail(AMC_E_HIP, "%s: component %zu logged %llu merges", fn, c, (unsigned long long)in_comp);
                nmerges += in_comp;
            }
            if (rc == AMC_OK) {
                result->num_merges = nmerges;
                result->root_return = (uint32_t*)std::calloc(std::max<uint64_t>(nroots, 1), 4);
                result->root_merge_offsets = (uint64_t*)std::calloc(nroots + 1, 8);
                result->merge_current = (uint32_t*)std::calloc(std::max<uint64_t>(nmerges, 1), 4);
                result->merge_other = (uint32_t*)std::calloc(std::max<uint64_t>(nmerges, 1), 4);
                result->merge_xyz = (double*)std::calloc(std::max<uint64_t>(3 * nmerges, 1), 8);
                if (!result->root_return || !result->root_merge_offsets || !result->merge_current || !result->merge_other || !result->merge_xyz)
                    throw std::bad_alloc();
                uint64_t at = 0;
                for (size_t c = 0; c < nc; ++c) {
                    uint64_t from = pb->comp_point_offsets[c];
                    for (uint64_t r = pb->comp_root_offsets[c]; r < pb->comp_root_offsets[c + 1]; ++r) {
                        result->root_return[r] = raw.root_ret[r];
                        result->root_merge_offsets[r] = at;
                        for (uint32_t j = 0; j < raw.root_nmerge[r]; ++j, ++at, ++from) {
                            result->merge_current[at] = raw.log_cur[from];
                            result->merge_other[at] = raw.log_other[from];
                            for (int a = 0; a < 3; ++a) result->merge_xyz[3 * at + a] = raw.log_xyz[3 * from + a];
                        }
                    }
                    result->num_pairs_tried += raw.comp_tried[c];
                }
                result->root_merge_offsets[nroots] = at;
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

void free_arrays(amc_complete_result* r) {
    std::free(r->cand_sq_error);
    std::free(r->cand_pass);
    r->cand_sq_error = nullptr;
    r->cand_pass = nullptr;
}

int run_batches(amc_ctx* ctx, const amc_complete_problem& pb, const amc_complete_opts& op, uint64_t batch,
                const std::vector<uint32_t>& cand_item, amc_complete_result* result) {
    static const char* const hipchk_who = "amc_complete_tracks";
    const size_t ncam = pb.num_cameras, nimg = pb.num_images, nit = pb.num_items;
    const uint64_t ncand = pb.item_offsets[nit];
    const size_t mc = (size_t)std::min<uint64_t>(batch, ncand);
    const CtxView cv = ctx_view(ctx);
    HIPCHK(hipSetDevice(cv.device));
    hipStream_t st = cv.stream;
    Dev d{};
    int32_t* d_cmodel;
    uint32_t *d_icam, *d_citem, *d_cimg;
    double *d_cparams, *d_q, *d_t, *d_X, *d_cxy;
    DevBuf<void> mem;  // the call's working set: allocated here, freed on return
    DevParts parts;
    parts.part(&d_cmodel, ncam).part(&d_cparams, kKC * ncam).part(&d_icam, nimg).part(&d_q, 4 * nimg).part(&d_t, 3 * nimg)
        .part(&d_X, 3 * nit).part(&d_citem, mc).part(&d_cimg, mc).part(&d_cxy, 2 * mc).part(&d.e2, mc).part(&d.pass, mc);
    {
        const auto t0 = std::chrono::steady_clock::now();
        const hipError_t e = parts.carve(mem);
        if (e == hipErrorOutOfMemory) return api_fail(AMC_E_NOMEM, "%s: out of device memory", hipchk_who);
        HIPCHK(e);
        result->alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    // an early return must not leave copies in flight that read the plan or write the result's arrays
    struct Drain {
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{st};
    StreamTimer timer(st), copies(st);  // timer: the device clock and the kernels' spans; copies: the copies' spans
    HIPCHK(timer.start());
    d.max2 = op.complete_max_reproj_error * op.complete_max_reproj_error;
    d.cmodel = d_cmodel;
    d.cparams = d_cparams;
    d.icam = d_icam;
    d.q = d_q;
    d.t = d_t;
    d.X = d_X;
    d.citem = d_citem;
    d.cimg = d_cimg;
    d.cxy = d_cxy;
    auto up = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    auto down = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
    HIPCHK(copies.span_begin());
    HIPCHK(up(d_cmodel, pb.camera_models, ncam * 4));
    HIPCHK(up(d_cparams, pb.camera_params, ncam * kKC * 8));
    HIPCHK(up(d_icam, pb.image_cameras, nimg * 4));
    HIPCHK(up(d_q, pb.qvec, nimg * 32));
    HIPCHK(up(d_t, pb.tvec, nimg * 24));
    HIPCHK(up(d_X, pb.item_xyz, nit * 24));
    HIPCHK(copies.span_end());
    // The batches follow one another on the stream and reuse the device buffers; every host array a copy reads or
    // writes (the caller's, the plan's, the result's) lives until timer.stop() below has waited for the stream.
    uint32_t nb = 0;
    for (uint64_t first = 0; first < ncand; first += batch, ++nb) {
        const size_t n = (size_t)std::min<uint64_t>(batch, ncand - first);
        d.ncand = (uint32_t)n;
        HIPCHK(copies.span_begin());
        HIPCHK(up(d_citem, cand_item.data() + first, n * 4));
        HIPCHK(up(d_cimg, pb.cand_image + first, n * 4));
        HIPCHK(up(d_cxy, pb.cand_xy + 2 * first, n * 16));
        HIPCHK(copies.span_end());
        HIPCHK(timer.span_begin());
        hipLaunchKernelGGL(complete_error_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, d);
        HIPCHK(hipGetLastError());
        HIPCHK(timer.span_end());
        HIPCHK(copies.span_begin());
        HIPCHK(down(result->cand_sq_error + first, d.e2, n * 8));
        HIPCHK(down(result->cand_pass + first, d.pass, n));
        HIPCHK(copies.span_end());
    }
    result->num_batches = nb;
    HIPCHK(timer.stop(result->device_ms));
    HIPCHK(timer.spans(result->kernel_ms));
    HIPCHK(copies.spans(result->copy_ms));
    return AMC_OK;
}

int run(amc_ctx* ctx, const amc_complete_problem* pb, const amc_complete_opts* options, amc_complete_result* result) {
    const char* fn = "amc_complete_tracks";
    const auto host_t0 = std::chrono::steady_clock::now();
    if (result) std::memset(result, 0, sizeof *result);
    if (!ctx || !pb || !result) return api_fail(AMC_E_INVALID, "%s: NULL argument", fn);
    amc_complete_opts op;
    amc_complete_opts_default(&op);
    if (options) op = *options;
    // (the test hook is read before anything can fail, once per call)
    const uint64_t batch = (uint64_t)env_int("AMC_TRACKS_BATCH_CANDS", (long long)AMC_TRACKS_MAX_BATCH_CANDIDATES, 1,
                                             (long long)AMC_TRACKS_MAX_BATCH_CANDIDATES);
    std::string bad = trk::check_options(op);
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: invalid options (%s)", fn, bad.c_str());
    bad = trk::check_problem(*pb);
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: %s", fn, bad.c_str());
    const uint64_t ncand = pb->item_offsets[pb->num_items];
    result->num_items = pb->num_items;
    result->num_candidates = ncand;
    result->cand_sq_error = (double*)std::calloc(std::max<uint64_t>(ncand, 1), 8);
    result->cand_pass = (uint8_t*)std::calloc(std::max<uint64_t>(ncand, 1), 1);
    if (!result->cand_sq_error || !result->cand_pass) {
        free_arrays(result);
        return api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    int rc = AMC_OK;
    if (ncand) {  // nothing to test: no device call
        try {
            const std::vector<uint32_t> cand_item = trk::candidate_items(*pb);
            rc = run_batches(ctx, *pb, op, batch, cand_item, result);
        } catch (const std::bad_alloc&) {
            rc = api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
        }
    }
    if (rc != AMC_OK) {
        free_arrays(result);
        return rc;
    }
    for (uint64_t k = 0; k < ncand; ++k) result->num_passed += result->cand_pass[k] != 0;
    result->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count() - result->device_ms;
    return AMC_OK;
}

}  // namespace

extern "C" {

void amc_complete_opts_default(amc_complete_opts* o) {
    if (!o) return;
    o->complete_max_reproj_error = 4.0;  // IncrementalTriangulator::Options' complete_max_reproj_error
    o->reserved = 0;
}

int amc_complete_tracks(amc_ctx* ctx, const amc_complete_problem* problem, const amc_complete_opts* options,
                        amc_complete_result* result) {
    return run(ctx, problem, options, result);
}

void amc_complete_result_free(amc_complete_result* r) {
    if (!r) return;
    free_arrays(r);
}

void amc_merge_opts_default(amc_merge_opts* o) {
    if (!o) return;
    o->merge_max_reproj_error = 4.0;  // IncrementalTriangulator::Options' merge_max_reproj_error
    o->reserved = 0;
}

int amc_merge_tracks(amc_ctx* ctx, const amc_merge_problem* problem, const amc_merge_opts* options, amc_merge_result* result) {
    return run_merge(ctx, problem, options, result);
}

void amc_merge_result_free(amc_merge_result* r) {
    if (!r) return;
    free_arrays(r);
}

}  // extern "C"
