// amc_verify.hip — host side of libamc.so, two-view verification: the verification run (VerifyRun) behind
// amc_verify_pairs, amc_ransac_pairs and amc_match_verify_pairs, relative pose (amc_pose_pairs), and the small geometry
// entry points.  No kernels here: the launches are in tvg_e.hip, tvg_fh.hip, their _big builds and pose.hip.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <random>
#include <thread>
#include <vector>

#include "amc_ctx.h"
#include "camera_math.h"
#include "pose_math.h"  // median_angle_host

using namespace amc;

extern "C" {

namespace {

struct VerifyPriv {
    std::vector<amc_tvg> tvg;
    std::vector<uint8_t> mask;
    std::vector<amc_pose> pose;
    // single-geometry calls: plain storage, every element written from the device results (a vector would
    // zero tens of megabytes first)
    std::unique_ptr<amc_tvg[]> tvg_raw;
    std::unique_ptr<uint8_t[]> mask_raw;
    // verify_impl: pinned buffers leased from the context's pool (the D2H copies land in them; amc_verify_result_free
    // hands them back for the next call - no page faults on fresh heap memory, no copy out of a staging buffer)
    std::shared_ptr<PinnedPool> pool;
    PinBuf<uint32_t> tvg_pin, mask_pin;
    ~VerifyPriv() {
        if (pool) {
            pool->give_back(std::move(tvg_pin));
            pool->give_back(std::move(mask_pin));
        }
    }
};

void pose_default(amc_pose* q, int32_t config) {
    std::memset(q, 0, sizeof *q);
    q->config = config;
    q->qvec[0] = 1.0;
    q->R[0] = q->R[4] = q->R[8] = 1.0;
}

}  // namespace

// EstimateTwoViewGeometryPose for every listed pair (pose.hip); `inlier_matches` in CSR layout.
// kernel_ms (optional): the pose kernel's duration.
static int pose_impl(amc_ctx* c, const char* who, const uint32_t* slot1, const uint32_t* slot2, size_t npairs,
                     const uint64_t* match_offsets, const uint32_t* inlier_matches, const amc_tvg* geoms,
                     amc_pose* out, double* kernel_ms, const uint64_t* resident_mask_off = nullptr,
                     const uint32_t* resident_matches = nullptr, const uint64_t* resident_match_off = nullptr) {
    // resident_mask_off != nullptr (amc_verify_pairs): the matches of this call are still on the device - at
    // resident_matches, pair p's list at resident_match_off[p] (default: d_tmatches, the call's CSR offsets) - and
    // pair p's inlier bytes at d_mask_packed + resident_mask_off[p] (the packed masks: the call's CSR offsets); nothing
    // is uploaded again and the kernel takes the rows whose byte is set.  Their indices have been checked.
    const bool resident = resident_mask_off != nullptr;
    if (kernel_ms) *kernel_ms = 0.0;
    if (!c) return api_fail(AMC_E_INVALID, "%s: NULL ctx", who);
    if (npairs == 0) return AMC_OK;
    if (!slot1 || !slot2 || !match_offsets || !geoms || !out)
        return api_fail(AMC_E_INVALID, "%s: NULL pair arrays", who);
    const uint64_t total = match_offsets[npairs];
    if (total > 0 && !inlier_matches && !resident) return api_fail(AMC_E_INVALID, "%s: NULL matches", who);
    if (npairs > 0xFFFFFFFFull) return api_fail(AMC_E_INVALID, "%s: too many pairs", who);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));  // (an earlier call's upload of the staging buffer is over: every entry point blocks)
    HIPCHK(c->h_ppairs.ensure(npairs));
    PosePair* pp = c->h_ppairs.p;
    std::vector<uint8_t> need_lift(c->slots.size(), 0);
    for (size_t p = 0; p < npairs; ++p) {
        if (slot1[p] >= c->slots.size() || slot2[p] >= c->slots.size())
            return api_fail(AMC_E_INVALID, "%s: pair %zu references slot out of range", who, p);
        const Slot& a = c->slots[slot1[p]];
        const Slot& b = c->slots[slot2[p]];
        if (!a.has_kp || !b.has_kp || !a.has_cam || !b.has_cam)
            return api_fail(AMC_E_STATE, "%s: pair %zu: keypoints/camera not uploaded", who, p);
        // an offset past the last one names rows that the index check below must not read
        if (match_offsets[p + 1] < match_offsets[p] || match_offsets[p + 1] > total)
            return api_fail(AMC_E_INVALID, "%s: match_offsets not monotone at %zu", who, p);
        const uint64_t M = match_offsets[p + 1] - match_offsets[p];
        if (M > 0xFFFFFFFFull) return api_fail(AMC_E_INVALID, "%s: pair %zu has too many matches", who, p);
        const int32_t cfg = geoms[p].config;
        const bool has_geometry = cfg == AMC_TVG_CALIBRATED || cfg == AMC_TVG_UNCALIBRATED || cfg == AMC_TVG_PLANAR ||
                                  cfg == AMC_TVG_PANORAMIC || cfg == AMC_TVG_PLANAR_OR_PANORAMIC;
        if (has_geometry) need_lift[slot1[p]] = need_lift[slot2[p]] = 1;
        if (!resident)
            for (uint64_t k = match_offsets[p]; k < match_offsets[p + 1]; ++k)
                if (inlier_matches[2 * k] >= a.kp_rows || inlier_matches[2 * k + 1] >= b.kp_rows)
                    return api_fail(AMC_E_INVALID, "%s: pair %zu match %llu indexes past the keypoints", who, p,
                                    (unsigned long long)(k - match_offsets[p]));
        pp[p].slot1 = slot1[p];
        pp[p].slot2 = slot2[p];
        pp[p].match_off = (resident && resident_match_off) ? resident_match_off[p] : match_offsets[p];
        pp[p].ws_off = match_offsets[p];
        pp[p].mask_off = resident ? resident_mask_off[p] : 0;
        pp[p].M = (uint32_t)M;
        pp[p].config = cfg;
        std::memcpy(pp[p].E, geoms[p].E, sizeof pp[p].E);
        std::memcpy(pp[p].H, geoms[p].H, sizeof pp[p].H);
    }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    for (size_t i = 0; i < need_lift.size(); ++i)
        if (need_lift[i]) {
            const int rc = ensure_normalized(c, (uint32_t)i);
            if (rc != AMC_OK) return rc;
        }
    std::vector<TvgImage> timgs;
    fill_tvg_images(c, timgs);
    HIPCHK(c->d_timgs.ensure(timgs.size()));
    HIPCHK(c->d_ppairs.ensure(npairs));
    if (!resident) HIPCHK(c->d_pmatches.ensure(std::max<size_t>(2 * total, 2)));
    HIPCHK(c->d_pcos.ensure(std::max<size_t>(total, 1)));
    HIPCHK(c->d_pout.ensure(npairs));
    HIPCHK(hipMemcpyAsync(c->d_timgs.p, timgs.data(), timgs.size() * sizeof(TvgImage), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->d_ppairs.p, pp, npairs * sizeof(PosePair), hipMemcpyHostToDevice, st));
    if (total && !resident)
        HIPCHK(hipMemcpyAsync(c->d_pmatches.p, inlier_matches, 2 * total * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(c->ev[4], st));
    HIPCHK(launch_pose(c->d_timgs.p, c->d_ppairs.p, (uint32_t)npairs,
                       resident ? (resident_matches ? resident_matches : c->d_tmatches.p) : c->d_pmatches.p,
                       resident ? c->d_mask_packed.p : nullptr, c->d_pcos.p, c->d_pout.p, st));
    HIPCHK(hipEventRecord(c->ev[5], st));
    HIPCHK(c->h_pout.ensure(npairs));
    const PoseOut* h = c->h_pout.p;
    HIPCHK(hipMemcpyAsync(c->h_pout.p, c->d_pout.p, npairs * sizeof(PoseOut), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (kernel_ms) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->ev[4], c->ev[5]);
        *kernel_ms = ms;
    }
    for (size_t p = 0; p < npairs; ++p) {
        amc_pose& q = out[p];
        pose_default(&q, geoms[p].config);
        if (!h[p].ok) continue;
        q.ok = 1;
        std::memcpy(q.R, h[p].R, sizeof q.R);
        std::memcpy(q.tvec, h[p].t, sizeof q.tvec);
        std::memcpy(q.qvec, h[p].q, sizeof q.qvec);
        q.num_points3D = h[p].num_points3D;
        // Median(CalculateTriangulationAngles(...)): libm acos of the selected cosine(s)
        q.tri_angle = amc::tvg::median_angle_host(h[p].num_points3D, h[p].cmed);
        if (q.config == AMC_TVG_PLANAR_OR_PANORAMIC) {
            if (h[p].t_is_zero) {
                q.config = AMC_TVG_PANORAMIC;
                q.tri_angle = 0.0;
            } else {
                q.config = AMC_TVG_PLANAR;
            }
        }
    }
    return AMC_OK;
}

// The sample stream: std::mt19937(seed)'s output words (operator() tempers them), `need` of them, kept across calls
// with the same seed.  Blocking (the ctx's stream is drained: the host vector goes out of scope).
static hipError_t ensure_sample_stream(amc_ctx* c, uint32_t seed, size_t need) {
    if (c->d_stream.p && c->stream_seed == seed && c->stream_len >= need) return hipSuccess;
    std::vector<uint32_t> words(need);
    std::mt19937 gen(seed);
    for (size_t i = 0; i < need; ++i) words[i] = (uint32_t)gen();
    hipError_t e = hipStreamSynchronize(c->stream);  // (a relaunch: nothing may still read the table that is freed below)
    if (e != hipSuccess) return e;
    e = c->d_stream.ensure(need);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(c->d_stream.p, words.data(), need * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(c->stream);  // `words` goes out of scope
    c->stream_seed = seed;
    c->stream_len = e == hipSuccess ? need : 0;
    return e;
}
// nothing of a verification run is left in flight (error paths; before buffers its kernels read are freed)
static void verify_streams_sync(amc_ctx* c) {
    if (c->aux_stream) (void)hipStreamSynchronize(c->aux_stream);
    if (c->vstream) (void)hipStreamSynchronize(c->vstream);
    (void)hipStreamSynchronize(c->stream);
}

// ---- verification as a run of SLICES ---------------------------------------------------------------------------------
// A verification call used to be two kernel launches behind each other - tvg_e_kernel over every calibrated pair, then
// tvg_fh_kernel over every pair - and amc_match_verify_pairs ran them after the last match batch.  Both are persistent
// kernels whose tails (the last few long pairs on a few waves) leave most of the machine idle, and between them sat a
// kernel-level barrier; the host's preparation for 10^5 pairs (pair records, trial tables, class lists) ran with the
// device idle.  Round 6: the pairs of a call are cut into slices.  All essential-matrix launches go to one stream, all
// F/H launches to another, slice k's F/H waits for slice k's E by event: tvg_e_kernel(slice k + 1) runs beside
// tvg_fh_kernel(slice k), and a kernel's tail is filled by the other stream's waves.  amc_match_verify_pairs hands the
// pairs of match batch k to the OPEN slice as soon as batch k's counts are on the host: the host prepares them while
// the device scans batch k + 1, and closes and launches one slice behind the last batch.  The kernels, the per-pair
// arithmetic and the results are unchanged: a pair's result does not depend on its slice (every pair re-seeds its
// generator and owns its output record).
//
// mode 0: EstimateTwoViewGeometry; 1 / 2 / 3: a single F / H / E LO-RANSAC per pair, reported
// through the same record (config = success, num_inliers, the model, its trial count, the mask)
namespace {

constexpr int kMaxVerifySlices = 12;

struct VerifyClassLaunch {  // one size class of one slice, as launched (kept for the rare relaunch after a stream overrun)
    int cls = 0;
    bool on_aux = false;
    uint32_t n = 0, n_e = 0, mcap = 0, waves_e = 0, waves_fh = 0;
    int wpb = 4;
};
struct VerifySliceInfo {
    size_t begin = 0, end = 0;
    uint64_t mask_bytes = 0;
    std::vector<VerifyClassLaunch> launches;
};

struct VerifyRun {
    amc_ctx* c;
    int mode;
    const uint32_t* slot1;
    const uint32_t* slot2;
    size_t npairs;
    amc_tvg_opts o;
    uint32_t seed;
    TvgParams P{};
    TvgPair* tp = nullptr;  // npairs records in the ctx's pinned buffer (uploaded as they are by the packing step)
    std::vector<double> wm_cut;
    std::vector<VerifySliceInfo> slices;
    size_t submitted = 0;          // pairs [0, submitted) have been handed over
    const uint32_t* kernel_matches = nullptr;
    hipStream_t st_e = nullptr, st_fh = nullptr;  // all E launches / all F/H launches of the bulk classes
    bool started = false, aux_used = false;
    uint32_t launches = 0;
    uint32_t maxM = 0;
    int cus = 256;
    double t_tables = 0.0, t_lists = 0.0;
    // the run's environment switches (a run lives for one call)
    const bool prof_host = env_flag("AMC_VERIFY_PROFILE");  // wall-clock of the call's host phases on stderr
    const bool prof_kernels = env_flag("AMC_TVG_PROFILE");  // the kernels' per-pair cycle counters on stderr
    const bool serial_classes = env_flag("AMC_TVG_SERIAL_CLASSES");

    bool uses_E(size_t p) const {
        if (mode == 3) return true;
        if (mode != 0 || o.force_H_use) return false;
        if (tp[p].M < (uint32_t)std::max(o.min_num_inliers, 0)) return false;
        return c->slots[slot1[p]].cam.has_prior != 0 && c->slots[slot2[p]].cam.has_prior != 0;
    }
    bool trivial(uint32_t M) const { return mode == 0 && M < (uint32_t)std::max(o.min_num_inliers, 0); }

    // everything that does not depend on the matches: option checks, the sample stream, the image table, the zeroed
    // records.  Issued on the ctx's stream; the verification streams wait for it (vev_setup).
    int begin(size_t total_hint);
    // pairs [begin, end): offs = the call's CSR (offs[p + 1] - offs[p] matches), dev_off = where pair p's rows start in
    // `matches_dev` (nullptr: at offs[p]); `ready` (may be null): an event after which the rows are in place
    int submit(size_t begin, size_t end, const uint64_t* offs, const uint64_t* dev_off, const uint32_t* matches_dev,
               const uint32_t* matches_host, hipEvent_t ready);
    // the two halves of submit(): pairs join the open slice (host only: checks, records, trial tables, size classes);
    // the slice is closed (class lists, uploads, launches).  amc_match_verify_pairs adds every match batch's pairs beside
    // the next batch's scan and closes ONE slice behind the last batch.
    int add_pairs(size_t begin, size_t end, const uint64_t* offs, const uint64_t* dev_off, const uint32_t* matches_dev,
                  const uint32_t* matches_host);
    int close_slice(hipEvent_t ready);
    struct OpenSlice {
        bool active = false;
        size_t begin = 0;
        uint32_t maxM = 0;
        uint64_t mask_bytes = 0;
        std::vector<uint32_t> tabs;
        std::vector<int64_t> tab_of_M;
        std::vector<size_t> cls[4];
    } open;
    int launch_slice(size_t si, hipEvent_t ready);
    int join();
};

int VerifyRun::begin(size_t) {
    if (o.compute_relative_pose && mode != 0)
        return api_fail(AMC_E_INVALID, "amc_verify_pairs: internal: compute_relative_pose outside mode 0");
    if (o.multiple_models)
        return api_fail(AMC_E_INVALID, "amc_verify_pairs: internal: multiple_models reaches verify_impl");
    if (o.ransac.max_num_trials < 0 || o.ransac.min_num_trials < 0 || o.ransac.max_num_trials > (1 << 30))
        return api_fail(AMC_E_INVALID, "amc_verify_pairs: bad trial limits");
    std::vector<uint8_t> need_lift(c->slots.size(), 0);
    for (size_t p = 0; p < npairs; ++p) {
        if (slot1[p] >= c->slots.size() || slot2[p] >= c->slots.size())
            return api_fail(AMC_E_INVALID, "amc_verify_pairs: pair %zu references slot out of range", p);
        const Slot& a = c->slots[slot1[p]];
        const Slot& b = c->slots[slot2[p]];
        const bool need_cam = mode == 0 || mode == 3;
        if (!a.has_kp || !b.has_kp || (need_cam && (!a.has_cam || !b.has_cam)))
            return api_fail(AMC_E_STATE, "amc_verify_pairs: pair %zu: keypoints/camera not uploaded", p);
        const bool e = mode == 0 ? (!o.force_H_use && a.cam.has_prior && b.cam.has_prior) : mode == 3;
        if (e) need_lift[slot1[p]] = need_lift[slot2[p]] = 1;
    }
    P.min_num_inliers = o.min_num_inliers;
    P.detect_watermark = o.detect_watermark;
    P.force_H_use = o.force_H_use;
    P.min_num_trials = (int32_t)std::min<int64_t>(o.ransac.min_num_trials, 1 << 30);
    const double conf = o.ransac.confidence, mult = o.ransac.dyn_num_trials_multiplier;
    P.max_trials[0] = (int32_t)tvg::ransac_max_trials(o.ransac.max_num_trials, o.ransac.min_inlier_ratio, conf, mult, 5);
    P.max_trials[1] = (int32_t)tvg::ransac_max_trials(o.ransac.max_num_trials, o.ransac.min_inlier_ratio, conf, mult, 7);
    P.max_trials[2] = (int32_t)tvg::ransac_max_trials(o.ransac.max_num_trials, o.ransac.min_inlier_ratio, conf, mult, 4);
    P.max_trials[3] = (int32_t)tvg::ransac_max_trials(o.ransac.max_num_trials, o.watermark_min_inlier_ratio, conf, mult, 1);
    P.min_E_F_inlier_ratio = o.min_E_F_inlier_ratio;
    P.max_H_inlier_ratio = o.max_H_inlier_ratio;
    P.watermark_min_inlier_ratio = o.watermark_min_inlier_ratio;
    P.watermark_border_size = o.watermark_border_size;
    P.max_error = o.ransac.max_error;
    P.force_slow_sampler = (int32_t)env_int("AMC_TVG_SLOW_SAMPLER", 0, 0, 1);  // (test hooks: "1" is on)
    P.no_fast_count = (int32_t)env_int("AMC_TVG_EXACT_COUNT", 0, 0, 1);
    P.no_fast32 = (int32_t)env_int("AMC_TVG_NO_S32", 0, 0, 1);
    P.mode = mode;
    P.bad_index_count = c->d_vscalars;
    // inlier-ratio cut-offs of the watermark RANSAC's dynamic trial count (TvgParams::wm_cut)
    if (mode == 0 && o.detect_watermark) {
        auto dyn_of_ratio = [&](double r) -> size_t {  // ComputeNumTrials with inlier_ratio = r, kMinNumSamples = 1
            return tvg::num_trials_of_ratio(r, conf, mult, 1);
        };
        const int nT = std::max(P.max_trials[3], 0);
        // (the cut-offs depend on (confidence, multiplier, max_trials) only: kept across calls)
        if (c->wm_cut_cache.size() == (size_t)nT + 1 && c->wm_cut_conf == o.ransac.confidence &&
            c->wm_cut_mult == o.ransac.dyn_num_trials_multiplier) {
            wm_cut = c->wm_cut_cache;
        } else {
            wm_cut.assign((size_t)nT + 1, 2.0);
            for (int T = 0; T <= nT; ++T) {
                if (dyn_of_ratio(1.0) > (size_t)T) continue;  // not even r = 1 gets there: stays 2.0
                // doubles in [0, 1] order like their bit patterns: bisect the smallest r with dyn(r) <= T
                uint64_t lo = 0, hi = 0x3FF0000000000000ull;  // dyn(lo) > T (or lo is the answer at 0), dyn(hi) <= T
                if (dyn_of_ratio(0.0) <= (size_t)T) { wm_cut[T] = 0.0; continue; }
                while (hi - lo > 1) {
                    const uint64_t mid = lo + (hi - lo) / 2;
                    double r;
                    std::memcpy(&r, &mid, sizeof r);
                    if (dyn_of_ratio(r) <= (size_t)T) hi = mid; else lo = mid;
                }
                std::memcpy(&wm_cut[T], &hi, sizeof(double));
            }
            if (o.ransac.confidence == o.ransac.confidence && o.ransac.dyn_num_trials_multiplier == o.ransac.dyn_num_trials_multiplier) {
                c->wm_cut_cache = wm_cut;
                c->wm_cut_conf = o.ransac.confidence;
                c->wm_cut_mult = o.ransac.dyn_num_trials_multiplier;
            }
        }
    }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
    HIPCHK(c->h_tp.ensure(std::max<size_t>(npairs, 1)));
    tp = c->h_tp.p;
    if (npairs == 0) return AMC_OK;
    // image table (cameras with distortion parameters: CamFromImg of their keypoints first)
    for (size_t i = 0; i < need_lift.size(); ++i)
        if (need_lift[i]) {
            const int rc = ensure_normalized(c, (uint32_t)i);
            if (rc != AMC_OK) return rc;
        }
    std::vector<TvgImage> timgs;
    fill_tvg_images(c, timgs);
    // The sample stream: std::mt19937(seed)'s output words (operator() tempers them).  Every pair re-seeds (D4), so
    // they all read the same table; its length covers every RANSAC of a pair running to its trial cap, plus the
    // words a chunk draws ahead and a margin for Lemire rejections.  Kept across calls with the same seed.
    size_t stream_need = (size_t)5 * P.max_trials[0] + (size_t)7 * P.max_trials[1] + (size_t)4 * P.max_trials[2] +
                         (size_t)P.max_trials[3] + 4 * 64 * 7 + 4096;
    // (test hook: a table a quarter as long, so that long RANSACs run off it and the relaunch path - every slice again on
    // a table twice as long - is exercised; production tables only ever overrun by a Lemire rejection streak)
    if (env_flag("AMC_TVG_STREAM_SHORT")) stream_need = std::max<size_t>(8192, stream_need / 4);
    if (stream_need > kMaxStreamWords)
        return api_fail(AMC_E_INVALID, "amc_verify_pairs: ransac.max_num_trials / min_inlier_ratio allow %zu draws per pair: "
                        "more than the sample-stream table holds (%zu)", stream_need, kMaxStreamWords);
    HIPCHK(ensure_sample_stream(c, seed, stream_need));
    HIPCHK(c->d_timgs.ensure(timgs.size()));
    HIPCHK(c->d_estate.ensure(npairs));
    HIPCHK(c->d_tout.ensure(npairs));
    if (prof_kernels) HIPCHK(c->h_tout.ensure(npairs));
    // the image table: uploaded (from pinned memory) only when it differs from what the device holds
    if (c->timgs_on_device.size() != timgs.size() ||
        (!timgs.empty() && std::memcmp(c->timgs_on_device.data(), timgs.data(), timgs.size() * sizeof(TvgImage)) != 0)) {
        HIPCHK(hipStreamSynchronize(st));  // (h_timgs may still feed an earlier copy)
        HIPCHK(c->h_timgs.ensure(std::max<size_t>(timgs.size(), 1)));
        if (!timgs.empty()) std::memcpy(c->h_timgs.p, timgs.data(), timgs.size() * sizeof(TvgImage));
        c->timgs_on_device.clear();
        HIPCHK(hipMemcpyAsync(c->d_timgs.p, c->h_timgs.p, timgs.size() * sizeof(TvgImage), hipMemcpyHostToDevice, st));
        c->timgs_on_device = timgs;
    }
    P.wm_cut = nullptr;
    if (!wm_cut.empty()) {
        const bool same = c->wm_cut_on_device && c->wm_cut_cache.size() == wm_cut.size() && c->d_wmcut.cap >= wm_cut.size() &&
                          std::memcmp(c->wm_cut_cache.data(), wm_cut.data(), wm_cut.size() * sizeof(double)) == 0;
        if (!same) {
            HIPCHK(c->d_wmcut.ensure(wm_cut.size()));
            c->wm_cut_on_device = false;
            HIPCHK(hipMemcpy(c->d_wmcut.p, wm_cut.data(), wm_cut.size() * sizeof(double), hipMemcpyHostToDevice));  // (rare: options changed)
            c->wm_cut_on_device = c->wm_cut_cache.size() == wm_cut.size() &&
                                  std::memcmp(c->wm_cut_cache.data(), wm_cut.data(), wm_cut.size() * sizeof(double)) == 0;
        }
        P.wm_cut = c->d_wmcut.p;
    }
    // [0] pairs with a bad match index, [1] waves that ran off the stream table, [2 ..] the launches' queue heads; the
    // records' profile and work counters are accumulated by both kernels
    HIPCHK(memset_async(c->d_vscalars, 0, kVScalarWords * sizeof(uint32_t), st));
    HIPCHK(memset_async(c->d_tout.p, 0, npairs * sizeof(TvgOut), st));
    HIPCHK(hipEventRecord(c->vev_setup, st));
    P.stream = c->d_stream.p;
    P.stream_len = (uint32_t)std::min<size_t>(c->stream_len, 0xFFFFFFFFu);
    P.stream_err = c->d_vscalars + 1;
    started = true;
    return AMC_OK;
}

// add_pairs: pairs [begin, end) join the OPEN slice - checks, pair records, trial tables, size classes (host only).
int VerifyRun::add_pairs(size_t begin, size_t end, const uint64_t* offs, const uint64_t* dev_off, const uint32_t* matches_dev,
                         const uint32_t* matches_host) {
    if (begin != submitted || end < begin || end > npairs) return api_fail(AMC_E_INVALID, "amc_verify_pairs: internal: slices out of order");
    if (end == begin) return AMC_OK;
    kernel_matches = matches_dev;
    const auto t0 = std::chrono::steady_clock::now();
    if (!open.active) {
        open = OpenSlice{};
        open.active = true;
        open.begin = begin;
    }
    uint32_t add_maxM = 0;
    for (size_t p = begin; p < end; ++p) {
        if (offs[p + 1] < offs[p]) return api_fail(AMC_E_INVALID, "amc_verify_pairs: match_offsets not monotone at %zu", p);
        const uint64_t M = offs[p + 1] - offs[p];
        if (M > 65535) return api_fail(AMC_E_INVALID, "amc_verify_pairs: pair %zu has %llu matches (> 65535)", p, (unsigned long long)M);
        add_maxM = std::max<uint32_t>(add_maxM, (uint32_t)M);
        // Match indices are checked by the kernel where it gathers the points (bad_index_count); only the pairs no
        // kernel looks at - fewer matches than min_num_inliers - are checked here.
        if (trivial((uint32_t)M) && matches_host) {
            const Slot& a = c->slots[slot1[p]];
            const Slot& b = c->slots[slot2[p]];
            const uint32_t* mm = matches_host + 2 * offs[p];
            for (uint64_t k = 0; k < M; ++k)
                if (mm[2 * k] >= a.kp_rows || mm[2 * k + 1] >= b.kp_rows)
                    return api_fail(AMC_E_INVALID, "amc_verify_pairs: pair %zu match %llu indexes past the keypoints", p, (unsigned long long)k);
        }
    }
    maxM = std::max(maxM, add_maxM);
    open.maxM = std::max(open.maxM, add_maxM);
    if (open.tab_of_M.size() < (size_t)open.maxM + 1) open.tab_of_M.resize((size_t)open.maxM + 1, -1);
    const int kmins[3] = {5, 7, 4};
    auto make_table = [&](uint32_t M) {  // ComputeNumTrials for every inlier count 0 .. M and the three minimal sample sizes
        std::vector<uint32_t> t3;
        t3.reserve(3 * ((size_t)M + 1));
        for (int t = 0; t < 3; ++t)
            for (uint32_t i = 0; i <= M; ++i) {
                const size_t v = M ? tvg::compute_num_trials(i, M, o.ransac.confidence, o.ransac.dyn_num_trials_multiplier, kmins[t]) : 0;
                t3.push_back(v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v);
            }
        return t3;
    };
    // The tables these pairs need and the cache does not hold (a pow and two logs per entry: the first call of a run
    // sees a few hundred new match counts, ~40 ms on one core) are computed ahead on a few threads.
    const bool tabs_cacheable = o.ransac.confidence == o.ransac.confidence &&
                                o.ransac.dyn_num_trials_multiplier == o.ransac.dyn_num_trials_multiplier;
    std::vector<int32_t> fresh_of((size_t)add_maxM + 1, -1);
    std::vector<uint32_t> fresh_M;
    std::vector<std::vector<uint32_t>> fresh_tab;
    {
        size_t words = 0;
        for (size_t p = begin; p < end; ++p) {
            const uint32_t M = (uint32_t)(offs[p + 1] - offs[p]);
            if (trivial(M) || fresh_of[M] != -1 || open.tab_of_M[M] >= 0) continue;
            fresh_of[M] = -2;  // seen
            if (tabs_cacheable && c->trial_tabs.count(TrialTabKey{M, o.ransac.confidence, o.ransac.dyn_num_trials_multiplier})) continue;
            fresh_of[M] = (int32_t)fresh_M.size();
            fresh_M.push_back(M);
            words += 3 * ((size_t)M + 1);
        }
        fresh_tab.resize(fresh_M.size());
        const unsigned nth = words >= 65536 ? std::min(8u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
        std::atomic<size_t> next{0};
        auto work = [&] {
            for (size_t k; (k = next.fetch_add(1)) < fresh_M.size();) fresh_tab[k] = make_table(fresh_M[k]);
        };
        std::vector<std::thread> th;
        for (unsigned k = 1; k < nth; ++k) th.emplace_back(work);
        work();
        for (auto& t : th) t.join();
    }
    std::vector<uint32_t>& tabs = open.tabs;
    for (size_t p = begin; p < end; ++p) {
        const uint32_t M = (uint32_t)(offs[p + 1] - offs[p]);
        TvgPair& q = tp[p];
        q.slot1 = slot1[p];
        q.slot2 = slot2[p];
        q.match_off = dev_off ? dev_off[p] : offs[p];
        q.M = M;
        q.orig = (uint32_t)p;
        q.mask_off = 0;
        q.tab_off[0] = q.tab_off[1] = q.tab_off[2] = 0;
        if (trivial(M)) continue;  // DEGENERATE without a kernel: pack_verify_kernel writes the record
        if (open.tab_of_M[M] < 0) {
            open.tab_of_M[M] = (int64_t)tabs.size();
            // the table of one match count depends on (M, confidence, multiplier) only: kept across calls
            // (a pow and two logs per entry; a pipeline sees the same few hundred counts again and again)
            const TrialTabKey key{M, o.ransac.confidence, o.ransac.dyn_num_trials_multiplier};
            // (NaN options would break the map's ordering: those tables are rebuilt every time)
            auto it = tabs_cacheable ? c->trial_tabs.find(key) : c->trial_tabs.end();
            if (it == c->trial_tabs.end()) {
                std::vector<uint32_t> t3 = (M <= add_maxM && fresh_of[M] >= 0) ? std::move(fresh_tab[(size_t)fresh_of[M]]) : make_table(M);
                if (!tabs_cacheable) {
                    tabs.insert(tabs.end(), t3.begin(), t3.end());
                } else {
                    if (c->trial_tab_words + t3.size() > kTrialTabCacheWords) {  // bounded: start over
                        c->trial_tabs.clear();
                        c->trial_tab_words = 0;
                    }
                    c->trial_tab_words += t3.size();
                    it = c->trial_tabs.emplace(key, std::move(t3)).first;
                }
            }
            if (it != c->trial_tabs.end()) tabs.insert(tabs.end(), it->second.begin(), it->second.end());
        }
        q.mask_off = open.mask_bytes;
        open.mask_bytes += ((uint64_t)M + 127) / 128 * 128;
        for (int t = 0; t < 3; ++t) q.tab_off[t] = (uint32_t)(open.tab_of_M[M] + (int64_t)t * (M + 1));
        // Size classes.  A wave's LDS share holds, besides a few KB of fixed state, two uint16 index arrays of mcap
        // entries (the sampler's permutation and the inlier list); everything else of a pair lives in the wave's global
        // workspace.  Pairs up to ~1,800 matches run at both kernels' full occupancy (E 2, F/H 3 waves per SIMD), 4 waves
        // per workgroup; larger ones in launches of their own with fewer resident waves; the largest (M <= ~38 k: covers
        // max_num_matches = 32768) one wave per workgroup with up to the whole 160 KB; beyond that (class 3, up to the
        // 65,535 matches the 16-bit indices name) the "big" builds of the kernels keep the two arrays in global memory.
        const uint32_t mc = std::max<uint32_t>(64, round_up(M, 64));
        const size_t lds = tvg_lds_bytes(mc, 1) + 64;
        const size_t lds_e = tvg_lds_bytes_e(mc, 1) + 64;  // (the E kernel's waves also carry the root finder's coefficients)
        if (lds <= 160 * 1024 / (4 * (size_t)kTvgFhWavesPerSimd) && lds_e <= 160 * 1024 / (4 * (size_t)kTvgEWavesPerSimd))
            open.cls[0].push_back(p);  // (full occupancy of BOTH kernels)
        else if (lds_e <= 160 * 1024 / 4) open.cls[1].push_back(p);  // 4-wave workgroups of either kernel fit a CU
        else if (lds_e <= 160 * 1024) open.cls[2].push_back(p);
        else open.cls[3].push_back(p);  // M <= 65535 was checked above
    }
    submitted = end;
    t_tables += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return AMC_OK;
}

// close_slice: the open slice's class lists (largest pairs first), its uploads and its launches
int VerifyRun::close_slice(hipEvent_t ready) {
    if (!open.active) return AMC_OK;
    if (slices.size() >= (size_t)kMaxVerifySlices) return api_fail(AMC_E_INVALID, "amc_verify_pairs: internal: too many slices");
    const auto t1 = std::chrono::steady_clock::now();
    VerifySliceInfo sl;
    sl.begin = open.begin;
    sl.end = submitted;
    sl.mask_bytes = open.mask_bytes;
    const size_t si = slices.size();
    if (c->vslices.size() <= si) c->vslices.resize(si + 1);
    if (!c->vslices[si]) c->vslices[si].reset(new (std::nothrow) VerifySliceBufs());
    if (!c->vslices[si]) return api_fail(AMC_E_NOMEM, "amc_verify_pairs: out of host memory");
    VerifySliceBufs& B = *c->vslices[si];
    const std::vector<uint32_t>& tabs = open.tabs;
    const uint32_t slice_maxM = open.maxM;
    std::vector<size_t>(&cls)[4] = open.cls;
    HIPCHK(B.tabs.ensure(std::max<size_t>(tabs.size(), 1)));
    HIPCHK(B.outmask.ensure(std::max<size_t>(open.mask_bytes, 128)));
    HIPCHK(B.emask.ensure(std::max<size_t>(open.mask_bytes, 128)));
    // (pageable sources: these copies are done when the calls return - the vectors may go out of scope - and need no
    // stream synchronisation)
    if (!tabs.empty()) {
        HIPCHK(B.h_tabs.ensure(tabs.size()));
        std::memcpy(B.h_tabs.p, tabs.data(), tabs.size() * sizeof(uint32_t));
        HIPCHK(hipMemcpy(B.tabs.p, B.h_tabs.p, tabs.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    // The first non-empty class (the bulk of a slice) runs on the E / F/H streams; the others - few pairs, each several
    // milliseconds on one wave whatever the machine around it does - on the low-priority stream with their own lists
    // and workspaces, so that they fill the bulk class's tails instead of adding launches of pure latency behind it.
    int bulk = 0;
    while (bulk < 4 && cls[bulk].empty()) ++bulk;
    const bool serial = serial_classes || !c->aux_stream;
    for (int k = 3; k >= 0; --k) {  // (the aux classes first: their few waves take their slots before the bulk class fills the machine)
        if (cls[k].empty()) continue;
        VerifyClassLaunch L;
        L.cls = k;
        L.on_aux = k != bulk && !serial;
        L.wpb = k >= 2 ? 1 : 4;
        const bool big = k == 3;  // index arrays in global memory (tvg_*_big.hip)
        // The waves pull pairs from a queue in this order.  A pair's cost grows with its match count (every
        // trial scores all matches), so the largest go first: what is left for the tail of the launch, when
        // most waves have run dry, are the cheap ones.  Results are stored by pair, the order is free.
        // (stable counting sort by match count, descending: M <= 65535)
        std::vector<size_t> idx(cls[k].size());
        {
            std::vector<uint32_t> start((size_t)slice_maxM + 2, 0);
            for (size_t p : cls[k]) ++start[slice_maxM - tp[p].M + 1];
            for (size_t b = 1; b <= (size_t)slice_maxM + 1; ++b) start[b] += start[b - 1];
            for (size_t p : cls[k]) idx[start[slice_maxM - tp[p].M]++] = p;
        }
        VerifyClassSlot& S = B.cls[k];
        HIPCHK(S.h_pairs.ensure(std::max<size_t>(idx.size(), 1)));
        HIPCHK(S.h_pairs_e.ensure(std::max<size_t>(idx.size(), 1)));
        TvgPair* const sub = S.h_pairs.p;      // the lists are written where the copies read them: pinned memory
        TvgPair* const sub_e = S.h_pairs_e.p;
        size_t n_e = 0;
        uint32_t cm = 0;
        for (size_t i = 0; i < idx.size(); ++i) {
            sub[i] = tp[idx[i]];
            cm = std::max(cm, sub[i].M);
            if (uses_E(idx[i])) sub_e[n_e++] = sub[i];
        }
        L.mcap = std::max<uint32_t>(64, round_up(cm, 64));
        auto waves_for = [&](size_t n, int waves_per_simd, size_t lds_block) {
            const uint32_t blocks_per_cu = (uint32_t)std::max<size_t>(
                1, std::min<size_t>(4 * (size_t)waves_per_simd / L.wpb, (160 * 1024) / std::max<size_t>(lds_block, 1)));
            uint32_t nw = (uint32_t)std::min<size_t>(n, (size_t)cus * blocks_per_cu * L.wpb);
            return std::max<uint32_t>(L.wpb, (nw + L.wpb - 1) / L.wpb * L.wpb);
        };
        const bool run_fh = mode != 3;
        L.n = (uint32_t)idx.size();
        L.n_e = (uint32_t)n_e;
        L.waves_e = n_e == 0 ? 0 : waves_for(n_e, kTvgEWavesPerSimd, big ? tvg_big_lds_bytes_e(L.wpb) : tvg_lds_bytes_e(L.mcap, L.wpb));
        L.waves_fh = run_fh ? waves_for(idx.size(), kTvgFhWavesPerSimd, big ? tvg_big_lds_bytes(L.wpb) : tvg_lds_bytes(L.mcap, L.wpb)) : 0;
        HIPCHK(S.pairs.ensure(idx.size()));
        HIPCHK(S.pairs_e.ensure(std::max<size_t>(n_e, 1)));
        const size_t idx_ws = big ? tvg_big_idx_doubles_host(L.mcap) : 0;  // per wave, behind the point workspaces
        // (E and F/H of one slice run behind each other, but slice k's F/H runs beside slice k + 1's E: own workspaces)
        HIPCHK(S.ws_e.ensure(std::max<size_t>((size_t)L.waves_e * (tvg_ws_doubles_e_host(L.mcap) + idx_ws), 1)));
        HIPCHK(S.ws.ensure(std::max<size_t>((size_t)L.waves_fh * (tvg_ws_doubles_host(L.mcap) + idx_ws), 1)));
        HIPCHK(S.maskws.ensure((size_t)std::max<uint32_t>(L.waves_fh, 1) * tvg_ws_mask_bytes_host(L.mcap)));
        HIPCHK(hipMemcpy(S.pairs.p, sub, idx.size() * sizeof(TvgPair), hipMemcpyHostToDevice));
        if (n_e) HIPCHK(hipMemcpy(S.pairs_e.p, sub_e, n_e * sizeof(TvgPair), hipMemcpyHostToDevice));
        sl.launches.push_back(L);
    }
    t_lists += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    slices.push_back(std::move(sl));
    open = OpenSlice{};
    return launch_slice(si, ready);
}

int VerifyRun::submit(size_t begin, size_t end, const uint64_t* offs, const uint64_t* dev_off, const uint32_t* matches_dev,
                      const uint32_t* matches_host, hipEvent_t ready) {
    if (const int rc = add_pairs(begin, end, offs, dev_off, matches_dev, matches_host)) return rc;
    return close_slice(ready);
}

// the launches of slice si: every class's E kernel(s), then - behind an event - its F/H kernel(s)
int VerifyRun::launch_slice(size_t si, hipEvent_t ready) {
    const VerifySliceInfo& sl = slices[si];
    VerifySliceBufs& B = *c->vslices[si];
    if (!B.ev[0]) {  // the slice's six events: all of them, or none and the call fails
        const unsigned flags[6] = {hipEventDefault, hipEventDefault, hipEventDefault, hipEventDefault,
                                   hipEventDisableTiming, hipEventDisableTiming};
        hipEvent_t e[6];
        if (create_events(e, 6, flags) != hipSuccess) return api_fail(AMC_E_HIP, "amc_verify_pairs: hipEventCreate failed");
        std::copy(e, e + 4, B.ev);
        B.ev_e_done = e[4];
        B.ev_aux_done = e[5];
    }
    auto wait_inputs = [&](hipStream_t s) -> hipError_t {
        hipError_t e = s == c->stream ? hipSuccess : hipStreamWaitEvent(s, c->vev_setup, 0);
        if (e == hipSuccess && ready) e = hipStreamWaitEvent(s, ready, 0);
        return e;
    };
    bool any_aux = false, any_bulk_e = false;
    for (const VerifyClassLaunch& L : sl.launches) any_aux |= L.on_aux;
    if (any_aux) HIPCHK(wait_inputs(c->aux_stream));
    HIPCHK(wait_inputs(st_e));
    if (st_fh != st_e) HIPCHK(wait_inputs(st_fh));
    HIPCHK(hipEventRecord(B.ev[0], st_e));
    // E kernels: bulk classes on st_e, aux classes (E and F/H behind each other) on the aux stream
    for (const VerifyClassLaunch& L : sl.launches) {
        VerifyClassSlot& S = B.cls[L.cls];
        const bool big = L.cls == 3;
        uint32_t* const qhead = c->d_vscalars + 2 + 8 * si + 2 * L.cls;
        hipStream_t ks = L.on_aux ? c->aux_stream : st_e;
        if (L.n_e) {
            HIPCHK((big ? launch_tvg_e_big : launch_tvg_e)(c->d_timgs.p, S.pairs_e.p, L.n_e, kernel_matches, B.tabs.p, P, S.ws_e.p,
                                                            L.mcap, L.waves_e, L.wpb, qhead, c->d_estate.p, B.emask.p, c->d_tout.p,
                                                            B.outmask.p, ks));
            ++launches;
            any_bulk_e |= !L.on_aux;
        }
        if (L.on_aux && mode != 3) {
            HIPCHK((big ? launch_tvg_fh_big : launch_tvg_fh)(c->d_timgs.p, S.pairs.p, L.n, kernel_matches, B.tabs.p, P, S.ws.p,
                                                              S.maskws.p, L.mcap, L.waves_fh, L.wpb, qhead + 1, c->d_estate.p, B.emask.p,
                                                              c->d_tout.p, B.outmask.p, ks));
            ++launches;
        }
    }
    HIPCHK(hipEventRecord(B.ev[1], st_e));
    if (st_fh != st_e) {
        HIPCHK(hipEventRecord(B.ev_e_done, st_e));
        HIPCHK(hipStreamWaitEvent(st_fh, B.ev_e_done, 0));
    }
    (void)any_bulk_e;
    HIPCHK(hipEventRecord(B.ev[2], st_fh));
    if (mode != 3)
        for (const VerifyClassLaunch& L : sl.launches) {
            if (L.on_aux) continue;
            VerifyClassSlot& S = B.cls[L.cls];
            const bool big = L.cls == 3;
            uint32_t* const qhead = c->d_vscalars + 2 + 8 * si + 2 * L.cls;
            HIPCHK((big ? launch_tvg_fh_big : launch_tvg_fh)(c->d_timgs.p, S.pairs.p, L.n, kernel_matches, B.tabs.p, P, S.ws.p,
                                                              S.maskws.p, L.mcap, L.waves_fh, L.wpb, qhead + 1, c->d_estate.p, B.emask.p,
                                                              c->d_tout.p, B.outmask.p, st_fh));
            ++launches;
        }
    HIPCHK(hipEventRecord(B.ev[3], st_fh));
    if (any_aux) {
        HIPCHK(hipEventRecord(B.ev_aux_done, c->aux_stream));
        aux_used = true;
        B.aux_pending = true;
    }
    return AMC_OK;
}

// every launch of the run is done (the ctx's stream joins the others and is drained)
int VerifyRun::join() {
    hipStream_t st = c->stream;
    for (size_t si = 0; si < slices.size(); ++si) {
        VerifySliceBufs& B = *c->vslices[si];
        HIPCHK(hipStreamWaitEvent(st, B.ev[3], 0));
        HIPCHK(hipStreamWaitEvent(st, B.ev[1], 0));
        if (B.aux_pending) {
            HIPCHK(hipStreamWaitEvent(st, B.ev_aux_done, 0));
            B.aux_pending = false;
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    return AMC_OK;
}

}  // namespace

// dev_matches != nullptr (amc_match_verify_pairs without the streamed hand-over): the matches are already on this device -
// pair p's list starts at dev_matches + 2 * dev_off[p] and has match_offsets[p + 1] - match_offsets[p] rows; `matches` is not read.
// verify_finish: what is left when every pair of the run has been submitted - the join, the packing, the download.
static int verify_finish(amc_ctx* c, VerifyRun& run, const uint64_t* match_offsets, const uint32_t* matches,
                         amc_verify_result* out, VerifyPriv* priv, const uint32_t* dev_matches, const uint64_t* dev_off,
                         double t_pre_ms);

static int verify_impl(amc_ctx* c, int mode, const uint32_t* slot1, const uint32_t* slot2, size_t npairs,
                       const uint64_t* match_offsets, const uint32_t* matches,
                       const amc_tvg_opts* opts_in, uint32_t seed, amc_verify_result* out,
                       const uint32_t* dev_matches = nullptr, const uint64_t* dev_off = nullptr) {
    if (!c || !out) return api_fail(AMC_E_INVALID, "amc_verify_pairs: NULL ctx/out");
    std::memset(out, 0, sizeof *out);
    c->vres = amc::VerifyResident{};
    if (npairs > 0 && (!slot1 || !slot2 || !match_offsets))
        return api_fail(AMC_E_INVALID, "amc_verify_pairs: NULL pair arrays");
    const auto wall0 = std::chrono::steady_clock::now();
    VerifyRun run{};
    run.c = c;
    run.mode = mode;
    run.slot1 = slot1;
    run.slot2 = slot2;
    run.npairs = npairs;
    if (opts_in) run.o = *opts_in; else amc_tvg_opts_default(&run.o);
    run.seed = seed;
    const uint64_t total = npairs ? match_offsets[npairs] : 0;
    if (total > 0 && !matches && !dev_matches) return api_fail(AMC_E_INVALID, "amc_verify_pairs: NULL matches");
    for (size_t p = 0; p < npairs; ++p)
        if (match_offsets[p + 1] < match_offsets[p])
            return api_fail(AMC_E_INVALID, "amc_verify_pairs: match_offsets not monotone at %zu", p);
    int rc = run.begin(total);
    if (rc != AMC_OK) return rc;
    VerifyPriv* priv = new (std::nothrow) VerifyPriv();
    if (!priv) return api_fail(AMC_E_NOMEM, "amc_verify_pairs: out of host memory");
    // every failure below (HIPCHK returns included) frees the result's storage and hands back a zeroed struct
    // - after nothing of the call is left in flight: launches on the other streams still run when an error returns, and
    // the next call would rewrite their lists and workspaces under them
    struct Guard {
        amc_ctx* c;
        VerifyPriv* p;
        amc_verify_result* o;
        ~Guard() {
            if (p) {
                verify_streams_sync(c);
                delete p;
                std::memset(o, 0, sizeof *o);
            }
        }
    } guard{c, priv, out};
    hipStream_t st = c->stream;
    if (npairs) {
        // the matches: uploaded once (host path), or where the matcher left them
        const uint32_t* km = dev_matches;
        if (!dev_matches) {
            HIPCHK(c->d_tmatches.ensure(std::max<size_t>(2 * total, 2)));
            if (total) HIPCHK(hipMemcpyAsync(c->d_tmatches.p, matches, 2 * total * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIPCHK(hipEventRecord(c->vev_matches, st));
            km = c->d_tmatches.p;
        }
        // Slices: E launches on the ctx's stream, F/H launches on the verification stream.  A slice wants enough pairs
        // to fill the machine several times over (its own tail is only hidden by the NEXT slice's E kernel).
        run.st_e = st;
        run.st_fh = c->vstream ? c->vstream : st;
        size_t nver = 0;
        for (size_t p = 0; p < npairs; ++p) nver += !run.trivial((uint32_t)(match_offsets[p + 1] - match_offsets[p]));
        // One slice by default since the kernels lost their scratch traffic (round 6, final code, 124,750 pairs, kernels:
        // 1 slice 338 ms, 2: 343, 3: 350, 4: 355 - profiles/r06/ab_slices_final_v1.txt): a SIMD that holds an E wave beside
        // F/H waves runs fewer of them, and the kernels' own tails are ~1 % of such a call.  Before that two slices were
        // +1.2 % (1 slice 433-439 ms, 2: 434-435, 4: 441, 8: 480 - ab_pipeline_v1.txt).  AMC_TVG_SLICES: the A/B hook and the
        // tests' way to the sliced path, which amc_match_verify_pairs' batches still take.
        const int want = (int)env_int("AMC_TVG_SLICES", 1, 1, kMaxVerifySlices);
        // two full F/H machine loads per slice (AMC_TVG_MIN_PER_SLICE: test hook)
        const size_t min_per_slice = (size_t)env_int("AMC_TVG_MIN_PER_SLICE", (long long)run.cus * 12 * 2, 1, std::numeric_limits<int>::max());
        const int ns = (int)std::max<size_t>(1, std::min<size_t>((size_t)want, nver / std::max<size_t>(min_per_slice, 1)));
        if (ns <= 1) run.st_fh = st;  // one slice: E and F/H behind each other on the ctx's stream, as before
        // cut at equal shares of the verified pairs (the trivial ones cost nothing)
        size_t begin = 0, seen = 0;
        for (int k = 0; k < ns; ++k) {
            size_t end = begin;
            const size_t upto = k + 1 == ns ? nver : (nver * (size_t)(k + 1)) / (size_t)ns;
            if (k + 1 == ns) end = npairs;
            else
                while (end < npairs && seen < upto) {
                    seen += !run.trivial((uint32_t)(match_offsets[end + 1] - match_offsets[end]));
                    ++end;
                }
            rc = run.submit(begin, end, match_offsets, dev_off, km, dev_matches ? nullptr : matches,
                            dev_matches ? nullptr : c->vev_matches);
            if (rc != AMC_OK) return rc;
            begin = end;
        }
    }
    const double t_pre = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    rc = verify_finish(c, run, match_offsets, matches, out, priv, dev_matches, dev_off, t_pre);
    if (rc != AMC_OK) return rc;
    guard.p = nullptr;
    return AMC_OK;
}

static int verify_finish(amc_ctx* c, VerifyRun& run, const uint64_t* match_offsets, const uint32_t* matches,
                         amc_verify_result* out, VerifyPriv* priv, const uint32_t* dev_matches, const uint64_t* dev_off,
                         double t_pre_ms) {
    const size_t npairs = run.npairs;
    const uint64_t total = npairs ? match_offsets[npairs] : 0;
    const auto wall0 = std::chrono::steady_clock::now();
    hipStream_t st = c->stream;
    priv->pool = c->verify_pool;
    priv->tvg_pin = c->verify_pool->acquire((std::max<size_t>(npairs, 1) * sizeof(amc_tvg) + 3) / 4);
    priv->mask_pin = c->verify_pool->acquire((size_t)(std::max<uint64_t>(total, 1) + 3) / 4);
    if (priv->tvg_pin.ensure((std::max<size_t>(npairs, 1) * sizeof(amc_tvg) + 3) / 4) != hipSuccess ||
        priv->mask_pin.ensure((size_t)(std::max<uint64_t>(total, 1) + 3) / 4) != hipSuccess)
        return api_fail(AMC_E_NOMEM, "amc_verify_pairs: out of pinned host memory");
    out->npairs = npairs;
    out->_priv = priv;
    out->tvg = reinterpret_cast<amc_tvg*>(priv->tvg_pin.p);
    out->inlier_mask = reinterpret_cast<uint8_t*>(priv->mask_pin.p);
    if (npairs == 0) return AMC_OK;
    if (run.submitted != npairs) return api_fail(AMC_E_INVALID, "amc_verify_pairs: internal: %zu of %zu pairs submitted", run.submitted, npairs);
    double kernel_ms = 0.0;
    for (int attempt = 0;; ++attempt) {
        {
            const int rc = run.join();
            if (rc != AMC_OK) return rc;
        }
        // kernel time: from the first slice's first launch to the last launch's end (the slices run back to back)
        kernel_ms = 0.0;
        if (!run.slices.empty()) {
            HIPCHK(hipEventRecord(c->ev[3], st));
            HIPCHK(hipEventSynchronize(c->ev[3]));
            float kms = 0.f;
            (void)hipEventElapsedTime(&kms, c->vslices[0]->ev[0], c->ev[3]);
            kernel_ms = kms;
        }
        uint32_t vs[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(vs, c->d_vscalars, sizeof vs, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (!vs[1]) break;
        // a Lemire rejection loop ran past the table (probability ~1e-6 per 4096 spare words): lay out more, redo -
        // every slice again (the lists are still on the device), behind each other
        if (attempt >= 4 || c->stream_len * 2 > kMaxStreamWords)
            return api_fail(AMC_E_HIP, "amc_verify_pairs: the sample stream table was exhausted %d times", attempt + 1);
        HIPCHK(ensure_sample_stream(c, run.seed, c->stream_len * 2));
        run.P.stream = c->d_stream.p;
        run.P.stream_len = (uint32_t)std::min<size_t>(c->stream_len, 0xFFFFFFFFu);
        HIPCHK(memset_async(c->d_vscalars, 0, kVScalarWords * sizeof(uint32_t), st));
        HIPCHK(memset_async(c->d_tout.p, 0, npairs * sizeof(TvgOut), st));
        HIPCHK(hipEventRecord(c->vev_setup, st));
        for (size_t si = 0; si < run.slices.size(); ++si) {
            const int rc = run.launch_slice(si, nullptr);
            if (rc != AMC_OK) return rc;
        }
    }
    // The kernel stores a pair's record at the caller's pair index (TvgPair::orig) and its mask at a 128-byte
    // aligned offset of its slice's buffer; pack_verify_kernel lays both out as the caller reads them (records without
    // their counters, masks at the input's CSR offsets; a pair no kernel looked at - fewer matches than min_num_inliers -
    // becomes the DEGENERATE record EstimateTwoViewGeometry returns for it) and sums the work counters, so the copies
    // below land in the result itself.
    HIPCHK(c->d_tvg_packed.ensure(npairs));
    HIPCHK(c->d_mask_packed.ensure(std::max<uint64_t>(total, 1)));
    HIPCHK(c->d_moff.ensure(npairs + 1));
    HIPCHK(c->d_tp_all.ensure(npairs));
    HIPCHK(c->d_worksum.ensure(12));
    HIPCHK(c->h_moff.ensure(npairs + 1));
    std::memcpy(c->h_moff.p, match_offsets, (npairs + 1) * sizeof(uint64_t));
    HIPCHK(hipMemcpyAsync(c->d_moff.p, c->h_moff.p, (npairs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->d_tp_all.p, run.tp, npairs * sizeof(TvgPair), hipMemcpyHostToDevice, st));
    HIPCHK(memset_async(c->d_worksum.p, 0, 12 * sizeof(unsigned long long), st));
    const int32_t trivial_below = run.mode == 0 ? std::max(run.o.min_num_inliers, 0) : 0;
    for (size_t si = 0; si < run.slices.size(); ++si) {
        const VerifySliceInfo& sl = run.slices[si];
        HIPCHK(launch_pack_verify(c->d_tout.p + sl.begin, c->d_tp_all.p + sl.begin, (uint32_t)(sl.end - sl.begin),
                                  c->vslices[si]->outmask.p, c->d_moff.p + sl.begin, c->d_tvg_packed.p + sl.begin,
                                  c->d_mask_packed.p, c->d_worksum.p, trivial_below, st));
    }
    HIPCHK(hipMemcpyAsync(out->tvg, c->d_tvg_packed.p, npairs * sizeof(amc_tvg), hipMemcpyDeviceToHost, st));
    if (total) HIPCHK(hipMemcpyAsync(out->inlier_mask, c->d_mask_packed.p, total, hipMemcpyDeviceToHost, st));
    unsigned long long worksum[12];
    HIPCHK(hipMemcpyAsync(worksum, c->d_worksum.p, sizeof worksum, hipMemcpyDeviceToHost, st));
    if (run.prof_kernels)  // the per-pair cycle counters live in the full records
        HIPCHK(hipMemcpyAsync(c->h_tout.p, c->d_tout.p, npairs * sizeof(TvgOut), hipMemcpyDeviceToHost, st));
    uint32_t bad_pairs = 0;
    HIPCHK(hipMemcpyAsync(&bad_pairs, c->d_vscalars, sizeof bad_pairs, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(c->ev[1], st));
    HIPCHK(hipEventSynchronize(c->ev[1]));
    if (bad_pairs) {  // the kernel met an index past an image's keypoints: find it for the message
        for (size_t p = 0; p < npairs && matches; ++p) {
            const Slot& a = c->slots[run.slot1[p]];
            const Slot& b = c->slots[run.slot2[p]];
            for (uint64_t k = match_offsets[p]; k < match_offsets[p + 1]; ++k)
                if (matches[2 * k] >= a.kp_rows || matches[2 * k + 1] >= b.kp_rows)
                    return api_fail(AMC_E_INVALID, "amc_verify_pairs: pair %zu match %llu indexes past the keypoints", p,
                                    (unsigned long long)(k - match_offsets[p]));
        }
        return api_fail(AMC_E_INVALID, "amc_verify_pairs: %u pairs index past the keypoints", bad_pairs);
    }
    if (run.prof_kernels) {
        const TvgOut* h_out = c->h_tout.p;
        tvg_diag_report();
        tvg_diag_report_e();
        unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (size_t p = 0; p < npairs; ++p)
            for (int i = 0; i < 8; ++i) acc[i] += h_out[p].prof[i];
        if (acc[4] == 0)
            std::fprintf(stderr, "[amc tvg profile] the kernels' cycle counters are compiled out of this build (-DAMC_TVG_PROF or the "
                         "-DAMC_TVG_LODIAG build: tools/variant_build_tvg.sh)\n");
        else
        std::fprintf(stderr, "[amc tvg profile] pairs=%zu cycles/pair: sampling=%.0f minimal=%.0f replay+score=%.0f "
                     "(of which LO=%.0f) total=%.0f\n", npairs, (double)acc[0] / npairs, (double)acc[1] / npairs,
                     (double)acc[2] / npairs, (double)acc[3] / npairs, (double)acc[4] / npairs);
        if (acc[4] != 0)
        std::fprintf(stderr, "[amc tvg profile] per pair: counting loop=%.0f local_estimate(E5)=%.0f local_estimate(F8)=%.0f\n",
                     (double)acc[5] / npairs, (double)acc[6] / npairs, (double)acc[7] / npairs);
    }
    for (int i = 0; i < 12; ++i) out->work[i] += worksum[i];
    float ms = 0.f;
    if (!run.slices.empty()) (void)hipEventElapsedTime(&ms, c->vslices[0]->ev[0], c->ev[1]);
    const double t_post = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    out->device_ms = (double)ms;
    out->kernel_ms = kernel_ms;
    out->kernel_launches = run.launches;
    if (run.prof_host)
        std::fprintf(stderr, "[amc verify profile] pairs=%zu slices=%zu: host before the join %.1f ms (tables %.1f, lists + uploads %.1f), "
                     "join + pack + download %.1f (kernels %.1f)\n", npairs, run.slices.size(),
                     t_pre_ms, run.t_tables, run.t_lists, t_post, kernel_ms);
    if (run.o.compute_relative_pose) {
        // EstimateTwoViewGeometryPose on the selected inlier matches (mask order = match order): the matches
        // and the packed masks of this call are still on the device
        priv->pose.resize(npairs);
        double pose_ms = 0.0;
        const int rc = pose_impl(c, "amc_verify_pairs", run.slot1, run.slot2, npairs, match_offsets, matches, out->tvg,
                                 priv->pose.data(), &pose_ms, match_offsets, dev_matches, dev_off);
        if (rc != AMC_OK) return rc;
        for (size_t p = 0; p < npairs; ++p) out->tvg[p].config = priv->pose[p].config;
        out->pose = priv->pose.data();
        out->device_ms += pose_ms;
        out->kernel_ms += pose_ms;
        out->pose_kernel_ms = pose_ms;
        out->kernel_launches += 1;
    }
    if (run.mode == 0) {  // what the exchange step's verification half reads in place (amc_allgather_pair_records / _inlier_tables)
        c->vres.npairs = npairs;
        c->vres.total = total;
        // (EstimateTwoViewGeometryPose settles PLANAR_OR_PANORAMIC on the host copy of the records only)
        c->vres.tvg = run.o.compute_relative_pose ? nullptr : c->d_tvg_packed.p;
        c->vres.mask = c->d_mask_packed.p;
        c->vres.moff = c->d_moff.p;
        c->vres.tp = c->d_tp_all.p;
        c->vres.matches = run.kernel_matches;
    }
    return AMC_OK;
}

// EstimateMultipleTwoViewGeometries (TwoViewGeometryOptions.multiple_models): rounds of
// EstimateTwoViewGeometry over all still-active pairs at once, each on the matches its earlier
// rounds left over, until a pair's round comes back DEGENERATE.  All estimation runs in the kernel;
// the host only shrinks the match lists between rounds.
static int verify_multiple(amc_ctx* c, const uint32_t* slot1, const uint32_t* slot2, size_t npairs,
                           const uint64_t* match_offsets, const uint32_t* matches, const amc_tvg_opts& o,
                           uint32_t seed, amc_verify_result* out) {
    std::memset(out, 0, sizeof *out);
    if (npairs > 0 && (!slot1 || !slot2 || !match_offsets))
        return api_fail(AMC_E_INVALID, "amc_verify_pairs: NULL pair arrays");
    const uint64_t total = npairs ? match_offsets[npairs] : 0;
    if (total > 0 && !matches) return api_fail(AMC_E_INVALID, "amc_verify_pairs: NULL matches");
    for (size_t p = 0; p < npairs; ++p)
        if (match_offsets[p + 1] < match_offsets[p])
            return api_fail(AMC_E_INVALID, "amc_verify_pairs: match_offsets not monotone at %zu", p);
    amc_tvg_opts single = o;
    single.multiple_models = 0;
    VerifyPriv* priv = new (std::nothrow) VerifyPriv();
    if (!priv) return api_fail(AMC_E_NOMEM, "amc_verify_pairs: out of host memory");
    priv->tvg.resize(npairs);
    priv->mask.assign(total, 0);
    std::vector<std::vector<uint32_t>> remaining(npairs);  // indices into the pair's original matches
    std::vector<std::vector<amc_tvg>> kept(npairs);
    std::vector<amc_pose> first_pose(npairs);  // pose of a pair's first kept geometry
    for (size_t p = 0; p < npairs; ++p) pose_default(&first_pose[p], AMC_TVG_UNDEFINED);
    std::vector<size_t> active;
    for (size_t p = 0; p < npairs; ++p) {
        const size_t M = (size_t)(match_offsets[p + 1] - match_offsets[p]);
        remaining[p].resize(M);
        for (size_t i = 0; i < M; ++i) remaining[p][i] = (uint32_t)i;
        active.push_back(p);
    }
    double device_ms = 0.0, kernel_ms = 0.0, pose_ms = 0.0;
    uint64_t work[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t launches = 0;
    int rc = AMC_OK;
    for (int round = 0; round < 254 && !active.empty() && rc == AMC_OK; ++round) {
        std::vector<uint32_t> s1(active.size()), s2(active.size()), rm;
        std::vector<uint64_t> off(active.size() + 1, 0);
        for (size_t a = 0; a < active.size(); ++a) {
            const size_t p = active[a];
            s1[a] = slot1[p];
            s2[a] = slot2[p];
            const uint32_t* mm = matches + 2 * match_offsets[p];
            for (uint32_t i : remaining[p]) {
                rm.push_back(mm[2 * (size_t)i]);
                rm.push_back(mm[2 * (size_t)i + 1]);
            }
            off[a + 1] = off[a] + remaining[p].size();
        }
        amc_verify_result r;
        rc = verify_impl(c, 0, s1.data(), s2.data(), active.size(), off.data(), rm.data(), &single, seed, &r);
        if (rc != AMC_OK) break;
        device_ms += r.device_ms;
        kernel_ms += r.kernel_ms;
        for (int i = 0; i < 12; ++i) work[i] += r.work[i];
        pose_ms += r.pose_kernel_ms;
        launches += r.kernel_launches;
        std::vector<size_t> still;
        for (size_t a = 0; a < active.size(); ++a) {
            const size_t p = active[a];
            const amc_tvg& g = r.tvg[a];
            if (g.config == AMC_TVG_DEGENERATE) continue;  // this pair is finished
            const bool keep = !(o.multiple_ignore_watermark && g.config == AMC_TVG_WATERMARK);
            if (keep) {
                kept[p].push_back(g);
                if (kept[p].size() == 1 && r.pose) first_pose[p] = r.pose[a];
            }
            const uint8_t* mask = r.inlier_mask + off[a];
            std::vector<uint32_t> next;
            for (size_t k = 0; k < remaining[p].size(); ++k) {
                if (mask[k]) {
                    if (keep) priv->mask[match_offsets[p] + remaining[p][k]] = (uint8_t)kept[p].size();
                } else {
                    next.push_back(remaining[p][k]);
                }
            }
            if (next.size() == remaining[p].size()) continue;  // nothing left the pool: stop, do not spin
            remaining[p].swap(next);
            still.push_back(p);
        }
        amc_verify_result_free(&r);
        active.swap(still);
    }
    if (rc != AMC_OK) {
        delete priv;
        return rc;
    }
    if (o.compute_relative_pose) priv->pose.resize(npairs);
    for (size_t p = 0; p < npairs; ++p) {
        amc_tvg& t = priv->tvg[p];
        std::memset(&t, 0, sizeof t);
        if (o.compute_relative_pose) pose_default(&priv->pose[p], AMC_TVG_UNDEFINED);
        if (kept[p].empty()) {
            t.config = AMC_TVG_DEGENERATE;
            std::fill(priv->mask.begin() + match_offsets[p], priv->mask.begin() + match_offsets[p + 1], 0);
        } else if (kept[p].size() == 1) {
            t = kept[p][0];
            if (o.compute_relative_pose) priv->pose[p] = first_pose[p];
        } else {
            t.config = AMC_TVG_MULTIPLE;  // the models of a MULTIPLE geometry stay default (zero)
            for (const amc_tvg& g : kept[p]) t.num_inliers += g.num_inliers;
        }
        if (o.compute_relative_pose) priv->pose[p].config = t.config;
    }
    out->npairs = npairs;
    out->_priv = priv;
    out->tvg = priv->tvg.data();
    out->inlier_mask = priv->mask.data();
    out->pose = o.compute_relative_pose ? priv->pose.data() : nullptr;
    out->pose_kernel_ms = pose_ms;
    out->device_ms = device_ms;
    out->kernel_ms = kernel_ms;
    out->kernel_launches = launches;
    for (int i = 0; i < 12; ++i) out->work[i] = work[i];
    c->vres = amc::VerifyResident{};  // (the rounds' calls left the LAST round's shrunken lists: not this call's result)
    return AMC_OK;
}

int amc_verify_pairs(amc_ctx* c, const uint32_t* slot1, const uint32_t* slot2, size_t npairs,
                     const uint64_t* match_offsets, const uint32_t* matches,
                     const amc_tvg_opts* opts_in, uint32_t seed, amc_verify_result* out) {
    const uint64_t total = (c && out && npairs > 0 && match_offsets) ? match_offsets[npairs] : 0;
    if (total > 0 && !matches) {
        // the resident match table (amc_upload_matches, or the last match call's rows) instead of rows over PCIe
        if (opts_in && opts_in->multiple_models) {
            std::memset(out, 0, sizeof *out);
            return api_fail(AMC_E_INVALID, "amc_verify_pairs: multiple_models needs the match rows on the host (matches is NULL)");
        }
        if (c->resident_matches != total) {
            std::memset(out, 0, sizeof *out);
            return api_fail(AMC_E_STATE, "amc_verify_pairs: matches is NULL and the resident match table holds %llu rows, not the "
                            "%llu of match_offsets", (unsigned long long)c->resident_matches, (unsigned long long)total);
        }
        const uint64_t keep = c->resident_matches;  // (verify_impl drops a resident verification result, not the match table)
        const int rc = verify_impl(c, 0, slot1, slot2, npairs, match_offsets, nullptr, opts_in, seed, out, c->d_keep.p, match_offsets);
        c->resident_matches = keep;
        return rc;
    }
    if (c && out && opts_in && opts_in->multiple_models)
        return verify_multiple(c, slot1, slot2, npairs, match_offsets, matches, *opts_in, seed, out);
    return verify_impl(c, 0, slot1, slot2, npairs, match_offsets, matches, opts_in, seed, out);
}

int amc_match_verify_pairs(amc_ctx* c, const uint32_t* slot1, const uint32_t* slot2, size_t npairs,
                           const amc_match_opts* match_opts, const amc_tvg_opts* tvg_opts, uint32_t seed,
                           amc_match_result* match_out, amc_verify_result* verify_out) {
    if (!c || !match_out || !verify_out) return api_fail(AMC_E_INVALID, "amc_match_verify_pairs: NULL ctx/out");
    std::memset(verify_out, 0, sizeof *verify_out);
    const bool serial = env_flag("AMC_PIPELINE_SERIAL");  // (A/B hook: the stages behind each other, as before round 6)
    if (tvg_opts && tvg_opts->multiple_models) {
        // EstimateMultipleTwoViewGeometries shrinks the match lists on the host between rounds: no resident path
        int rc = match_impl(c, slot1, slot2, npairs, match_opts, nullptr, 0.0, match_out);
        if (rc != AMC_OK) return rc;
        rc = amc_verify_pairs(c, slot1, slot2, npairs, match_out->offsets, match_out->matches, tvg_opts, seed, verify_out);
        if (rc != AMC_OK) amc_match_result_free(match_out);
        return rc;
    }
    if (serial) {
        std::vector<uint64_t> keep_off;
        int rc = match_impl(c, slot1, slot2, npairs, match_opts, nullptr, 0.0, match_out, &keep_off);
        if (rc != AMC_OK) return rc;
        rc = verify_impl(c, 0, slot1, slot2, npairs, match_out->offsets, match_out->matches, tvg_opts, seed, verify_out,
                         c->d_keep.p ? c->d_keep.p : reinterpret_cast<const uint32_t*>(c->d_scalars), keep_off.data());
        if (rc != AMC_OK) amc_match_result_free(match_out);
        return rc;
    }
    // The HOST sides of the two stages interleaved: the verification run is set up first (nothing of it depends on the
    // matches), and every match batch hands its pairs over while the next batch is scanned - their checks, pair records,
    // trial tables and size classes are done beside that scan.  ONE slice is closed and launched when the last batch
    // is done (three slices of ~3,000 verified pairs each have three tails: 38.9 ms of kernels against 35.3 for one,
    // profiles/r06/ab_final_v1.txt): on the device the stages stay behind each other, because the chip is bound by its
    // power budget - verification beside a scan takes from the scan what it gets (profiles/r06/ab_cus_v2.txt: the scan
    // leaving 24 .. 96 CUs to the verification of the batch before, 3 .. 8 batches, all within 1 % of the serial order;
    // DESIGN.md section 6).
    std::memset(match_out, 0, sizeof *match_out);
    if (npairs > 0 && (!slot1 || !slot2)) return api_fail(AMC_E_INVALID, "amc_match_verify_pairs: NULL pair arrays");
    c->vres = amc::VerifyResident{};
    const auto wall0 = std::chrono::steady_clock::now();
    VerifyRun run{};
    run.c = c;
    run.mode = 0;
    run.slot1 = slot1;
    run.slot2 = slot2;
    run.npairs = npairs;
    if (tvg_opts) run.o = *tvg_opts; else amc_tvg_opts_default(&run.o);
    run.seed = seed;
    for (size_t p = 0; p < npairs; ++p)  // (the match call checks this too; the verification set-up reads the slots first)
        if (slot1[p] >= c->slots.size() || slot2[p] >= c->slots.size())
            return api_fail(AMC_E_INVALID, "amc_match_verify_pairs: pair %zu references slot out of range", p);
    int rc = run.begin(0);
    if (rc != AMC_OK) return rc;
    const double t_setup = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    run.st_e = run.st_fh = c->stream;  // the one slice of this call: E and F/H behind each other on the ctx's stream
    VerifyPriv* priv = new (std::nothrow) VerifyPriv();
    if (!priv) return api_fail(AMC_E_NOMEM, "amc_match_verify_pairs: out of host memory");
    struct Guard {  // every failure: nothing left in flight, both results zeroed
        amc_ctx* c;
        VerifyPriv* p;
        amc_verify_result* o;
        amc_match_result* m;
        bool match_done = false;
        ~Guard() {
            if (p) {
                verify_streams_sync(c);
                delete p;
                std::memset(o, 0, sizeof *o);
                if (match_done) amc_match_result_free(m);
            }
        }
    } guard{c, priv, verify_out, match_out};
    std::vector<uint64_t> keep_off;
    // every match batch's pairs join the open slice (host only; the slice is closed below)
    const BatchHook hook = [&](size_t, size_t end, const uint64_t* offsets, const uint64_t* koff) -> int {
        const uint32_t* km = c->d_keep.p ? c->d_keep.p : reinterpret_cast<const uint32_t*>(c->d_scalars);
        return run.add_pairs(run.submitted, end, offsets, koff, km, nullptr);
    };
    rc = match_impl(c, slot1, slot2, npairs, match_opts, nullptr, 0.0, match_out, &keep_off, npairs ? &hook : nullptr);
    if (rc != AMC_OK) return rc;
    guard.match_done = true;
    const double t_match = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    {
        const uint32_t* km = c->d_keep.p ? c->d_keep.p : reinterpret_cast<const uint32_t*>(c->d_scalars);
        if (run.submitted < npairs) {
            rc = run.add_pairs(run.submitted, npairs, match_out->offsets, keep_off.data(), km, nullptr);
            if (rc != AMC_OK) return rc;
        }
        run.kernel_matches = km;  // (the resident table may have moved while it grew)
        rc = run.close_slice(nullptr);
        if (rc != AMC_OK) return rc;
    }
    const double t_pre = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    rc = verify_finish(c, run, match_out->offsets, match_out->matches, verify_out, priv,
                       c->d_keep.p ? c->d_keep.p : reinterpret_cast<const uint32_t*>(c->d_scalars), keep_off.data(), t_pre);
    if (rc != AMC_OK) return rc;
    guard.p = nullptr;
    {
        const double t_end = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        const double tl[8] = {t_setup, t_match, t_pre, t_end, t_end, c->last_hook_ms, 0.0, 0.0};
        std::memcpy(c->timeline, tl, sizeof tl);
    }
    if (run.prof_host)  // the call's timeline on the host (ms since entry)
        std::fprintf(stderr, "[amc pipeline profile] pairs=%zu: verification set up at %.2f, match call back at %.2f, slice closed + launched at %.2f, "
                     "results on the host at %.2f\n", npairs, t_setup, t_match, t_pre,
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count());
    return AMC_OK;
}

int amc_ctx_last_timeline(amc_ctx* c, double out_ms[8]) {
    if (!c || !out_ms) return api_fail(AMC_E_INVALID, "amc_ctx_last_timeline: NULL argument");
    std::memcpy(out_ms, c->timeline, sizeof c->timeline);
    return AMC_OK;
}

int amc_pose_pairs(amc_ctx* c, const uint32_t* slot1, const uint32_t* slot2, size_t npairs,
                   const uint64_t* match_offsets, const uint32_t* inlier_matches, const amc_tvg* geoms,
                   amc_pose* out) {
    return pose_impl(c, "amc_pose_pairs", slot1, slot2, npairs, match_offsets, inlier_matches, geoms, out, nullptr);
}

namespace {
struct RansacPriv {
    std::vector<amc_ransac_report> reports;
    std::vector<uint8_t> mask;
};
}  // namespace

int amc_ransac_pairs(amc_ctx* c, int kind, const uint32_t* slot1, const uint32_t* slot2, size_t npairs,
                     const uint64_t* match_offsets, const uint32_t* matches,
                     const amc_ransac_opts* ropts, uint32_t seed, amc_ransac_result* out) {
    if (!c || !out) return api_fail(AMC_E_INVALID, "amc_ransac_pairs: NULL ctx/out");
    std::memset(out, 0, sizeof *out);
    if (kind != AMC_RANSAC_F && kind != AMC_RANSAC_H && kind != AMC_RANSAC_E)
        return api_fail(AMC_E_INVALID, "amc_ransac_pairs: unknown estimator kind %d", kind);
    amc_tvg_opts o;
    amc_tvg_opts_default(&o);
    if (ropts) o.ransac = *ropts;
    o.detect_watermark = 0;
    amc_verify_result v;
    const int mode = kind == AMC_RANSAC_F ? 1 : (kind == AMC_RANSAC_H ? 2 : 3);
    const int rc = verify_impl(c, mode, slot1, slot2, npairs, match_offsets, matches, &o, seed, &v);
    if (rc != AMC_OK) return rc;
    RansacPriv* priv = new (std::nothrow) RansacPriv();
    if (!priv) {
        amc_verify_result_free(&v);
        return api_fail(AMC_E_NOMEM, "amc_ransac_pairs: out of host memory");
    }
    const uint64_t total = npairs ? match_offsets[npairs] : 0;
    priv->reports.resize(npairs);
    priv->mask.assign(v.inlier_mask, v.inlier_mask + total);
    const int which = kind == AMC_RANSAC_F ? 1 : (kind == AMC_RANSAC_H ? 2 : 0);  // num_trials / inliers slot
    for (size_t p = 0; p < npairs; ++p) {
        const amc_tvg& g = v.tvg[p];
        amc_ransac_report& r = priv->reports[p];
        r.success = g.config;
        r.num_inliers = g.num_inliers;
        r.num_trials = g.num_trials[which];
        const double* m = kind == AMC_RANSAC_F ? g.F : (kind == AMC_RANSAC_H ? g.H : g.E);
        for (int i = 0; i < 9; ++i) r.model[i] = m[i];
    }
    out->npairs = npairs;
    out->reports = priv->reports.data();
    out->inlier_mask = priv->mask.data();
    out->device_ms = v.device_ms;
    out->_priv = priv;
    amc_verify_result_free(&v);
    return AMC_OK;
}

void amc_ransac_result_free(amc_ransac_result* r) {
    if (!r) return;
    delete static_cast<RansacPriv*>(r->_priv);
    std::memset(r, 0, sizeof *r);
}

int amc_squared_sampson_error(amc_ctx* c, const double* points1, const double* points2, size_t n,
                              const double E[9], double* out) {
    if (!c) return api_fail(AMC_E_INVALID, "amc_squared_sampson_error: ctx is NULL");
    if (n == 0) return AMC_OK;
    if (!points1 || !points2 || !E || !out) return api_fail(AMC_E_INVALID, "amc_squared_sampson_error: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    DevBuf<double> buf;
    HIPCHK(buf.ensure(5 * n + 16));
    double* d1 = buf.p;
    double* d2 = d1 + 2 * n;
    double* dout = d2 + 2 * n;
    double* dE = dout + n;
    hipStream_t st = c->stream;
    int rc = AMC_OK;
    auto chk = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == AMC_OK) rc = api_fail(AMC_E_HIP, "amc_squared_sampson_error: %s: %s", what, hipGetErrorString(e));
    };
    chk(hipMemcpyAsync(d1, points1, 2 * n * sizeof(double), hipMemcpyHostToDevice, st), "copy points1");
    chk(hipMemcpyAsync(d2, points2, 2 * n * sizeof(double), hipMemcpyHostToDevice, st), "copy points2");
    chk(hipMemcpyAsync(dE, E, 9 * sizeof(double), hipMemcpyHostToDevice, st), "copy E");
    if (rc == AMC_OK) chk(launch_sampson(d1, d2, n, dE, dout, st), "launch");
    if (rc == AMC_OK) chk(hipMemcpyAsync(out, dout, n * sizeof(double), hipMemcpyDeviceToHost, st), "copy out");
    chk(hipStreamSynchronize(st), "sync");
    return rc;
}

int amc_homography_decomposition(amc_ctx* c, const double H[9], const double K1[9], const double K2[9],
                                 const double* points1, const double* points2, size_t n, double R[9], double t[3],
                                 double normal[3], double* points3D, uint64_t* num_points3D) {
    if (!c) return api_fail(AMC_E_INVALID, "amc_homography_decomposition: ctx is NULL");
    if (!H || !K1 || !K2 || !R || !t || !normal || !num_points3D || (n > 0 && (!points1 || !points2 || !points3D)))
        return api_fail(AMC_E_INVALID, "amc_homography_decomposition: NULL argument");
    if (n > 0xFFFFFFFFull / 4) return api_fail(AMC_E_INVALID, "amc_homography_decomposition: too many points");
    HIPCHK(hipSetDevice(c->device));
    DevBuf<double> buf;
    HIPCHK(buf.ensure(7 * n + 27 + 16 + 8));
    double* d1 = buf.p;
    double* d2 = d1 + 2 * n;
    double* dX = d2 + 2 * n;
    double* din = dX + 3 * n;
    double* dout = din + 27;
    hipStream_t st = c->stream;
    int rc = AMC_OK;
    auto chk = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == AMC_OK) rc = api_fail(AMC_E_HIP, "amc_homography_decomposition: %s: %s", what, hipGetErrorString(e));
    };
    double in[27], o[16];
    std::memcpy(in, H, 9 * sizeof(double));
    std::memcpy(in + 9, K1, 9 * sizeof(double));
    std::memcpy(in + 18, K2, 9 * sizeof(double));
    if (n) {
        chk(hipMemcpyAsync(d1, points1, 2 * n * sizeof(double), hipMemcpyHostToDevice, st), "copy points1");
        chk(hipMemcpyAsync(d2, points2, 2 * n * sizeof(double), hipMemcpyHostToDevice, st), "copy points2");
    }
    chk(hipMemcpyAsync(din, in, sizeof in, hipMemcpyHostToDevice, st), "copy H, K1, K2");
    if (rc == AMC_OK) chk(launch_homography_decomposition(din, d1, d2, (uint32_t)n, dout, dX, st), "launch");
    if (rc == AMC_OK) chk(hipMemcpyAsync(o, dout, sizeof o, hipMemcpyDeviceToHost, st), "copy out");
    chk(hipStreamSynchronize(st), "sync");
    if (rc == AMC_OK) {
        std::memcpy(R, o, 9 * sizeof(double));
        std::memcpy(t, o + 9, 3 * sizeof(double));
        std::memcpy(normal, o + 12, 3 * sizeof(double));
        const uint64_t m = (uint64_t)o[15];
        *num_points3D = m;
        if (m) {
            chk(hipMemcpyAsync(points3D, dX, 3 * m * sizeof(double), hipMemcpyDeviceToHost, st), "copy points3D");
            chk(hipStreamSynchronize(st), "sync");
        }
    }
    return rc;
}

void amc_verify_result_free(amc_verify_result* r) {
    if (!r) return;
    delete static_cast<VerifyPriv*>(r->_priv);
    std::memset(r, 0, sizeof *r);
}

}  // extern "C"
