// amc_ctx.h — private to the host units of libamc.so (amc_api.hip, amc_match.hip, amc_verify.hip): the context behind
// the opaque amc_ctx of include/amc.h, the types it is made of, and the few functions that cross those units.
#pragma once

#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "amc_internal.h"
#include "slot_arena.h"
#include "scan_accept.h"

namespace amc {

inline uint32_t round_up(uint32_t x, uint32_t m) { return (x + m - 1) / m * m; }

struct Slot {
    void* base = nullptr;  // one allocation: raw | prep | rs128
    ImageDev dev{};
    uint32_t maxsq = 0;    // max_r |raw[r]|^2
    bool valid = false;
    float* kp = nullptr;   // rows x 2 float32 keypoints (x, y)
    double* kp64 = nullptr;  // or rows x 2 float64 points (amc_upload_points_f64)
    double* kpn = nullptr;   // rows x 2 float64 CamFromImg of the points (cameras with distortion), see ensure_normalized
    bool kpn_valid = false;  // kpn matches the current points and camera
    uint32_t kp_rows = 0;
    bool has_kp = false, has_cam = false;
    CameraDev cam{};
    void* grid_base = nullptr;  // guided matching's keypoint grid: sxy | sidx | cell_start (one allocation)
    GridDev grid{};             // n == 0: none (no float32 keypoints, or non-finite coordinates)
};

// The slots' device memory: amc::SlotArenaT (slot_arena.h) over the HIP allocator.
struct HipRaw {
    static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
    static void free(void* p) { (void)hipFree(p); }
    static void clear_error() { (void)hipGetLastError(); }
};
struct SlotArena : amc::SlotArenaT<HipRaw> {
    template <class T>
    hipError_t alloc(T** out, size_t bytes) {
        return (hipError_t)amc::SlotArenaT<HipRaw>::alloc(out, bytes);
    }
};

// Pinned host buffers behind amc_match_result.matches.  A result leases one (the D2H copies of a call land in it
// directly); amc_match_result_free returns it for the next call, so a pipeline allocates pinned memory once.  The
// pool is shared-owned: results may outlive their context.
struct PinnedPool {
    // Idle buffers are kept for the next call, but not without bound: at most three, and at most kMaxIdleBytes in
    // total (a dense 500 x 4096 call returns a 1 GiB table: one such buffer stays, a second one does not).  With one
    // context per device (gpu_index "-1") the bound holds per device.  amc_ctx_trim empties the pool.
    static constexpr size_t kMaxIdleBytes = (size_t)3 << 29;  // 1.5 GiB
    std::mutex mu;
    std::vector<PinBuf<uint32_t>> idle;
    // want (elements): the smallest idle buffer that holds it, else the largest (the caller grows it).  A call that leases
    // two buffers of different sizes (verification: records and masks) would otherwise hand the larger one to whichever
    // lease comes first and re-allocate the other - a hipHostMalloc of tens of MB in every early call of a run.
    PinBuf<uint32_t> acquire(size_t want = 0) {
        std::lock_guard<std::mutex> lock(mu);
        if (idle.empty()) return PinBuf<uint32_t>();
        auto better = [&](const PinBuf<uint32_t>& a, const PinBuf<uint32_t>& b) {
            const bool fa = a.cap >= want, fb = b.cap >= want;
            if (want && fa != fb) return fa;       // one that fits beats one that does not
            if (want && fa) return a.cap < b.cap;  // both fit: the smaller
            return a.cap > b.cap;                  // neither fits (or no wish): the larger
        };
        size_t best = 0;
        for (size_t i = 1; i < idle.size(); ++i)
            if (better(idle[i], idle[best])) best = i;
        PinBuf<uint32_t> b = std::move(idle[best]);
        idle.erase(idle.begin() + best);
        return b;
    }
    void give_back(PinBuf<uint32_t> b) {
        if (!b.p) return;
        std::lock_guard<std::mutex> lock(mu);
        idle.push_back(std::move(b));
        auto total = [&] {
            size_t t = 0;
            for (auto& x : idle) t += x.cap * sizeof(uint32_t);
            return t;
        };
        // drop the smallest until the bounds hold (the largest is the one the next call of a pipeline wants); a single
        // buffer above the byte bound is dropped as well
        while (!idle.empty() && (idle.size() > 3 || total() > kMaxIdleBytes)) {
            size_t small = 0;
            for (size_t i = 1; i < idle.size(); ++i)
                if (idle[i].cap < idle[small].cap) small = i;
            idle.erase(idle.begin() + small);
        }
    }
    void trim() {
        std::lock_guard<std::mutex> lock(mu);
        idle.clear();
    }
};

// Verification runs as slices (VerifyRun below).  A slice owns its trial tables and mask buffers, and per size class its
// pair lists, workspaces and queue heads: slice k's F/H kernel runs beside slice k + 1's essential-matrix kernel, and
// the masks stay where they are until the call's packing step.  Grow-only, kept by the context across calls.
struct VerifyClassSlot {
    PinBuf<TvgPair> h_pairs, h_pairs_e;  // pinned staging of the two lists
    DevBuf<TvgPair> pairs, pairs_e;
    DevBuf<double> ws, ws_e;
    DevBuf<uint8_t> maskws;
    void release() { pairs.release(); pairs_e.release(); ws.release(); ws_e.release(); maskws.release(); h_pairs.release(); h_pairs_e.release(); }
};
struct VerifySliceBufs {
    PinBuf<uint32_t> h_tabs;
    DevBuf<uint32_t> tabs;
    DevBuf<uint8_t> outmask, emask;
    VerifyClassSlot cls[4];
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // E launches begin / end, F/H launches begin / end
    hipEvent_t ev_e_done = nullptr, ev_aux_done = nullptr;
    bool aux_pending = false;
    void release() {
        tabs.release(); outmask.release(); emask.release(); h_tabs.release();
        for (auto& k : cls) k.release();
    }
    ~VerifySliceBufs() {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
        if (ev_e_done) (void)hipEventDestroy(ev_e_done);
        if (ev_aux_done) (void)hipEventDestroy(ev_aux_done);
    }
};
constexpr size_t kVScalarWords = 128;  // [0] bad match indices, [1] stream overruns, [2 + 8 slice + 2 class (+ 1)] queue heads
constexpr size_t kMaxStreamWords = (size_t)1 << 28;  // 1 GiB of words: max_num_trials ~ 1.6e7 at the default ratio

// key of a cached dyn_max_num_trials table
struct TrialTabKey {
    uint32_t M;
    double confidence, multiplier;
    bool operator<(const TrialTabKey& o) const {
        if (M != o.M) return M < o.M;
        if (confidence != o.confidence) return confidence < o.confidence;
        return multiplier < o.multiplier;
    }
};
constexpr size_t kTrialTabCacheWords = size_t(64) << 20;  // 256 MB of uint32

}  // namespace amc

using namespace amc;  // (amc_ctx is the C header's global name; the three units that include this say the same themselves)

struct amc_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;  // D2H of a batch's matches, beside the next batch's kernels
    hipEvent_t cev[2] = {nullptr, nullptr};  // batch set k's matches are in place in d_keep
    // verification: the launches of the larger size classes (few pairs, each several milliseconds on one wave) run on this
    // stream beside the bulk class on `stream` instead of behind it, with their own pair lists and workspaces
    hipStream_t aux_stream = nullptr;
    hipEvent_t aev[2] = {nullptr, nullptr};
    std::vector<Slot> slots;
    bool table_dirty = true;
    DevBuf<ImageDev> d_imgs;
    DevBuf<GridDev> d_grids;   // guided matching's keypoint grids, by slot (uploaded with d_imgs)
    float* d_lut = nullptr;
    std::vector<float> h_lut;
    // the scan's accept-bit thresholds (scan_accept.h) for the last (max_ratio, max_distance) a match call used
    ScanAccept* d_accept = nullptr;
    ScanAccept h_accept{};
    float accept_ratio = 0.f, accept_distance = 0.f;
    bool accept_valid = false;
    uint32_t* d_scalars = nullptr;  // [0] cursor, [1] queue head, [2] maxsq scratch, [3] resolve errors, [4] stream overrun, [5] mfma items, [6] forward scan's runs, [7] copy parts taken, [8] [9] [10] lengths of the live lists (forward order, pair order, reverse order)
    // per-batch scratch of the match loop: a batch's cross-check chain (resolve, candidate selection, reverse scan,
    // finalize) is done before the next batch's forward scan writes the tables (match_impl)
    struct MatchScratch {
        DevBuf<PairDev> d_pairs;
        DevBuf<Dot4Work> d_work;
        DevBuf<uint32_t> d_order, d_order2;
        // mfma work items: group cuts of the two queue orders, scratch of the packing kernels, the descriptors
        DevBuf<uint32_t> d_grp, d_grp2, d_seg_base, d_grp_segs, d_grp_item_base;
        DevBuf<SegDesc> d_segs;
        DevBuf<uint32_t> d_run_base, d_run_items;  // the forward scan's run table (match_mfma.hip, "Runs")
        DevBuf<Top2> d_rowbuf, d_colbuf;
        DevBuf<uint32_t> d_accmask;  // one accept bit per row-table entry (mfma pairs)
        DevBuf<GuidedDev> d_guided;  // guided matching: one filter model per pair of the batch
        DevBuf<uint32_t> d_pair_off, d_pair_cnt, d_matches, d_cand_cnt, d_candbuf;
        // live pairs of the batch (launch_live_pairs): the per-pair flag and the three ordered lists the cross-check
        // chain's kernels index - d_order's live mfma pairs, every live pair, d_order2's pairs with candidates
        DevBuf<uint32_t> d_live, d_live_fwd, d_live_all, d_live_rev, d_live_scan;  // (d_live_scan: the compactions' scratch)
        void release_all() {
            d_pairs.release(); d_work.release(); d_order.release(); d_order2.release();
            d_grp.release(); d_grp2.release(); d_seg_base.release(); d_grp_segs.release();
            d_grp_item_base.release(); d_segs.release(); d_run_base.release(); d_run_items.release();
            d_rowbuf.release(); d_colbuf.release(); d_accmask.release(); d_guided.release();
            d_pair_off.release(); d_pair_cnt.release(); d_matches.release();
            d_cand_cnt.release(); d_candbuf.release();
            d_live.release(); d_live_fwd.release(); d_live_all.release(); d_live_rev.release();
            d_live_scan.release();
        }
        void release_large() {  // (amc_ctx_trim)
            d_rowbuf.release(); d_colbuf.release(); d_accmask.release(); d_matches.release(); d_candbuf.release();
            d_segs.release(); d_seg_base.release(); d_run_items.release();
        }
    };
    MatchScratch ms;
    // amc_match_verify_pairs: the matches of every batch of the call stay here (appended batch after batch), so
    // that the verification kernel reads them where the matcher left them instead of from a host round trip
    DevBuf<uint32_t> d_keep;
    DevBuf<uint64_t> d_csr;                 // per batch: where each pair's matches go in d_keep (pair order)
    uint64_t resident_matches = 0;          // matches of the LAST match call, in its result's CSR order, at d_keep (amc_ctx_resident_matches)
    PinBuf<uint64_t> h_csr[2];
    std::shared_ptr<PinnedPool> result_pool = std::make_shared<PinnedPool>();
    SlotArena arena;  // the slots' device memory
    // host staging of a match batch, two sets: batch k+1 is prepared and enqueued while the results of
    // batch k are still being copied out and scattered (match_impl)
    PinBuf<PairDev> h_pairs[2];
    PinBuf<Dot4Work> h_work[2];
    PinBuf<uint32_t> h_order[2], h_order2[2], h_pair_off[2], h_pair_cnt[2], h_matches[2], h_bscalars[2];
    PinBuf<uint32_t> h_grp[2], h_grp2[2];  // where the streamed image changes in h_order / h_order2 (ngroups + 1 cuts)
    PinBuf<uint32_t> h_scalars;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t bev[2][5] = {{nullptr, nullptr, nullptr, nullptr, nullptr},
                            {nullptr, nullptr, nullptr, nullptr, nullptr}};  // scan start/end, cross end, small D2H, matches
    // verification scratch
    DevBuf<TvgImage> d_timgs;
    DevBuf<uint32_t> d_tmatches;
    DevBuf<TvgEState> d_estate;       // essential-matrix kernel -> F/H kernel hand-off, by pair
    // the slices of a verification run (lists, workspaces, tables, masks), its streams and events
    std::vector<std::unique_ptr<VerifySliceBufs>> vslices;
    hipStream_t vstream = nullptr;  // a sliced run's F/H launches (the E launches go to `stream`)
    hipEvent_t vev_setup = nullptr, vev_matches = nullptr;
    uint32_t* d_vscalars = nullptr;   // kVScalarWords
    std::vector<double> wm_cut_cache; // TvgParams::wm_cut for (wm_cut_conf, wm_cut_mult)
    double wm_cut_conf = 0.0, wm_cut_mult = 0.0;
    bool wm_cut_on_device = false;    // d_wmcut holds wm_cut_cache
    // Every upload of a verification call comes from pinned memory (round 6: the pageable ones - a few hundred KB each -
    // stalled a call by 10-20 ms once in ten to twenty calls, profiles/r06/pipeline_timeline_v1.txt), and the image table
    // is uploaded only when it changed.
    PinBuf<TvgImage> h_timgs;
    std::vector<TvgImage> timgs_on_device;
    PinBuf<TvgPair> h_tp;             // the call's pair records in the caller's order (VerifyRun::tp)
    PinBuf<uint64_t> h_moff;
    // tempered words of std::mt19937(seed): the sample stream every pair consumes (TvgParams::stream)
    DevBuf<uint32_t> d_stream;
    uint32_t stream_seed = 0;
    size_t stream_len = 0;
    DevBuf<double> d_wmcut;
    DevBuf<TvgOut> d_tout;
    // the call's results in the caller's layout (pack_verify_kernel): records without their counters, masks at the
    // input's CSR offsets - copied straight into the pinned buffers the result leases
    DevBuf<amc_tvg> d_tvg_packed;
    DevBuf<uint8_t> d_mask_packed;
    DevBuf<uint64_t> d_moff;
    DevBuf<TvgPair> d_tp_all;
    DevBuf<unsigned long long> d_worksum;
    amc::VerifyResident vres;  // the last verification call's results, where they lie (amc_internal.h)
    double timeline[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // amc_ctx_last_timeline
    double last_hook_ms = 0.0;
    std::shared_ptr<PinnedPool> verify_pool = std::make_shared<PinnedPool>();
    PinBuf<TvgOut> h_tout;    // where the records and masks of a verification call land (copied out before return)
    PinBuf<uint8_t> h_tmask;
    // dyn_max_num_trials tables by (match count, confidence, multiplier), see verify_impl
    std::map<TrialTabKey, std::vector<uint32_t>> trial_tabs;
    size_t trial_tab_words = 0;
    // relative-pose scratch
    DevBuf<PosePair> d_ppairs;
    DevBuf<uint32_t> d_pmatches;
    DevBuf<double> d_pcos;
    DevBuf<PoseOut> d_pout;
    PinBuf<PosePair> h_ppairs;  // pose_impl's staging (pinned, kept: 10^5 pairs are 23 + 32 MB; pageable vectors cost their
    PinBuf<PoseOut> h_pout;     //  first touch and a staged copy in every call)
};

namespace amc {

// amc_match.hip.  amc_match_pairs, and with `geoms` != nullptr guided matching (every pair then runs the dot4
// kernel with the pair's float32 filter; geoms[p] must have a configuration COLMAP guides on)
// keep_off != nullptr: the matches also stay on the device (c->d_keep) and keep_off[p] receives the position
// (in matches) of pair p's list there.
// batch_hook (amc_match_verify_pairs): called once per batch, in order, as soon as the batch's matches are in the
// resident table and the NEXT batch has been enqueued - with the pairs [begin, end) of the batch, the call's CSR offsets
// (valid up to `end`) and where each pair's rows start in the resident table.  Its host work runs beside the next
// batch's scan.
using BatchHook = std::function<int(size_t begin, size_t end, const uint64_t* offsets, const uint64_t* keep_off)>;
int match_impl(amc_ctx* c, const uint32_t* slot1, const uint32_t* slot2, size_t npairs, const amc_match_opts* opts_in,
               const amc_tvg* geoms, double max_error, amc_match_result* out, std::vector<uint64_t>* keep_off = nullptr,
               const BatchHook* batch_hook = nullptr);

// amc_api.hip.  Camera::CamFromImg of all keypoints of a slot, once per (points, camera); the verification kernels'
// image table from the slots.
int ensure_normalized(amc_ctx* c, uint32_t slot);
void fill_tvg_images(const amc_ctx* c, std::vector<TvgImage>& timgs);

}  // namespace amc
