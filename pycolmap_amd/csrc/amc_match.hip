// amc_match.hip — host side of libamc.so, matching: the batch loop behind amc_match_pairs and amc_match_guided_pairs
// (match_impl, which amc_match_verify_pairs in amc_verify.hip drives too).  No kernels here: the launches are in
// match_common.hip, match_mfma.hip, match_dot4.hip and match_guided.hip.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <vector>

#include "amc_ctx.h"
#include "scan_run.h"

using namespace amc;

namespace {

struct ResultPriv {
    std::vector<uint64_t> offsets;
    PinBuf<uint32_t> matches;               // leased from the context's pool, returned by amc_match_result_free
    std::shared_ptr<PinnedPool> pool;
    ~ResultPriv() {
        if (pool) pool->give_back(std::move(matches));
    }
};

// limits for one batch (bytes of device scratch)
// sized for 288 GB of HBM: few, large batches (each batch ends in a host synchronisation)
constexpr size_t kMaxTop2Entries = (size_t)256 << 20;  // 256 Mi entries x 16 B = 4 GiB per side
constexpr size_t kMaxMatchCap = (size_t)256 << 20;     // worst-case matches of a batch: x 8 B = 2 GiB (device)

}  // namespace

// Whether a guided pair may take the candidate-generation kernel (match_guided.hip), and what that kernel needs
// beyond the float model: guided_region.h's guided_pair_setup on the two images' keypoint boxes.  Anything it turns
// down keeps the dense kernel, which evaluates the filter on all n1 x n2 pairings.
static void guided_grid_setup(GuidedDev& g, const GridDev& g1, const GridDev& g2, bool dense_only) {
    g.grid_ok = 0;
    g.bound[0] = g.bound[1] = 0.0;
    for (int k = 0; k < 9; ++k) g.minv[k] = 0.0;
    if (dense_only || g1.n == 0 || g2.n == 0) return;
    const float box1[4] = {g1.x0, g1.y0, g1.bx1, g1.by1}, box2[4] = {g2.x0, g2.y0, g2.bx1, g2.by1};
    g.grid_ok = guided::guided_pair_setup(g.kind, g.m, g.max_residual, box1, box2, g.bound, g.minv) ? 1 : 0;
}

// amc_match_pairs, guided matching and the match half of amc_match_verify_pairs (the arguments: amc_ctx.h)
int amc::match_impl(amc_ctx* c, const uint32_t* slot1, const uint32_t* slot2, size_t npairs,
                    const amc_match_opts* opts_in, const amc_tvg* geoms, double max_error,
                    amc_match_result* out, std::vector<uint64_t>* keep_off, const BatchHook* batch_hook) {
    if (!c || !out) return api_fail(AMC_E_INVALID, "amc_match_pairs: NULL ctx/out");
    std::memset(out, 0, sizeof *out);
    if (npairs > 0 && (!slot1 || !slot2))
        return api_fail(AMC_E_INVALID, "amc_match_pairs: NULL pair arrays");
    // the call's environment switches
    const bool prof = env_flag("AMC_MATCH_PROFILE");  // wall-clock of the call's host phases on stderr
    const bool guided_dense_only = env_flag("AMC_GUIDED_DENSE");      // (test hook: the dense kernel for every pair)
    const bool accept_trivial = env_flag("AMC_SCAN_ACCEPT_TRIVIAL");  // (test hook: keep every row with best >= min_best)
    const bool resolve_ungrouped = env_flag("AMC_RESOLVE_UNGROUPED"); // (test hook: the per-row kernel)
    // (test hook: a smaller per-batch budget, so that small inputs exercise the multi-batch pipeline; 0: not set)
    const size_t batch_entries = (size_t)env_int("AMC_MATCH_BATCH_ENTRIES", 0, 0, (long long)kMaxTop2Entries);
    const char* const d2h_env = std::getenv("AMC_D2H");  // "memcpy" / "stream": how a batch's matches reach the host (below)
    // (smaller copies are not worth a scan's prologue; the tests take the path with small inputs)
    const size_t fuse_min_bytes = (size_t)env_int("AMC_D2H_FUSE_MIN_BYTES", 1 << 20, 0, std::numeric_limits<long long>::max());
    // the forward scan's run length (scan_run.h): 0 auto, 1 off, 2 / 4 / 8 forced (test and A/B hook)
    const int scan_run_env = (int)env_int("AMC_SCAN_RUN", 0, 0, 8);
    const int hook_split_mode = (int)env_int("AMC_HOOK_SPLIT", 1, 0, 2);  // 0: off; 2: also calls of a few pairs (the tests' way to the path)
    const auto wall0 = std::chrono::steady_clock::now();
    double t_prepare = 0.0, t_collect = 0.0, t_enqueue = 0.0, t_scatter = 0.0;
    auto since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    amc_match_opts o;
    if (opts_in) o = *opts_in; else amc_match_opts_default(&o);
    if (o.kernel != AMC_KERNEL_AUTO && o.kernel != AMC_KERNEL_MFMA && o.kernel != AMC_KERNEL_DOT4)
        return api_fail(AMC_E_INVALID, "amc_match_pairs: unknown kernel %d", o.kernel);
    uint64_t rows_total = 0;  // rows of image 1 (padded) over the call: what is left when a batch is carved
    for (size_t i = 0; i < npairs; ++i) {
        if (slot1[i] >= c->slots.size() || slot2[i] >= c->slots.size())
            return api_fail(AMC_E_INVALID, "amc_match_pairs: pair %zu references slot out of range", i);
        if (!c->slots[slot1[i]].valid || !c->slots[slot2[i]].valid)
            return api_fail(AMC_E_STATE, "amc_match_pairs: pair %zu references a slot with no "
                            "descriptors uploaded", i);
        rows_total += c->slots[slot1[i]].dev.rows_pad;  // (one pass over the pair list: a loop-closure call has 10^7 pairs)
    }
    std::vector<GuidedDev> h_guided;
    if (geoms) {
        h_guided.resize(npairs);
        for (size_t i = 0; i < npairs; ++i) {
            const int cfg = geoms[i].config;
            GuidedDev& g = h_guided[i];
            g.kind = (cfg == AMC_TVG_CALIBRATED || cfg == AMC_TVG_UNCALIBRATED) ? kGuidedF
                     : (cfg == AMC_TVG_PLANAR || cfg == AMC_TVG_PANORAMIC || cfg == AMC_TVG_PLANAR_OR_PANORAMIC)
                         ? kGuidedH : kGuidedNone;
            if (g.kind == kGuidedNone)
                return api_fail(AMC_E_INVALID, "amc_match_guided_pairs: pair %zu: configuration %d has no guided "
                                "matching (COLMAP keeps the inlier matches it has)", i, cfg);
            const double* m = g.kind == kGuidedF ? geoms[i].F : geoms[i].H;
            for (int k = 0; k < 9; ++k) g.m[k] = (float)m[k];
            g.max_residual = (float)(max_error * max_error);
            const Slot& a = c->slots[slot1[i]];
            const Slot& b = c->slots[slot2[i]];
            if (!a.kp || !b.kp || a.kp_rows < a.dev.rows || b.kp_rows < b.dev.rows)
                return api_fail(AMC_E_STATE, "amc_match_guided_pairs: pair %zu: float32 keypoints (one per descriptor) "
                                "must be uploaded for both images", i);
            guided_grid_setup(g, a.grid, b.grid, guided_dense_only);
        }
    }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;

    if (c->table_dirty) {
        HIPCHK(c->d_imgs.ensure(c->slots.size()));
        std::vector<ImageDev> t(c->slots.size());
        for (size_t i = 0; i < t.size(); ++i) t[i] = c->slots[i].dev;
        if (!t.empty())
            HIPCHK(hipMemcpy(c->d_imgs.p, t.data(), t.size() * sizeof(ImageDev),
                             hipMemcpyHostToDevice));
        HIPCHK(c->d_grids.ensure(c->slots.size()));
        std::vector<GridDev> gt(c->slots.size());
        for (size_t i = 0; i < gt.size(); ++i) gt[i] = c->slots[i].grid;
        if (!gt.empty())
            HIPCHK(hipMemcpy(c->d_grids.p, gt.data(), gt.size() * sizeof(GridDev), hipMemcpyHostToDevice));
        c->table_dirty = false;
    }

    const float max_ratio_f = (float)o.max_ratio;
    FinalizeParams fp;
    fp.max_ratio = max_ratio_f;
    fp.max_distance = (float)o.max_distance;
    fp.cross_check = o.cross_check ? 1 : 0;
    fp.reserved = 0;

    // the scan's accept thresholds for these options: built (and proven against the acos table) once per option pair
    if (!c->accept_valid || std::memcmp(&c->accept_ratio, &fp.max_ratio, sizeof(float)) != 0 ||
        std::memcmp(&c->accept_distance, &fp.max_distance, sizeof(float)) != 0) {
        c->h_accept = build_scan_accept(c->h_lut.data(), (uint32_t)c->h_lut.size(), fp.max_ratio, fp.max_distance);
        if (accept_trivial) c->h_accept.trivial = 1;
        if (!c->d_accept) HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->d_accept), sizeof(ScanAccept)));
        HIPCHK(hipStreamSynchronize(st));  // a previous call's kernels may still read the old thresholds
        HIPCHK(hipMemcpy(c->d_accept, &c->h_accept, sizeof(ScanAccept), hipMemcpyHostToDevice));
        c->accept_ratio = fp.max_ratio;
        c->accept_distance = fp.max_distance;
        c->accept_valid = true;
    }
    HIPCHK(hipEventRecord(c->ev[0], st));
    // (everything above returns through HIPCHK: from here on errors go through rc / hc, which give the result's
    // pinned lease back)
    ResultPriv* priv = new (std::nothrow) ResultPriv();
    if (!priv) return api_fail(AMC_E_NOMEM, "amc_match_pairs: out of host memory");
    priv->offsets.assign(npairs + 1, 0);
    priv->pool = c->result_pool;
    priv->matches = c->result_pool->acquire();
    size_t keep_used = 0;  // matches of this call in c->d_keep so far (pair order: the result's CSR layout)
    c->resident_matches = 0;
    c->vres = amc::VerifyResident{};  // (a resident verification result indexes the table this call rewrites)
    if (keep_off) keep_off->assign(npairs, 0);

    const size_t mfma_max_cols = kSelectMaxCols;  // cross-check candidate bitmap (image 2 rows)

    uint64_t num_dist = 0, n_mfma = 0, n_dot4 = 0, n_grid = 0;
    double kernel_ms = 0.0, cross_ms = 0.0;
    uint32_t kernel_launches = 0, scan_run_max = 0;
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
    const size_t scan_workgroups = 2 * (size_t)cus;  // (match_mfma.hip: two workgroups share a CU)

    int rc = AMC_OK;
    auto hc = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == AMC_OK)
            rc = api_fail(AMC_E_HIP, "amc_match_pairs: %s: %s", what, hipGetErrorString(e));
        return e == hipSuccess;
    };
    const size_t max_entries = batch_entries ? batch_entries : kMaxTop2Entries;

    // A batch goes through four steps.  Steps of consecutive batches are interleaved so that the device
    // never waits for the host between them:
    //   prepare(k+1)   host only: route pairs to kernels, queue orders, staging set (k+1)&1   } while the device
    //   collect(k)     wait for batch k's counters, enqueue the copy of its matches            } runs batch k
    //   enqueue(k+1)   H2D + all kernels + the counters' D2H, behind that copy in stream order
    //   scatter(k)     wait for the matches, append them to the result                         (device runs k+1)
    struct Batch {
        size_t begin = 0, end = 0, nb = 0, top_rows = 0, top_cols = 0, cap = 0;
        size_t row_off = 0, nwork = 0, nord = 0, nwork_grid = 0;
        uint32_t max_cols = 0;  // largest image 2 among the batch's mfma pairs (select_candidates' bitmap)
        size_t ngrp = 0, ngrp2 = 0, seg_cap = 0;  // mfma: groups of the two queue orders, descriptors to provide for
        int set = 0;
        uint32_t total = 0;
        bool grouped_resolve = true;
        int run = 1;  // forward scan: consecutive streamed images that share resident X segments (scan_run.h)
    };
    // rows of image 1 (padded) from pair i to the end of the call: how much is left when a batch is carved
    // (a running total, not an array: a loop-closure call has 10^7 pairs, and 80 MB of suffix sums cost more than the
    // tail they shape)
    uint64_t rows_carved = 0, rows_collected = 0;
    // How a batch's matches reach the host.  The copy of batch k is handed to batch k + 1's forward scan, whose first
    // few workgroups carry it out (CopyJob, match_mfma.hip); the last batch's copy, and any the next launch cannot
    // take, goes to the copy stream as a small-grid kernel (launch_host_copy).  AMC_D2H=memcpy: hipMemcpyAsync for
    // all of them (A/B: its copy kernel takes every CU while PCIe moves the data, and the next scan waits);
    // AMC_D2H=stream: never fused.
    const int d2h_mode = !d2h_env ? 0 : (std::strcmp(d2h_env, "memcpy") == 0 ? 2 : (std::strcmp(d2h_env, "stream") == 0 ? 1 : 0));
    struct PendingCopy {
        void* dst = nullptr;
        const void* src = nullptr;
        size_t bytes = 0;
        int set = -1;  // the batch set whose bev[set][4] marks the copy done; -1: nothing pending
    } pending;
    constexpr uint32_t kCopyParts = 64 / kSegsPerItem;  // 64 waves copy, whatever a scan workgroup holds
    auto sync_batch_streams = [&](const char* what) { return hc(hipStreamSynchronize(st), what); };
    const bool hook_split = batch_hook && hook_split_mode != 0;
    const size_t hook_split_min_pairs = hook_split_mode == 2 ? 2 : 4096;
    auto carve = [&](size_t begin, int set) {
        Batch b;
        b.begin = b.end = begin;
        b.set = set;
        // The copy of a batch's matches to the host runs beside the NEXT batch's kernels; the last batch's copy has
        // nothing to hide behind.  So a call of several batches ends on a small one: when what is left would be the
        // last batch and is more than a quarter of a full one, this batch stops a quarter short of the end (on the
        // dense 500 x 4096 set the exposed copy is 530 MB otherwise).
        size_t limit = max_entries;
        const uint64_t rows_left = rows_total - rows_carved;  // (carve() is called for consecutive batches, in order)
        if (begin > 0 && rows_left <= max_entries && rows_left > max_entries / 4)
            limit = (size_t)(rows_left - max_entries / 4);
        // amc_match_verify_pairs hands a batch's pairs to the verification's host side (checks, trial tables, class lists:
        // 3 - 25 ms for 33 k pairs) when the batch's counts are on the host - beside the NEXT batch's scan.  A call that
        // fits one batch has no next scan to hide that behind: it is cut in two (AMC_HOOK_SPLIT=0: A/B hook).
        if (begin == 0 && hook_split && rows_total <= max_entries && npairs >= hook_split_min_pairs)
            limit = (size_t)(rows_total * 6 / 10);
        while (b.end < npairs) {
            const Slot& x = c->slots[slot1[b.end]];
            const Slot& y = c->slots[slot2[b.end]];
            const size_t nr = x.dev.rows_pad, nc = y.dev.rows_pad;
            // cross-checked matches are one-to-one; without the cross check every row of image 1
            // may match (several rows may share a column)
            const size_t mc = o.cross_check ? std::min(x.dev.rows, y.dev.rows) : x.dev.rows;
            if (b.end > b.begin && (b.top_rows + nr > limit || b.top_cols + nc > max_entries ||
                                    b.cap + mc > kMaxMatchCap || b.end - b.begin >= (1u << 24)))
                break;
            b.top_rows += nr; b.top_cols += nc; b.cap += mc; ++b.end;
        }
        b.nb = b.end - b.begin;
        rows_carved += b.top_rows;
        return b;
    };
    // host side of a batch: which kernel takes each pair, the work queues (mfma: one item per pair, in
    // an order that keeps co-resident workgroups on the same streamed image; dot4: one item per 64 rows)
    // The reverse scan's queue order, (image 1, image 2), and its group cuts.  Nothing needs them before the batch's
    // forward scan is enqueued: the call's first batch builds them behind enqueue_scan, beside the scan, instead of
    // with the device idle (every later batch is prepared beside the scan before it anyway).
    auto build_reverse_order = [&](Batch& b) {
        const int k = b.set;
        const size_t nord = b.nord;
        if (!nord || !o.cross_check) return;
        const PairDev* hp = c->h_pairs[k].p;
        const size_t nslots = c->slots.size();
        std::vector<uint32_t> cnt(nslots + 1), tmp(nord);
        auto by_slot = [&](const uint32_t* src, uint32_t* dst, bool key_is_slot2) {
            std::fill(cnt.begin(), cnt.end(), 0u);
            for (size_t q = 0; q < nord; ++q) ++cnt[(key_is_slot2 ? hp[src[q]].slot2 : hp[src[q]].slot1) + 1];
            for (size_t v = 0; v < nslots; ++v) cnt[v + 1] += cnt[v];
            for (size_t q = 0; q < nord; ++q) dst[cnt[key_is_slot2 ? hp[src[q]].slot2 : hp[src[q]].slot1]++] = src[q];
        };
        uint32_t* ord2 = c->h_order2[k].p;
        by_slot(c->h_order[k].p, tmp.data(), true);  // minor key: image 2
        by_slot(tmp.data(), ord2, false);            // major key: image 1 (stable)
        size_t ngrp2 = 0;
        for (size_t q = 0; q < nord; ++q)
            if (q == 0 || hp[ord2[q]].slot1 != hp[ord2[q - 1]].slot1) c->h_grp2[k].p[ngrp2++] = (uint32_t)q;
        c->h_grp2[k].p[ngrp2] = (uint32_t)nord;  // (ngrp2 == b.ngrp2: prepare() counted the distinct images 1)
    };
    auto prepare = [&](Batch& b, bool defer_reverse) {
        const int k = b.set;
        const size_t nb = b.nb, begin = b.begin;
        if (!hc(c->h_pairs[k].ensure(nb), "pinned pairs") || !hc(c->h_order[k].ensure(nb), "pinned order") ||
            !hc(c->h_order2[k].ensure(nb), "pinned order2") || !hc(c->h_pair_off[k].ensure(nb), "pinned pair_off") ||
            !hc(c->h_pair_cnt[k].ensure(nb), "pinned pair_cnt") || !hc(c->h_bscalars[k].ensure(16), "pinned scalars"))
            return false;
        // mfma: exact for any u8 values and sizes; the lazy cross check's candidate bitmap
        // (select_candidates_kernel) holds kSelectMaxCols = 1 Mi image-2 rows, larger images take the dot4 path.
        std::vector<uint8_t> want_mfma(nb, 0);
        for (size_t i = 0; i < nb; ++i) {
            const Slot& x = c->slots[slot1[begin + i]];
            const Slot& y = c->slots[slot2[begin + i]];
            const bool nonempty = x.dev.rows > 0 && y.dev.rows > 0;
            want_mfma[i] = nonempty && o.kernel != AMC_KERNEL_DOT4 && !geoms &&
                           (!o.cross_check || y.dev.rows_pad <= mfma_max_cols);
        }
        PairDev* hp = c->h_pairs[k].p;
        size_t row_off = 0, col_off = 0, nwork = 0, nord = 0, nimg1 = 0;
        std::vector<uint8_t> seen1(c->slots.size(), 0);  // images 1 of the mfma pairs: the reverse order's groups
        b.grouped_resolve = !resolve_ungrouped;
        for (size_t i = 0; i < nb; ++i) {
            const Slot& x = c->slots[slot1[begin + i]];
            const Slot& y = c->slots[slot2[begin + i]];
            const bool nonempty = x.dev.rows > 0 && y.dev.rows > 0;
            if (o.kernel == AMC_KERNEL_MFMA && nonempty && !want_mfma[i]) {
                rc = api_fail(AMC_E_INVALID,
                              "amc_match_pairs: kernel=MFMA forced but pair %zu is not eligible "
                              "(rows_pad=%u, cols_pad=%u > %zu)", begin + i, x.dev.rows_pad,
                              y.dev.rows_pad, mfma_max_cols);
                return false;
            }
            PairDev& pd = hp[i];
            pd.slot1 = slot1[begin + i];
            pd.slot2 = slot2[begin + i];
            pd.mode = want_mfma[i] ? 1u : 0u;
            pd.pad = 0;
            pd.row_off = row_off;
            pd.col_off = col_off;
            row_off += x.dev.rows_pad;
            col_off += y.dev.rows_pad;
            num_dist += (uint64_t)x.dev.rows * y.dev.rows;
            if (!nonempty) continue;
            if (want_mfma[i]) {
                c->h_order[k].p[nord++] = (uint32_t)i;
                if (!seen1[pd.slot1]) { seen1[pd.slot1] = 1; ++nimg1; }
                ++n_mfma;
                b.max_cols = std::max(b.max_cols, y.dev.rows);
                // the tile-grouped resolve needs both images' tiles to fit its LDS histogram
                if (std::max(x.dev.rows_pad, y.dev.rows_pad) > resolve_grouped_max_rows()) b.grouped_resolve = false;
            } else {
                nwork += (x.dev.rows + 63) / 64;
                if (o.cross_check) nwork += (y.dev.rows + 63) / 64;
                if (geoms && h_guided[begin + i].grid_ok) ++n_grid; else ++n_dot4;
            }
        }
        // mfma queue orders: by (image 2, image 1) for the forward scan - co-resident workgroups stream the same Y - and
        // by (image 1, image 2) for the reverse scan.  Two stable counting sorts each (least significant key first):
        // O(pairs + slots) instead of a comparison sort through the pair array (this runs unhidden for the call's
        // first batch: 2.8 ms of a 180 ms call with std::stable_sort).
        if (nord) {
            const size_t nslots = c->slots.size();
            std::vector<uint32_t> cnt(nslots + 1), tmp(nord);
            auto by_slot = [&](const uint32_t* src, uint32_t* dst, bool key_is_slot2) {
                std::fill(cnt.begin(), cnt.end(), 0u);
                for (size_t q = 0; q < nord; ++q) ++cnt[(key_is_slot2 ? hp[src[q]].slot2 : hp[src[q]].slot1) + 1];
                for (size_t v = 0; v < nslots; ++v) cnt[v + 1] += cnt[v];
                for (size_t q = 0; q < nord; ++q) dst[cnt[key_is_slot2 ? hp[src[q]].slot2 : hp[src[q]].slot1]++] = src[q];
            };
            uint32_t* ord = c->h_order[k].p;
            by_slot(ord, tmp.data(), false);   // minor key: image 1
            by_slot(tmp.data(), ord, true);    // major key: image 2 (stable)
        }
        // Cut both orders where the streamed image changes (the packing kernels fill whole items per image),
        // and bound the number of segment descriptors: ceil(rows / 128) per pair plus up to one item of padding
        // per group.  The reverse scan's X side is the candidate list, at most every row of image 2.
        b.ngrp = b.ngrp2 = 0;
        b.seg_cap = 0;
        if (nord) {
            if (!hc(c->h_grp[k].ensure(nord + 1), "pinned group cuts") ||
                (o.cross_check && !hc(c->h_grp2[k].ensure(nord + 1), "pinned group cuts")))
                return false;
            size_t seg1 = 0, seg2 = 0;
            for (size_t q = 0; q < nord; ++q) {
                const PairDev& pq = hp[c->h_order[k].p[q]];
                if (q == 0 || pq.slot2 != hp[c->h_order[k].p[q - 1]].slot2) c->h_grp[k].p[b.ngrp++] = (uint32_t)q;
                seg1 += (c->slots[pq.slot1].dev.rows + kSegRows - 1) / kSegRows;
                seg2 += (c->slots[pq.slot2].dev.rows + kSegRows - 1) / kSegRows;
            }
            c->h_grp[k].p[b.ngrp] = (uint32_t)nord;
            if (o.cross_check) b.ngrp2 = nimg1;  // (the cuts themselves: build_reverse_order)
            b.seg_cap = std::max(seg1 + kSegsPerItem * b.ngrp, o.cross_check ? seg2 + kSegsPerItem * b.ngrp2 : 0);
            const uint32_t* ord = c->h_order[k].p;
            b.run = choose_scan_run_by([hp, ord](size_t q) { return hp[ord[q]].slot1; }, c->h_grp[k].p, b.ngrp,
                                       seg1 / kSegsPerItem, scan_workgroups, scan_run_env);
            scan_run_max = std::max(scan_run_max, (uint32_t)b.run);
        }
        b.nwork_grid = 0;
        if (nwork) {
            if (!hc(c->h_work[k].ensure(nwork), "pinned work")) return false;
            size_t w = 0;
            // guided pairs the candidate-generation kernel takes come first: one launch per kernel over its part
            for (int pass = geoms ? 0 : 1; pass < 2; ++pass) {
                for (size_t i = 0; i < nb; ++i) {
                    if (hp[i].mode) continue;
                    if (geoms && (h_guided[begin + i].grid_ok != 0) != (pass == 0)) continue;
                    const Slot& x = c->slots[slot1[begin + i]];
                    const Slot& y = c->slots[slot2[begin + i]];
                    if (x.dev.rows == 0 || y.dev.rows == 0) continue;
                    for (uint32_t rb = 0; rb < (x.dev.rows + 63) / 64; ++rb)
                        c->h_work[k].p[w++] = Dot4Work{(uint32_t)i, 0u, rb};
                    if (o.cross_check)
                        for (uint32_t rb = 0; rb < (y.dev.rows + 63) / 64; ++rb)
                            c->h_work[k].p[w++] = Dot4Work{(uint32_t)i, 1u, rb};
                }
                if (pass == 0) b.nwork_grid = w;
            }
        }
        b.row_off = row_off;
        b.nwork = nwork;
        b.nord = nord;
        if (!defer_reverse) build_reverse_order(b);
        return true;
    };
    // device side of a batch, first part, on the stream: H2D of the queues, segment packing, the scans
    auto enqueue_scan = [&](Batch& b) {
        const int k = b.set;
        amc_ctx::MatchScratch& S = c->ms;
        const size_t nb = b.nb, nord = b.nord, nwork = b.nwork;
        // the run table (match_mfma.hip, "Runs"): a run per block of b.run groups and item position, at most as many
        // runs as the launch has items (a block's runs are the items of its longest group), b.run entries each
        const size_t run_blocks = b.run > 1 ? (b.ngrp + b.run - 1) / b.run : 0;
        const size_t run_entries = b.run > 1 ? (b.seg_cap / kSegsPerItem + 1) * b.run : 0;
        // device scratch only ever grows; growing frees the old allocation, so drain the stream first
        const bool grow = S.d_pairs.cap < nb || S.d_order.cap < nb || S.d_order2.cap < nb ||
                          S.d_rowbuf.cap < b.top_rows || S.d_colbuf.cap < b.top_cols ||
                          S.d_accmask.cap < b.top_rows / 32 + 8 || S.d_pair_off.cap < nb || S.d_pair_cnt.cap < nb ||
                          S.d_matches.cap < 2 * b.cap || S.d_cand_cnt.cap < nb || S.d_candbuf.cap < b.top_cols ||
                          S.d_live.cap < nb || S.d_live_fwd.cap < nb || S.d_live_all.cap < nb || S.d_live_rev.cap < nb ||
                          S.d_live_scan.cap < live_scratch_words(nb) ||
                          S.d_work.cap < nwork || (geoms && S.d_guided.cap < nb) || S.d_segs.cap < b.seg_cap ||
                          S.d_seg_base.cap < nord || S.d_grp.cap < b.ngrp + 1 || S.d_grp2.cap < b.ngrp2 + 1 ||
                          S.d_grp_segs.cap < std::max(b.ngrp, b.ngrp2) || S.d_grp_item_base.cap < std::max(b.ngrp, b.ngrp2) ||
                          S.d_run_base.cap < run_blocks || S.d_run_items.cap < run_entries;
        if (grow && !sync_batch_streams("sync before growing device scratch")) return false;
        if (!hc(S.d_pairs.ensure(nb), "dev pairs") || !hc(S.d_order.ensure(nb), "dev order") ||
            !hc(S.d_order2.ensure(nb), "dev order2") ||
            !hc(S.d_rowbuf.ensure(b.top_rows), "row top2") || !hc(S.d_colbuf.ensure(b.top_cols), "col top2") ||
            !hc(S.d_accmask.ensure(b.top_rows / 32 + 8), "accept mask") ||
            !hc(S.d_pair_off.ensure(nb), "pair_off") || !hc(S.d_pair_cnt.ensure(nb), "pair_cnt") ||
            !hc(S.d_matches.ensure(2 * b.cap), "dev matches") ||
            !hc(S.d_cand_cnt.ensure(nb), "cand_cnt") || !hc(S.d_candbuf.ensure(b.top_cols), "candbuf") ||
            !hc(S.d_live.ensure(nb), "live flags") || !hc(S.d_live_fwd.ensure(nb), "live list (forward)") ||
            !hc(S.d_live_all.ensure(nb), "live list") || !hc(S.d_live_rev.ensure(nb), "live list (reverse)") ||
            !hc(S.d_live_scan.ensure(live_scratch_words(nb)), "live list scratch") ||
            (nwork && !hc(S.d_work.ensure(nwork), "dev work")) || (geoms && !hc(S.d_guided.ensure(nb), "dev guided")) ||
            !hc(S.d_segs.ensure(b.seg_cap), "segment descriptors") || !hc(S.d_seg_base.ensure(nord), "segment bases") ||
            !hc(S.d_grp.ensure(b.ngrp + 1), "group cuts") || !hc(S.d_grp2.ensure(b.ngrp2 + 1), "group cuts") ||
            !hc(S.d_grp_segs.ensure(std::max(b.ngrp, b.ngrp2)), "group segments") ||
            !hc(S.d_grp_item_base.ensure(std::max(b.ngrp, b.ngrp2)), "group items") ||
            !hc(S.d_run_base.ensure(run_blocks), "run bases") || !hc(S.d_run_items.ensure(run_entries), "run table"))
            return false;
        bool okq = hc(hipMemcpyAsync(S.d_pairs.p, c->h_pairs[k].p, nb * sizeof(PairDev),
                                     hipMemcpyHostToDevice, st), "H2D pairs") &&
                   hc(memset_async(c->d_scalars, 0, 2 * sizeof(uint32_t), st), "memset cursor") &&
                   hc(memset_async(c->d_scalars + 3, 0, sizeof(uint32_t), st), "memset errcount");
        if (okq && nord)
            okq = hc(hipMemcpyAsync(S.d_order.p, c->h_order[k].p, nord * sizeof(uint32_t),
                                    hipMemcpyHostToDevice, st), "H2D order") &&
                  hc(hipMemcpyAsync(S.d_grp.p, c->h_grp[k].p, (b.ngrp + 1) * sizeof(uint32_t),
                                    hipMemcpyHostToDevice, st), "H2D group cuts") &&
                  // segments no wave owns (beyond an image's last row) never write their words
                  hc(memset_async(S.d_accmask.p, 0, (b.row_off / 32 + 8) * sizeof(uint32_t), st), "memset accmask");
        if (okq && nwork)
            okq = hc(hipMemcpyAsync(S.d_work.p, c->h_work[k].p, nwork * sizeof(Dot4Work),
                                    hipMemcpyHostToDevice, st), "H2D work");
        if (okq && geoms)  // this batch's slice of the filter models (pageable source: the copy is staged)
            okq = hc(hipMemcpyAsync(S.d_guided.p, h_guided.data() + b.begin, nb * sizeof(GuidedDev),
                                    hipMemcpyHostToDevice, st), "H2D guided");
        if (!okq) return false;
        if (nord &&  // pack the pairs' 128-row segments into items (per streamed image) ...
            !hc(launch_build_segments(0, c->d_imgs.p, S.d_pairs.p, S.d_order.p, S.d_grp.p, (uint32_t)b.ngrp,
                                      S.d_cand_cnt.p, S.d_candbuf.p, S.d_rowbuf.p, S.d_seg_base.p, S.d_grp_segs.p,
                                      S.d_grp_item_base.p, S.d_segs.p, c->d_scalars + 5, st), "segment packing"))
            return false;
        if (nord && b.run > 1 &&  // ... line item t of b.run consecutive streamed images up behind each other ...
            !hc(launch_build_runs(S.d_segs.p, S.d_grp_segs.p, S.d_grp_item_base.p, (uint32_t)b.ngrp, (uint32_t)b.run,
                                  S.d_run_base.p, S.d_run_items.p, c->d_scalars + 6, st), "run packing"))
            return false;
        if (!hc(hipEventRecord(c->bev[k][0], st), "event record")) return false;
        if (nord) {  // ... and scan them (the events bracket the scan kernel alone: bench.py's roofline leg)
            CopyJob job;
            const uintptr_t ps = reinterpret_cast<uintptr_t>(pending.src), pd = reinterpret_cast<uintptr_t>(pending.dst);
            const bool take = pending.set >= 0 && d2h_mode == 0 && b.seg_cap > 0 && pending.bytes >= fuse_min_bytes &&
                              (ps & 15) == (pd & 15);
            int done_set = -1;
            if (take) {  // the previous batch's matches ride in this launch; head / tail bytes around the 16-byte units first
                const size_t head = (ps & 15) ? 16 - (ps & 15) : 0, n16 = (pending.bytes - head) / 16;
                const size_t tail = pending.bytes - head - n16 * 16;
                if (head && !hc(memcpy_async(pending.dst, pending.src, head, hipMemcpyDeviceToHost, st), "D2H matches (head)"))
                    return false;
                if (tail && !hc(memcpy_async(static_cast<char*>(pending.dst) + head + n16 * 16,
                                             static_cast<const char*>(pending.src) + head + n16 * 16, tail,
                                             hipMemcpyDeviceToHost, st), "D2H matches (tail)"))
                    return false;
                job.src = static_cast<const char*>(pending.src) + head;
                job.dst = static_cast<char*>(pending.dst) + head;
                job.n16 = n16;
                job.parts = kCopyParts;
                done_set = pending.set;
                pending.set = -1;
            }
            if (!hc(launch_match_mfma(0, S.d_segs.p, c->d_scalars + 5, (uint32_t)std::min<size_t>(b.seg_cap, 0xFFFFFFFFu),
                                      c->d_scalars + 1, S.d_accmask.p, c->d_accept, st, job, c->d_scalars + 7,
                                      b.run > 1 ? S.d_run_items.p : nullptr, (uint32_t)b.run, c->d_scalars + 6), "forward scan"))
                return false;
            // that batch's matches are on the host when this scan is done
            if (done_set >= 0 && !hc(hipEventRecord(c->bev[done_set][4], st), "event record")) return false;
        }
        if (b.nwork_grid &&
            !hc(launch_match_guided_grid(c->d_imgs.p, c->d_grids.p, S.d_pairs.p, S.d_work.p, (uint32_t)b.nwork_grid,
                                         S.d_rowbuf.p, S.d_colbuf.p, S.d_guided.p, st), "guided scan"))
            return false;
        if (nwork > b.nwork_grid &&
            !hc(launch_match_dot4(c->d_imgs.p, S.d_pairs.p, S.d_work.p + b.nwork_grid, (uint32_t)(nwork - b.nwork_grid),
                                  S.d_rowbuf.p, S.d_colbuf.p, geoms ? S.d_guided.p : nullptr, st), "dot4 scan"))
            return false;
        kernel_launches += (nord ? 1 : 0) + (b.nwork_grid ? 1 : 0) + (nwork > b.nwork_grid ? 1 : 0);
        return hc(hipEventRecord(c->bev[k][1], st), "event record");
    };
    // second part, behind the scans: the live pairs, tile -> index, lazy cross check, finalize, D2H of the counters.
    // Every per-pair kernel of the chain visits a live list (amc_internal.h, launch_live_pairs): d_scalars[8] pairs of
    // d_live_fwd, [9] of d_live_all, [10] of d_live_rev.
    auto enqueue_chain = [&](Batch& b) {
        const int k = b.set;
        amc_ctx::MatchScratch& S = c->ms;
        const size_t nb = b.nb, nord = b.nord;
        uint32_t* const nlive = c->d_scalars + 8;
        if (!hc(launch_live_pairs(c->d_imgs.p, S.d_pairs.p, (uint32_t)nb, S.d_accmask.p, S.d_order.p, (uint32_t)nord,
                                  S.d_live.p, S.d_live_fwd.p, S.d_live_all.p, nlive, S.d_cand_cnt.p, S.d_pair_cnt.p,
                                  S.d_pair_off.p, S.d_live_scan.p, st), "live pairs"))
            return false;
        if (nord &&  // tile -> exact index for the accepted rows
            !hc(launch_resolve_index(0, c->d_imgs.p, S.d_pairs.p, S.d_rowbuf.p, S.d_accmask.p, c->d_lut,
                                     fp, S.d_cand_cnt.p, S.d_candbuf.p, c->d_scalars + 3, b.grouped_resolve,
                                     S.d_live_fwd.p, nlive, (uint32_t)nord, st), "resolve (rows)"))
            return false;
        if (nord && o.cross_check) {
            // lazy cross check: reverse scan only for the columns accepted rows point at
            if (!hc(launch_select_candidates(c->d_imgs.p, S.d_pairs.p, (uint32_t)nb, b.max_cols, S.d_rowbuf.p,
                                             S.d_accmask.p, c->d_lut, fp, S.d_cand_cnt.p, S.d_candbuf.p,
                                             S.d_live_all.p, nlive + 1, st),
                    "candidate selection"))
                return false;
            if (!hc(hipMemcpyAsync(S.d_order2.p, c->h_order2[k].p, nord * sizeof(uint32_t),
                                   hipMemcpyHostToDevice, st), "H2D order2") ||
                !hc(hipMemcpyAsync(S.d_grp2.p, c->h_grp2[k].p, (b.ngrp2 + 1) * sizeof(uint32_t),
                                   hipMemcpyHostToDevice, st), "H2D group cuts"))
                return false;
            // the candidate counts exist only on the device: the packing kernels read them there, and the reverse
            // resolve visits the pairs that have any
            if (!hc(launch_compact_order(S.d_order2.p, (uint32_t)nord, (uint32_t)nb, S.d_cand_cnt.p, S.d_live_rev.p, nlive + 2,
                                         S.d_live_scan.p, st),
                    "live pairs (reverse)") ||
                !hc(launch_build_segments(1, c->d_imgs.p, S.d_pairs.p, S.d_order2.p, S.d_grp2.p, (uint32_t)b.ngrp2,
                                          S.d_cand_cnt.p, S.d_candbuf.p, S.d_colbuf.p, S.d_seg_base.p, S.d_grp_segs.p,
                                          S.d_grp_item_base.p, S.d_segs.p, c->d_scalars + 5, st), "segment packing (reverse)") ||
                !hc(launch_match_mfma(1, S.d_segs.p, c->d_scalars + 5, (uint32_t)std::min<size_t>(b.seg_cap, 0xFFFFFFFFu),
                                      c->d_scalars + 1, S.d_accmask.p, c->d_accept, st), "reverse scan") ||
                !hc(launch_resolve_index(1, c->d_imgs.p, S.d_pairs.p, S.d_colbuf.p, S.d_accmask.p, c->d_lut,
                                         fp, S.d_cand_cnt.p, S.d_candbuf.p, c->d_scalars + 3, b.grouped_resolve,
                                         S.d_live_rev.p, nlive + 2, (uint32_t)nord, st), "resolve (columns)"))
                return false;
        }
        if (!hc(hipEventRecord(c->bev[k][2], st), "event record") ||
            !hc(launch_finalize(c->d_imgs.p, S.d_pairs.p, (uint32_t)nb, S.d_live_all.p, nlive + 1, S.d_rowbuf.p, S.d_colbuf.p,
                                S.d_accmask.p, c->d_lut, fp, c->d_scalars, (uint32_t)std::min(b.cap, (size_t)0xFFFFFFFFu),
                                S.d_pair_off.p, S.d_pair_cnt.p, S.d_matches.p, st), "finalize"))
            return false;
        return hc(hipMemcpyAsync(c->h_bscalars[k].p, c->d_scalars, 4 * sizeof(uint32_t),
                                 hipMemcpyDeviceToHost, st), "D2H cursor") &&
               hc(hipMemcpyAsync(c->h_pair_off[k].p, S.d_pair_off.p, nb * sizeof(uint32_t),
                                 hipMemcpyDeviceToHost, st), "D2H pair_off") &&
               hc(hipMemcpyAsync(c->h_pair_cnt[k].p, S.d_pair_cnt.p, nb * sizeof(uint32_t),
                                 hipMemcpyDeviceToHost, st), "D2H pair_cnt") &&
               hc(hipEventRecord(c->bev[k][3], st), "event record");
    };
    // the batch's counters are on the host: check them, enqueue the copy of exactly `total` matches
    auto collect = [&](Batch& b) {
        const int k = b.set;
        amc_ctx::MatchScratch& S = c->ms;
        if (!hc(hipEventSynchronize(c->bev[k][3]), "wait for the batch")) return false;
        b.total = c->h_bscalars[k].p[0];
        if (c->h_bscalars[k].p[3] != 0) {
            rc = api_fail(AMC_E_HIP, "amc_match_pairs: internal: %u accepted rows could not be resolved "
                          "to an index (scan/recompute mismatch)", c->h_bscalars[k].p[3]);
            return false;
        }
        if (b.total > b.cap) {
            rc = api_fail(AMC_E_HIP, "amc_match_pairs: internal: %u matches exceed capacity %zu", b.total, b.cap);
            return false;
        }
        // The batch's matches lie in d_matches in the order the workgroups claimed space (atomic cursor).  Put them
        // in pair order behind the batches before it in d_keep - the CSR layout of the result - and copy that
        // straight into the result's pinned buffer: no per-pair scatter on the host, and amc_match_verify_pairs
        // reads the same table.
        if (!hc(c->h_csr[k].ensure(b.nb), "pinned csr")) return false;
        uint64_t run = keep_used;
        for (size_t i = 0; i < b.nb; ++i) {
            c->h_csr[k].p[i] = run;
            if (keep_off) (*keep_off)[b.begin + i] = run;
            run += c->h_pair_cnt[k].p[i];
            priv->offsets[b.begin + i + 1] = run;  // the result's CSR (offsets[0] = 0; batches are collected in order)
        }
        if (run - keep_used != b.total) {
            rc = api_fail(AMC_E_HIP, "amc_match_pairs: internal: pair counts (%llu) disagree with the cursor (%u)",
                          (unsigned long long)(run - keep_used), b.total);
            return false;
        }
        rows_collected += b.top_rows;
        if (b.total) {
            const auto tgrow = std::chrono::steady_clock::now();
            const size_t need = 2 * (keep_used + (size_t)b.total);
            // what the whole call will need if the batches to come match like the ones so far (+ 10 %): a table that has to
            // grow is sized for that at once - three batches otherwise pin (and copy) 2.4 times the final result
            // (at most four times what is needed now, and what is needed now if the larger request fails)
            size_t want = need;
            if (rows_collected > 0 && rows_collected < rows_total) {
                const double est = std::min((double)need * ((double)rows_total / (double)rows_collected) * 1.1, 4.0 * (double)need);
                want = std::max(need, (size_t)est / 2 * 2);
            }
            if (need > c->d_keep.cap) {
                DevBuf<uint32_t> bigger;
                if (bigger.ensure(std::max(want, 2 * c->d_keep.cap)) != hipSuccess) {
                    (void)hipGetLastError();
                    if (!hc(bigger.ensure(need), "resident match table")) return false;
                }
                if (keep_used &&
                    !hc(hipMemcpyAsync(bigger.p, c->d_keep.p, 2 * keep_used * sizeof(uint32_t), hipMemcpyDeviceToDevice, st),
                        "move resident match table"))
                    return false;
                if (!sync_batch_streams("sync before freeing the old resident table") ||
                    !hc(hipStreamSynchronize(c->copy_stream), "sync before freeing the old resident table"))
                    return false;
                c->d_keep = std::move(bigger);
            }
            if (need > priv->matches.cap) {  // grow the result buffer (first calls only: the pool keeps it)
                if (!sync_batch_streams("sync before growing the result buffer") ||
                    !hc(hipStreamSynchronize(c->copy_stream), "sync before growing the result buffer"))
                    return false;
                PinBuf<uint32_t> bigger;
                if (bigger.ensure(std::max(want, 2 * priv->matches.cap)) != hipSuccess) {
                    (void)hipGetLastError();
                    if (prof) std::fprintf(stderr, "[amc match profile] pinned result: %zu words refused, asking for %zu\n", want, need);
                    if (!hc(bigger.ensure(need), "pinned result")) return false;
                }
                if (keep_used) std::memcpy(bigger.p, priv->matches.p, 2 * keep_used * sizeof(uint32_t));
                priv->matches = std::move(bigger);
            }
            if (prof && since(tgrow) > 5.0)
                std::fprintf(stderr, "[amc match profile] batch of %zu pairs: %.1f ms growing the result tables to %zu words\n", b.nb,
                             since(tgrow), priv->matches.cap);
            if (!hc(c->d_csr.ensure(b.nb), "dev csr") ||
                !hc(hipMemcpyAsync(c->d_csr.p, c->h_csr[k].p, b.nb * sizeof(uint64_t), hipMemcpyHostToDevice, st), "H2D csr"))
                return false;
            // the copy to the host happens beside the next batch's kernels (which write d_matches and, later, d_keep
            // beyond this batch - never what is being copied): flush_copy() or the next enqueue() issues it
            if (!hc(launch_reorder_matches(S.d_pair_off.p, S.d_pair_cnt.p, c->d_csr.p, (uint32_t)b.nb, S.d_matches.p,
                                           c->d_keep.p, st), "reorder launch"))
                return false;
            pending.dst = priv->matches.p + 2 * keep_used;
            pending.src = c->d_keep.p + 2 * keep_used;
            pending.bytes = (size_t)b.total * 2 * sizeof(uint32_t);
            pending.set = k;
            keep_used += b.total;
            return true;
        }
        return hc(hipEventRecord(c->bev[k][4], st), "event record");
    };
    double t_hook = 0.0;
    auto run_hook = [&](const Batch& b) {
        if (!batch_hook) return true;
        const auto th = std::chrono::steady_clock::now();
        const int hrc = (*batch_hook)(b.begin, b.end, priv->offsets.data(), keep_off ? keep_off->data() : nullptr);
        t_hook += since(th);
        if (hrc != AMC_OK && rc == AMC_OK) rc = hrc;  // (the hook has set the message)
        return hrc == AMC_OK;
    };
    // the pending copy on the copy stream (the last batch's, or one the next launch does not take)
    auto flush_copy = [&]() {
        if (pending.set < 0) return true;
        const int k = pending.set;
        pending.set = -1;
        if (!hc(hipEventRecord(c->cev[k], st), "event record") || !hc(hipStreamWaitEvent(c->copy_stream, c->cev[k], 0), "stream wait"))
            return false;
        if (d2h_mode == 2) {
            if (!hc(hipMemcpyAsync(pending.dst, pending.src, pending.bytes, hipMemcpyDeviceToHost, c->copy_stream), "D2H matches"))
                return false;
        } else {
            if (!hc(launch_host_copy(pending.dst, pending.src, pending.bytes, c->copy_stream), "D2H matches")) return false;
        }
        return hc(hipEventRecord(c->bev[k][4], c->copy_stream), "event record");
    };
    // append the batch's matches to the result CSR (pairs keep the caller's order)
    auto scatter = [&](Batch& b) {
        const int k = b.set;
        if (!hc(hipEventSynchronize(c->bev[k][4]), "wait for the matches")) return false;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->bev[k][0], c->bev[k][1]) == hipSuccess) kernel_ms += ms;
        if (hipEventElapsedTime(&ms, c->bev[k][1], c->bev[k][2]) == hipSuccess) cross_ms += ms;
        return true;  // (the offsets were filled by collect(): this set's pinned counts may be gone by now)
    };

    if (npairs > 0) {
        Batch cur = carve(0, 0);
        auto tp = std::chrono::steady_clock::now();
        bool ok = prepare(cur, true);
        t_prepare += since(tp);
        tp = std::chrono::steady_clock::now();
        ok = ok && enqueue_scan(cur);
        if (ok) build_reverse_order(cur);  // (beside the scan)
        ok = ok && enqueue_chain(cur);
        t_enqueue += since(tp);
        // The host runs one batch ahead of the device: while batch `cur` is scanned, the next batch's lists are
        // prepared; the matches of the batch BEFORE cur are read out (scatter) only after that - their copy rides in
        // cur's scan and is done when that scan is, and waiting for it earlier would leave the device idle while the
        // host prepares (a 10^7-pair loop-closure call: 8 ms of preparation per batch against a 3 ms cross-check stage).
        Batch prev;
        bool have_prev = false;
        while (ok) {
            Batch next;
            const bool have_next = cur.end < npairs;
            if (have_next) {
                tp = std::chrono::steady_clock::now();
                next = carve(cur.end, cur.set ^ 1);
                ok = prepare(next, false);
                t_prepare += since(tp);
            }
            tp = std::chrono::steady_clock::now();
            if (ok && have_prev) ok = scatter(prev);  // (before enqueue(next) re-records that set's events)
            t_scatter += since(tp);
            tp = std::chrono::steady_clock::now();
            ok = ok && collect(cur);
            t_collect += since(tp);
            tp = std::chrono::steady_clock::now();
            if (ok && have_next) ok = enqueue_scan(next) && enqueue_chain(next);
            ok = ok && flush_copy();  // (not taken by a scan launch: the last batch's, a small one, dot4-only batches)
            t_enqueue += since(tp);
            ok = ok && run_hook(cur);  // (the device is busy with `next` - or, for the last batch, with the copy)
            if (!have_next) {
                tp = std::chrono::steady_clock::now();
                ok = ok && scatter(cur);
                t_scatter += since(tp);
                break;
            }
            prev = cur;
            have_prev = true;
            cur = next;
        }
        if (!ok && rc == AMC_OK) rc = api_fail(AMC_E_HIP, "amc_match_pairs: batch failed");
        if (rc != AMC_OK) {  // nothing of this call stays in flight
            (void)hipStreamSynchronize(st);
            (void)hipStreamSynchronize(c->copy_stream);
        }
    }
    // device_ms ends with the last result byte on the host: the stream joins the copy stream first
    if (rc == AMC_OK && npairs > 0 &&
        hc(hipEventRecord(c->cev[0], c->copy_stream), "event record"))
        hc(hipStreamWaitEvent(st, c->cev[0], 0), "stream wait");
    if (rc == AMC_OK && hc(hipEventRecord(c->ev[1], st), "event record")) hc(hipEventSynchronize(c->ev[1]), "wait for the call");
    if (rc != AMC_OK) {
        delete priv;
        return rc;
    }
    float total_ms = 0.f;
    (void)hipEventElapsedTime(&total_ms, c->ev[0], c->ev[1]);

    out->npairs = npairs;
    c->resident_matches = keep_used;
    out->offsets = priv->offsets.data();
    out->matches = priv->offsets[npairs] ? priv->matches.p : nullptr;
    out->num_distances = num_dist;
    out->pairs_mfma = n_mfma;
    out->pairs_dot4 = n_dot4;
    out->pairs_guided_grid = n_grid;
    out->device_ms = total_ms;
    out->match_kernel_ms = kernel_ms;
    out->match_kernel_launches = kernel_launches;
    out->scan_run = scan_run_max;
    out->cross_kernel_ms = cross_ms;
    out->_priv = priv;
    c->last_hook_ms = t_hook;
    if (prof)
        std::fprintf(stderr, "[amc match profile] pairs=%zu wall=%.1f ms: prepare %.1f, enqueue %.1f, collect(wait+reorder+D2H enqueue) %.1f, "
                     "scatter(wait) %.1f, batch hook %.1f; device events %.1f ms (scan %.1f, cross %.1f)\n", npairs, since(wall0), t_prepare,
                     t_enqueue, t_collect, t_scatter, t_hook, (double)total_ms, kernel_ms, cross_ms);
    return AMC_OK;
}

extern "C" {

int amc_match_pairs(amc_ctx* c, const uint32_t* slot1, const uint32_t* slot2, size_t npairs,
                    const amc_match_opts* opts_in, amc_match_result* out) {
    return match_impl(c, slot1, slot2, npairs, opts_in, nullptr, 0.0, out);
}

int amc_match_guided_pairs(amc_ctx* c, const uint32_t* slot1, const uint32_t* slot2, size_t npairs,
                           const amc_tvg* geoms, double max_error, const amc_match_opts* opts_in,
                           amc_match_result* out) {
    if (npairs > 0 && !geoms) {
        if (out) std::memset(out, 0, sizeof *out);
        return api_fail(AMC_E_INVALID, "amc_match_guided_pairs: NULL geometries");
    }
    if (!(max_error >= 0.0)) {
        if (out) std::memset(out, 0, sizeof *out);
        return api_fail(AMC_E_INVALID, "amc_match_guided_pairs: max_error must be >= 0");
    }
    static const amc_tvg kNone{};
    return match_impl(c, slot1, slot2, npairs, opts_in, npairs ? geoms : &kNone, max_error, out);
}

void amc_match_result_free(amc_match_result* r) {
    if (!r) return;
    delete static_cast<ResultPriv*>(r->_priv);
    std::memset(r, 0, sizeof *r);
}

}  // extern "C"
