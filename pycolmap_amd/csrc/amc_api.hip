// amc_api.hip — host side of libamc.so: implements include/amc.h on top of the HIP kernels.  This unit: errors, the
// context, slots and uploads, the camera entry points; matching is amc_match.hip, verification and pose amc_verify.hip.
// No CPU fallback: every entry point that computes needs a gfx950 device.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "amc_ctx.h"
#include "camera_math.h"

using namespace amc;

namespace {
thread_local std::string g_err;
}  // namespace

namespace amc {
int api_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
CtxView ctx_view(amc_ctx* c) {
    return CtxView{c->device, c->stream, c->resident_matches ? c->d_keep.p : nullptr, c->resident_matches};
}
VerifyResident verify_resident(amc_ctx* c) { return c->vres; }
}  // namespace amc

extern "C" {

const char* amc_last_error(void) { return g_err.c_str(); }
int amc_abi_version(void) { return AMC_ABI_VERSION; }

int amc_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        if (e == hipErrorNoDevice) return 0;
        return api_fail(AMC_E_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    return n;
}

void amc_match_opts_default(amc_match_opts* o) {
    if (!o) return;
    o->max_ratio = 0.8;     // SiftMatchingOptions defaults, SURVEY.md A.2
    o->max_distance = 0.7;
    o->cross_check = 1;
    o->kernel = AMC_KERNEL_AUTO;
}

int amc_ctx_create(int device_id, amc_ctx** out) {
    if (!out) return api_fail(AMC_E_INVALID, "amc_ctx_create: out is NULL");
    *out = nullptr;
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device_id < 0 || device_id >= n)
        return api_fail(AMC_E_INVALID, "amc_ctx_create: device %d out of range (%d devices)",
                        device_id, n);
    HIPCHK(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device_id));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return api_fail(AMC_E_HIP, "amc_ctx_create: device %d is %s; this library is gfx950-only",
                        device_id, prop.gcnArchName);
    amc_ctx* c = new (std::nothrow) amc_ctx();
    if (!c) return api_fail(AMC_E_NOMEM, "amc_ctx_create: out of host memory");
    c->device = device_id;
    hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return api_fail(AMC_E_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    c->stream = c->own_stream;
    e = hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        (void)hipStreamDestroy(c->own_stream);
        delete c;
        return api_fail(AMC_E_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    bool ev_ok = true;  // (an event that was never created would fail every later record: fail here instead)
    for (auto& ev : c->cev) ev_ok &= hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess;
    {
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);  // (0, 0 when it fails: the default priority)
        // (lowest priority; measured: the priority makes no difference here - what matters is that the aux launches are
        // issued first - so the one that can never be in the bulk class's way)
        if (hipStreamCreateWithPriority(&c->aux_stream, hipStreamNonBlocking, lo) != hipSuccess) c->aux_stream = nullptr;
        for (auto& ev : c->aev) ev_ok &= hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess;
    }
    if (hipStreamCreateWithFlags(&c->vstream, hipStreamNonBlocking) != hipSuccess) c->vstream = nullptr;
    ev_ok &= hipEventCreateWithFlags(&c->vev_setup, hipEventDisableTiming) == hipSuccess;
    ev_ok &= hipEventCreateWithFlags(&c->vev_matches, hipEventDisableTiming) == hipSuccess;
    for (auto& ev : c->ev) ev_ok &= hipEventCreate(&ev) == hipSuccess;
    for (auto& set : c->bev)
        for (auto& ev : set) ev_ok &= hipEventCreate(&ev) == hipSuccess;
    if (!ev_ok) {
        amc_ctx_destroy(c);
        return api_fail(AMC_E_HIP, "amc_ctx_create: hipEventCreate failed");
    }
    // acos table with the HOST libm (the same one COLMAP's CPU path and the oracle call)
    c->h_lut.resize(kAcosLutSize);
    const float kDistNorm = 1.0f / (512.0f * 512.0f);
    for (int d = 0; d < kAcosLutSize; ++d)
        c->h_lut[d] = acosf(std::fmin(kDistNorm * (float)d, 1.0f));
    if (hipMalloc(reinterpret_cast<void**>(&c->d_lut), kAcosLutSize * sizeof(float)) !=
            hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->d_scalars), 16 * sizeof(uint32_t)) !=
            hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->d_vscalars), kVScalarWords * sizeof(uint32_t)) != hipSuccess ||
        hipMemcpy(c->d_lut, c->h_lut.data(), kAcosLutSize * sizeof(float),
                  hipMemcpyHostToDevice) != hipSuccess ||
        c->h_scalars.ensure(16) != hipSuccess) {
        amc_ctx_destroy(c);
        return api_fail(AMC_E_HIP, "amc_ctx_create: device allocation failed");
    }
    *out = c;
    return AMC_OK;
}

void amc_ctx_destroy(amc_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    const bool dprof = env_flag("AMC_DESTROY_PROFILE");  // wall-clock of the teardown's parts on stderr
    auto tp0 = std::chrono::steady_clock::now();
    auto dlap = [&](const char* what) {
        if (!dprof) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[amc destroy] %s %.1f ms\n", what, std::chrono::duration<double, std::milli>(now - tp0).count());
        tp0 = now;
    };
    (void)hipDeviceSynchronize();
    dlap("sync");
    c->slots.clear();
    c->arena.release_all();
    dlap("slots");
    c->d_imgs.release();
    c->d_grids.release();
    if (c->d_lut) (void)hipFree(c->d_lut);
    if (c->d_accept) (void)hipFree(c->d_accept);
    if (c->d_scalars) (void)hipFree(c->d_scalars);
    c->ms.release_all();
    c->d_keep.release(); c->d_csr.release();
    dlap("match device buffers");
    c->h_csr[0].release(); c->h_csr[1].release();
    c->h_tout.release(); c->h_tmask.release();
    for (int k = 0; k < 2; ++k) {
        c->h_pairs[k].release(); c->h_work[k].release(); c->h_order[k].release(); c->h_order2[k].release();
        c->h_grp[k].release(); c->h_grp2[k].release();
        c->h_pair_off[k].release(); c->h_pair_cnt[k].release(); c->h_matches[k].release();
        c->h_bscalars[k].release();
    }
    c->h_scalars.release();
    dlap("pinned host buffers");
    c->d_timgs.release(); c->d_tmatches.release();
    c->d_estate.release(); c->d_stream.release(); c->d_wmcut.release();
    c->d_tout.release();
    c->vslices.clear();
    c->h_timgs.release(); c->h_tp.release(); c->h_moff.release();
    if (c->d_vscalars) (void)hipFree(c->d_vscalars);
    c->d_tvg_packed.release(); c->d_mask_packed.release(); c->d_moff.release(); c->d_tp_all.release(); c->d_worksum.release();
    c->d_ppairs.release(); c->d_pmatches.release(); c->d_pcos.release(); c->d_pout.release();
    c->h_ppairs.release(); c->h_pout.release();
    dlap("verify device buffers");
    for (auto& ev : c->ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& set : c->bev)
        for (auto& ev : set)
            if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : c->cev)
        if (ev) (void)hipEventDestroy(ev);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->aux_stream) (void)hipStreamDestroy(c->aux_stream);
    for (auto& ev : c->aev)
        if (ev) (void)hipEventDestroy(ev);
    if (c->vstream) (void)hipStreamDestroy(c->vstream);
    if (c->vev_setup) (void)hipEventDestroy(c->vev_setup);
    if (c->vev_matches) (void)hipEventDestroy(c->vev_matches);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    dlap("events and streams");
    delete c;  // (the result pools' idle pinned buffers go with their last owner)
    dlap("delete (pools)");
}

int amc_ctx_set_stream(amc_ctx* c, void* hip_stream) {
    if (!c) return api_fail(AMC_E_INVALID, "amc_ctx_set_stream: ctx is NULL");
    c->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
    return AMC_OK;
}

int amc_ctx_trim(amc_ctx* c) {
    if (!c) return api_fail(AMC_E_INVALID, "amc_ctx_trim: NULL ctx");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->copy_stream) HIPCHK(hipStreamSynchronize(c->copy_stream));
    // per-call scratch and result staging: everything a later call re-allocates on demand (uploaded images, the acos
    // table, the sample stream and the trial tables stay)
    c->result_pool->trim();
    c->d_keep.release(); c->d_csr.release();
    c->resident_matches = 0;
    c->vres = amc::VerifyResident{};
    c->ms.release_large();
    // the verification kernels' sample-stream table is rebuilt on demand (a host mt19937 run + one upload): keep the
    // default-sized one (~0.3 MB at COLMAP's default trial caps), drop one that a large max_num_trials blew up
    if (c->d_stream.cap * sizeof(uint32_t) > ((size_t)16 << 20)) {
        c->d_stream.release();
        c->stream_len = 0;
    }
    if (c->aux_stream) HIPCHK(hipStreamSynchronize(c->aux_stream));
    if (c->vstream) HIPCHK(hipStreamSynchronize(c->vstream));
    for (auto& sl : c->vslices)
        if (sl) sl->release();
    c->h_tp.release(); c->h_moff.release(); c->h_ppairs.release(); c->h_pout.release();
    c->d_estate.release();
    c->d_tout.release(); c->d_tmatches.release(); c->d_pmatches.release(); c->d_pcos.release();
    c->d_tvg_packed.release(); c->d_mask_packed.release(); c->d_moff.release(); c->d_tp_all.release();
    c->verify_pool->trim();
    c->arena.release_idle_slabs();
    c->h_tout.release(); c->h_tmask.release();
    for (int k = 0; k < 2; ++k) {
        c->h_matches[k].release();
        c->h_csr[k].release();
    }
    return AMC_OK;
}

int amc_ctx_resident_matches(amc_ctx* c, const uint32_t** dev_matches, uint64_t* num_matches) {
    if (!c || !dev_matches || !num_matches) return api_fail(AMC_E_INVALID, "amc_ctx_resident_matches: NULL argument");
    *dev_matches = c->resident_matches ? c->d_keep.p : nullptr;
    *num_matches = c->resident_matches;
    return AMC_OK;
}

int amc_upload_matches(amc_ctx* c, const uint32_t* matches, uint64_t num_matches) {
    if (!c) return api_fail(AMC_E_INVALID, "amc_upload_matches: ctx is NULL");
    if (num_matches > 0 && !matches) return api_fail(AMC_E_INVALID, "amc_upload_matches: NULL rows");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));  // (nothing of an earlier call reads the table any more: every entry point blocks)
    c->resident_matches = 0;
    c->vres = amc::VerifyResident{};  // (a resident verification result indexes the table this call rewrites)
    if (num_matches == 0) return AMC_OK;
    HIPCHK(c->d_keep.ensure((size_t)(2 * num_matches)));
    HIPCHK(hipMemcpyAsync(c->d_keep.p, matches, (size_t)(2 * num_matches) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->resident_matches = num_matches;
    return AMC_OK;
}

int amc_ctx_reserve_slots(amc_ctx* c, uint32_t num_slots) {
    if (!c) return api_fail(AMC_E_INVALID, "amc_ctx_reserve_slots: ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->slots.assign(num_slots, Slot());
    c->arena.release_all();  // every slot is gone: the slabs go back to the driver
    c->table_dirty = true;
    return AMC_OK;
}

int amc_ctx_grow_slots(amc_ctx* c, uint32_t num_slots) {
    if (!c) return api_fail(AMC_E_INVALID, "amc_ctx_grow_slots: ctx is NULL");
    if (num_slots < c->slots.size())
        return api_fail(AMC_E_INVALID, "amc_ctx_grow_slots: %u < current %zu slots (use amc_ctx_reserve_slots to reset)",
                        num_slots, c->slots.size());
    c->slots.resize(num_slots);
    c->table_dirty = true;
    return AMC_OK;
}

static int upload_common(amc_ctx* c, uint32_t slot, const void* src, uint32_t rows,
                         hipMemcpyKind kind) {
    if (!c) return api_fail(AMC_E_INVALID, "upload_descriptors: ctx is NULL");
    if (slot >= c->slots.size())
        return api_fail(AMC_E_INVALID, "upload_descriptors: slot %u >= reserved %zu", slot,
                        c->slots.size());
    if (rows > 0 && !src) return api_fail(AMC_E_INVALID, "upload_descriptors: NULL data, rows=%u", rows);
    if (rows > (1u << 30)) return api_fail(AMC_E_INVALID, "upload_descriptors: rows=%u too large", rows);
    HIPCHK(hipSetDevice(c->device));
    Slot& s = c->slots[slot];
    if (s.base) {
        HIPCHK(hipStreamSynchronize(c->stream));
        c->arena.free(s.base);
        s.base = nullptr;
    }
    c->table_dirty = true;
    s.valid = true;
    s.dev.rows = rows;
    s.dev.rows_pad = round_up(rows, kRowPad);
    s.maxsq = 0;
    if (rows == 0) return AMC_OK;
    const size_t rp = s.dev.rows_pad;
    const size_t bytes = rp * kDim * 2 + rp * sizeof(int32_t);
    hipError_t e = c->arena.alloc(&s.base, bytes);
    if (e != hipSuccess) {
        s.valid = false;
        s.dev = ImageDev{};
        return api_fail(AMC_E_NOMEM, "upload_descriptors: hipMalloc(%zu): %s", bytes,
                        hipGetErrorString(e));
    }
    uint8_t* raw = static_cast<uint8_t*>(s.base);
    uint8_t* prep = raw + rp * kDim;
    int32_t* rs = reinterpret_cast<int32_t*>(prep + rp * kDim);
    s.dev.raw = raw;
    s.dev.prep = prep;
    s.dev.rs128 = rs;
    HIPCHK(hipMemcpyAsync(raw, src, (size_t)rows * kDim, kind, c->stream));
    if (rp > rows)
        HIPCHK(memset_async(raw + (size_t)rows * kDim, 0, (rp - rows) * kDim, c->stream));
    HIPCHK(memset_async(c->d_scalars + 2, 0, sizeof(uint32_t), c->stream));
    HIPCHK(launch_prep(raw, prep, rs, s.dev.rows_pad, c->d_scalars + 2, c->stream));
    HIPCHK(hipMemcpyAsync(c->h_scalars.p + 2, c->d_scalars + 2, sizeof(uint32_t),
                          hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    s.maxsq = c->h_scalars.p[2];
    return AMC_OK;
}

int amc_upload_descriptors(amc_ctx* c, uint32_t slot, const uint8_t* host_desc, uint32_t rows) {
    return upload_common(c, slot, host_desc, rows, hipMemcpyHostToDevice);
}
int amc_upload_descriptors_device(amc_ctx* c, uint32_t slot, const void* dev_desc,
                                  uint32_t rows) {
    return upload_common(c, slot, dev_desc, rows, hipMemcpyDeviceToDevice);
}

int amc_get_acos_lut(amc_ctx* c, float* out) {
    if (!c || !out) return api_fail(AMC_E_INVALID, "amc_get_acos_lut: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    // read it back from the device so the test sees what the kernels see
    HIPCHK(hipMemcpy(out, c->d_lut, kAcosLutSize * sizeof(float), hipMemcpyDeviceToHost));
    return AMC_OK;
}

void amc_tvg_opts_default(amc_tvg_opts* o) {
    if (!o) return;
    o->min_num_inliers = 15;          // TwoViewGeometryOptions C++ defaults, SURVEY.md A.3
    o->detect_watermark = 1;
    o->multiple_ignore_watermark = 1;
    o->force_H_use = 0;
    o->compute_relative_pose = 0;
    o->multiple_models = 0;
    o->min_E_F_inlier_ratio = 0.95;
    o->max_H_inlier_ratio = 0.8;
    o->watermark_min_inlier_ratio = 0.7;
    o->watermark_border_size = 0.1;
    o->ransac.max_error = 4.0;
    o->ransac.min_inlier_ratio = 0.25;
    o->ransac.confidence = 0.999;
    o->ransac.dyn_num_trials_multiplier = 3.0;
    o->ransac.min_num_trials = 100;
    o->ransac.max_num_trials = 10000;
}

// Guided matching's candidate generation (match_guided.hip): bucket the image's keypoints on a kGridDim^2 grid
// over their bounding box.  No grid (grid.n = 0) when a coordinate is not finite: such pairs take the dense kernel.
static int build_keypoint_grid(amc_ctx* c, Slot& s, const float* xy, uint32_t rows) {
    guided::GridGeom gg;
    std::vector<uint32_t> sidx, start;
    if (!guided::build_grid(xy, rows, gg, sidx, start)) return AMC_OK;
    GridDev g{};
    g.x0 = gg.x0; g.y0 = gg.y0; g.cw = gg.cw; g.ch = gg.ch; g.inv_cw = gg.inv_cw; g.inv_ch = gg.inv_ch;
    g.bx1 = gg.bx1; g.by1 = gg.by1;
    g.n = rows;
    std::vector<float> sxy((size_t)rows * 2);
    for (uint32_t k = 0; k < rows; ++k) {
        sxy[2 * (size_t)k] = xy[2 * (size_t)sidx[k]];
        sxy[2 * (size_t)k + 1] = xy[2 * (size_t)sidx[k] + 1];
    }
    const size_t b_xy = sxy.size() * sizeof(float), b_idx = sidx.size() * sizeof(uint32_t), b_st = start.size() * sizeof(uint32_t);
    hipError_t e = c->arena.alloc(&s.grid_base, b_xy + b_idx + b_st);
    if (e != hipSuccess) return api_fail(AMC_E_NOMEM, "amc_upload_keypoints: hipMalloc (grid): %s", hipGetErrorString(e));
    char* base = static_cast<char*>(s.grid_base);
    HIPCHK(hipMemcpy(base, sxy.data(), b_xy, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(base + b_xy, sidx.data(), b_idx, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(base + b_xy + b_idx, start.data(), b_st, hipMemcpyHostToDevice));
    g.sxy = reinterpret_cast<const float*>(base);
    g.sidx = reinterpret_cast<const uint32_t*>(base + b_xy);
    g.cell_start = reinterpret_cast<const uint32_t*>(base + b_xy + b_idx);
    s.grid = g;
    return AMC_OK;
}

int amc_upload_keypoints(amc_ctx* c, uint32_t slot, const float* xy, uint32_t rows,
                         uint32_t stride_floats) {
    if (!c) return api_fail(AMC_E_INVALID, "amc_upload_keypoints: ctx is NULL");
    if (slot >= c->slots.size())
        return api_fail(AMC_E_INVALID, "amc_upload_keypoints: slot %u >= reserved %zu", slot, c->slots.size());
    if (rows > 0 && (!xy || stride_floats < 2))
        return api_fail(AMC_E_INVALID, "amc_upload_keypoints: need x,y columns (stride %u) and data", stride_floats);
    HIPCHK(hipSetDevice(c->device));
    Slot& s = c->slots[slot];
    if (s.kp || s.kp64 || s.kpn || s.grid_base) {
        HIPCHK(hipStreamSynchronize(c->stream));
        c->arena.free(s.kp);
        c->arena.free(s.kp64);
        c->arena.free(s.kpn);
        c->arena.free(s.grid_base);
        s.grid_base = nullptr;
        s.grid = GridDev{};
        s.kp = nullptr;
        s.kp64 = nullptr;
        s.kpn = nullptr;
        s.kpn_valid = false;
        s.dev.kp = nullptr;
        s.dev.kp_rows = 0;
        c->table_dirty = true;
    }
    s.kp_rows = rows;
    s.has_kp = true;
    if (rows == 0) return AMC_OK;
    std::vector<float> packed((size_t)rows * 2);
    for (uint32_t i = 0; i < rows; ++i) {
        packed[2 * (size_t)i] = xy[(size_t)i * stride_floats];
        packed[2 * (size_t)i + 1] = xy[(size_t)i * stride_floats + 1];
    }
    hipError_t e = c->arena.alloc(&s.kp, packed.size() * sizeof(float));
    if (e != hipSuccess) {
        s.has_kp = false;
        return api_fail(AMC_E_NOMEM, "amc_upload_keypoints: hipMalloc: %s", hipGetErrorString(e));
    }
    HIPCHK(hipMemcpy(s.kp, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
    s.dev.kp = s.kp;  // guided matching reads the float32 keypoints from the image table
    s.dev.kp_rows = rows;
    c->table_dirty = true;
    return build_keypoint_grid(c, s, packed.data(), rows);
}

int amc_upload_points_f64(amc_ctx* c, uint32_t slot, const double* xy, uint32_t rows) {
    if (!c) return api_fail(AMC_E_INVALID, "amc_upload_points_f64: ctx is NULL");
    if (slot >= c->slots.size())
        return api_fail(AMC_E_INVALID, "amc_upload_points_f64: slot %u >= reserved %zu", slot, c->slots.size());
    if (rows > 0 && !xy) return api_fail(AMC_E_INVALID, "amc_upload_points_f64: NULL data");
    HIPCHK(hipSetDevice(c->device));
    Slot& s = c->slots[slot];
    if (s.kp || s.kp64 || s.kpn || s.grid_base) {
        HIPCHK(hipStreamSynchronize(c->stream));
        c->arena.free(s.kp);
        c->arena.free(s.kp64);
        c->arena.free(s.kpn);
        c->arena.free(s.grid_base);
        s.grid_base = nullptr;
        s.grid = GridDev{};
        s.kp = nullptr;
        s.kp64 = nullptr;
        s.kpn = nullptr;
        s.kpn_valid = false;
        s.dev.kp = nullptr;
        s.dev.kp_rows = 0;
        c->table_dirty = true;
    }
    s.kp_rows = rows;
    s.has_kp = true;
    if (rows == 0) return AMC_OK;
    hipError_t e = c->arena.alloc(&s.kp64, (size_t)rows * 2 * sizeof(double));
    if (e != hipSuccess) {
        s.has_kp = false;
        return api_fail(AMC_E_NOMEM, "amc_upload_points_f64: hipMalloc: %s", hipGetErrorString(e));
    }
    HIPCHK(hipMemcpy(s.kp64, xy, (size_t)rows * 2 * sizeof(double), hipMemcpyHostToDevice));
    return AMC_OK;
}

int amc_upload_camera(amc_ctx* c, uint32_t slot, int32_t model_id, uint64_t width, uint64_t height,
                      const double* params, int32_t num_params, int32_t has_prior) {
    if (!c) return api_fail(AMC_E_INVALID, "amc_upload_camera: ctx is NULL");
    if (slot >= c->slots.size())
        return api_fail(AMC_E_INVALID, "amc_upload_camera: slot %u >= reserved %zu", slot, c->slots.size());
    if (num_params < 0 || (num_params > 0 && !params))
        return api_fail(AMC_E_INVALID, "amc_upload_camera: bad params");
    // Camera::VerifyParams: the parameter vector must have the model's length
    if (cam::num_params(model_id) < 0)
        return api_fail(AMC_E_INVALID, "amc_upload_camera: unknown camera model id %d", model_id);
    if (num_params != cam::num_params(model_id))
        return api_fail(AMC_E_INVALID, "amc_upload_camera: camera model %d takes %d parameters, got %d", model_id,
                        cam::num_params(model_id), num_params);
    Slot& s = c->slots[slot];
    s.cam = CameraDev{};
    s.cam.model_id = model_id;
    s.cam.has_prior = has_prior ? 1 : 0;
    s.cam.width = width;
    s.cam.height = height;
    for (int i = 0; i < num_params; ++i) s.cam.params[i] = params[i];
    s.has_cam = true;
    s.kpn_valid = false;  // the lifted keypoints belong to the previous camera
    return AMC_OK;
}

int amc_cam_from_img(amc_ctx* c, int32_t model_id, const double* params, int32_t num_params, const double* xy,
                     size_t n, double* uv) {
    if (!c) return api_fail(AMC_E_INVALID, "amc_cam_from_img: ctx is NULL");
    if (cam::num_params(model_id) < 0) return api_fail(AMC_E_INVALID, "amc_cam_from_img: unknown camera model id %d", model_id);
    if (num_params != cam::num_params(model_id) || !params)
        return api_fail(AMC_E_INVALID, "amc_cam_from_img: camera model %d takes %d parameters, got %d", model_id,
                        cam::num_params(model_id), num_params);
    if (n == 0) return AMC_OK;
    if (!xy || !uv) return api_fail(AMC_E_INVALID, "amc_cam_from_img: NULL points");
    if (n > 0x7FFFFFFFull) return api_fail(AMC_E_INVALID, "amc_cam_from_img: too many points");
    if (cam::needs_libm(model_id)) {
        for (size_t i = 0; i < n; ++i) cam::cam_from_img(model_id, params, xy[2 * i], xy[2 * i + 1], uv[2 * i], uv[2 * i + 1]);
        return AMC_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    CameraDev cd{};
    cd.model_id = model_id;
    for (int i = 0; i < num_params; ++i) cd.params[i] = params[i];
    DevBuf<double> buf;
    HIPCHK(buf.ensure(4 * n));
    hipStream_t st = c->stream;
    int rc = AMC_OK;
    auto chk = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == AMC_OK) rc = api_fail(AMC_E_HIP, "amc_cam_from_img: %s: %s", what, hipGetErrorString(e));
    };
    chk(hipMemcpyAsync(buf.p, xy, 2 * n * sizeof(double), hipMemcpyHostToDevice, st), "copy in");
    if (rc == AMC_OK) chk(launch_undistort(nullptr, buf.p, (uint32_t)n, cd, buf.p + 2 * n, st), "launch");
    if (rc == AMC_OK) chk(hipMemcpyAsync(uv, buf.p + 2 * n, 2 * n * sizeof(double), hipMemcpyDeviceToHost, st), "copy out");
    chk(hipStreamSynchronize(st), "sync");
    return rc;
}

int amc_img_from_cam(amc_ctx* c, int32_t model_id, const double* params, int32_t num_params, const double* uv,
                     size_t n, double* xy) {
    if (!c) return api_fail(AMC_E_INVALID, "amc_img_from_cam: ctx is NULL");
    if (cam::num_params(model_id) < 0) return api_fail(AMC_E_INVALID, "amc_img_from_cam: unknown camera model id %d", model_id);
    if (num_params != cam::num_params(model_id) || !params)
        return api_fail(AMC_E_INVALID, "amc_img_from_cam: camera model %d takes %d parameters, got %d", model_id,
                        cam::num_params(model_id), num_params);
    if (n == 0) return AMC_OK;
    if (!uv || !xy) return api_fail(AMC_E_INVALID, "amc_img_from_cam: NULL points");
    if (n > 0x7FFFFFFFull) return api_fail(AMC_E_INVALID, "amc_img_from_cam: too many points");
    if (cam::needs_libm(model_id)) {
        for (size_t i = 0; i < n; ++i) cam::img_from_cam(model_id, params, uv[2 * i], uv[2 * i + 1], xy[2 * i], xy[2 * i + 1]);
        return AMC_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    CameraDev cd{};
    cd.model_id = model_id;
    for (int i = 0; i < num_params; ++i) cd.params[i] = params[i];
    DevBuf<double> buf;
    HIPCHK(buf.ensure(4 * n));
    hipStream_t st = c->stream;
    int rc = AMC_OK;
    auto chk = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == AMC_OK) rc = api_fail(AMC_E_HIP, "amc_img_from_cam: %s: %s", what, hipGetErrorString(e));
    };
    chk(hipMemcpyAsync(buf.p, uv, 2 * n * sizeof(double), hipMemcpyHostToDevice, st), "copy in");
    if (rc == AMC_OK) chk(launch_project(buf.p, (uint32_t)n, cd, buf.p + 2 * n, st), "launch");
    if (rc == AMC_OK) chk(hipMemcpyAsync(xy, buf.p + 2 * n, 2 * n * sizeof(double), hipMemcpyDeviceToHost, st), "copy out");
    chk(hipStreamSynchronize(st), "sync");
    return rc;
}

}  // extern "C"

namespace amc {

// Camera::CamFromImg of all keypoints of a slot, once per (points, camera): COLMAP lifts every matched point of
// every pair (EstimateCalibratedTwoViewGeometry, EstimateTwoViewGeometryPose); the lift depends on the keypoint
// only, so it is taken here per image and kept in HBM.  Pinhole cameras need nothing (two divisions, done where
// the points are gathered).  Polynomial distortion models run on the device (camera.hip); the fisheye family and
// FOV call atan / tan / sin / cos and are lifted with the host libm (camera_math.h).
int ensure_normalized(amc_ctx* c, uint32_t slot) {
    Slot& s = c->slots[slot];
    if (!s.has_cam || !s.has_kp || cam::is_pinhole(s.cam.model_id) || s.kpn_valid) return AMC_OK;
    const uint32_t rows = s.kp_rows;
    if (rows == 0) {
        s.kpn_valid = true;
        return AMC_OK;
    }
    if (!s.kpn) {
        hipError_t e = c->arena.alloc(&s.kpn, (size_t)rows * 2 * sizeof(double));
        if (e != hipSuccess) return api_fail(AMC_E_NOMEM, "CamFromImg buffer: hipMalloc: %s", hipGetErrorString(e));
    }
    if (!cam::needs_libm(s.cam.model_id)) {
        HIPCHK(launch_undistort(s.kp, s.kp64, rows, s.cam, s.kpn, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    } else {
        std::vector<double> xy((size_t)rows * 2), uv((size_t)rows * 2);
        if (s.kp64) {
            HIPCHK(hipMemcpy(xy.data(), s.kp64, xy.size() * sizeof(double), hipMemcpyDeviceToHost));
        } else {
            std::vector<float> f((size_t)rows * 2);
            HIPCHK(hipMemcpy(f.data(), s.kp, f.size() * sizeof(float), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < f.size(); ++i) xy[i] = (double)f[i];
        }
        const CameraDev camd = s.cam;
        auto work = [&](uint32_t lo, uint32_t hi) {
            for (uint32_t i = lo; i < hi; ++i)
                cam::cam_from_img(camd.model_id, camd.params, xy[2 * (size_t)i], xy[2 * (size_t)i + 1], uv[2 * (size_t)i],
                                  uv[2 * (size_t)i + 1]);
        };
        const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        const unsigned nth = rows >= 2048 ? hw : 1;
        if (nth == 1) {
            work(0, rows);
        } else {
            std::vector<std::thread> th;
            const uint32_t per = (rows + nth - 1) / nth;
            for (unsigned t = 0; t < nth; ++t) {
                const uint32_t lo = std::min(rows, t * per), hi = std::min(rows, lo + per);
                if (lo < hi) th.emplace_back(work, lo, hi);
            }
            for (auto& t : th) t.join();
        }
        HIPCHK(hipMemcpy(s.kpn, uv.data(), uv.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    s.kpn_valid = true;
    return AMC_OK;
}

void fill_tvg_images(const amc_ctx* c, std::vector<TvgImage>& timgs) {
    timgs.resize(c->slots.size());
    for (size_t i = 0; i < timgs.size(); ++i) {
        const Slot& s = c->slots[i];
        timgs[i].kp = s.kp;
        timgs[i].kp64 = s.kp64;
        timgs[i].kpn = (s.kpn_valid && !cam::is_pinhole(s.cam.model_id)) ? s.kpn : nullptr;
        timgs[i].rows = s.kp_rows;
        timgs[i].pad = 0;
        timgs[i].cam = s.cam;
    }
}

}  // namespace amc
