// undistort.hip — image undistortion on gfx950 (include/amc_undistort.h): COLMAP 3.9.1's UndistortCamera and
// WarpImageBetweenCameras, restated in DESIGN.md section 14.  Every FP64 operation below is written in the order of
// that section, the order tests/undistort_ref/undistort_ref.cc follows too: the two are bit-identical.  The projection
// through the source model is abspose_core.h's img_from_cam_t<double> with the project's own atan / sin / cos; FP
// contraction is off.
//
// Work split (14.5).  warp_kernel: one lane owns four consecutive target pixels of the image's row-major pixel order,
// computes each pixel's source coordinate once for all its channels, gathers the four neighbours per channel and
// stores the group as `channels` aligned 32-bit words (a pixel group starts at byte 4 g channels of a 256-byte aligned
// image, whatever the row length); the last, partial group of an image is stored by bytes.  Neighbouring lanes hold
// neighbouring target pixels, hence neighbouring source pixels: a wave's gathers stay within a few source rows.  The
// anti-aliasing pre-pass is two more kernels (resize_rows_kernel, resize_cols_kernel) over host-built weight tables.
// No atomics; a pixel depends on its own image only, never on the batch.  The lane's 12 output bytes are indexed by
// the channel count, so the compiler keeps them in LDS (3 KiB per block, profiles/undistort/kernel_resource_usage.txt);
// no scratch, 118 VGPRs, four waves per SIMD.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "amc_internal.h"
#include "abspose_core.h"
#include "../../include/amc_undistort.h"

using namespace amc;

namespace {

constexpr int kBlock = 256;
constexpr int kGroup = 4;  // target pixels per lane
// device batch bound in bytes (sources, resize scratch, weight tables, targets); AMC_UNDISTORT_BATCH_BYTES overrides it
constexpr long long kBatchBytes = (long long)1 << 30;
constexpr uint64_t kMaxSide = (uint64_t)1 << 30;

struct WarpJob {
    const uint8_t* src;  // sw x sh x ch, tightly packed
    uint8_t* dst;        // dw x dh x ch, tightly packed
    int32_t sw, sh, dw, dh, ch, model;
    double sp[cam::kMaxParams];  // the source camera's parameters (rescaled when the pre-pass ran)
    double fx, fy, cx, cy;       // the PINHOLE target
};

struct ResizeJob {
    const uint8_t* in;
    uint8_t* out;
    const int32_t* left;  // per output coordinate: the first input coordinate of its window
    const int32_t* cnt;   // ... the window's length
    const double* w;      // ... its weights, k per output coordinate
    int32_t k;
    int32_t in_w, in_h, out_w, out_h, ch;
};

// 14.3: round half up (the values are not negative) without forming value + 0.5, then clamp to a byte
AMC_HD uint8_t round_byte(double v) {
    if (!(v > 0.0)) return 0;
    if (v >= 255.0) return 255;
    double r = __builtin_floor(v);
    if (v - r >= 0.5) r = r + 1.0;
    return (uint8_t)(int)r;
}

// 14.3: one target pixel, all channels
AMC_HD void warp_pixel(const WarpJob& j, int x, int y, uint8_t* out) {
    const double u = (((double)x + 0.5) - j.cx) / j.fx;
    const double v = (((double)y + 0.5) - j.cy) / j.fy;
    double sx, sy;
    ap::img_from_cam_t<double>(j.model, j.sp, u, v, 1.0, sx, sy);
    const double xs = sx - 0.5;
    const double iy = (double)(j.sh - 1) - (sy - 0.5);  // rows counted from the bottom
    const double x0 = __builtin_floor(xs), y0 = __builtin_floor(iy);
    const bool inside = x0 >= 0.0 && x0 + 1.0 < (double)j.sw && y0 >= 0.0 && y0 + 1.0 < (double)j.sh;
    if (!inside) {  // (a NaN coordinate fails every comparison)
        for (int c = 0; c < j.ch; ++c) out[c] = 0;
        return;
    }
    const double dx = xs - x0, dy = iy - y0;
    const int xi = (int)x0, yi = (int)y0;
    const size_t row = (size_t)j.sw * (size_t)j.ch;
    const uint8_t* r0 = j.src + (size_t)(j.sh - 1 - yi) * row + (size_t)xi * (size_t)j.ch;  // bottom-up row y0
    const uint8_t* r1 = r0 - row;                                                          // bottom-up row y0 + 1
    for (int c = 0; c < j.ch; ++c) {
        const double v0 = (1.0 - dx) * (double)r0[c] + dx * (double)r0[j.ch + c];
        const double v1 = (1.0 - dx) * (double)r1[c] + dx * (double)r1[j.ch + c];
        out[c] = round_byte((1.0 - dy) * v0 + dy * v1);
    }
}

// one lane's work: pixel group g of the image
AMC_HD void warp_group(const WarpJob& j, uint64_t g) {
    const uint64_t npix = (uint64_t)j.dw * (uint64_t)j.dh;
    const uint64_t p0 = g * kGroup;
    if (p0 >= npix) return;
    uint8_t out[kGroup * 3];
    const int n = (int)(npix - p0 < (uint64_t)kGroup ? npix - p0 : (uint64_t)kGroup);
    int y = (int)(p0 / (uint64_t)j.dw), x = (int)(p0 - (uint64_t)y * (uint64_t)j.dw);
    for (int k = 0; k < kGroup; ++k) {
        if (k < n) {
            warp_pixel(j, x, y, out + k * j.ch);
            if (++x == j.dw) {
                x = 0;
                ++y;
            }
        }
    }
    uint8_t* d = j.dst + p0 * (uint64_t)j.ch;
    if (n == kGroup) {  // 4 g ch bytes into a 256-byte aligned image: word aligned
        uint32_t* d32 = reinterpret_cast<uint32_t*>(d);
        for (int wd = 0; wd < j.ch; ++wd)
            d32[wd] = (uint32_t)out[4 * wd] | ((uint32_t)out[4 * wd + 1] << 8) | ((uint32_t)out[4 * wd + 2] << 16) |
                      ((uint32_t)out[4 * wd + 3] << 24);
    } else {
        for (int b = 0; b < n * j.ch; ++b) d[b] = out[b];
    }
}
__global__ __launch_bounds__(kBlock) void warp_kernel(WarpJob j) {
    warp_group(j, (uint64_t)blockIdx.x * kBlock + threadIdx.x);
}

// 14.4, first pass: every input row is resampled along x; i = the output sample
AMC_HD void resize_rows_at(const ResizeJob& r, uint64_t i) {
    if (i >= (uint64_t)r.out_w * (uint64_t)r.out_h) return;
    const int y = (int)(i / (uint64_t)r.out_w), x = (int)(i - (uint64_t)y * (uint64_t)r.out_w);
    const int l = r.left[x], n = r.cnt[x];
    const double* w = r.w + (size_t)x * (size_t)r.k;
    const uint8_t* in = r.in + ((size_t)y * (size_t)r.in_w + (size_t)l) * (size_t)r.ch;
    for (int c = 0; c < r.ch; ++c) {
        double acc = 0.0;
        for (int k = 0; k < n; ++k) acc = acc + w[k] * (double)in[(size_t)k * (size_t)r.ch + c];
        r.out[i * (uint64_t)r.ch + c] = round_byte(acc);
    }
}
// second pass: every column of the first pass's output is resampled along y
AMC_HD void resize_cols_at(const ResizeJob& r, uint64_t i) {
    if (i >= (uint64_t)r.out_w * (uint64_t)r.out_h) return;
    const int y = (int)(i / (uint64_t)r.out_w), x = (int)(i - (uint64_t)y * (uint64_t)r.out_w);
    const int l = r.left[y], n = r.cnt[y];
    const double* w = r.w + (size_t)y * (size_t)r.k;
    const size_t row = (size_t)r.in_w * (size_t)r.ch;
    const uint8_t* in = r.in + (size_t)l * row + (size_t)x * (size_t)r.ch;
    for (int c = 0; c < r.ch; ++c) {
        double acc = 0.0;
        for (int k = 0; k < n; ++k) acc = acc + w[k] * (double)in[(size_t)k * row + c];
        r.out[i * (uint64_t)r.ch + c] = round_byte(acc);
    }
}
__global__ __launch_bounds__(kBlock) void resize_rows_kernel(ResizeJob r) {
    resize_rows_at(r, (uint64_t)blockIdx.x * kBlock + threadIdx.x);
}
__global__ __launch_bounds__(kBlock) void resize_cols_kernel(ResizeJob r) {
    resize_cols_at(r, (uint64_t)blockIdx.x * kBlock + threadIdx.x);
}

// ---- host side ------------------------------------------------------------------------------------------------------

// 14.4: the weight table of one axis, `in` samples to `out` samples (a tent whose support widens by the reduction)
struct AxisWeights {
    std::vector<int32_t> left, cnt;
    std::vector<double> w;
    int32_t k = 1;
};
void build_axis_weights(int64_t in, int64_t out, AxisWeights& t) {
    const double scale = (double)out / (double)in;
    const double width = scale < 1.0 ? 1.0 / scale : 1.0;
    const double fscale = scale < 1.0 ? scale : 1.0;
    const double offset = 0.5 / scale;
    t.left.assign((size_t)out, 0);
    t.cnt.assign((size_t)out, 0);
    std::vector<std::vector<double>> rows((size_t)out);
    t.k = 1;
    for (int64_t u = 0; u < out; ++u) {
        const double center = (double)u / scale + offset;
        int64_t left = (int64_t)(center - width + 0.5), right = (int64_t)(center + width + 0.5);
        if (left < 0) left = 0;
        if (right > in) right = in;
        std::vector<double>& w = rows[(size_t)u];
        double total = 0.0;
        for (int64_t i = left; i < right; ++i) {
            double d = fscale * (((double)i + 0.5) - center);
            if (d < 0.0) d = -d;
            const double wi = d < 1.0 ? fscale * (1.0 - d) : 0.0;
            w.push_back(wi);
            total = total + wi;
        }
        if (!(total > 0.0)) {  // no sample under the tent: the nearest one
            int64_t i = (int64_t)center;
            if (i > in - 1) i = in - 1;
            left = i;
            w.assign(1, 1.0);
            total = 1.0;
        }
        for (double& wi : w) wi = wi / total;
        t.left[(size_t)u] = (int32_t)left;
        t.cnt[(size_t)u] = (int32_t)w.size();
        t.k = std::max<int32_t>(t.k, (int32_t)w.size());
    }
    t.w.assign((size_t)out * (size_t)t.k, 0.0);
    for (int64_t u = 0; u < out; ++u) std::copy(rows[(size_t)u].begin(), rows[(size_t)u].end(), t.w.begin() + (size_t)u * (size_t)t.k);
}

// Camera::Rescale(width, height) on the parameters: principal point by axis, one focal length by the mean scale
void rescale_params(int model, double* p, double sx, double sy) {
    const int nf = cam::num_focal(model);
    p[nf] = p[nf] * sx;
    p[nf + 1] = p[nf + 1] * sy;
    if (nf == 1) {
        p[0] = p[0] * ((sx + sy) / 2.0);
    } else {
        p[0] = p[0] * sx;
        p[1] = p[1] * sy;
    }
}

bool all_extra_finite(const amc_undistort_cam& c) {
    const int np = cam::num_params(c.model);
    for (int i = 0; i < np; ++i)
        if (!std::isfinite(c.params[i])) return false;
    return true;
}

// one image's place in a device batch
struct Placed {
    size_t src = 0, tmp = 0, small = 0, dst = 0;        // byte offsets (256-aligned)
    size_t lx = 0, cx = 0, wx = 0, ly = 0, cy = 0, wy = 0;  // the two weight tables
    bool resize = false;
    AxisWeights ax, ay;
};

}  // namespace

extern "C" {

void amc_undistort_opts_default(amc_undistort_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->blank_pixels = 0.0;  // UndistortCameraOptions()
    o->min_scale = 0.2;
    o->max_scale = 2.0;
    o->max_image_size = -1;
    o->roi_min_x = 0.0;
    o->roi_min_y = 0.0;
    o->roi_max_x = 1.0;
    o->roi_max_y = 1.0;
}

int amc_undistort_camera(const amc_undistort_opts* opts, const amc_undistort_cam* camera, amc_undistort_cam* undistorted) {
    if (!opts || !camera || !undistorted) return api_fail(AMC_E_INVALID, "amc_undistort_camera: NULL argument");
    const amc_undistort_opts o = *opts;
    const amc_undistort_cam c = *camera;
    if (cam::num_params(c.model) < 0) return api_fail(AMC_E_INVALID, "amc_undistort_camera: unknown camera model id %d", c.model);
    if (c.width == 0 || c.height == 0 || c.width > kMaxSide || c.height > kMaxSide)
        return api_fail(AMC_E_INVALID, "amc_undistort_camera: camera size %llu x %llu", (unsigned long long)c.width,
                        (unsigned long long)c.height);
    // 14.2 step 1: the option checks
    if (!(o.blank_pixels >= 0.0) || !(o.blank_pixels <= 1.0))
        return api_fail(AMC_E_INVALID, "amc_undistort_camera: blank_pixels %g is outside [0, 1]", o.blank_pixels);
    if (!(o.min_scale > 0.0) || !(o.min_scale <= o.max_scale))
        return api_fail(AMC_E_INVALID, "amc_undistort_camera: needs 0 < min_scale <= max_scale, got %g and %g", o.min_scale, o.max_scale);
    if (o.max_image_size == 0) return api_fail(AMC_E_INVALID, "amc_undistort_camera: max_image_size is 0");
    if (!(o.roi_min_x >= 0.0) || !(o.roi_min_y >= 0.0) || !(o.roi_max_x <= 1.0) || !(o.roi_max_y <= 1.0) ||
        !(o.roi_min_x < o.roi_max_x) || !(o.roi_min_y < o.roi_max_y))
        return api_fail(AMC_E_INVALID, "amc_undistort_camera: the ROI (%g, %g) - (%g, %g) is not inside [0, 1] with min < max",
                        o.roi_min_x, o.roi_min_y, o.roi_max_x, o.roi_max_y);

    // step 2: PINHOLE of the source's size, focal length(s) and principal point
    const int nf = cam::num_focal(c.model);
    const double W = (double)c.width, H = (double)c.height;
    double fx = c.params[0], fy = c.params[nf - 1], cx = c.params[nf], cy = c.params[nf + 1];
    double uw = W, uh = H;
    // step 3: the region of interest in pixels
    const bool roi = o.roi_min_x > 0.0 || o.roi_min_y > 0.0 || o.roi_max_x < 1.0 || o.roi_max_y < 1.0;
    double rx0 = 0.0, ry0 = 0.0, rx1 = W, ry1 = H;
    if (roi) {
        rx0 = std::round(o.roi_min_x * W);
        ry0 = std::round(o.roi_min_y * H);
        rx1 = std::round(o.roi_max_x * W);
        ry1 = std::round(o.roi_max_y * H);
        rx0 = std::min(rx0, W - 1.0);
        ry0 = std::min(ry0, H - 1.0);
        rx1 = std::max(rx1, rx0 + 1.0);
        ry1 = std::max(ry1, ry0 + 1.0);
        uw = rx1 - rx0;
        uh = ry1 - ry0;
        cx = cx - rx0;
        cy = cy - ry0;
    }
    // step 4: the four borders, lifted with the source model and projected with the undistorted one
    if (roi || !cam::is_pinhole(c.model)) {
        double left_min = DBL_MAX, left_max = -DBL_MAX, right_min = DBL_MAX, right_max = -DBL_MAX;
        double top_min = DBL_MAX, top_max = -DBL_MAX, bottom_min = DBL_MAX, bottom_max = -DBL_MAX;
        for (double y = ry0; y < ry1; y += 1.0) {
            double u, v;
            cam::cam_from_img(c.model, c.params, 0.5, y + 0.5, u, v);
            const double xl = fx * u + cx;
            left_min = std::min(left_min, xl);
            left_max = std::max(left_max, xl);
            cam::cam_from_img(c.model, c.params, W - 0.5, y + 0.5, u, v);
            const double xr = fx * u + cx;
            right_min = std::min(right_min, xr);
            right_max = std::max(right_max, xr);
        }
        for (double x = rx0; x < rx1; x += 1.0) {
            double u, v;
            cam::cam_from_img(c.model, c.params, x + 0.5, 0.5, u, v);
            const double yt = fy * v + cy;
            top_min = std::min(top_min, yt);
            top_max = std::max(top_max, yt);
            cam::cam_from_img(c.model, c.params, x + 0.5, H - 0.5, u, v);
            const double yb = fy * v + cy;
            bottom_min = std::min(bottom_min, yb);
            bottom_max = std::max(bottom_max, yb);
        }
        const double min_scale_x = std::min(cx / (cx - left_min), (uw - 0.5 - cx) / (right_max - cx));
        const double min_scale_y = std::min(cy / (cy - top_min), (uh - 0.5 - cy) / (bottom_max - cy));
        const double max_scale_x = std::max(cx / (cx - left_max), (uw - 0.5 - cx) / (right_min - cx));
        const double max_scale_y = std::max(cy / (cy - top_max), (uh - 0.5 - cy) / (bottom_min - cy));
        double scale_x = 1.0 / (min_scale_x * o.blank_pixels + max_scale_x * (1.0 - o.blank_pixels));
        double scale_y = 1.0 / (min_scale_y * o.blank_pixels + max_scale_y * (1.0 - o.blank_pixels));
        scale_x = std::min(std::max(scale_x, o.min_scale), o.max_scale);  // (a NaN scale stays NaN: no comparison holds)
        scale_y = std::min(std::max(scale_y, o.min_scale), o.max_scale);
        const double nw = std::max(1.0, scale_x * uw), nh = std::max(1.0, scale_y * uh);  // (... and gives one sample)
        if (!(nw <= (double)kMaxSide) || !(nh <= (double)kMaxSide))
            return api_fail(AMC_E_INVALID, "amc_undistort_camera: the undistorted size %g x %g is out of range", nw, nh);
        const double new_w = (double)(uint64_t)nw, new_h = (double)(uint64_t)nh;
        cx = cx * new_w / uw;
        cy = cy * new_h / uh;
        uw = new_w;
        uh = new_h;
    }
    // step 5: Camera::Rescale(scale) down to max_image_size
    if (o.max_image_size > 0) {
        const double s = std::min((double)o.max_image_size / uw, (double)o.max_image_size / uh);
        if (s < 1.0) {
            const double rw = std::round(s * uw), rh = std::round(s * uh);
            const double sx = rw / uw, sy = rh / uh;
            uw = std::max(1.0, rw);
            uh = std::max(1.0, rh);
            cx = cx * sx;
            cy = cy * sy;
            fx = fx * sx;
            fy = fy * sy;
        }
    }
    amc_undistort_cam out;
    std::memset(&out, 0, sizeof out);
    out.model = cam::PINHOLE;
    out.width = (uint64_t)uw;
    out.height = (uint64_t)uh;
    out.params[0] = fx;
    out.params[1] = fy;
    out.params[2] = cx;
    out.params[3] = cy;
    *undistorted = out;
    return AMC_OK;
}

int amc_undistort_points(const amc_undistort_cam* camera, const amc_undistort_cam* undistorted, size_t n,
                         const double* xy_in, double* xy_out) {
    if (!camera || !undistorted || (n && (!xy_in || !xy_out)))
        return api_fail(AMC_E_INVALID, "amc_undistort_points: NULL argument");
    if (cam::num_params(camera->model) < 0)
        return api_fail(AMC_E_INVALID, "amc_undistort_points: unknown camera model id %d", camera->model);
    if (undistorted->model != cam::PINHOLE)
        return api_fail(AMC_E_INVALID, "amc_undistort_points: the undistorted camera's model id %d is not PINHOLE", undistorted->model);
    const double* q = undistorted->params;
    for (size_t i = 0; i < n; ++i) {
        double u, v;
        cam::cam_from_img(camera->model, camera->params, xy_in[2 * i], xy_in[2 * i + 1], u, v);
        xy_out[2 * i] = q[0] * u + q[2];
        xy_out[2 * i + 1] = q[1] * v + q[3];
    }
    return AMC_OK;
}

int amc_undistort_images(amc_ctx* ctx, size_t nimages, const amc_undistort_image* images, amc_undistort_result* result) {
    const char* const hipchk_who = "amc_undistort_images";
    const long long batch_bytes = env_int("AMC_UNDISTORT_BATCH_BYTES", kBatchBytes, 1, (long long)1 << 40);
    if (!ctx || !result || (nimages && !images)) return api_fail(AMC_E_INVALID, "amc_undistort_images: NULL argument");
    std::memset(result, 0, sizeof *result);
    for (size_t i = 0; i < nimages; ++i) {
        const amc_undistort_image& im = images[i];
        const amc_undistort_cam &s = im.src_camera, &d = im.dst_camera;
        if (!im.src || !im.dst) return api_fail(AMC_E_INVALID, "amc_undistort_images: image %zu has a NULL pixel pointer", i);
        if (im.channels != 1 && im.channels != 3)
            return api_fail(AMC_E_INVALID, "amc_undistort_images: image %zu has %d channels (1 or 3)", i, im.channels);
        if (s.width == 0 || s.height == 0 || d.width == 0 || d.height == 0 || s.width > kMaxSide || s.height > kMaxSide ||
            d.width > kMaxSide || d.height > kMaxSide || s.width * s.height > ((uint64_t)1 << 31) ||
            d.width * d.height > ((uint64_t)1 << 31))
            return api_fail(AMC_E_INVALID, "amc_undistort_images: image %zu: source %llu x %llu, target %llu x %llu", i,
                            (unsigned long long)s.width, (unsigned long long)s.height, (unsigned long long)d.width,
                            (unsigned long long)d.height);
        if (im.src_stride < s.width * (uint64_t)im.channels)
            return api_fail(AMC_E_INVALID, "amc_undistort_images: image %zu: stride %llu is below its row of %llu bytes", i,
                            (unsigned long long)im.src_stride, (unsigned long long)(s.width * (uint64_t)im.channels));
        if (cam::num_params(s.model) < 0)
            return api_fail(AMC_E_INVALID, "amc_undistort_images: image %zu: unknown source camera model id %d", i, s.model);
        if (d.model != cam::PINHOLE)
            return api_fail(AMC_E_INVALID, "amc_undistort_images: image %zu: the target camera's model id %d is not PINHOLE", i, d.model);
        if (!all_extra_finite(s) || !all_extra_finite(d) || d.params[0] == 0.0 || d.params[1] == 0.0)
            return api_fail(AMC_E_INVALID, "amc_undistort_images: image %zu: a camera parameter is not finite, or a target focal length is 0", i);
    }
    if (nimages == 0) return AMC_OK;

    // each image's device bytes, then contiguous batches under the bound (a larger image is a batch of its own)
    std::vector<uint64_t> offs(nimages + 1, 0);
    std::vector<uint8_t> resize(nimages, 0);
    for (size_t i = 0; i < nimages; ++i) {
        const amc_undistort_image& im = images[i];
        const uint64_t sw = im.src_camera.width, sh = im.src_camera.height, dw = im.dst_camera.width, dh = im.dst_camera.height;
        const uint64_t ch = (uint64_t)im.channels;
        uint64_t b = align256(sw * sh * ch) + align256(dw * dh * ch);
        resize[i] = dw * dh < sw * sh;  // 14.4
        if (resize[i])  // first pass output, second pass output, the two tables (the window is at most 2 reduction + 2)
            b += align256(dw * sh * ch) + align256(dw * dh * ch) + 2 * (align256(dw * 4) + align256(dh * 4)) +
                 align256(dw * 8 * (2 * (sw / dw + 1) + 3)) + align256(dh * 8 * (2 * (sh / dh + 1) + 3));
        offs[i + 1] = offs[i] + b;
    }
    const Batches batches = split_batches(offs.data(), nimages, ~(uint64_t)0, (uint64_t)batch_bytes);
    const size_t nbatch = batches.count();

    const CtxView cv = ctx_view(ctx);
    HIPCHK(hipSetDevice(cv.device));
    hipStream_t st = cv.stream;
    StreamTimer timer(st);
    HIPCHK(timer.start());
    DevBuf<void> mem;
    {
        const hipError_t e = mem.ensure((size_t)batches.most_elems + 256);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            return api_fail(AMC_E_NOMEM, "amc_undistort_images: out of device memory for a batch of %llu bytes",
                            (unsigned long long)batches.most_elems);
        }
        HIPCHK(e);
    }
    char* const base = static_cast<char*>(mem.p);
    std::vector<std::vector<Placed>> placed(nbatch);  // host tables stay alive until the stream is drained
    for (size_t bi = 0; bi < nbatch; ++bi) {
        const size_t i0 = batches.start[bi], i1 = batches.start[bi + 1];
        std::vector<Placed>& pl = placed[bi];
        pl.resize(i1 - i0);
        size_t at = 0;
        auto take = [&](size_t bytes) {
            const size_t o = at;
            at += align256(bytes);
            return o;
        };
        // place and upload
        for (size_t i = i0; i < i1; ++i) {
            const amc_undistort_image& im = images[i];
            Placed& p = pl[i - i0];
            const size_t sw = im.src_camera.width, sh = im.src_camera.height, dw = im.dst_camera.width, dh = im.dst_camera.height;
            const size_t ch = (size_t)im.channels;
            p.resize = resize[i] != 0;
            p.src = take(sw * sh * ch);
            p.dst = take(dw * dh * ch);
            HIPCHK(hipMemcpy2DAsync(base + p.src, sw * ch, im.src, im.src_stride, sw * ch, sh, hipMemcpyHostToDevice, st));
            if (p.resize) {
                build_axis_weights((int64_t)sw, (int64_t)dw, p.ax);
                build_axis_weights((int64_t)sh, (int64_t)dh, p.ay);
                p.tmp = take(dw * sh * ch);
                p.small = take(dw * dh * ch);
                p.lx = take(dw * 4);
                p.cx = take(dw * 4);
                p.wx = take(p.ax.w.size() * 8);
                p.ly = take(dh * 4);
                p.cy = take(dh * 4);
                p.wy = take(p.ay.w.size() * 8);
                HIPCHK(hipMemcpyAsync(base + p.lx, p.ax.left.data(), dw * 4, hipMemcpyHostToDevice, st));
                HIPCHK(hipMemcpyAsync(base + p.cx, p.ax.cnt.data(), dw * 4, hipMemcpyHostToDevice, st));
                HIPCHK(hipMemcpyAsync(base + p.wx, p.ax.w.data(), p.ax.w.size() * 8, hipMemcpyHostToDevice, st));
                HIPCHK(hipMemcpyAsync(base + p.ly, p.ay.left.data(), dh * 4, hipMemcpyHostToDevice, st));
                HIPCHK(hipMemcpyAsync(base + p.cy, p.ay.cnt.data(), dh * 4, hipMemcpyHostToDevice, st));
                HIPCHK(hipMemcpyAsync(base + p.wy, p.ay.w.data(), p.ay.w.size() * 8, hipMemcpyHostToDevice, st));
            }
            if (at > mem.cap)
                return api_fail(AMC_E_STATE, "amc_undistort_images: batch %zu needs %zu bytes, %zu were sized", bi, at, mem.cap);
        }
        // kernels
        HIPCHK(timer.span_begin());
        for (size_t i = i0; i < i1; ++i) {
            const amc_undistort_image& im = images[i];
            const Placed& p = pl[i - i0];
            const int sw = (int)im.src_camera.width, sh = (int)im.src_camera.height, dw = (int)im.dst_camera.width,
                      dh = (int)im.dst_camera.height;
            WarpJob j{};
            j.src = reinterpret_cast<const uint8_t*>(base + p.src);
            j.dst = reinterpret_cast<uint8_t*>(base + p.dst);
            j.sw = sw;
            j.sh = sh;
            j.dw = dw;
            j.dh = dh;
            j.ch = im.channels;
            j.model = im.src_camera.model;
            std::memcpy(j.sp, im.src_camera.params, sizeof j.sp);
            j.fx = im.dst_camera.params[0];
            j.fy = im.dst_camera.params[1];
            j.cx = im.dst_camera.params[2];
            j.cy = im.dst_camera.params[3];
            if (p.resize) {
                ResizeJob r{};
                r.in = j.src;
                r.out = reinterpret_cast<uint8_t*>(base + p.tmp);
                r.left = reinterpret_cast<const int32_t*>(base + p.lx);
                r.cnt = reinterpret_cast<const int32_t*>(base + p.cx);
                r.w = reinterpret_cast<const double*>(base + p.wx);
                r.k = p.ax.k;
                r.in_w = sw;
                r.in_h = sh;
                r.out_w = dw;
                r.out_h = sh;
                r.ch = im.channels;
                uint64_t n = (uint64_t)dw * (uint64_t)sh;
                hipLaunchKernelGGL(resize_rows_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, r);
                HIPCHK(hipGetLastError());
                r.in = r.out;
                r.out = reinterpret_cast<uint8_t*>(base + p.small);
                r.left = reinterpret_cast<const int32_t*>(base + p.ly);
                r.cnt = reinterpret_cast<const int32_t*>(base + p.cy);
                r.w = reinterpret_cast<const double*>(base + p.wy);
                r.k = p.ay.k;
                r.in_w = dw;
                r.in_h = sh;
                r.out_w = dw;
                r.out_h = dh;
                n = (uint64_t)dw * (uint64_t)dh;
                hipLaunchKernelGGL(resize_cols_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, r);
                HIPCHK(hipGetLastError());
                // the warp reads the resized image through the camera rescaled to its size
                j.src = r.out;
                j.sw = dw;
                j.sh = dh;
                rescale_params(j.model, j.sp, (double)dw / (double)sw, (double)dh / (double)sh);
                result->num_resized += 1;
            }
            const uint64_t groups = ((uint64_t)dw * (uint64_t)dh + kGroup - 1) / kGroup;
            hipLaunchKernelGGL(warp_kernel, dim3((unsigned)((groups + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, j);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(timer.span_end());
        for (size_t i = i0; i < i1; ++i) {
            const amc_undistort_image& im = images[i];
            const size_t bytes = (size_t)im.dst_camera.width * (size_t)im.dst_camera.height * (size_t)im.channels;
            HIPCHK(hipMemcpyAsync(im.dst, base + pl[i - i0].dst, bytes, hipMemcpyDeviceToHost, st));
        }
    }
    HIPCHK(timer.stop(result->device_ms));
    HIPCHK(timer.spans(result->kernel_ms));
    result->num_batches = (uint32_t)nbatch;
    return AMC_OK;
}

}  // extern "C"
