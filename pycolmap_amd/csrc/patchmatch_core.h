// patchmatch_core.h — the arithmetic of PatchMatch stereo as host-and-device functions, shared by
// the kernels (patchmatch.hip) and the sequential reference (tests/patchmatch_ref/patchmatch_ref.cc) the way tri_core.h
// and ba_core.h are.  Everything is float32 in the written order (the build has -ffp-contract=off -fno-fast-math);
// exp and acos are the polynomials below on both sides, sqrt and the division are IEEE's correctly rounded ones.  The
// derived constants of a call (Params) are computed once on the host, in double with libm, by make_params.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PM_HD __host__ __device__ __forceinline__
#else
#define PM_HD inline
#endif

namespace pm {

constexpr int kMaxSources = 32;       // AMC_PATCHMATCH_MAX_SOURCES
constexpr int kMaxWindowRadius = 32;  // COLMAP's kMaxPatchMatchWindowRadius
constexpr int kNumHyps = 5;
constexpr float kMaxCost = 2.0f;
constexpr float kMinVar = 1e-5f;          // 22.3: a window with less weighted variance has no NCC
constexpr float kTransProb = 0.001f;      // 22.5: probability that the selection state changes between two pixels
constexpr float kFilterMinSelProb = 0.5f; // 22.7
constexpr float kSelProbLo = 0.01f, kSelProbHi = 0.99f;
constexpr uint32_t kSweepInit = 0xffffffffu;  // the `sweep` of the initialisation's draws

// what a call derives from its options (22.2); the same record on the device and in the reference
struct Params {
    int32_t half, step, side;  // window offsets (i - half) * step, i in [0, side)
    int32_t num_samples, geom, filter, filter_min_num;
    uint32_t seed;
    float inv_2ss, inv_2sc;    // 1 / (2 sigma_spatial^2), 1 / (2 sigma_color^2)
    float inv_2ncc, ncc_norm;  // 1 / (2 ncc_sigma^2), the density's normaliser on [0, 2]
    float inv_2inc;            // 1 / (2 incident_angle_sigma^2)
    float cos_min_tri, cos_filter_tri;
    float geom_reg, geom_max, filter_min_ncc, filter_geom_max;
};

struct Cam {
    float fx, fy, cx, cy;
};
struct View {
    const uint8_t* px;  // h x w grey bytes
    int32_t w, h;
    Cam k;
};
// a source relative to its reference: x_src = R x_ref + t; C is the source's centre in the reference's frame
struct Rel {
    float R[9], t[3], C[3];
};

// ---- random numbers (22.1): a stateless hash of (seed, image, row, column, sweep, draw) -------------------------------
PM_HD uint32_t mix(uint32_t h, uint32_t v) {
    h ^= v;
    h *= 0x9e3779b1u;
    h ^= h >> 15;
    h *= 0x85ebca77u;
    h ^= h >> 13;
    return h;
}
struct Rng {
    uint32_t base;  // the hash of everything but the draw index
    PM_HD float u(uint32_t draw) const {  // uniform in [0, 1), 24 bits
        uint32_t h = mix(base, draw);
        h ^= h >> 16;
        h *= 0x85ebca6bu;
        h ^= h >> 13;
        h *= 0xc2b2ae35u;
        h ^= h >> 16;
        return (float)(h >> 8) * (1.0f / 16777216.0f);
    }
};
PM_HD Rng rng_at(uint32_t seed, uint32_t image, uint32_t row, uint32_t col, uint32_t sweep) {
    Rng r;
    r.base = mix(mix(mix(mix(mix(0x811c9dc5u, seed), image), row), col), sweep);
    return r;
}

// ---- exp and acos (22.2) ----------------------------------------------------------------------------------------------
// exp(x) for x <= 0 (a positive x is taken as 0, NaN gives 0): x = k ln2 + r, |r| <= ln2 / 2, a degree-6 Taylor polynomial
// in Horner form, 2^k through the exponent bits.  Relative error under 3e-7.
PM_HD float exp_neg(float x) {
    if (!(x < 0.0f)) return x == x ? 1.0f : 0.0f;
    if (x < -87.0f) return 0.0f;
    const float kf = floorf(x * 1.44269504088896341f + 0.5f);
    const float r = (x - kf * 0.693145751953125f) - kf * 1.42860682030941723e-6f;
    float p = 1.0f / 720.0f;
    p = p * r + 1.0f / 120.0f;
    p = p * r + 1.0f / 24.0f;
    p = p * r + 1.0f / 6.0f;
    p = p * r + 0.5f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    const int32_t k = (int32_t)kf;  // in [-126, 0]
    union {
        uint32_t u;
        float f;
    } s;
    s.u = (uint32_t)(k + 127) << 23;
    return p * s.f;
}
// acos(x), x clamped to [-1, 1] (NaN gives 0): Abramowitz & Stegun 4.4.46, absolute error under 2e-8 before rounding
PM_HD float acos_poly(float x) {
    if (!(x == x)) return 0.0f;
    const float a = fminf(fabsf(x), 1.0f);
    float p = -0.0012624911f;
    p = p * a + 0.0066700901f;
    p = p * a + -0.0170881256f;
    p = p * a + 0.0308918810f;
    p = p * a + -0.0501743046f;
    p = p * a + 0.0889789874f;
    p = p * a + -0.2145988016f;
    p = p * a + 1.5707963050f;
    const float r = sqrtf(1.0f - a) * p;
    return x < 0.0f ? 3.14159265358979f - r : r;
}

// ---- geometry -----------------------------------------------------------------------------------------------------------
// the ray of pixel (row, col) with z = 1: pixel centres lie at + 0.5 (COLMAP's convention)
PM_HD void pixel_ray(const Cam& k, int row, int col, float ray[3]) {
    ray[0] = ((float)col + 0.5f - k.cx) / k.fx;
    ray[1] = ((float)row + 0.5f - k.cy) / k.fy;
    ray[2] = 1.0f;
}
PM_HD float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// n scaled to unit length and turned to face the camera along `ray`; false when it has no direction
PM_HD bool face_camera(const float ray[3], float n[3]) {
    const float len = sqrtf(dot3(n, n));
    if (!(len > 1e-12f) || !(len < 1e30f)) return false;
    n[0] /= len;
    n[1] /= len;
    n[2] /= len;
    if (dot3(n, ray) > 0.0f) {
        n[0] = -n[0];
        n[1] = -n[1];
        n[2] = -n[2];
    }
    return true;
}

// 22.4 the random hypothesis: draws d0 .. d0 + 16.  Marsaglia's rejection, at most 8 rounds, then (0, 0, -1).
PM_HD void random_hyp(const Rng& g, uint32_t d0, const float ray[3], float dmin, float dmax, float& depth, float n[3]) {
    depth = dmin + g.u(d0) * (dmax - dmin);
    n[0] = 0.0f;
    n[1] = 0.0f;
    n[2] = -1.0f;
    for (uint32_t k = 0; k < 8; ++k) {
        const float v1 = 2.0f * g.u(d0 + 1 + 2 * k) - 1.0f, v2 = 2.0f * g.u(d0 + 2 + 2 * k) - 1.0f;
        const float s = v1 * v1 + v2 * v2;
        if (s < 1.0f) {
            const float q = sqrtf(1.0f - s);
            n[0] = 2.0f * v1 * q;
            n[1] = 2.0f * v2 * q;
            n[2] = 1.0f - 2.0f * s;
            break;
        }
    }
    if (!face_camera(ray, n)) {
        n[0] = 0.0f;
        n[1] = 0.0f;
        n[2] = -1.0f;
    }
}

// 22.4 the depth at pixel (row, col) of the plane through the predecessor's point with its normal; the caller checks
// the range
PM_HD float propagate_depth(const Cam& k, int prow, int pcol, float pdepth, const float pn[3], int row, int col) {
    float rp[3], r[3];
    pixel_ray(k, prow, pcol, rp);
    pixel_ray(k, row, col, r);
    const float num = pdepth * dot3(pn, rp);
    const float den = dot3(pn, r);
    return num / den;
}

// ---- the reference window (22.3) ------------------------------------------------------------------------------------
PM_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
PM_HD float pixel_value(const View& v, int row, int col) { return (float)v.px[(size_t)row * (size_t)v.w + (size_t)col] / 255.0f; }

// sample i of the window at (row, col): the clamped pixel's position, value and bilateral weight
PM_HD void window_sample(const Params& p, const View& ref, int row, int col, int i, float& x, float& y, float& val, float& wgt) {
    const int dr = (i / p.side - p.half) * p.step, dc = (i % p.side - p.half) * p.step;
    const int rr = clampi(row + dr, 0, ref.h - 1), cc = clampi(col + dc, 0, ref.w - 1);
    val = pixel_value(ref, rr, cc);
    const float dv = val - pixel_value(ref, row, col);
    const float d2 = (float)(dr * dr + dc * dc);
    wgt = exp_neg(-(d2 * p.inv_2ss) - (dv * dv) * p.inv_2sc);
    x = (float)cc + 0.5f;
    y = (float)rr + 0.5f;
}
// the window recomputed per sample (the reference, and the kernels that take a lane per pixel)
struct DirectWindow {
    const Params* p;
    const View* ref;
    int row, col;
    PM_HD void get(int i, float& x, float& y, float& val, float& wgt) const { window_sample(*p, *ref, row, col, i, x, y, val, wgt); }
};

// ---- the cost of a hypothesis in a source (22.3): 1 - bilaterally weighted NCC, in [0, 2] -----------------------------
template <class Window>
PM_HD float ncc_cost(const Params& p, const Cam& kr, const View& src, const Rel& rel, int row, int col, float depth,
                     const float n[3], const Window& win) {
    if (src.w < 2 || src.h < 2) return kMaxCost;
    float ray[3];
    pixel_ray(kr, row, col, ray);
    const float delta = depth * dot3(n, ray);  // n^T X
    if (!(fabsf(delta) > 1e-20f) || !(fabsf(delta) < 1e20f)) return kMaxCost;
    const float m[3] = {n[0] / delta, n[1] / delta, n[2] / delta};
    float A[9];  // R + t n^T / (n^T X)
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[3 * i + j] = rel.R[3 * i + j] + rel.t[i] * m[j];
    float sw = 0.0f, sr = 0.0f, ss = 0.0f, srr = 0.0f, sss = 0.0f, srs = 0.0f;
    const int count = p.side * p.side;
    for (int i = 0; i < count; ++i) {
        float x, y, r, w;
        win.get(i, x, y, r, w);
        const float qx = (x - kr.cx) / kr.fx, qy = (y - kr.cy) / kr.fy;
        const float px = (A[0] * qx + A[1] * qy) + A[2];
        const float py = (A[3] * qx + A[4] * qy) + A[5];
        const float pz = (A[6] * qx + A[7] * qy) + A[8];
        if (!(pz > 1e-6f)) return kMaxCost;
        const float u = src.k.fx * (px / pz) + src.k.cx - 0.5f;
        const float v = src.k.fy * (py / pz) + src.k.cy - 0.5f;
        if (!(u >= 0.0f && u <= (float)(src.w - 1) && v >= 0.0f && v <= (float)(src.h - 1))) return kMaxCost;
        int x0 = (int)floorf(u), y0 = (int)floorf(v);
        if (x0 > src.w - 2) x0 = src.w - 2;
        if (y0 > src.h - 2) y0 = src.h - 2;
        const float a = u - (float)x0, b = v - (float)y0;
        const float top = pixel_value(src, y0, x0) * (1.0f - a) + pixel_value(src, y0, x0 + 1) * a;
        const float bot = pixel_value(src, y0 + 1, x0) * (1.0f - a) + pixel_value(src, y0 + 1, x0 + 1) * a;
        const float s = top * (1.0f - b) + bot * b;
        sw += w;
        sr += w * r;
        ss += w * s;
        srr += w * (r * r);
        sss += w * (s * s);
        srs += w * (r * s);
    }
    if (!(sw > 0.0f)) return kMaxCost;
    const float mr = sr / sw, ms = ss / sw;
    const float vr = srr / sw - mr * mr, vs = sss / sw - ms * ms;
    if (!(vr >= kMinVar) || !(vs >= kMinVar)) return kMaxCost;
    const float cov = srs / sw - mr * ms;
    const float c = 1.0f - cov / sqrtf(vr * vs);
    if (!(c == c)) return kMaxCost;
    return c < 0.0f ? 0.0f : (c > kMaxCost ? kMaxCost : c);
}

// ---- the forward-backward reprojection error (22.6), in pixels; `big` when the path leaves an image or meets no depth -----
PM_HD float fb_error(const Cam& kr, const Cam& ks, int sw, int sh, const float* sdepth, const Rel& rel, int row, int col, float depth,
                     float big) {
    float ray[3];
    pixel_ray(kr, row, col, ray);
    const float X[3] = {depth * ray[0], depth * ray[1], depth};
    const float xs = dot3(rel.R, X) + rel.t[0], ys = dot3(rel.R + 3, X) + rel.t[1], zs = dot3(rel.R + 6, X) + rel.t[2];
    if (!(zs > 1e-6f)) return big;
    const float u = ks.fx * (xs / zs) + ks.cx, v = ks.fy * (ys / zs) + ks.cy;
    if (!(u >= 0.0f && u < (float)sw && v >= 0.0f && v < (float)sh)) return big;
    const int iu = clampi((int)floorf(u), 0, sw - 1), iv = clampi((int)floorf(v), 0, sh - 1);
    const float ds = sdepth[(size_t)iv * (size_t)sw + (size_t)iu];
    if (!(ds > 0.0f) || !(ds < 1e30f)) return big;
    const float Y[3] = {ds * ((u - ks.cx) / ks.fx) - rel.t[0], ds * ((v - ks.cy) / ks.fy) - rel.t[1], ds - rel.t[2]};
    // R^T (X_s - t)
    const float bx = (rel.R[0] * Y[0] + rel.R[3] * Y[1]) + rel.R[6] * Y[2];
    const float by = (rel.R[1] * Y[0] + rel.R[4] * Y[1]) + rel.R[7] * Y[2];
    const float bz = (rel.R[2] * Y[0] + rel.R[5] * Y[1]) + rel.R[8] * Y[2];
    if (!(bz > 1e-6f)) return big;
    const float du = (kr.fx * (bx / bz) + kr.cx) - ((float)col + 0.5f), dv = (kr.fy * (by / bz) + kr.cy) - ((float)row + 0.5f);
    const float e = sqrtf(du * du + dv * dv);
    return e <= big ? e : big;  // (NaN gives big)
}

// cosine of the triangulation angle at X between the reference's centre (the origin) and the source's centre C; 1 (no
// angle) where it is not defined
PM_HD float cos_tri_angle(const float X[3], const float C[3]) {
    const float b[3] = {X[0] - C[0], X[1] - C[1], X[2] - C[2]};
    const float den = sqrtf(dot3(X, X) * dot3(b, b));
    if (!(den > 1e-30f) || !(den < 1e30f)) return 1.0f;
    const float c = dot3(X, b) / den;
    return c == c ? c : 1.0f;
}

// ---- view selection (22.5), the part of one source: the forward message and the selection probability are updated, the
// weight the source is drawn with is returned (finite, >= 0) -------------------------------------------------------------
PM_HD float source_weight(const Params& p, float cost0, const float X[3], const float n[3], const float C[3], float& fwd, float& sel) {
    const float like = exp_neg(-(cost0 * cost0) * p.inv_2ncc) * p.ncc_norm;
    const float as = like * (fwd * (1.0f - kTransProb) + (1.0f - fwd) * kTransProb);
    const float au = 0.5f * ((1.0f - fwd) * (1.0f - kTransProb) + fwd * kTransProb);
    float a = as / (as + au);
    if (!(a >= 0.0f && a <= 1.0f)) a = 0.5f;
    fwd = a;
    const float q = sel;  // the previous sweep's probability as the backward term
    float z = (a * q) / (a * q + (1.0f - a) * (1.0f - q));
    if (!(z >= 0.0f && z <= 1.0f)) z = 0.5f;
    z = z < kSelProbLo ? kSelProbLo : (z > kSelProbHi ? kSelProbHi : z);
    sel = z;
    // the triangulation-angle prior: 1 from min_triangulation_angle on, below it (1 - cos) / (1 - cos min), at least 0.01
    const float ct = cos_tri_angle(X, C);
    float tri = 1.0f;
    if (ct > p.cos_min_tri) {
        tri = (1.0f - ct) / (1.0f - p.cos_min_tri);
        if (!(tri >= 0.01f)) tri = 0.01f;
        if (tri > 1.0f) tri = 1.0f;
    }
    // the incident-angle prior: the angle between the normal and the direction from the point to the source
    const float d[3] = {C[0] - X[0], C[1] - X[1], C[2] - X[2]};
    const float len = sqrtf(dot3(d, d));
    float inc = 1.0f;
    if (len > 1e-30f && len < 1e30f) {
        const float ang = acos_poly(dot3(n, d) / len);
        inc = exp_neg(-(ang * ang) * p.inv_2inc);
    }
    const float w = (z * tri) * inc;
    return (w >= 0.0f && w < 1e30f) ? w : 0.0f;
}

// 22.5 the draws and the arg-min: `wgt` S weights, `cost` and `geo` kNumHyps x S (hypothesis-major; geo is read only in
// the geometric pass).  Draws d0 .. d0 + num_samples; a hypothesis sums the costs of the drawn sources in draw order.
// Returns the winning hypothesis, ties to the lowest index.
PM_HD int pick_hypothesis(const Params& p, int S, const float* wgt, const float* cost, const float* geo, const Rng& g, uint32_t d0) {
    float total = 0.0f;
    for (int s = 0; s < S; ++s) total += wgt[s];
    const bool uniform = !(total > 0.0f) || !(total < 1e30f);
    if (uniform) total = (float)S;
    float sum[kNumHyps];
    for (int h = 0; h < kNumHyps; ++h) sum[h] = 0.0f;
    for (int j = 0; j < p.num_samples; ++j) {
        const float target = g.u(d0 + (uint32_t)j) * total;
        float cdf = 0.0f;
        int sel = S - 1;
        for (int s = 0; s < S; ++s) {
            cdf += uniform ? 1.0f : wgt[s];
            if (cdf > target) {
                sel = s;
                break;
            }
        }
        for (int h = 0; h < kNumHyps; ++h) {
            float c = cost[h * S + sel];
            if (p.geom) c = c + p.geom_reg * geo[h * S + sel];
            sum[h] += c;
        }
    }
    int best = 0;
    for (int h = 1; h < kNumHyps; ++h)
        if (sum[h] / (float)p.num_samples < sum[best] / (float)p.num_samples) best = h;
    return best;
}

// 22.4 the five hypotheses of a pixel.  prev: the predecessor on the line (has_prev), already updated in this sweep.
struct Hyps {
    float depth[kNumHyps];
    float n[kNumHyps][3];
};
PM_HD void make_hyps(const Cam& k, const Rng& g, int iter, float dmin, float dmax, int row, int col, float depth, const float n[3],
                     bool has_prev, int prow, int pcol, float pdepth, const float pn[3], Hyps& H) {
    float ray[3];
    pixel_ray(k, row, col, ray);
    for (int h = 0; h < kNumHyps; ++h) {
        H.depth[h] = depth;
        H.n[h][0] = n[0];
        H.n[h][1] = n[1];
        H.n[h][2] = n[2];
    }
    if (has_prev) {  // 1: the predecessor's plane met by this pixel's ray
        const float d = propagate_depth(k, prow, pcol, pdepth, pn, row, col);
        if (d >= dmin && d <= dmax) {
            float m[3] = {pn[0], pn[1], pn[2]};
            if (face_camera(ray, m)) {
                H.depth[1] = d;
                H.n[1][0] = m[0];
                H.n[1][1] = m[1];
                H.n[1][2] = m[2];
            }
        }
    }
    random_hyp(g, 0, ray, dmin, dmax, H.depth[2], H.n[2]);  // 2: draws 0 .. 16
    float pert = 0.5f;  // halves with every iteration
    for (int i = 0; i < iter && i < 30; ++i) pert *= 0.5f;
    {  // 3: the current depth, a perturbed normal (draws 17 .. 19)
        float m[3] = {n[0] + pert * (2.0f * g.u(17) - 1.0f), n[1] + pert * (2.0f * g.u(18) - 1.0f), n[2] + pert * (2.0f * g.u(19) - 1.0f)};
        if (face_camera(ray, m)) {
            H.n[3][0] = m[0];
            H.n[3][1] = m[1];
            H.n[3][2] = m[2];
        }
    }
    {  // 4: a perturbed depth (draw 20), the current normal
        float d = depth * (1.0f + pert * (2.0f * g.u(20) - 1.0f));
        d = d < dmin ? dmin : (d > dmax ? dmax : d);
        if (d == d) H.depth[4] = d;
    }
}
constexpr uint32_t kDrawSamples = 32;  // the view-selection draws start here

// ---- host only: the derived constants of a call (double, libm) ---------------------------------------------------------
struct Options {  // the fields of amc_patch_match_opts that the arithmetic reads
    int window_radius, window_step, num_samples, geom, filter, filter_min_num;
    double sigma_spatial, sigma_color, ncc_sigma, min_tri_deg, incident_sigma, geom_reg, geom_max, filter_min_ncc,
        filter_min_tri_deg, filter_geom_max;
    uint32_t seed;
};
inline Params make_params(const Options& o) {
    Params p;
    p.step = o.window_step;
    p.half = o.window_radius / o.window_step;
    p.side = 2 * p.half + 1;
    p.num_samples = o.num_samples;
    p.geom = o.geom ? 1 : 0;
    p.filter = o.filter ? 1 : 0;
    p.filter_min_num = o.filter_min_num;
    p.seed = o.seed;
    const double ss = o.sigma_spatial > 0.0 ? o.sigma_spatial : (double)o.window_radius;  // COLMAP: <= 0 means the radius
    p.inv_2ss = (float)(1.0 / (2.0 * ss * ss));
    p.inv_2sc = (float)(1.0 / (2.0 * o.sigma_color * o.sigma_color));
    p.inv_2ncc = (float)(1.0 / (2.0 * o.ncc_sigma * o.ncc_sigma));
    p.ncc_norm = (float)(1.0 / (o.ncc_sigma * sqrt(1.57079632679489661923) * erf(2.0 / (o.ncc_sigma * 1.41421356237309504880))));
    p.inv_2inc = (float)(1.0 / (2.0 * o.incident_sigma * o.incident_sigma));
    const double rad = 0.0174532925199432957692;
    p.cos_min_tri = (float)cos(o.min_tri_deg * rad);
    p.cos_filter_tri = (float)cos(o.filter_min_tri_deg * rad);
    p.geom_reg = (float)o.geom_reg;
    p.geom_max = (float)o.geom_max;
    p.filter_min_ncc = (float)o.filter_min_ncc;
    p.filter_geom_max = (float)o.filter_geom_max;
    return p;
}
// a source relative to its reference from the two world-to-camera poses (row-major R, t), in double, rounded once
inline Rel make_rel(const double* Rr, const double* tr, const double* Rs, const double* ts) {
    double R[9], t[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = Rs[3 * i] * Rr[3 * j] + Rs[3 * i + 1] * Rr[3 * j + 1] + Rs[3 * i + 2] * Rr[3 * j + 2];
    for (int i = 0; i < 3; ++i) t[i] = ts[i] - (R[3 * i] * tr[0] + R[3 * i + 1] * tr[1] + R[3 * i + 2] * tr[2]);
    Rel rel;
    for (int i = 0; i < 9; ++i) rel.R[i] = (float)R[i];
    for (int i = 0; i < 3; ++i) {
        rel.t[i] = (float)t[i];
        rel.C[i] = (float)-(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
    }
    return rel;
}

}  // namespace pm
