// sift.hip — SIFT feature extraction on gfx950 (include/amc_sift.h): VLFeat's SIFT as COLMAP's CPU extractor drives
// it, restated in DESIGN.md section 10.  Every float32 operation below is written in the order of
// tests/sift_ref/sift_ref.cc, the CPU reference it is bit-identical to; the transcendentals are the project's own
// definitions (+ - * /, correctly rounded sqrtf and a host-built table), and sums that cross lanes use the D3 rule:
// each lane sums a fixed strided subset of the window in order, then a fixed butterfly sums the lanes.  No atomics.
//
// Per octave: the base level (the input at first_octave, or the previous octave's level octave_resolution taken at
// every other pixel), then each level blurred from the one before (separable, replicated borders; the DoG is the
// vertical pass's epilogue); detection and refinement per pixel, counted per (level, row) and written at the rows'
// prefix sums so that the keypoints come out in (level, y, x) order; one wave per keypoint for the orientation
// histogram, one wave per (keypoint, orientation) for the descriptor.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "amc_internal.h"
#include "../../include/amc_sift.h"

using namespace amc;

namespace {

constexpr float kPi = 3.14159265358979323846f;
constexpr float kTwoPi = 6.28318530717958647692f;
constexpr int kWave = 64;
constexpr int kExpnSize = 258;  // exp(-k * 25 / 256), k = 0 .. 257
constexpr int kDetectThreads = 256;

struct Kp {
    float x, y, sn, sigma;  // octave coordinates, refined level, sigma in octave pixels
    int o, d;               // octave, DoG level of detection
};

// ---- the project's transcendental definitions ------------------------------------------
__device__ __forceinline__ float fast_expn(const float* __restrict__ tab, float x) {
    if (x > 25.0f) return 0.0f;
    x = x * 10.24f;
    const int i = (int)floorf(x);
    const float r = x - (float)i;
    const float a = tab[i], b = tab[i + 1];
    return a + r * (b - a);
}

__device__ __forceinline__ float fast_atan2(float y, float x) {
    const float c3 = 0.1821f, c1 = 0.9675f;
    const float abs_y = fabsf(y) + 1.19209290e-07f;
    float r, angle;
    if (x >= 0.0f) {
        r = (x - abs_y) / (x + abs_y);
        angle = 0.785398163397448309616f;
    } else {
        r = (x + abs_y) / (abs_y - x);
        angle = 2.356194490192344928847f;
    }
    angle += (c3 * r * r - c1) * r;
    return (y < 0.0f) ? -angle : angle;
}

__device__ __forceinline__ float mod_2pi(float x) {
    while (x > kTwoPi) x -= kTwoPi;
    while (x < 0.0f) x += kTwoPi;
    return x;
}

__device__ __forceinline__ float pow2f(float t) {
    const float n = floorf(t);
    const float u = (t - n) * 0.693147180559945309f;
    float p = 1.0f + u * (1.0f + u * ((float)(1.0 / 2) + u * ((float)(1.0 / 6) + u * ((float)(1.0 / 24) +
              u * ((float)(1.0 / 120) + u * ((float)(1.0 / 720) + u * ((float)(1.0 / 5040) + u * ((float)(1.0 / 40320) +
              u * ((float)(1.0 / 362880) + u * (float)(1.0 / 3628800))))))))));
    for (int k = (int)n; k > 0; --k) p *= 2.0f;
    for (int k = (int)n; k < 0; ++k) p *= 0.5f;
    return p;
}

__device__ __forceinline__ void fast_sincos(float th, float* s, float* c) {
    const float t = (th > kPi) ? th - kTwoPi : th;
    const float t2 = t * t;
    *s = t * (1.0f + t2 * ((float)(-1.0 / 6) + t2 * ((float)(1.0 / 120) + t2 * ((float)(-1.0 / 5040) +
         t2 * ((float)(1.0 / 362880) + t2 * ((float)(-1.0 / 39916800) + t2 * ((float)(1.0 / 6227020800.0) +
         t2 * ((float)(-1.0 / 1307674368000.0) + t2 * ((float)(1.0 / 355687428096000.0) +
         t2 * (float)(-1.0 / 121645100408832000.0))))))))));
    *c = 1.0f + t2 * ((float)(-1.0 / 2) + t2 * ((float)(1.0 / 24) + t2 * ((float)(-1.0 / 720) +
         t2 * ((float)(1.0 / 40320) + t2 * ((float)(-1.0 / 3628800) + t2 * ((float)(1.0 / 479001600) +
         t2 * ((float)(-1.0 / 87178291200.0) + t2 * ((float)(1.0 / 20922789888000.0) +
         t2 * (float)(-1.0 / 6402373705728000.0)))))))));
}

// ---- scale space ------------------------------------------------------------------------------------------------
// The octave's base: v / 255 of the input at first_octave (x2 bilinear upsampling for -1, every 2^o-th pixel for o > 0)
__global__ void k_base(const uint8_t* __restrict__ src, int w, int h, long pitch, int o, float* __restrict__ dst, int wo,
                       int ho) {
    const int X = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y;
    if (X >= wo || Y >= ho) return;
    float v;
    if (o == -1) {
        const int x = X >> 1, y = Y >> 1, x1 = min(x + 1, w - 1), y1 = min(y + 1, h - 1);
        const float a = (float)src[(size_t)y * pitch + x] / 255.0f;
        const float b = (float)src[(size_t)y * pitch + x1] / 255.0f;
        const float c = (float)src[(size_t)y1 * pitch + x] / 255.0f;
        const float d = (float)src[(size_t)y1 * pitch + x1] / 255.0f;
        if (!(X & 1) && !(Y & 1)) v = a;
        else if (!(Y & 1)) v = 0.5f * (a + b);
        else if (!(X & 1)) v = 0.5f * (a + c);
        else v = 0.25f * (a + b + c + d);
    } else {
        v = (float)src[(size_t)(Y << o) * pitch + (X << o)] / 255.0f;
    }
    dst[(size_t)Y * wo + X] = v;
}

// the next octave's base: the previous octave's level S at every other pixel
__global__ void k_down(const float* __restrict__ in, int wi, float* __restrict__ out, int wo, int ho) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= wo || y >= ho) return;
    out[(size_t)y * wo + x] = in[(size_t)(2 * y) * wi + 2 * x];
}

// Horizontal pass: a row segment and its 2W-pixel apron through LDS (replicated borders), taps in order
constexpr int kBlurTile = 256;
__global__ void __launch_bounds__(kBlurTile) k_hblur(const float* __restrict__ in, float* __restrict__ out, int w, int h,
                                                     const float* __restrict__ taps, int W) {
    extern __shared__ float row[];  // kBlurTile + 2W
    const int y = blockIdx.y, x0 = blockIdx.x * kBlurTile;
    const float* src = in + (size_t)y * w;
    for (int i = threadIdx.x; i < kBlurTile + 2 * W; i += kBlurTile) row[i] = src[min(max(x0 - W + i, 0), w - 1)];
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= w) return;
    float acc = 0.0f;
    for (int k = 0; k <= 2 * W; ++k) acc += taps[k] * row[threadIdx.x + k];
    out[(size_t)y * w + x] = acc;
}

// Vertical pass (a column strip of 64 pixels x 16 rows and its apron through LDS) with the DoG in the epilogue:
// dog = level - prev
constexpr int kVbx = 64, kVby = 16;
__global__ void __launch_bounds__(kVbx * 4) k_vblur(const float* __restrict__ in, float* __restrict__ out,
                                                    const float* __restrict__ prev, float* __restrict__ dog, int w, int h,
                                                    const float* __restrict__ taps, int W) {
    extern __shared__ float col[];  // (kVby + 2W) x kVbx
    const int x0 = blockIdx.x * kVbx, y0 = blockIdx.y * kVby;
    const int tx = threadIdx.x % kVbx, ty = threadIdx.x / kVbx;
    const int x = min(x0 + tx, w - 1);
    for (int r = ty; r < kVby + 2 * W; r += 4) col[r * kVbx + tx] = in[(size_t)min(max(y0 - W + r, 0), h - 1) * w + x];
    __syncthreads();
    if (x0 + tx >= w) return;
    for (int r = ty; r < kVby; r += 4) {
        const int y = y0 + r;
        if (y >= h) break;
        float acc = 0.0f;
        for (int k = 0; k <= 2 * W; ++k) acc += taps[k] * col[(r + k) * kVbx + tx];
        const size_t i = (size_t)y * w + x0 + tx;
        out[i] = acc;
        if (dog) dog[i] = acc - prev[i];
    }
}

// ---- detection ------------------------------------------------------------------------------------------------
__device__ void solve3(float A[3][3], float b[3]) {
    for (int j = 0; j < 3; ++j) {
        float maxa = 0.0f, maxabsa = 0.0f;
        int maxi = -1;
        for (int i = j; i < 3; ++i) {
            const float a = A[i][j], absa = fabsf(a);
            if (absa > maxabsa) {
                maxa = a;
                maxabsa = absa;
                maxi = i;
            }
        }
        if (maxabsa < 1e-10f) {
            b[0] = b[1] = b[2] = 0.0f;
            return;
        }
        const int i = maxi;
        for (int jj = j; jj < 3; ++jj) {
            const float t = A[i][jj];
            A[i][jj] = A[j][jj];
            A[j][jj] = t;
        }
        const float tb = b[i];
        b[i] = b[j];
        b[j] = tb;
        for (int jj = j; jj < 3; ++jj) A[j][jj] = A[j][jj] / maxa;
        b[j] = b[j] / maxa;
        for (int ii = j + 1; ii < 3; ++ii) {
            const float x = A[ii][j];
            for (int jj = j; jj < 3; ++jj) A[ii][jj] = A[ii][jj] - x * A[j][jj];
            b[ii] = b[ii] - x * b[j];
        }
    }
    for (int i = 2; i >= 0; --i) {
        float x = b[i];
        for (int ii = i + 1; ii < 3; ++ii) x = x - A[i][ii] * b[ii];
        b[i] = x;
    }
}

struct DetectParams {
    int w, h, S, o;
    float tp, te, sigma0;
};

// The extremum test at (x0, y0) of DoG level d, then refinement; true and *out for a kept keypoint
__device__ bool detect_at(const float* __restrict__ dog, const DetectParams& P, int d, int x0, int y0, Kp* out) {
    const size_t plane = (size_t)P.w * P.h;
    const float* D = dog + (size_t)d * plane;
    const float v = D[(size_t)y0 * P.w + x0];
    bool mx = v >= 0.8f * P.tp, mn = v <= -0.8f * P.tp;
    if (!mx && !mn) return false;
    for (int ds = -1; ds <= 1; ++ds)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (!ds && !dy && !dx) continue;
                const float u = D[(long)ds * (long)plane + (long)(y0 + dy) * P.w + (x0 + dx)];
                mx = mx && v > u;
                mn = mn && v < u;
            }
    if (!mx && !mn) return false;
    int x = x0, y = y0;
    auto at = [&](int dx, int dy, int ds) { return D[(long)ds * (long)plane + (long)(y + dy) * P.w + (x + dx)]; };
    float b[3] = {0, 0, 0}, Dx = 0, Dy = 0, Ds = 0, Dxx = 0, Dyy = 0, Dxy = 0;
    for (int it = 0; it < 5; ++it) {
        Dx = 0.5f * (at(1, 0, 0) - at(-1, 0, 0));
        Dy = 0.5f * (at(0, 1, 0) - at(0, -1, 0));
        Ds = 0.5f * (at(0, 0, 1) - at(0, 0, -1));
        Dxx = at(1, 0, 0) + at(-1, 0, 0) - 2.0f * at(0, 0, 0);
        Dyy = at(0, 1, 0) + at(0, -1, 0) - 2.0f * at(0, 0, 0);
        const float Dss = at(0, 0, 1) + at(0, 0, -1) - 2.0f * at(0, 0, 0);
        Dxy = 0.25f * (at(1, 1, 0) + at(-1, -1, 0) - at(-1, 1, 0) - at(1, -1, 0));
        const float Dxs = 0.25f * (at(1, 0, 1) + at(-1, 0, -1) - at(-1, 0, 1) - at(1, 0, -1));
        const float Dys = 0.25f * (at(0, 1, 1) + at(0, -1, -1) - at(0, -1, 1) - at(0, 1, -1));
        float A[3][3] = {{Dxx, Dxy, Dxs}, {Dxy, Dyy, Dys}, {Dxs, Dys, Dss}};
        b[0] = -Dx;
        b[1] = -Dy;
        b[2] = -Ds;
        solve3(A, b);
        const int mvx = ((b[0] > 0.6f && x < P.w - 2) ? 1 : 0) + ((b[0] < -0.6f && x > 1) ? -1 : 0);
        const int mvy = ((b[1] > 0.6f && y < P.h - 2) ? 1 : 0) + ((b[1] < -0.6f && y > 1) ? -1 : 0);
        if (mvx == 0 && mvy == 0) break;
        x += mvx;
        y += mvy;
    }
    const float val = at(0, 0, 0) + 0.5f * (Dx * b[0] + Dy * b[1] + Ds * b[2]);
    const float score = (Dxx + Dyy) * (Dxx + Dyy) / (Dxx * Dyy - Dxy * Dxy);
    const float xn = (float)x + b[0], yn = (float)y + b[1], sn = (float)(d - 1) + b[2];
    const float te = P.te;
    const bool good = fabsf(val) > P.tp && score < (te + 1.0f) * (te + 1.0f) / te && score >= 0.0f &&
                      fabsf(b[0]) < 1.5f && fabsf(b[1]) < 1.5f && fabsf(b[2]) < 1.5f && xn >= 0.0f &&
                      xn <= (float)(P.w - 1) && yn >= 0.0f && yn <= (float)(P.h - 1) && sn >= -1.0f &&
                      sn <= (float)(P.S + 1);
    if (!good) return false;
    *out = Kp{xn, yn, sn, P.sigma0 * pow2f(sn / (float)P.S), P.o, d};
    return true;
}

// One block per (DoG level d = 1 .. S, row y = 1 .. h - 2).  Pass 1 (row_off == nullptr): the row's keypoint count.
// Pass 2: the row's keypoints at row_off[row], in x order (a block prefix sum per chunk of 256 pixels).
__global__ void __launch_bounds__(kDetectThreads) k_detect(const float* __restrict__ dog, DetectParams P,
                                                           int* __restrict__ row_cnt, const int* __restrict__ row_off,
                                                           Kp* __restrict__ kps) {
    __shared__ int scan[kDetectThreads];
    const int y0 = blockIdx.x + 1, d = blockIdx.y + 1;
    const int row = blockIdx.y * (P.h - 2) + blockIdx.x;
    const int t = threadIdx.x;
    int base = row_off ? row_off[row] : 0, mine = 0;
    for (int c = 1; c < P.w - 1; c += kDetectThreads) {
        const int x0 = c + t;
        Kp k;
        const bool hit = x0 < P.w - 1 && detect_at(dog, P, d, x0, y0, &k);
        if (!row_off) {
            mine += hit ? 1 : 0;
            continue;
        }
        scan[t] = hit ? 1 : 0;
        __syncthreads();
        for (int off = 1; off < kDetectThreads; off *= 2) {  // inclusive Hillis-Steele scan
            const int add = t >= off ? scan[t - off] : 0;
            __syncthreads();
            scan[t] += add;
            __syncthreads();
        }
        if (hit) kps[base + scan[t] - 1] = k;
        base += scan[kDetectThreads - 1];
        __syncthreads();
    }
    if (!row_off) {
        scan[t] = mine;
        __syncthreads();
        for (int s = kDetectThreads / 2; s > 0; s /= 2) {
            if (t < s) scan[t] += scan[t + s];
            __syncthreads();
        }
        if (t == 0) row_cnt[row] = scan[0];
    }
}

// ---- orientation and descriptor -----------------------------------------------------------------------------------
__device__ __forceinline__ void gradient(const float* __restrict__ G, int w, int h, int x, int y, float* mod, float* ang) {
    const float* r = G + (size_t)y * w;
    const float gx = (x == 0) ? r[1] - r[0] : (x == w - 1) ? r[x] - r[x - 1] : 0.5f * (r[x + 1] - r[x - 1]);
    const float gy = (y == 0) ? G[(size_t)w + x] - G[x]
                   : (y == h - 1) ? r[x] - G[(size_t)(y - 1) * w + x]
                                  : 0.5f * (G[(size_t)(y + 1) * w + x] - G[(size_t)(y - 1) * w + x]);
    *mod = sqrtf(gx * gx + gy * gy);
    *ang = mod_2pi(fast_atan2(gy, gx) + kTwoPi);
}

__device__ __forceinline__ float wave_butterfly(float v) {
    for (int o = kWave / 2; o >= 1; o /= 2) v = v + __shfl_xor(v, o, kWave);
    return v;
}

// One wave per keypoint: 36-bin histogram (lane-private partial sums in LDS, butterfly), six circular box
// smoothings, up to min(4, max_orient) peaks in bin order
__global__ void __launch_bounds__(kWave) k_orient(const Kp* __restrict__ kps, const float* __restrict__ G, int w, int h,
                                                  const float* __restrict__ tab, int max_orient,
                                                  float* __restrict__ angles, int* __restrict__ nang) {
    __shared__ float part[36 * kWave];
    __shared__ float hist[36];
    const Kp k = kps[blockIdx.x];
    const int l = threadIdx.x;
    const float* L = G + (size_t)k.d * w * h;
    const int xi = (int)(k.x + 0.5f), yi = (int)(k.y + 0.5f);
    if (xi < 0 || xi > w - 1 || yi < 0 || yi > h - 1) {
        if (l == 0) nang[blockIdx.x] = 0;
        return;
    }
    for (int b = 0; b < 36; ++b) part[b * kWave + l] = 0.0f;
    const float sigmaw = 1.5f * k.sigma;
    const int W = max((int)floorf(3.0f * sigmaw), 1);
    const int ys0 = max(-W, -yi), ys1 = min(W, h - 1 - yi);
    const int xs0 = max(-W, -xi), xs1 = min(W, w - 1 - xi);
    const int nx = xs1 - xs0 + 1, n = nx * (ys1 - ys0 + 1);
    for (int p = l; p < n; p += kWave) {
        const int ys = ys0 + p / nx, xs = xs0 + p % nx;
        const float dx = (float)(xi + xs) - k.x, dy = (float)(yi + ys) - k.y;
        const float r2 = dx * dx + dy * dy;
        if (r2 >= (float)(W * W) + 0.6f) continue;
        const float wgt = fast_expn(tab, r2 / (2.0f * sigmaw * sigmaw));
        float mod, ang;
        gradient(L, w, h, xi + xs, yi + ys, &mod, &ang);
        const float fbin = 36.0f * ang / kTwoPi;
        const int bin = (int)floorf(fbin - 0.5f);
        const float rbin = fbin - (float)bin - 0.5f;
        part[((bin + 36) % 36) * kWave + l] += (1.0f - rbin) * mod * wgt;
        part[((bin + 1) % 36) * kWave + l] += rbin * mod * wgt;
    }
    for (int b = 0; b < 36; ++b) {
        const float s = wave_butterfly(part[b * kWave + l]);
        if (l == 0) hist[b] = s;
    }
    if (l != 0) return;
    for (int it = 0; it < 6; ++it) {
        float prev = hist[35];
        const float first = hist[0];
        for (int i = 0; i < 35; ++i) {
            const float nh = (prev + hist[i] + hist[i + 1]) / 3.0f;
            prev = hist[i];
            hist[i] = nh;
        }
        hist[35] = (prev + hist[35] + first) / 3.0f;
    }
    float maxh = hist[0];
    for (int i = 1; i < 36; ++i) maxh = fmaxf(maxh, hist[i]);
    int na = 0;
    for (int i = 0; i < 36 && na < 4; ++i) {
        const float h0 = hist[i], hm = hist[(i + 35) % 36], hp = hist[(i + 1) % 36];
        if (h0 > 0.8f * maxh && h0 > hm && h0 > hp) {
            const float di = -0.5f * (hp - hm) / (hp + hm - 2.0f * h0);
            angles[blockIdx.x * 4 + na++] = kTwoPi * ((float)i + di + 0.5f) / 36.0f;
        }
    }
    nang[blockIdx.x] = min(na, max_orient);
}

__device__ void normalize_l2_eps(float* d) {
    float norm = 0.0f;
    for (int i = 0; i < 128; ++i) norm += d[i] * d[i];
    norm = sqrtf(norm) + 1.19209290e-07f;
    for (int i = 0; i < 128; ++i) d[i] = d[i] / norm;
}

// One wave per (keypoint, orientation): 4 x 4 x 8 trilinear histogram (lane-private partial sums, butterfly), the
// normalisations and the byte conversion; the feature's keypoint row in COLMAP's convention
__global__ void __launch_bounds__(kWave) k_descr(const Kp* __restrict__ kps, const uint32_t* __restrict__ fkp,
                                                 const float* __restrict__ fth, const float* __restrict__ G, int w, int h,
                                                 const float* __restrict__ tab, int normalization, float p2,
                                                 float* __restrict__ kp_out, uint8_t* __restrict__ desc_out) {
    __shared__ float part[128 * kWave];
    __shared__ float dsc[128], tr[128];
    const int f = blockIdx.x, l = threadIdx.x;
    const Kp k = kps[fkp[f]];
    const float th = fth[f];
    const float* L = G + (size_t)k.d * w * h;
    const int xi = (int)(k.x + 0.5f), yi = (int)(k.y + 0.5f);
    const float SBP = 3.0f * k.sigma;
    const int W = (int)floorf(1.41421356237309504880f * SBP * 5.0f / 2.0f + 0.5f);
    float st0, ct0;
    fast_sincos(th, &st0, &ct0);
    const int ys0 = max(-W, 1 - yi), ys1 = min(W, h - 2 - yi);
    const int xs0 = max(-W, 1 - xi), xs1 = min(W, w - 2 - xi);
    const int nx = xs1 - xs0 + 1, n = (xs1 >= xs0 && ys1 >= ys0) ? nx * (ys1 - ys0 + 1) : 0;
    for (int b = 0; b < 128; ++b) part[b * kWave + l] = 0.0f;
    for (int p = l; p < n; p += kWave) {
        const int ys = ys0 + p / nx, xs = xs0 + p % nx;
        float mod, ang;
        gradient(L, w, h, xi + xs, yi + ys, &mod, &ang);
        const float theta = mod_2pi(ang - th);
        const float dx = (float)(xi + xs) - k.x, dy = (float)(yi + ys) - k.y;
        const float nx_ = (ct0 * dx + st0 * dy) / SBP, ny_ = (-st0 * dx + ct0 * dy) / SBP;
        const float nt = 8.0f * theta / kTwoPi;
        const float win = fast_expn(tab, (nx_ * nx_ + ny_ * ny_) / 8.0f);
        const int binx = (int)floorf(nx_ - 0.5f), biny = (int)floorf(ny_ - 0.5f), bint = (int)floorf(nt);
        const float rbinx = nx_ - ((float)binx + 0.5f), rbiny = ny_ - ((float)biny + 0.5f), rbint = nt - (float)bint;
        for (int dbx = 0; dbx < 2; ++dbx)
            for (int dby = 0; dby < 2; ++dby)
                for (int dbt = 0; dbt < 2; ++dbt) {
                    const int bx = binx + dbx, by = biny + dby;
                    if (bx < -2 || bx >= 2 || by < -2 || by >= 2) continue;
                    const float wgt = win * mod * fabsf(1.0f - (float)dbx - rbinx) * fabsf(1.0f - (float)dby - rbiny) *
                                      fabsf(1.0f - (float)dbt - rbint);
                    part[((bint + dbt) % 8 + 8 * (bx + 2) + 32 * (by + 2)) * kWave + l] += wgt;
                }
    }
    for (int b = 0; b < 128; ++b) {
        const float s = wave_butterfly(part[b * kWave + l]);
        if (l == 0) dsc[b] = s;
    }
    if (l != 0) return;
    normalize_l2_eps(dsc);
    for (int i = 0; i < 128; ++i)
        if (dsc[i] > 0.2f) dsc[i] = 0.2f;
    normalize_l2_eps(dsc);
    for (int j = 0; j < 4; ++j)  // to Lowe's layout: y flipped, orientations reversed
        for (int i = 0; i < 4; ++i) {
            const int o = 8 * i + 32 * j, op = 8 * i + 32 * (3 - j);
            tr[op] = dsc[o];
            for (int b = 1; b < 8; ++b) tr[8 - b + op] = dsc[b + o];
        }
    if (normalization == AMC_SIFT_L1_ROOT) {
        float s = 0.0f;
        for (int i = 0; i < 128; ++i) s += fabsf(tr[i]);
        if (s > 0.0f)
            for (int i = 0; i < 128; ++i) tr[i] = sqrtf(tr[i] / s);
    } else {
        float s = 0.0f;
        for (int i = 0; i < 128; ++i) s += tr[i] * tr[i];
        s = sqrtf(s);
        if (s > 0.0f)
            for (int i = 0; i < 128; ++i) tr[i] = tr[i] / s;
    }
    uint8_t* out = desc_out + (size_t)f * 128;
    for (int i = 0; i < 128; ++i) {
        const float v = roundf(512.0f * tr[i]);
        out[i] = (uint8_t)(v > 255.0f ? 255.0f : v);
    }
    float* kp = kp_out + (size_t)f * 4;
    kp[0] = k.x * p2 + 0.5f;
    kp[1] = k.y * p2 + 0.5f;
    kp[2] = k.sigma * p2;
    kp[3] = th > kPi ? th - kTwoPi : th;
}

// ---- host side ------------------------------------------------------------------------------------------------------
std::vector<float> gauss_taps(double sigma) {  // ceil(4 sigma) taps each side, normalised in double
    const int W = (int)std::ceil(4.0 * sigma);
    std::vector<double> g(2 * W + 1);
    double acc = 0.0;
    for (int i = -W; i <= W; ++i) {
        const double u = (double)i / sigma;
        g[i + W] = std::exp(-0.5 * u * u);
        acc += g[i + W];
    }
    std::vector<float> out(2 * W + 1);
    for (int i = 0; i <= 2 * W; ++i) out[i] = (float)(g[i] / acc);
    return out;
}

struct OctaveDims {
    int o, w, h;
};

std::vector<OctaveDims> octaves_of(int w, int h, const amc_sift_opts& op) {
    std::vector<OctaveDims> v;
    for (int oi = 0; oi < op.num_octaves; ++oi) {
        const int o = op.first_octave + oi;
        const int wo = o < 0 ? w << -o : w >> o, ho = o < 0 ? h << -o : h >> o;
        if (std::min(wo, ho) < 8) break;
        v.push_back({o, wo, ho});
    }
    return v;
}

struct HostResult {
    std::vector<float> kp;
    std::vector<uint8_t> desc;
};

}  // namespace

extern "C" {

void amc_sift_opts_default(amc_sift_opts* o) {
    if (!o) return;
    o->first_octave = -1;  // SiftExtractionOptions() of COLMAP 3.9.1
    o->num_octaves = 4;
    o->octave_resolution = 3;
    o->peak_threshold = 0.02 / 3;
    o->edge_threshold = 10.0;
    o->max_num_orientations = 2;
    o->upright = 0;
    o->normalization = AMC_SIFT_L1_ROOT;
    o->max_num_features = 8192;
    o->max_image_size = 3200;
}

void amc_sift_result_free(amc_sift_result* r) {
    if (!r) return;
    std::free(r->offsets);
    std::free(r->keypoints);
    std::free(r->descriptors);
    std::memset(r, 0, sizeof *r);
}

int amc_sift_extract(amc_ctx* ctx, const amc_sift_image* images, size_t nimages, const amc_sift_opts* opts,
                     amc_sift_result* result) {
    const char* const hipchk_who = "amc_sift_extract";
    if (!ctx || !opts || !result || (nimages && !images)) return api_fail(AMC_E_INVALID, "amc_sift_extract: NULL argument");
    std::memset(result, 0, sizeof *result);
    const amc_sift_opts op = *opts;
    if (op.first_octave < -1 || op.first_octave > 16 || op.num_octaves < 1 || op.num_octaves > 32 ||
        op.octave_resolution < 1 || op.octave_resolution > 32 || op.max_num_orientations < 1 ||
        !(op.peak_threshold >= 0.0) || !(op.edge_threshold > 0.0) ||
        (op.normalization != AMC_SIFT_L1_ROOT && op.normalization != AMC_SIFT_L2))
        return api_fail(AMC_E_INVALID, "amc_sift_extract: invalid options (first_octave %d, num_octaves %d, "
                        "octave_resolution %d, max_num_orientations %d, normalization %d)", op.first_octave,
                        op.num_octaves, op.octave_resolution, op.max_num_orientations, op.normalization);
    for (size_t i = 0; i < nimages; ++i) {
        const amc_sift_image& im = images[i];
        if (!im.pixels || im.width < 1 || im.height < 1 || im.pitch < im.width)
            return api_fail(AMC_E_INVALID, "amc_sift_extract: image %zu: bad pixels / size / pitch", i);
        if (im.width > op.max_image_size || im.height > op.max_image_size)
            return api_fail(AMC_E_INVALID, "amc_sift_extract: image %zu is %d x %d, larger than max_image_size %d", i,
                            im.width, im.height, op.max_image_size);
    }
    const CtxView cv = ctx_view(ctx);
    HIPCHK(hipSetDevice(cv.device));
    hipStream_t st = cv.stream;
    const int S = op.octave_resolution, nlev = S + 3;
    const double sigma0 = 1.6 * std::pow(2.0, 1.0 / S), sigman = 0.5;
    const double kk = std::pow(2.0, 1.0 / S), dsigma0 = sigma0 * std::sqrt(1.0 - 1.0 / (kk * kk));

    // every blur's taps, one table: [0] the first octave's base (empty when none is needed), [L] level L of any octave
    std::vector<std::vector<float>> taps(nlev);
    {
        const double sa = sigma0 * std::pow(2.0, -1.0 / S), sb = sigman * std::pow(2.0, -op.first_octave);
        if (sa > sb) taps[0] = gauss_taps(std::sqrt(sa * sa - sb * sb));
        for (int L = 1; L < nlev; ++L) taps[L] = gauss_taps(dsigma0 * std::pow(kk, L - 1));
    }
    std::vector<int> tap_off(nlev);
    std::vector<float> h_consts;
    for (int k = 0; k < kExpnSize; ++k) h_consts.push_back((float)std::exp(-(double)k * 25.0 / 256.0));
    for (int L = 0; L < nlev; ++L) {
        tap_off[L] = (int)h_consts.size();
        h_consts.insert(h_consts.end(), taps[L].begin(), taps[L].end());
    }

    // the workspace for the largest image: constants | u8 image | base | tmp | levels of every octave | DoGs of one
    size_t need = 0;
    for (size_t i = 0; i < nimages; ++i) {
        const auto oct = octaves_of(images[i].width, images[i].height, op);
        size_t lev = 0, px0 = 0;
        for (const auto& od : oct) {
            lev += align256((size_t)nlev * od.w * od.h * sizeof(float));
            px0 = std::max(px0, (size_t)od.w * od.h);
        }
        const size_t u8 = align256((size_t)images[i].width * images[i].height);
        const size_t b = u8 + 2 * align256(px0 * sizeof(float)) + lev + align256((size_t)(nlev - 1) * px0 * sizeof(float));
        need = std::max(need, b);
    }
    const size_t const_bytes = align256(h_consts.size() * sizeof(float));
    DevBuf<void> ws, kpbuf, outbuf, cntbuf;  // device memory of the call, grow-only
    HIPCHK(ws.ensure(const_bytes + need));
    char* wsb = static_cast<char*>(ws.p);
    float* d_consts = reinterpret_cast<float*>(wsb);
    HIPCHK(hipMemcpyAsync(d_consts, h_consts.data(), h_consts.size() * sizeof(float), hipMemcpyHostToDevice, st));
    const float* d_tab = d_consts;

    // the whole batch's pixels in one pinned staging buffer (packed rows), so that every upload is a DMA from pinned
    // memory; freed when the call returns
    std::vector<size_t> stage_off(nimages + 1, 0);
    for (size_t i = 0; i < nimages; ++i) stage_off[i + 1] = stage_off[i] + (size_t)images[i].width * images[i].height;
    PinBuf<uint8_t> pinned;
    if (stage_off[nimages]) HIPCHK(pinned.ensure(stage_off[nimages]));
    for (size_t i = 0; i < nimages; ++i) {
        uint8_t* dst = pinned.p + stage_off[i];
        for (int y = 0; y < images[i].height; ++y)
            std::memcpy(dst + (size_t)y * images[i].width, images[i].pixels + (size_t)y * images[i].pitch, images[i].width);
    }

    StreamTimer total(st), stage(st);
    HIPCHK(total.start());
    double stage_ms[4] = {0, 0, 0, 0};
    std::vector<HostResult> res(nimages);

    for (size_t ii = 0; ii < nimages; ++ii) {
        const amc_sift_image& im = images[ii];
        const auto oct = octaves_of(im.width, im.height, op);
        char* cur = wsb + const_bytes;
        uint8_t* d_u8 = reinterpret_cast<uint8_t*>(cur);
        cur += align256((size_t)im.width * im.height);
        const size_t px0 = oct.empty() ? 0 : (size_t)oct[0].w * oct[0].h;
        float* d_base = reinterpret_cast<float*>(cur);
        cur += align256(px0 * sizeof(float));
        float* d_tmp = reinterpret_cast<float*>(cur);
        cur += align256(px0 * sizeof(float));
        std::vector<float*> d_lev(oct.size());
        for (size_t k = 0; k < oct.size(); ++k) {
            d_lev[k] = reinterpret_cast<float*>(cur);
            cur += align256((size_t)nlev * oct[k].w * oct[k].h * sizeof(float));
        }
        float* d_dog = reinterpret_cast<float*>(cur);
        if (oct.empty()) continue;  // too small for one octave: no features
        HIPCHK(hipMemcpyAsync(d_u8, pinned.p + stage_off[ii], stage_off[ii + 1] - stage_off[ii], hipMemcpyHostToDevice,
                              st));

        struct OctKps {
            int n = 0;
            std::vector<int> nang;
            std::vector<float> angles;
        };
        std::vector<OctKps> ok(oct.size());
        std::vector<size_t> kp_base(oct.size() + 1, 0);
        std::vector<std::vector<int>> row_cnt(oct.size());
        // pass over the octaves: scale space, detection, orientation
        for (size_t k = 0; k < oct.size(); ++k) {
            const int w = oct[k].w, h = oct[k].h;
            const size_t plane = (size_t)w * h;
            float* G = d_lev[k];
            HIPCHK(stage.start());
            const dim3 rows((w + 255) / 256, h);
            if (k == 0) {
                k_base<<<rows, 256, 0, st>>>(d_u8, im.width, im.height, im.width, oct[0].o, taps[0].empty() ? G : d_base,
                                             w, h);
                if (!taps[0].empty()) {
                    const int W = ((int)taps[0].size() - 1) / 2;
                    k_hblur<<<dim3((w + kBlurTile - 1) / kBlurTile, h), kBlurTile, (kBlurTile + 2 * W) * sizeof(float),
                              st>>>(d_base, d_tmp, w, h, d_consts + tap_off[0], W);
                    k_vblur<<<dim3((w + kVbx - 1) / kVbx, (h + kVby - 1) / kVby), kVbx * 4,
                              (kVby + 2 * W) * kVbx * sizeof(float), st>>>(d_tmp, G, nullptr, nullptr, w, h,
                                                                           d_consts + tap_off[0], W);
                }
            } else {
                k_down<<<rows, 256, 0, st>>>(d_lev[k - 1] + (size_t)S * oct[k - 1].w * oct[k - 1].h, oct[k - 1].w, G, w, h);
            }
            for (int L = 1; L < nlev; ++L) {
                const int W = ((int)taps[L].size() - 1) / 2;
                k_hblur<<<dim3((w + kBlurTile - 1) / kBlurTile, h), kBlurTile, (kBlurTile + 2 * W) * sizeof(float), st>>>(
                    G + (L - 1) * plane, d_tmp, w, h, d_consts + tap_off[L], W);
                k_vblur<<<dim3((w + kVbx - 1) / kVbx, (h + kVby - 1) / kVby), kVbx * 4,
                          (kVby + 2 * W) * kVbx * sizeof(float), st>>>(d_tmp, G + L * plane, G + (L - 1) * plane,
                                                                       d_dog + (L - 1) * plane, w, h,
                                                                       d_consts + tap_off[L], W);
            }
            HIPCHK(hipGetLastError());
            HIPCHK(stage.stop(stage_ms[0]));

            HIPCHK(stage.start());
            const DetectParams P{w, h, S, oct[k].o, (float)op.peak_threshold, (float)op.edge_threshold, (float)sigma0};
            const int nrows = S * (h - 2);
            HIPCHK(cntbuf.ensure(2 * (size_t)nrows * sizeof(int)));
            int* d_cnt = static_cast<int*>(cntbuf.p);
            int* d_off = d_cnt + nrows;
            k_detect<<<dim3(h - 2, S), kDetectThreads, 0, st>>>(d_dog, P, d_cnt, nullptr, nullptr);
            HIPCHK(hipGetLastError());
            row_cnt[k].resize(nrows);
            HIPCHK(hipMemcpyAsync(row_cnt[k].data(), d_cnt, nrows * sizeof(int), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            std::vector<int> off(nrows);
            int n = 0;
            for (int r = 0; r < nrows; ++r) {
                off[r] = n;
                n += row_cnt[k][r];
            }
            ok[k].n = n;
            kp_base[k + 1] = kp_base[k] + n;
            HIPCHK(stage.stop(stage_ms[1]));
            if (n == 0) continue;
            // keypoints of all octaves so far stay in kpbuf (Kp), followed by a scratch of 4 angles + 1 count each
            const size_t kp_bytes = align256(kp_base[k + 1] * sizeof(Kp));
            if (kpbuf.cap < kp_bytes + align256((size_t)n * 5 * sizeof(float))) {
                DevBuf<void> grown;
                HIPCHK(grown.ensure(2 * (kp_bytes + align256((size_t)n * 5 * sizeof(float)))));
                if (kp_base[k])
                    HIPCHK(hipMemcpyAsync(grown.p, kpbuf.p, kp_base[k] * sizeof(Kp), hipMemcpyDeviceToDevice, st));
                HIPCHK(hipStreamSynchronize(st));
                kpbuf = std::move(grown);
            }
            Kp* d_kps = static_cast<Kp*>(kpbuf.p) + kp_base[k];
            HIPCHK(stage.start());
            HIPCHK(hipMemcpyAsync(d_off, off.data(), nrows * sizeof(int), hipMemcpyHostToDevice, st));
            k_detect<<<dim3(h - 2, S), kDetectThreads, 0, st>>>(d_dog, P, d_cnt, d_off, d_kps);
            HIPCHK(hipGetLastError());
            HIPCHK(stage.stop(stage_ms[1]));
            ok[k].nang.assign(n, 1);
            ok[k].angles.assign((size_t)n * 4, 0.0f);
            if (!op.upright) {
                HIPCHK(stage.start());
                float* d_ang = reinterpret_cast<float*>(static_cast<char*>(kpbuf.p) + kp_bytes);
                int* d_nang = reinterpret_cast<int*>(d_ang + (size_t)n * 4);
                k_orient<<<n, kWave, 0, st>>>(d_kps, G, w, h, d_tab, op.max_num_orientations, d_ang, d_nang);
                HIPCHK(hipGetLastError());
                HIPCHK(hipMemcpyAsync(ok[k].angles.data(), d_ang, (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToHost,
                                      st));
                HIPCHK(hipMemcpyAsync(ok[k].nang.data(), d_nang, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
                HIPCHK(stage.stop(stage_ms[2]));
            }
        }
        // the cut: whole octaves from the coarsest down; the octave that crosses the limit keeps its first features
        std::vector<long> keep(oct.size(), 0);
        long cum = 0;
        for (int k = (int)oct.size() - 1; k >= 0; --k) {
            long cnt = 0;
            for (int a : ok[k].nang) cnt += a;
            if (op.max_num_features > 0 && cum + cnt > op.max_num_features) cnt = op.max_num_features - cum;
            keep[k] = cnt;
            cum += cnt;
        }
        // feature lists (keypoint index, angle) in output order, then the descriptors octave by octave
        std::vector<uint32_t> fkp;
        std::vector<float> fth;
        std::vector<size_t> fbase(oct.size() + 1, 0);
        for (size_t k = 0; k < oct.size(); ++k) {
            long left = keep[k];
            for (int j = 0; j < ok[k].n && left > 0; ++j)
                for (int r = 0; r < ok[k].nang[j] && left > 0; ++r, --left) {
                    fkp.push_back((uint32_t)j);
                    fth.push_back(ok[k].angles[(size_t)j * 4 + r]);
                }
            fbase[k + 1] = fkp.size();
        }
        const size_t nf = fkp.size();
        HostResult& hr = res[ii];
        hr.kp.resize(nf * 4);
        hr.desc.resize(nf * 128);
        if (nf == 0) continue;
        uint32_t* d_fkp;
        float *d_fth, *d_kpo;
        uint8_t* d_desc;
        HIPCHK(DevParts().part(&d_fkp, nf).part(&d_fth, nf).part(&d_kpo, 4 * nf).part(&d_desc, 128 * nf).carve(outbuf));
        HIPCHK(stage.start());
        HIPCHK(hipMemcpyAsync(d_fkp, fkp.data(), nf * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_fth, fth.data(), nf * sizeof(float), hipMemcpyHostToDevice, st));
        for (size_t k = 0; k < oct.size(); ++k) {
            const size_t m = fbase[k + 1] - fbase[k];
            if (!m) continue;
            const int o = oct[k].o;
            const float p2 = o < 0 ? 0.5f : (float)(1L << o);
            k_descr<<<(unsigned)m, kWave, 0, st>>>(static_cast<Kp*>(kpbuf.p) + kp_base[k], d_fkp + fbase[k],
                                                   d_fth + fbase[k], d_lev[k], oct[k].w, oct[k].h, d_tab,
                                                   op.normalization, p2, d_kpo + fbase[k] * 4, d_desc + fbase[k] * 128);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hr.kp.data(), d_kpo, nf * 4 * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hr.desc.data(), d_desc, nf * 128, hipMemcpyDeviceToHost, st));
        HIPCHK(stage.stop(stage_ms[3]));
    }
    HIPCHK(total.stop(result->device_ms));  // (result was zeroed on entry)
    for (int s = 0; s < 4; ++s) result->stage_ms[s] = stage_ms[s];

    size_t nf = 0;
    for (const auto& r : res) nf += r.kp.size() / 4;
    result->nimages = nimages;
    result->offsets = static_cast<uint64_t*>(std::malloc((nimages + 1) * sizeof(uint64_t)));
    result->keypoints = static_cast<float*>(std::malloc(std::max<size_t>(nf, 1) * 4 * sizeof(float)));
    result->descriptors = static_cast<uint8_t*>(std::malloc(std::max<size_t>(nf, 1) * 128));
    if (!result->offsets || !result->keypoints || !result->descriptors) {
        amc_sift_result_free(result);
        return api_fail(AMC_E_NOMEM, "amc_sift_extract: out of host memory for %zu features", nf);
    }
    size_t at = 0;
    result->offsets[0] = 0;
    for (size_t i = 0; i < nimages; ++i) {
        const size_t n = res[i].kp.size() / 4;
        if (n) {
            std::memcpy(result->keypoints + at * 4, res[i].kp.data(), n * 4 * sizeof(float));
            std::memcpy(result->descriptors + at * 128, res[i].desc.data(), n * 128);
        }
        at += n;
        result->offsets[i + 1] = at;
    }
    return AMC_OK;
}

}  // extern "C"
