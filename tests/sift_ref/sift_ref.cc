// sift_ref.cc — the CPU reference of the SIFT extractor (test infrastructure, never linked into the package).
//
// Plain single-threaded loops restating DESIGN.md section 10 from its text: the scale space, detection and refinement,
// the orientation histogram, the descriptor, the normalisations and the feature cut, with the same float32 operations
// in the same order as pycolmap_amd/csrc/sift.hip, so that the two agree bit for bit.  It includes no product header.
// Built by tests/sift_ref_lib.py: g++ -O2 -ffp-contract=off -fno-fast-math.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

const float kPi = 3.14159265358979323846f;
const float kTwoPi = 6.28318530717958647692f;
const int kLanes = 64;  // the device's wave: histogram partial sums are kept per lane, then summed by a butterfly

// ---- the project's transcendental definitions (+ - * /, sqrtf and a host table only) -------------------------
float expn_tab[258];  // expn_tab[k] = exp(-k * 25 / 256), double rounded to float

void init_tables() {
    for (int k = 0; k < 258; ++k) expn_tab[k] = (float)std::exp(-(double)k * 25.0 / 256.0);
}

float fast_expn(float x) {  // exp(-x), x >= 0: linear interpolation in the table; 0 beyond 25
    if (x > 25.0f) return 0.0f;
    x = x * 10.24f;
    const int i = (int)std::floor(x);
    const float r = x - (float)i;
    const float a = expn_tab[i], b = expn_tab[i + 1];
    return a + r * (b - a);
}

float fast_atan2(float y, float x) {  // VLFeat's published approximation, |error| < 0.008 rad
    const float c3 = 0.1821f, c1 = 0.9675f;
    const float abs_y = std::fabs(y) + 1.19209290e-07f;
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

float mod_2pi(float x) {
    while (x > kTwoPi) x -= kTwoPi;
    while (x < 0.0f) x += kTwoPi;
    return x;
}

float pow2f(float t) {  // 2^t: 2^floor(t) exactly times a degree-10 Taylor polynomial of e^(f ln 2), f in [0, 1)
    const float n = std::floor(t);
    const float u = (t - n) * 0.693147180559945309f;
    float p = 1.0f + u * (1.0f + u * ((float)(1.0 / 2) + u * ((float)(1.0 / 6) + u * ((float)(1.0 / 24) +
              u * ((float)(1.0 / 120) + u * ((float)(1.0 / 720) + u * ((float)(1.0 / 5040) + u * ((float)(1.0 / 40320) +
              u * ((float)(1.0 / 362880) + u * (float)(1.0 / 3628800))))))))));
    for (int k = (int)n; k > 0; --k) p *= 2.0f;
    for (int k = (int)n; k < 0; ++k) p *= 0.5f;
    return p;
}

void fast_sincos(float th, float* s, float* c) {  // th in [0, 2 pi]: Taylor polynomials (degree 19 / 18) on [-pi, pi]
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

// ---- scale space ----------------------------------------------------------------------------------------------
struct Img {
    int w = 0, h = 0;
    std::vector<float> v;
    float at(int x, int y) const { return v[(size_t)y * w + x]; }
    float& at(int x, int y) { return v[(size_t)y * w + x]; }
};

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

Img blur(const Img& in, const std::vector<float>& g) {  // horizontal, then vertical; replicated borders
    const int W = ((int)g.size() - 1) / 2;
    Img t{in.w, in.h, std::vector<float>(in.v.size())}, out{in.w, in.h, std::vector<float>(in.v.size())};
    for (int y = 0; y < in.h; ++y)
        for (int x = 0; x < in.w; ++x) {
            float acc = 0.0f;
            for (int k = 0; k <= 2 * W; ++k) acc += g[k] * in.at(std::min(std::max(x - W + k, 0), in.w - 1), y);
            t.at(x, y) = acc;
        }
    for (int y = 0; y < in.h; ++y)
        for (int x = 0; x < in.w; ++x) {
            float acc = 0.0f;
            for (int k = 0; k <= 2 * W; ++k) acc += g[k] * t.at(x, std::min(std::max(y - W + k, 0), in.h - 1));
            out.at(x, y) = acc;
        }
    return out;
}

struct Opts {
    int first_octave, num_octaves, S;
    float peak, edge;
    int max_orient, upright, norm, max_features;
};

struct Kp {
    float x, y, sn, sigma;  // octave coordinates, refined level, sigma in octave pixels
    int o, d;               // octave, DoG level of detection
};

void solve3(float A[3][3], float b[3]) {  // Gaussian elimination with partial pivoting
    for (int j = 0; j < 3; ++j) {
        float maxa = 0.0f, maxabsa = 0.0f;
        int maxi = -1;
        for (int i = j; i < 3; ++i) {
            const float a = A[i][j], absa = std::fabs(a);
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
        for (int jj = j; jj < 3; ++jj) std::swap(A[i][jj], A[j][jj]);
        std::swap(b[i], b[j]);
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

void gradient(const Img& G, int x, int y, float* mod, float* ang) {
    const float gx = (x == 0) ? G.at(1, y) - G.at(0, y)
                   : (x == G.w - 1) ? G.at(x, y) - G.at(x - 1, y) : 0.5f * (G.at(x + 1, y) - G.at(x - 1, y));
    const float gy = (y == 0) ? G.at(x, 1) - G.at(x, 0)
                   : (y == G.h - 1) ? G.at(x, y) - G.at(x, y - 1) : 0.5f * (G.at(x, y + 1) - G.at(x, y - 1));
    *mod = std::sqrt(gx * gx + gy * gy);
    *ang = mod_2pi(fast_atan2(gy, gx) + kTwoPi);
}

// lane partial sums -> one value per bin: part[l * nb + b], butterfly over the 64 lanes (lane 0's result)
void butterfly(const std::vector<float>& part, int nb, float* out) {
    float v[kLanes], nv[kLanes];
    for (int b = 0; b < nb; ++b) {
        for (int l = 0; l < kLanes; ++l) v[l] = part[(size_t)l * nb + b];
        for (int o = kLanes / 2; o >= 1; o /= 2) {
            for (int l = 0; l < kLanes; ++l) nv[l] = v[l] + v[l ^ o];
            std::memcpy(v, nv, sizeof v);
        }
        out[b] = v[0];
    }
}

int orientations(const Img& G, const Kp& k, float* angles) {
    const int xi = (int)(k.x + 0.5f), yi = (int)(k.y + 0.5f);
    if (xi < 0 || xi > G.w - 1 || yi < 0 || yi > G.h - 1) return 0;
    const float sigmaw = 1.5f * k.sigma;
    const int W = std::max((int)std::floor(3.0f * sigmaw), 1);
    const int ys0 = std::max(-W, -yi), ys1 = std::min(W, G.h - 1 - yi);
    const int xs0 = std::max(-W, -xi), xs1 = std::min(W, G.w - 1 - xi);
    const int nx = xs1 - xs0 + 1, n = nx * (ys1 - ys0 + 1);
    std::vector<float> part(kLanes * 36, 0.0f);
    for (int l = 0; l < kLanes; ++l)
        for (int p = l; p < n; p += kLanes) {
            const int ys = ys0 + p / nx, xs = xs0 + p % nx;
            const float dx = (float)(xi + xs) - k.x, dy = (float)(yi + ys) - k.y;
            const float r2 = dx * dx + dy * dy;
            if (r2 >= (float)(W * W) + 0.6f) continue;
            const float wgt = fast_expn(r2 / (2.0f * sigmaw * sigmaw));
            float mod, ang;
            gradient(G, xi + xs, yi + ys, &mod, &ang);
            const float fbin = 36.0f * ang / kTwoPi;
            const int bin = (int)std::floor(fbin - 0.5f);
            const float rbin = fbin - (float)bin - 0.5f;
            float* h = &part[(size_t)l * 36];
            h[(bin + 36) % 36] += (1.0f - rbin) * mod * wgt;
            h[(bin + 1) % 36] += rbin * mod * wgt;
        }
    float hist[36];
    butterfly(part, 36, hist);
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
    for (int i = 1; i < 36; ++i) maxh = std::max(maxh, hist[i]);
    int na = 0;
    for (int i = 0; i < 36 && na < 4; ++i) {
        const float h0 = hist[i], hm = hist[(i + 35) % 36], hp = hist[(i + 1) % 36];
        if (h0 > 0.8f * maxh && h0 > hm && h0 > hp) {
            const float di = -0.5f * (hp - hm) / (hp + hm - 2.0f * h0);
            angles[na++] = kTwoPi * ((float)i + di + 0.5f) / 36.0f;
        }
    }
    return na;
}

void normalize_l2_eps(float* d) {
    float norm = 0.0f;
    for (int i = 0; i < 128; ++i) norm += d[i] * d[i];
    norm = std::sqrt(norm) + 1.19209290e-07f;
    for (int i = 0; i < 128; ++i) d[i] = d[i] / norm;
}

// the histogram (VLFeat's bin order) -> the descriptor's bytes: normalise, clamp at 0.2, normalise, Lowe's layout,
// L1_ROOT or L2, min(255, round(512 x))
void finish_descriptor(float* d, int normalization, uint8_t* out) {
    float t[128];
    normalize_l2_eps(d);
    for (int i = 0; i < 128; ++i)
        if (d[i] > 0.2f) d[i] = 0.2f;
    normalize_l2_eps(d);
    for (int j = 0; j < 4; ++j)  // to Lowe's layout: y flipped, orientations reversed
        for (int i = 0; i < 4; ++i) {
            const int o = 8 * i + 32 * j, op = 8 * i + 32 * (3 - j);
            t[op] = d[o];
            for (int b = 1; b < 8; ++b) t[8 - b + op] = d[b + o];
        }
    if (normalization == 0) {  // L1_ROOT
        float s = 0.0f;
        for (int i = 0; i < 128; ++i) s += std::fabs(t[i]);
        if (s > 0.0f)
            for (int i = 0; i < 128; ++i) t[i] = std::sqrt(t[i] / s);
    } else {
        float s = 0.0f;
        for (int i = 0; i < 128; ++i) s += t[i] * t[i];
        s = std::sqrt(s);
        if (s > 0.0f)
            for (int i = 0; i < 128; ++i) t[i] = t[i] / s;
    }
    for (int i = 0; i < 128; ++i) {
        const float v = std::round(512.0f * t[i]);
        out[i] = (uint8_t)(v > 255.0f ? 255.0f : v);
    }
}

void descriptor(const Img& G, const Kp& k, float th, int normalization, uint8_t* out) {
    const int xi = (int)(k.x + 0.5f), yi = (int)(k.y + 0.5f);
    const float SBP = 3.0f * k.sigma;
    const int W = (int)std::floor(1.41421356237309504880f * SBP * 5.0f / 2.0f + 0.5f);
    float st0, ct0;
    fast_sincos(th, &st0, &ct0);
    const int ys0 = std::max(-W, 1 - yi), ys1 = std::min(W, G.h - 2 - yi);
    const int xs0 = std::max(-W, 1 - xi), xs1 = std::min(W, G.w - 2 - xi);
    const int nx = xs1 - xs0 + 1, n = (xs1 >= xs0 && ys1 >= ys0) ? nx * (ys1 - ys0 + 1) : 0;
    std::vector<float> part(kLanes * 128, 0.0f);
    for (int l = 0; l < kLanes; ++l)
        for (int p = l; p < n; p += kLanes) {
            const int ys = ys0 + p / nx, xs = xs0 + p % nx;
            float mod, ang;
            gradient(G, xi + xs, yi + ys, &mod, &ang);
            const float theta = mod_2pi(ang - th);
            const float dx = (float)(xi + xs) - k.x, dy = (float)(yi + ys) - k.y;
            const float nx_ = (ct0 * dx + st0 * dy) / SBP, ny_ = (-st0 * dx + ct0 * dy) / SBP;
            const float nt = 8.0f * theta / kTwoPi;
            const float win = fast_expn((nx_ * nx_ + ny_ * ny_) / 8.0f);
            const int binx = (int)std::floor(nx_ - 0.5f), biny = (int)std::floor(ny_ - 0.5f), bint = (int)std::floor(nt);
            const float rbinx = nx_ - ((float)binx + 0.5f), rbiny = ny_ - ((float)biny + 0.5f), rbint = nt - (float)bint;
            float* h = &part[(size_t)l * 128];
            for (int dbx = 0; dbx < 2; ++dbx)
                for (int dby = 0; dby < 2; ++dby)
                    for (int dbt = 0; dbt < 2; ++dbt) {
                        const int bx = binx + dbx, by = biny + dby;
                        if (bx < -2 || bx >= 2 || by < -2 || by >= 2) continue;
                        const float wgt = win * mod * std::fabs(1.0f - (float)dbx - rbinx) *
                                          std::fabs(1.0f - (float)dby - rbiny) * std::fabs(1.0f - (float)dbt - rbint);
                        h[(bint + dbt) % 8 + 8 * (bx + 2) + 32 * (by + 2)] += wgt;
                    }
        }
    float d[128];
    butterfly(part, 128, d);
    finish_descriptor(d, normalization, out);
}

struct Feature {
    float kp[4];
    uint8_t desc[128];
};
std::vector<Feature> g_out;

}  // namespace

extern "C" {

float sift_ref_atan2(float y, float x) { return fast_atan2(y, x); }
float sift_ref_expn(float x) {
    init_tables();
    return fast_expn(x);
}
float sift_ref_pow2(float t) { return pow2f(t); }
void sift_ref_sincos(float th, float* s, float* c) { fast_sincos(th, s, c); }
void sift_ref_finish_descriptor(const float* hist, int normalization, uint8_t* out) {
    float d[128];
    std::memcpy(d, hist, sizeof d);
    finish_descriptor(d, normalization, out);
}

// Run the extractor on one 8-bit grey image; returns the number of features (fetch them with sift_ref_fetch), or
// -1 for invalid arguments.
long sift_ref_extract(const uint8_t* pixels, int w, int h, long pitch, int first_octave, int num_octaves, int S,
                      double peak_threshold, double edge_threshold, int max_orient, int upright, int normalization,
                      int max_features) {
    g_out.clear();
    if (w < 1 || h < 1 || S < 1 || num_octaves < 1 || first_octave < -1 || first_octave > 30) return -1;
    init_tables();
    const Opts op{first_octave, num_octaves, S, (float)peak_threshold, (float)edge_threshold,
                  max_orient, upright, normalization, max_features};
    const double sigma0 = 1.6 * std::pow(2.0, 1.0 / S), sigman = 0.5;
    const float sigma0f = (float)sigma0;
    const double kk = std::pow(2.0, 1.0 / S), dsigma0 = sigma0 * std::sqrt(1.0 - 1.0 / (kk * kk));
    const int nlev = S + 3;

    struct Octave {
        int o;
        std::vector<Img> G;
        std::vector<Kp> kps;
        std::vector<std::vector<float>> angles;
    };
    std::vector<Octave> octs;
    Img base;
    for (int oi = 0; oi < num_octaves; ++oi) {
        const int o = first_octave + oi;
        const int wo = o < 0 ? w << -o : w >> o, ho = o < 0 ? h << -o : h >> o;
        if (std::min(wo, ho) < 8) break;
        Octave oc;
        oc.o = o;
        if (oi == 0) {  // the base image: v / 255 at octave first_octave, blurred from the nominal 0.5 to level -1's sigma
            base = Img{wo, ho, std::vector<float>((size_t)wo * ho)};
            auto src = [&](int x, int y) { return (float)pixels[(size_t)y * pitch + x] / 255.0f; };
            if (o == -1) {
                for (int y = 0; y < h; ++y)
                    for (int x = 0; x < w; ++x) {
                        const float a = src(x, y), b = src(std::min(x + 1, w - 1), y), c = src(x, std::min(y + 1, h - 1)),
                                    d = src(std::min(x + 1, w - 1), std::min(y + 1, h - 1));
                        base.at(2 * x, 2 * y) = a;
                        base.at(2 * x + 1, 2 * y) = 0.5f * (a + b);
                        base.at(2 * x, 2 * y + 1) = 0.5f * (a + c);
                        base.at(2 * x + 1, 2 * y + 1) = 0.25f * (a + b + c + d);
                    }
            } else {
                for (int y = 0; y < ho; ++y)
                    for (int x = 0; x < wo; ++x) base.at(x, y) = src(x << o, y << o);
            }
            const double sa = sigma0 * std::pow(2.0, -1.0 / S), sb = sigman * std::pow(2.0, -o);
            oc.G.push_back(sa > sb ? blur(base, gauss_taps(std::sqrt(sa * sa - sb * sb))) : base);
        } else {
            const Img& prev = octs.back().G[S];
            Img b{wo, ho, std::vector<float>((size_t)wo * ho)};
            for (int y = 0; y < ho; ++y)
                for (int x = 0; x < wo; ++x) b.at(x, y) = prev.at(2 * x, 2 * y);
            oc.G.push_back(b);
        }
        for (int L = 1; L < nlev; ++L) oc.G.push_back(blur(oc.G[L - 1], gauss_taps(dsigma0 * std::pow(kk, L - 1))));
        std::vector<Img> D(nlev - 1);
        for (int d = 0; d < nlev - 1; ++d) {
            D[d] = Img{wo, ho, std::vector<float>((size_t)wo * ho)};
            for (size_t i = 0; i < D[d].v.size(); ++i) D[d].v[i] = oc.G[d + 1].v[i] - oc.G[d].v[i];
        }
        // detection and refinement, in (level, y, x) order of the detected pixel
        const float tp = op.peak, te = op.edge;
        for (int d = 1; d <= S; ++d)
            for (int y0 = 1; y0 < ho - 1; ++y0)
                for (int x0 = 1; x0 < wo - 1; ++x0) {
                    const float v = D[d].at(x0, y0);
                    bool mx = v >= 0.8f * tp, mn = v <= -0.8f * tp;
                    for (int ds = -1; ds <= 1 && (mx || mn); ++ds)
                        for (int dy = -1; dy <= 1; ++dy)
                            for (int dx = -1; dx <= 1; ++dx) {
                                if (!ds && !dy && !dx) continue;
                                const float u = D[d + ds].at(x0 + dx, y0 + dy);
                                mx = mx && v > u;
                                mn = mn && v < u;
                            }
                    if (!mx && !mn) continue;
                    int x = x0, y = y0;
                    auto at = [&](int dx, int dy, int ds) { return D[d + ds].at(x + dx, y + dy); };
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
                        const int mvx = ((b[0] > 0.6f && x < wo - 2) ? 1 : 0) + ((b[0] < -0.6f && x > 1) ? -1 : 0);
                        const int mvy = ((b[1] > 0.6f && y < ho - 2) ? 1 : 0) + ((b[1] < -0.6f && y > 1) ? -1 : 0);
                        if (mvx == 0 && mvy == 0) break;
                        x += mvx;
                        y += mvy;
                    }
                    const float val = at(0, 0, 0) + 0.5f * (Dx * b[0] + Dy * b[1] + Ds * b[2]);
                    const float score = (Dxx + Dyy) * (Dxx + Dyy) / (Dxx * Dyy - Dxy * Dxy);
                    const float xn = (float)x + b[0], yn = (float)y + b[1], sn = (float)(d - 1) + b[2];
                    const bool good = std::fabs(val) > tp && score < (te + 1.0f) * (te + 1.0f) / te && score >= 0.0f &&
                                      std::fabs(b[0]) < 1.5f && std::fabs(b[1]) < 1.5f && std::fabs(b[2]) < 1.5f &&
                                      xn >= 0.0f && xn <= (float)(wo - 1) && yn >= 0.0f && yn <= (float)(ho - 1) &&
                                      sn >= -1.0f && sn <= (float)(S + 1);
                    if (!good) continue;
                    oc.kps.push_back(Kp{xn, yn, sn, sigma0f * pow2f(sn / (float)S), o, d});
                }
        for (const Kp& k : oc.kps) {
            std::vector<float> a;
            if (op.upright) {
                a.push_back(0.0f);
            } else {
                float ang[4];
                const int na = orientations(oc.G[k.d], k, ang);
                for (int j = 0; j < std::min(na, op.max_orient); ++j) a.push_back(ang[j]);
            }
            oc.angles.push_back(a);
        }
        octs.push_back(std::move(oc));
    }
    // the cut: whole octaves from the coarsest down; the octave that crosses the limit keeps its first features
    std::vector<long> keep(octs.size(), 0);
    long cum = 0;
    for (int i = (int)octs.size() - 1; i >= 0; --i) {
        long cnt = 0;
        for (const auto& a : octs[i].angles) cnt += (long)a.size();
        if (op.max_features > 0 && cum + cnt > op.max_features) cnt = op.max_features - cum;
        keep[i] = cnt;
        cum += cnt;
    }
    for (size_t i = 0; i < octs.size(); ++i) {
        const Octave& oc = octs[i];
        const float p2 = oc.o < 0 ? 0.5f : (float)(1L << oc.o);
        long left = keep[i];
        for (size_t j = 0; j < oc.kps.size() && left > 0; ++j)
            for (size_t r = 0; r < oc.angles[j].size() && left > 0; ++r, --left) {
                const Kp& k = oc.kps[j];
                const float th = oc.angles[j][r];
                Feature f;
                f.kp[0] = k.x * p2 + 0.5f;
                f.kp[1] = k.y * p2 + 0.5f;
                f.kp[2] = k.sigma * p2;
                f.kp[3] = th > kPi ? th - kTwoPi : th;
                descriptor(oc.G[k.d], k, th, op.norm, f.desc);
                g_out.push_back(f);
            }
    }
    return (long)g_out.size();
}

void sift_ref_fetch(float* kp, uint8_t* desc) {
    for (size_t i = 0; i < g_out.size(); ++i) {
        std::memcpy(kp + 4 * i, g_out[i].kp, sizeof g_out[i].kp);
        std::memcpy(desc + 128 * i, g_out[i].desc, 128);
    }
}

}  // extern "C"
