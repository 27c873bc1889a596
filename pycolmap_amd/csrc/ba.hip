// ba.hip — bundle adjustment on gfx950 (include/amc_ba.h): DESIGN.md section 15.  The per-observation arithmetic is
// ba_core.h's; this file is the kernels, the Levenberg-Marquardt loop that drives them and the C entry point.
//
// Work split (15.8).  Everything that is summed has one destination per lane or per wave, so there are no atomics: a
// lane per observation evaluates and stores the Jacobian blocks; a lane per point walks the point's observations (CSR by
// point); a wave per image reduces the image's observations (CSR by image) in the order of 12.10; a lane per camera joins
// its images' partials in image order.  The vector work of PCG (dot products, updates, the block preconditioner) runs in
// one wave, so that every dot product has the one order of 12.10 and the PCG scalars never leave the device.
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "amc_internal.h"
#include "ba_core.h"
#include "ba_plan.h"
#include "../../include/amc_ba.h"

using namespace amc;

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kKC = ba::kMaxParams;
constexpr int kPcgChunk = 8;             // PCG iterations queued between two looks at the stop flag
constexpr double kPcgTolerance = 1e-8;   // 15.6: |r| <= kPcgTolerance |b|
constexpr int kCamPart = 12 + 78 + 12 + 12;  // per-image partial of a camera block: diag, upper triangle, g, b

struct Scalars {
    double rz, bnorm;
    int32_t done, iters, kind, pad;  // kind: 1 = residual rule, 2 = iteration cap, 3 = breakdown (p.Sp <= 0)
    double out[8];
};

// the problem and the solver's state in device memory
struct Dev {
    uint32_t nimg, ncam, npts, nobs, nred, kc;
    int32_t loss;
    double loss_scale;
    // topology
    const uint32_t *oimg, *opt, *ioff, *poff, *pobs, *icam, *coff, *cimg;
    const int32_t* cmodel;
    const uint8_t *cvar, *ivar;
    const double* oxy;
    // scaling and the stored evaluation
    double *sc_c, *sc_p, *Jp, *Jc, *Jx, *res, *cost;
    // blocks
    double *Vinv, *gp, *vg, *diag_p, *g_c, *b_c, *D_c, *diag_c, *Minv_i, *Minv_c, *cost_img, *campart;
    // PCG and the step
    double *x, *r, *z, *p, *qv, *u, *campart2, *yp, *jy2_img;
    Scalars* s;
    const uint8_t* pvar;  // 15.12: 1 = the point is variable (last, so that every other field and buffer stays where it was)
};
struct Params {
    double *q, *t, *cp, *X;
};

// 12.10's order on the device: lane l's partial from f(l, .), then the xor butterfly m = 32 .. 1
template <int N, class F>
__device__ __forceinline__ void wsum(F f, double (&out)[N]) {
    double v[N];
    f((int)(threadIdx.x & 63u), v);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = v[i] + __shfl_xor(v[i], m);
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = v[i];
}

__global__ __launch_bounds__(kBlock) void ba_eval_kernel(Dev d, Params P, int jac) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    if (o >= d.nobs) return;
    const uint32_t i = d.oimg[o], j = d.opt[o], c = d.icam[i];
    double r[2], Jp[12], Jc[2 * kKC], Jx[6];
    d.cost[o] = ba::observation(d.cmodel[c], P.cp + kKC * c, P.q + 4 * i, P.t + 3 * i, P.X + 3 * j, d.oxy + 2 * o, d.loss,
                                d.loss_scale, jac != 0, r, Jp, Jc, Jx);
    if (!jac) return;
    d.res[2 * o] = r[0];
    d.res[2 * o + 1] = r[1];
    for (int a = 0; a < 2; ++a) {
        for (int k = 0; k < 6; ++k) d.Jp[12 * o + 6 * a + k] = d.ivar[6 * i + k] ? Jp[6 * a + k] * d.sc_c[6 * i + k] : 0.0;
        for (uint32_t k = 0; k < d.kc; ++k)
            d.Jc[(size_t)2 * d.kc * o + d.kc * a + k] =
                d.cvar[kKC * c + k] ? Jc[kKC * a + k] * d.sc_c[6 * d.nimg + kKC * c + k] : 0.0;
        for (int k = 0; k < 3; ++k) d.Jx[6 * o + 3 * a + k] = d.pvar[j] ? Jx[3 * a + k] * d.sc_p[3 * j + k] : 0.0;
    }
}

// 15.6 point blocks: V_j, its gradient, (V_j + D_j)^-1 and (V_j + D_j)^-1 g_j
__global__ __launch_bounds__(kBlock) void ba_point_kernel(Dev d, double radius) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= d.npts) return;
    double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
    for (uint32_t k = d.poff[j]; k < d.poff[j + 1]; ++k) {
        const uint32_t o = d.pobs[k];
        const double* J = d.Jx + 6 * o;
        const double r0 = d.res[2 * o], r1 = d.res[2 * o + 1];
        V[0] = V[0] + (J[0] * J[0] + J[3] * J[3]);
        V[1] = V[1] + (J[0] * J[1] + J[3] * J[4]);
        V[2] = V[2] + (J[0] * J[2] + J[3] * J[5]);
        V[3] = V[3] + (J[1] * J[1] + J[4] * J[4]);
        V[4] = V[4] + (J[1] * J[2] + J[4] * J[5]);
        V[5] = V[5] + (J[2] * J[2] + J[5] * J[5]);
        for (int a = 0; a < 3; ++a) g[a] = g[a] + (J[a] * r0 + J[3 + a] * r1);
    }
    d.diag_p[3 * j] = V[0];
    d.diag_p[3 * j + 1] = V[3];
    d.diag_p[3 * j + 2] = V[5];
    V[0] = V[0] + ba::lm_diag(V[0], radius);
    V[3] = V[3] + ba::lm_diag(V[3], radius);
    V[5] = V[5] + ba::lm_diag(V[5], radius);
    if (!d.pvar[j]) {  // 15.12: a constant point's block is the identity's (its J_x, hence V and g, are exact zeros)
        V[0] = V[3] = V[5] = 1.0;
        V[1] = V[2] = V[4] = 0.0;
    }
    double Vi[6], vg[3];
    ba::sym3_inverse(V, Vi);
    ba::sym3_mul(Vi, g, vg);
    for (int a = 0; a < 6; ++a) d.Vinv[6 * j + a] = Vi[a];
    for (int a = 0; a < 3; ++a) {
        d.gp[3 * j + a] = g[a];
        d.vg[3 * j + a] = vg[a];
    }
}

// what one observation's point block contributes to the reduced system: T = I - Jx Vinv Jx^T (2 x 2) and e = r - Jx vg
__device__ __forceinline__ void point_elimination(const Dev& d, uint32_t o, double (&T)[2][2], double (&e)[2]) {
    const uint32_t j = d.opt[o];
    const double* Jx = d.Jx + 6 * o;
    const double* Vi = d.Vinv + 6 * j;
    double Y[2][3];
    for (int a = 0; a < 2; ++a) ba::sym3_mul(Vi, Jx + 3 * a, Y[a]);
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b)
            T[a][b] = (a == b ? 1.0 : 0.0) - (Y[a][0] * Jx[3 * b] + Y[a][1] * Jx[3 * b + 1] + Y[a][2] * Jx[3 * b + 2]);
    const double* vg = d.vg + 3 * j;
    for (int a = 0; a < 2; ++a) e[a] = d.res[2 * o + a] - (Jx[3 * a] * vg[0] + Jx[3 * a + 1] * vg[1] + Jx[3 * a + 2] * vg[2]);
}

// 15.6 pose blocks: one wave per image.  Sums: cost, diag U (6), the preconditioner block (21), g (6), b (6)
__global__ __launch_bounds__(kWave) void ba_image_kernel(Dev d, double radius) {
    const uint32_t i = blockIdx.x;
    const uint32_t o0 = d.ioff[i], o1 = d.ioff[i + 1];
    double s[40];
    wsum<40>(
        [&](int l, double (&v)[40]) {
            for (int k = 0; k < 40; ++k) v[k] = 0.0;
            for (uint32_t o = o0 + (uint32_t)l; o < o1; o += kWave) {
                v[0] = v[0] + d.cost[o];
                double T[2][2], e[2], J[12], TJ[12];
                point_elimination(d, o, T, e);
                for (int k = 0; k < 12; ++k) J[k] = d.Jp[12 * o + k];
                const double r0 = d.res[2 * o], r1 = d.res[2 * o + 1];
                for (int m = 0; m < 6; ++m) {
                    TJ[m] = T[0][0] * J[m] + T[0][1] * J[6 + m];
                    TJ[6 + m] = T[1][0] * J[m] + T[1][1] * J[6 + m];
                }
                int tt = 7;
                for (int m = 0; m < 6; ++m) {
                    v[1 + m] = v[1 + m] + (J[m] * J[m] + J[6 + m] * J[6 + m]);
                    for (int n = m; n < 6; ++n, ++tt) v[tt] = v[tt] + (J[m] * TJ[n] + J[6 + m] * TJ[6 + n]);
                    v[28 + m] = v[28 + m] + (J[m] * r0 + J[6 + m] * r1);
                    v[34 + m] = v[34 + m] + (J[m] * e[0] + J[6 + m] * e[1]);
                }
            }
        },
        s);
    if (threadIdx.x != 0) return;
    d.cost_img[i] = s[0];
    double M[36];
    int tt = 7;
    for (int m = 0; m < 6; ++m)
        for (int n = m; n < 6; ++n, ++tt) M[6 * m + n] = M[6 * n + m] = s[tt];
    for (int m = 0; m < 6; ++m) {
        const double dg = ba::lm_diag(s[1 + m], radius);
        d.diag_c[6 * i + m] = s[1 + m];
        d.D_c[6 * i + m] = dg;
        d.g_c[6 * i + m] = s[28 + m];
        d.b_c[6 * i + m] = -s[34 + m];
        M[7 * m] = M[7 * m] + dg;
    }
    for (int m = 0; m < 6; ++m)
        if (!d.ivar[6 * i + m]) {
            for (int n = 0; n < 6; ++n) M[6 * m + n] = M[6 * n + m] = 0.0;
            M[7 * m] = 1.0;
        }
    ba::spd_inverse(M, 6);
    for (int k = 0; k < 36; ++k) d.Minv_i[36 * i + k] = M[k];
}

// 15.6 camera blocks, first pass: one wave per image, the image's partial of its camera's sums
__global__ __launch_bounds__(kWave) void ba_camimg_kernel(Dev d) {
    const uint32_t i = blockIdx.x;
    const uint32_t o0 = d.ioff[i], o1 = d.ioff[i + 1];
    double s[kCamPart];
    wsum<kCamPart>(
        [&](int l, double (&v)[kCamPart]) {
            for (int k = 0; k < kCamPart; ++k) v[k] = 0.0;
            for (uint32_t o = o0 + (uint32_t)l; o < o1; o += kWave) {
                double T[2][2], e[2], J[2 * kKC], TJ[2 * kKC];
                point_elimination(d, o, T, e);
                for (int a = 0; a < 2; ++a)
                    for (int k = 0; k < kKC; ++k)
                        J[kKC * a + k] = (uint32_t)k < d.kc ? d.Jc[(size_t)2 * d.kc * o + d.kc * a + k] : 0.0;
                const double r0 = d.res[2 * o], r1 = d.res[2 * o + 1];
                for (int m = 0; m < kKC; ++m) {
                    TJ[m] = T[0][0] * J[m] + T[0][1] * J[kKC + m];
                    TJ[kKC + m] = T[1][0] * J[m] + T[1][1] * J[kKC + m];
                }
                int tt = 12;
                for (int m = 0; m < kKC; ++m) {
                    v[m] = v[m] + (J[m] * J[m] + J[kKC + m] * J[kKC + m]);
                    for (int n = m; n < kKC; ++n, ++tt) v[tt] = v[tt] + (J[m] * TJ[n] + J[kKC + m] * TJ[kKC + n]);
                    v[90 + m] = v[90 + m] + (J[m] * r0 + J[kKC + m] * r1);
                    v[102 + m] = v[102 + m] + (J[m] * e[0] + J[kKC + m] * e[1]);
                }
            }
        },
        s);
    if (threadIdx.x != 0) return;
    for (int k = 0; k < kCamPart; ++k) d.campart[(size_t)kCamPart * i + k] = s[k];
}

// second pass: a lane per camera joins its images' partials in image order
__global__ __launch_bounds__(kBlock) void ba_camera_kernel(Dev d, double radius) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= d.ncam) return;
    double s[kCamPart];
    for (int k = 0; k < kCamPart; ++k) s[k] = 0.0;
    for (uint32_t k = d.coff[c]; k < d.coff[c + 1]; ++k) {
        const double* part = d.campart + (size_t)kCamPart * d.cimg[k];
        for (int m = 0; m < kCamPart; ++m) s[m] = s[m] + part[m];
    }
    double M[kKC * kKC];
    int tt = 12;
    for (int m = 0; m < kKC; ++m)
        for (int n = m; n < kKC; ++n, ++tt) M[kKC * m + n] = M[kKC * n + m] = s[tt];
    const uint32_t base = 6 * d.nimg + kKC * c;
    for (int m = 0; m < kKC; ++m) {
        const double dg = ba::lm_diag(s[m], radius);
        d.diag_c[base + m] = s[m];
        d.D_c[base + m] = dg;
        d.g_c[base + m] = s[90 + m];
        d.b_c[base + m] = -s[102 + m];
        M[(kKC + 1) * m] = M[(kKC + 1) * m] + dg;
    }
    for (int m = 0; m < kKC; ++m)
        if (!d.cvar[kKC * c + m]) {
            for (int n = 0; n < kKC; ++n) M[kKC * m + n] = M[kKC * n + m] = 0.0;
            M[(kKC + 1) * m] = 1.0;
        }
    ba::spd_inverse(M, kKC);
    for (int k = 0; k < kKC * kKC; ++k) d.Minv_c[(size_t)kKC * kKC * c + k] = M[k];
}

// with every camera constant the camera part of the reduced system is empty
__global__ __launch_bounds__(kBlock) void ba_camera_const_kernel(Dev d) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= kKC * d.ncam) return;
    const uint32_t at = 6 * d.nimg + k;
    d.diag_c[at] = 0.0;
    d.D_c[at] = 0.0;
    d.g_c[at] = 0.0;
    d.b_c[at] = 0.0;
}

__global__ __launch_bounds__(kBlock) void ba_set_scale_kernel(Dev d) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k < d.nred) d.sc_c[k] = 1.0 / (1.0 + ba::dsqrt(d.diag_c[k]));
    if (k < 3 * d.npts) d.sc_p[k] = 1.0 / (1.0 + ba::dsqrt(d.diag_p[k]));
}

// J_c v of one observation: the pose terms in column order from 0.0, then the camera terms in column order
__device__ __forceinline__ void obs_times_reduced(const Dev& d, uint32_t o, uint32_t i, const double* v, double (&a)[2]) {
    const uint32_t c = d.icam[i];
    const double* vi = v + 6 * i;
    const double* vc = v + 6 * d.nimg + kKC * c;
    for (int r = 0; r < 2; ++r) {
        double s = 0.0;
        for (int m = 0; m < 6; ++m) s = s + d.Jp[12 * o + 6 * r + m] * vi[m];
        for (uint32_t k = 0; k < d.kc; ++k) s = s + d.Jc[(size_t)2 * d.kc * o + d.kc * r + k] * vc[k];
        a[r] = s;
    }
}

// 15.6 Schur product, point pass: u_j = Vinv_j sum Jx^T (J_c v).  backsub: yp_j = -(Vinv_j (g_j + sum ...))
__global__ __launch_bounds__(kBlock) void ba_schur_point_kernel(Dev d, const double* v, int backsub) {
    if (!backsub && d.s->done) return;
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= d.npts) return;
    double w[3] = {0, 0, 0};
    for (uint32_t k = d.poff[j]; k < d.poff[j + 1]; ++k) {
        const uint32_t o = d.pobs[k];
        double a[2];
        obs_times_reduced(d, o, d.oimg[o], v, a);
        const double* J = d.Jx + 6 * o;
        for (int m = 0; m < 3; ++m) w[m] = w[m] + (J[m] * a[0] + J[3 + m] * a[1]);
    }
    double out[3];
    if (backsub) {
        for (int m = 0; m < 3; ++m) w[m] = d.gp[3 * j + m] + w[m];
        ba::sym3_mul(d.Vinv + 6 * j, w, out);
        for (int m = 0; m < 3; ++m) d.yp[3 * j + m] = -out[m];
    } else {
        ba::sym3_mul(d.Vinv + 6 * j, w, out);
        for (int m = 0; m < 3; ++m) d.u[3 * j + m] = out[m];
    }
}

// image pass: (S v)_i without the LM diagonal, and the image's part of its camera's rows
__global__ __launch_bounds__(kWave) void ba_schur_image_kernel(Dev d, const double* v) {
    if (d.s->done) return;
    const uint32_t i = blockIdx.x;
    const uint32_t o0 = d.ioff[i], o1 = d.ioff[i + 1];
    double s[18];
    wsum<18>(
        [&](int l, double (&acc)[18]) {
            for (int k = 0; k < 18; ++k) acc[k] = 0.0;
            for (uint32_t o = o0 + (uint32_t)l; o < o1; o += kWave) {
                double a[2];
                obs_times_reduced(d, o, i, v, a);
                const double* Jx = d.Jx + 6 * o;
                const double* u = d.u + 3 * d.opt[o];
                for (int r = 0; r < 2; ++r) a[r] = a[r] - (Jx[3 * r] * u[0] + Jx[3 * r + 1] * u[1] + Jx[3 * r + 2] * u[2]);
                for (int m = 0; m < 6; ++m) acc[m] = acc[m] + (d.Jp[12 * o + m] * a[0] + d.Jp[12 * o + 6 + m] * a[1]);
                for (int k = 0; k < kKC; ++k)
                    if ((uint32_t)k < d.kc)
                        acc[6 + k] = acc[6 + k] + (d.Jc[(size_t)2 * d.kc * o + k] * a[0] + d.Jc[(size_t)2 * d.kc * o + d.kc + k] * a[1]);
            }
        },
        s);
    if (threadIdx.x != 0) return;
    for (int m = 0; m < 6; ++m) d.qv[6 * i + m] = s[m];
    for (int k = 0; k < kKC; ++k) d.campart2[kKC * i + k] = s[6 + k];
}

// |J y|^2 of the whole step per image (15.5: the model cost change)
__global__ __launch_bounds__(kWave) void ba_jy_kernel(Dev d) {
    const uint32_t i = blockIdx.x;
    const uint32_t o0 = d.ioff[i], o1 = d.ioff[i + 1];
    double s[1];
    wsum<1>(
        [&](int l, double (&acc)[1]) {
            acc[0] = 0.0;
            for (uint32_t o = o0 + (uint32_t)l; o < o1; o += kWave) {
                double a[2];
                obs_times_reduced(d, o, i, d.x, a);
                const double* Jx = d.Jx + 6 * o;
                const double* y = d.yp + 3 * d.opt[o];
                for (int r = 0; r < 2; ++r) a[r] = a[r] + (Jx[3 * r] * y[0] + Jx[3 * r + 1] * y[1] + Jx[3 * r + 2] * y[2]);
                acc[0] = acc[0] + (a[0] * a[0] + a[1] * a[1]);
            }
        },
        s);
    if (threadIdx.x == 0) d.jy2_img[i] = s[0];
}

__global__ __launch_bounds__(kWave) void ba_cost_image_kernel(Dev d) {
    const uint32_t i = blockIdx.x;
    const uint32_t o0 = d.ioff[i], o1 = d.ioff[i + 1];
    double s[1];
    wsum<1>(
        [&](int l, double (&acc)[1]) {
            acc[0] = 0.0;
            for (uint32_t o = o0 + (uint32_t)l; o < o1; o += kWave) acc[0] = acc[0] + d.cost[o];
        },
        s);
    if (threadIdx.x == 0) d.cost_img[i] = s[0];
}

// ---- the one-wave kernels: every sum over a vector in the order of 12.10 -----------------------------------------------
template <class F>
__device__ __forceinline__ double wave_total(uint32_t n, F term) {
    double s[1];
    wsum<1>(
        [&](int l, double (&acc)[1]) {
            acc[0] = 0.0;
            for (uint32_t k = (uint32_t)l; k < n; k += kWave) acc[0] = acc[0] + term(k);
        },
        s);
    return s[0];
}

// z = M^-1 r, block by block (a lane takes whole blocks)
__device__ __forceinline__ void precondition(const Dev& d, const double* r, double* z) {
    for (uint32_t blk = threadIdx.x; blk < d.nimg + d.ncam; blk += kWave) {
        const bool img = blk < d.nimg;
        const int n = img ? 6 : kKC;
        const uint32_t at = img ? 6 * blk : 6 * d.nimg + kKC * (blk - d.nimg);
        const double* M = img ? d.Minv_i + 36 * blk : d.Minv_c + (size_t)kKC * kKC * (blk - d.nimg);
        for (int m = 0; m < n; ++m) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s = s + M[n * m + k] * r[at + k];
            z[at + m] = s;
        }
    }
}

__global__ __launch_bounds__(kWave) void ba_pcg_init_kernel(Dev d) {
    const uint32_t n = d.nred;
    for (uint32_t k = threadIdx.x; k < n; k += kWave) {
        d.x[k] = 0.0;
        d.r[k] = d.b_c[k];
    }
    __syncthreads();
    precondition(d, d.r, d.z);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n; k += kWave) d.p[k] = d.z[k];
    const double rz = wave_total(n, [&](uint32_t k) { return d.r[k] * d.z[k]; });
    const double bb = wave_total(n, [&](uint32_t k) { return d.b_c[k] * d.b_c[k]; });
    if (threadIdx.x == 0) {
        d.s->rz = rz;
        d.s->bnorm = ba::dsqrt(bb);
        d.s->iters = 0;
        d.s->kind = bb == 0.0 ? 1 : 0;
        d.s->done = bb == 0.0 ? 1 : 0;
    }
}

__global__ __launch_bounds__(kWave) void ba_pcg_step_kernel(Dev d, int camvar, int max_iters) {
    if (d.s->done) return;
    const uint32_t n = d.nred;
    // q = S p: the cameras' rows from their images' parts in image order, then the LM diagonal
    for (uint32_t c = threadIdx.x; c < d.ncam; c += kWave)
        for (int m = 0; m < kKC; ++m) {
            double s = 0.0;
            if (camvar)
                for (uint32_t k = d.coff[c]; k < d.coff[c + 1]; ++k) s = s + d.campart2[kKC * d.cimg[k] + m];
            d.qv[6 * d.nimg + kKC * c + m] = s;
        }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n; k += kWave) d.qv[k] = d.qv[k] + d.D_c[k] * d.p[k];
    __syncthreads();
    const double pq = wave_total(n, [&](uint32_t k) { return d.p[k] * d.qv[k]; });
    const double rz = d.s->rz;
    const int it = d.s->iters + 1;
    if (!(pq > 0.0) || !ap::finite(pq)) {  // breakdown: keep x
        __syncthreads();
        if (threadIdx.x == 0) {
            d.s->done = 1;
            d.s->kind = 3;
            d.s->iters = it;
        }
        return;
    }
    const double alpha = rz / pq;
    for (uint32_t k = threadIdx.x; k < n; k += kWave) {
        d.x[k] = d.x[k] + alpha * d.p[k];
        d.r[k] = d.r[k] - alpha * d.qv[k];
    }
    __syncthreads();
    const double rr = wave_total(n, [&](uint32_t k) { return d.r[k] * d.r[k]; });
    const bool conv = ba::dsqrt(rr) <= kPcgTolerance * d.s->bnorm;
    if (conv || it >= max_iters) {
        __syncthreads();
        if (threadIdx.x == 0) {
            d.s->done = 1;
            d.s->kind = conv ? 1 : 2;
            d.s->iters = it;
        }
        return;
    }
    precondition(d, d.r, d.z);
    __syncthreads();
    const double rz2 = wave_total(n, [&](uint32_t k) { return d.r[k] * d.z[k]; });
    const double beta = rz2 / rz;
    for (uint32_t k = threadIdx.x; k < n; k += kWave) d.p[k] = d.z[k] + beta * d.p[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        d.s->rz = rz2;
        d.s->iters = it;
    }
}

// the candidate x (+) scale * step
__global__ __launch_bounds__(kBlock) void ba_candidate_kernel(Dev d, Params P, Params N) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k < d.nimg) {
        double dl[6], qn[4];
        for (int m = 0; m < 6; ++m) dl[m] = d.sc_c[6 * k + m] * d.x[6 * k + m];
        ap::quat_plus(P.q + 4 * k, dl, qn);
        for (int m = 0; m < 4; ++m) N.q[4 * k + m] = qn[m];
        for (int m = 0; m < 3; ++m) N.t[3 * k + m] = P.t[3 * k + m] + dl[3 + m];
    }
    if (k < d.ncam)
        for (int m = 0; m < kKC; ++m) {
            const uint32_t at = 6 * d.nimg + kKC * k + m;
            N.cp[kKC * k + m] = P.cp[kKC * k + m] + d.sc_c[at] * d.x[at];
        }
    if (k < d.npts)
        for (int m = 0; m < 3; ++m) N.X[3 * k + m] = P.X[3 * k + m] + d.sc_p[3 * k + m] * d.yp[3 * k + m];
}

// the scalars one LM iteration reads back.  step = 0: cost and the gradient's max norm of the stored evaluation;
// step = 1: the candidate's cost, g.y, |J y|^2, |scale y|^2 and |x|^2
__global__ __launch_bounds__(kWave) void ba_lm_reduce_kernel(Dev d, Params P, int step) {
    const double cost = wave_total(d.nimg, [&](uint32_t i) { return d.cost_img[i]; });
    double o1 = 0.0, o2 = 0.0, o3 = 0.0, o4 = 0.0;
    if (!step) {
        double m = 0.0;
        for (uint32_t k = threadIdx.x; k < d.nred; k += kWave) m = tvg::dmax(m, ba::dabs(d.g_c[k] / d.sc_c[k]));
        for (uint32_t k = threadIdx.x; k < 3 * d.npts; k += kWave) m = tvg::dmax(m, ba::dabs(d.gp[k] / d.sc_p[k]));
        for (int w = 32; w >= 1; w >>= 1) m = tvg::dmax(m, __shfl_xor(m, w));
        o1 = m;
    } else {
        o1 = wave_total(d.nred, [&](uint32_t k) { return d.g_c[k] * d.x[k]; }) +
             wave_total(3 * d.npts, [&](uint32_t k) { return d.gp[k] * d.yp[k]; });
        o2 = wave_total(d.nimg, [&](uint32_t i) { return d.jy2_img[i]; });
        o3 = wave_total(d.nred, [&](uint32_t k) { const double v = d.sc_c[k] * d.x[k]; return v * v; }) +
             wave_total(3 * d.npts, [&](uint32_t k) { const double v = d.sc_p[k] * d.yp[k]; return v * v; });
        o4 = wave_total(4 * d.nimg, [&](uint32_t k) { return P.q[k] * P.q[k]; }) +
             wave_total(3 * d.nimg, [&](uint32_t k) { return P.t[k] * P.t[k]; }) +
             wave_total(kKC * d.ncam, [&](uint32_t k) { return d.cvar[k] ? P.cp[k] * P.cp[k] : 0.0; }) +
             wave_total(3 * d.npts, [&](uint32_t k) { return d.pvar[k / 3] ? P.X[k] * P.X[k] : 0.0; });
    }
    if (threadIdx.x == 0) {
        d.s->out[0] = cost;
        d.s->out[1] = o1;
        d.s->out[2] = o2;
        d.s->out[3] = o3;
        d.s->out[4] = o4;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
inline unsigned blocks_for(size_t n) { return (unsigned)std::max<size_t>((n + kBlock - 1) / kBlock, 1); }

int run(const char* fn, amc_ctx* ctx, amc_ba_problem* pb, const uint8_t* point_const, const amc_ba_opts* opts,
        amc_ba_result* result) {
    const char* const hipchk_who = fn;
    if (!ctx || !pb || !opts || !result) return api_fail(AMC_E_INVALID, "%s: NULL argument", fn);
    std::memset(result, 0, sizeof *result);
    const auto host_t0 = std::chrono::steady_clock::now();
    const amc_ba_opts op = *opts;
    std::string bad = ba::check_options(op);
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: invalid options: %s", fn, bad.c_str());
    // 15.2: the checks, the variable columns, the two CSR orders, the cameras' image lists
    ba::Plan plan;
    try {
        bad = ba::make_plan(*pb, point_const, &plan);
    } catch (const std::bad_alloc&) {
        return api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: %s", fn, bad.c_str());
    const size_t ncam = pb->num_cameras, nimg = pb->num_images, npts = pb->num_points, nobs = pb->num_observations;
    const uint32_t kc = plan.kc;
    const bool camvar = plan.camvar;
    const std::vector<uint8_t>&cvar = plan.cvar, &ivar = plan.ivar;
    const std::vector<uint32_t>&ioff = plan.ioff, &poff = plan.poff, &coff = plan.coff, &cimg = plan.cimg, &oimg = plan.oimg,
          &opt = plan.opt, &pobs = plan.pobs;
    const std::vector<double>& oxy = plan.oxy;
    result->num_images = nimg;
    result->num_points = npts;
    result->num_observations = nobs;
    result->num_variable_parameters = plan.num_variable;
    if (nobs == 0 || plan.num_variable == 0) {  // (no device call: both costs are reported as 0)
        result->termination = AMC_BA_NOTHING_TO_REFINE;
        return AMC_OK;
    }
    const uint32_t nred = (uint32_t)(6 * nimg + kKC * ncam);

    const CtxView cv = ctx_view(ctx);
    HIPCHK(hipSetDevice(cv.device));
    hipStream_t st = cv.stream;
    StreamTimer timer(st);
    HIPCHK(timer.start());
    Dev d{};
    d.nimg = (uint32_t)nimg;
    d.ncam = (uint32_t)ncam;
    d.npts = (uint32_t)npts;
    d.nobs = (uint32_t)nobs;
    d.nred = nred;
    d.kc = kc;
    d.loss = op.loss_function_type;
    d.loss_scale = op.loss_function_scale;
    uint32_t *d_oimg, *d_opt, *d_ioff, *d_poff, *d_pobs, *d_icam, *d_coff, *d_cimg;
    int32_t* d_cmodel;
    uint8_t *d_cvar, *d_ivar, *d_pvar;
    double* d_oxy;
    Params P[2];
    DevBuf<void> mem;
    DevParts parts;
    parts.part(&d_oimg, nobs).part(&d_opt, nobs).part(&d_ioff, nimg + 1).part(&d_poff, npts + 1).part(&d_pobs, nobs)
        .part(&d_icam, nimg).part(&d_coff, ncam + 1).part(&d_cimg, nimg).part(&d_cmodel, ncam)
        .part(&d_cvar, kKC * ncam).part(&d_ivar, 6 * nimg).part(&d_oxy, 2 * nobs);
    for (Params& p : P) parts.part(&p.q, 4 * nimg).part(&p.t, 3 * nimg).part(&p.cp, kKC * ncam).part(&p.X, 3 * npts);
    parts.part(&d.sc_c, nred).part(&d.sc_p, 3 * npts).part(&d.Jp, 12 * nobs).part(&d.Jc, (size_t)2 * kc * nobs)
        .part(&d.Jx, 6 * nobs).part(&d.res, 2 * nobs).part(&d.cost, nobs)
        .part(&d.Vinv, 6 * npts).part(&d.gp, 3 * npts).part(&d.vg, 3 * npts).part(&d.diag_p, 3 * npts)
        .part(&d.g_c, nred).part(&d.b_c, nred).part(&d.D_c, nred).part(&d.diag_c, nred)
        .part(&d.Minv_i, 36 * nimg).part(&d.Minv_c, (size_t)kKC * kKC * ncam).part(&d.cost_img, nimg)
        .part(&d.campart, camvar ? (size_t)kCamPart * nimg : 1)
        .part(&d.x, nred).part(&d.r, nred).part(&d.z, nred).part(&d.p, nred).part(&d.qv, nred)
        .part(&d.u, 3 * npts).part(&d.campart2, kKC * nimg).part(&d.yp, 3 * npts).part(&d.jy2_img, nimg)
        .part(&d.s, 1).part(&d_pvar, npts);
    {
        const hipError_t e = parts.carve(mem);
        if (e == hipErrorOutOfMemory) return api_fail(AMC_E_NOMEM, "%s: out of device memory", fn);
        HIPCHK(e);
    }
    d.oimg = d_oimg;
    d.opt = d_opt;
    d.ioff = d_ioff;
    d.poff = d_poff;
    d.pobs = d_pobs;
    d.icam = d_icam;
    d.coff = d_coff;
    d.cimg = d_cimg;
    d.cmodel = d_cmodel;
    d.cvar = d_cvar;
    d.ivar = d_ivar;
    d.pvar = d_pvar;
    d.oxy = d_oxy;
    auto up = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    const std::vector<double>& cp0 = plan.cparams;
    const std::vector<double> ones(std::max<size_t>(nred, 3 * npts), 1.0);
    HIPCHK(up(d_oimg, oimg.data(), nobs * 4));
    HIPCHK(up(d_opt, opt.data(), nobs * 4));
    HIPCHK(up(d_ioff, ioff.data(), (nimg + 1) * 4));
    HIPCHK(up(d_poff, poff.data(), (npts + 1) * 4));
    HIPCHK(up(d_pobs, pobs.data(), nobs * 4));
    HIPCHK(up(d_icam, pb->image_cameras, nimg * 4));
    HIPCHK(up(d_coff, coff.data(), (ncam + 1) * 4));
    HIPCHK(up(d_cimg, cimg.data(), nimg * 4));
    HIPCHK(up(d_cmodel, pb->camera_models, ncam * 4));
    HIPCHK(up(d_cvar, cvar.data(), kKC * ncam));
    HIPCHK(up(d_ivar, ivar.data(), 6 * nimg));
    HIPCHK(up(d_pvar, plan.pvar.data(), npts));
    HIPCHK(up(d_oxy, oxy.data(), nobs * 16));
    HIPCHK(up(P[0].q, pb->qvec, nimg * 32));
    HIPCHK(up(P[0].t, pb->tvec, nimg * 24));
    HIPCHK(up(P[0].cp, cp0.data(), ncam * kKC * 8));
    HIPCHK(up(P[0].X, pb->xyz, npts * 24));
    HIPCHK(up(d.sc_c, ones.data(), (size_t)nred * 8));
    HIPCHK(up(d.sc_p, ones.data(), npts * 24));
    // with every camera constant no kernel forms the cameras' preconditioner blocks, and precondition() still multiplies
    // them with the residual's exact zeros: they must be finite for the products to be zero
    if (!camvar && ncam) HIPCHK(hipMemsetAsync(d.Minv_c, 0, (size_t)kKC * kKC * ncam * 8, st));

    int cur = 0;
    Scalars hs{};
    auto read_scalars = [&]() -> int {
        HIPCHK(hipMemcpyAsync(&hs, d.s, sizeof hs, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return AMC_OK;
    };
#define BA_LAUNCH(kernel, grid, block, ...)                          \
    do {                                                             \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, __VA_ARGS__); \
        HIPCHK(hipGetLastError());                                   \
    } while (0)
    auto evaluate = [&](int which, int jac) -> int {
        BA_LAUNCH(ba_eval_kernel, blocks_for(nobs), kBlock, d, P[which], jac);
        return AMC_OK;
    };
    auto blocks = [&](double radius) -> int {
        BA_LAUNCH(ba_point_kernel, blocks_for(npts), kBlock, d, radius);
        BA_LAUNCH(ba_image_kernel, (unsigned)nimg, kWave, d, radius);
        if (camvar) {
            BA_LAUNCH(ba_camimg_kernel, (unsigned)nimg, kWave, d);
            BA_LAUNCH(ba_camera_kernel, blocks_for(ncam), kBlock, d, radius);
        } else {
            BA_LAUNCH(ba_camera_const_kernel, blocks_for(kKC * ncam), kBlock, d);
        }
        return AMC_OK;
    };
#define BA_TRY(expr)                   \
    do {                               \
        const int rc_ = (expr);        \
        if (rc_ != AMC_OK) return rc_; \
    } while (0)

    double radius = 1e4, decrease = 2.0;
    // the first evaluation fixes the Jacobi scaling (15.5), the second is the scaled one
    HIPCHK(timer.span_begin());
    BA_TRY(evaluate(cur, 1));
    BA_TRY(blocks(radius));
    BA_LAUNCH(ba_set_scale_kernel, blocks_for(std::max<size_t>(nred, 3 * npts)), kBlock, d);
    BA_TRY(evaluate(cur, 1));
    BA_TRY(blocks(radius));
    BA_LAUNCH(ba_lm_reduce_kernel, 1, kWave, d, P[cur], 0);
    HIPCHK(timer.span_end());
    BA_TRY(read_scalars());
    double cost = hs.out[0];
    result->initial_cost = cost;
    int term = AMC_BA_MAX_ITERATIONS;
    bool stop = false;
    if (!ap::finite(cost)) {
        term = AMC_BA_INVALID_STEPS;
        stop = true;
    } else if (hs.out[1] <= op.gradient_tolerance) {
        term = AMC_BA_GRADIENT_TOLERANCE;
        stop = true;
    }
    int invalid_run = 0;
    for (int it = 1; !stop && it <= op.max_num_iterations; ++it) {
        // the linear step: PCG on the Schur complement, queued kPcgChunk iterations at a time
        HIPCHK(timer.span_begin());
        BA_LAUNCH(ba_pcg_init_kernel, 1, kWave, d);
        HIPCHK(timer.span_end());
        for (;;) {
            HIPCHK(timer.span_begin());
            for (int k = 0; k < kPcgChunk; ++k) {
                BA_LAUNCH(ba_schur_point_kernel, blocks_for(npts), kBlock, d, (const double*)d.p, 0);
                BA_LAUNCH(ba_schur_image_kernel, (unsigned)nimg, kWave, d, (const double*)d.p);
                BA_LAUNCH(ba_pcg_step_kernel, 1, kWave, d, camvar ? 1 : 0, (int)op.max_linear_solver_iterations);
            }
            HIPCHK(timer.span_end());
            BA_TRY(read_scalars());
            if (hs.done) break;
        }
        result->num_pcg_iterations += (uint32_t)hs.iters;
        if (hs.kind == 1) ++result->num_pcg_stops_residual;
        if (hs.kind == 2) ++result->num_pcg_stops_cap;
        // back-substitution, the model cost change's terms, the candidate and its cost
        HIPCHK(timer.span_begin());
        BA_LAUNCH(ba_schur_point_kernel, blocks_for(npts), kBlock, d, (const double*)d.x, 1);
        BA_LAUNCH(ba_jy_kernel, (unsigned)nimg, kWave, d);
        BA_LAUNCH(ba_candidate_kernel, blocks_for(std::max(std::max(nimg, ncam), npts)), kBlock, d, P[cur], P[cur ^ 1]);
        BA_TRY(evaluate(cur ^ 1, 0));
        BA_LAUNCH(ba_cost_image_kernel, (unsigned)nimg, kWave, d);
        BA_LAUNCH(ba_lm_reduce_kernel, 1, kWave, d, P[cur], 1);
        HIPCHK(timer.span_end());
        BA_TRY(read_scalars());
        const double cand = hs.out[0], gy = hs.out[1], jy2 = hs.out[2], step2 = hs.out[3], x2 = hs.out[4];
        const double mcc = -(gy + 0.5 * jy2);
        bool rejected = false;
        if (!(ap::finite(mcc) && mcc > 0.0)) {  // an invalid step
            ++result->num_unsuccessful_steps;
            if (++invalid_run >= op.max_num_consecutive_invalid_steps) {
                term = AMC_BA_INVALID_STEPS;
                break;
            }
            rejected = true;
        } else {
            invalid_run = 0;
            if (ba::dsqrt(step2) <= op.parameter_tolerance * (ba::dsqrt(x2) + op.parameter_tolerance)) {
                term = AMC_BA_PARAMETER_TOLERANCE;
                break;
            }
            const double new_cost = ap::finite(cand) ? cand : DBL_MAX;
            const double change = cost - new_cost;
            if (ba::dabs(change) <= op.function_tolerance * cost) {
                term = AMC_BA_FUNCTION_TOLERANCE;
                break;
            }
            const double rel = change / mcc;
            if (rel > 1e-3) {
                ++result->num_successful_steps;
                cur ^= 1;
                const double z = 2.0 * rel - 1.0;
                const double f = 1.0 - z * z * z;
                radius = radius / (f > 1.0 / 3.0 ? f : 1.0 / 3.0);
                radius = radius < 1e16 ? radius : 1e16;
                decrease = 2.0;
                HIPCHK(timer.span_begin());
                BA_TRY(evaluate(cur, 1));
                BA_TRY(blocks(radius));
                BA_LAUNCH(ba_lm_reduce_kernel, 1, kWave, d, P[cur], 0);
                HIPCHK(timer.span_end());
                BA_TRY(read_scalars());
                cost = hs.out[0];
                if (hs.out[1] <= op.gradient_tolerance) {
                    term = AMC_BA_GRADIENT_TOLERANCE;
                    break;
                }
            } else {
                ++result->num_unsuccessful_steps;
                rejected = true;
            }
        }
        if (rejected) {
            radius = radius / decrease;
            decrease = 2.0 * decrease;
            if (radius < 1e-32) {
                term = AMC_BA_MIN_RADIUS;
                break;
            }
            HIPCHK(timer.span_begin());
            BA_TRY(blocks(radius));  // (cost[] now holds the candidate's terms, so cost_img does too: it is not read until the next candidate)
            HIPCHK(timer.span_end());
        }
    }
#undef BA_LAUNCH
#undef BA_TRY
    result->final_cost = cost;
    result->termination = term;
    std::vector<double> oq(4 * nimg), ot(3 * nimg), ocp(kKC * ncam), oX(3 * npts);
    HIPCHK(hipMemcpyAsync(oq.data(), P[cur].q, nimg * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(ot.data(), P[cur].t, nimg * 24, hipMemcpyDeviceToHost, st));
    if (ncam) HIPCHK(hipMemcpyAsync(ocp.data(), P[cur].cp, ncam * kKC * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(oX.data(), P[cur].X, npts * 24, hipMemcpyDeviceToHost, st));
    HIPCHK(timer.stop(result->device_ms));
    HIPCHK(timer.spans(result->kernel_ms));
    std::memcpy(pb->qvec, oq.data(), nimg * 32);
    std::memcpy(pb->tvec, ot.data(), nimg * 24);
    for (size_t c = 0; c < ncam; ++c)
        for (int k = 0; k < cam::num_params(pb->camera_models[c]); ++k) pb->camera_params[kKC * c + k] = ocp[kKC * c + k];
    std::memcpy(pb->xyz, oX.data(), npts * 24);
    result->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count() - result->device_ms;
    return AMC_OK;
}

}  // namespace

extern "C" {

void amc_ba_opts_default(amc_ba_opts* o) {
    if (!o) return;
    o->loss_function_type = AMC_BA_LOSS_TRIVIAL;  // BundleAdjustmentOptions() of COLMAP 3.9.1
    o->max_num_iterations = 100;
    o->max_linear_solver_iterations = 200;
    o->max_num_consecutive_invalid_steps = 10;
    o->loss_function_scale = 1.0;
    o->function_tolerance = 0.0;
    o->gradient_tolerance = 0.0;
    o->parameter_tolerance = 0.0;
}

int amc_bundle_adjust(amc_ctx* ctx, amc_ba_problem* problem, const amc_ba_opts* options, amc_ba_result* result) {
    return run("amc_bundle_adjust", ctx, problem, nullptr, options, result);
}

int amc_bundle_adjust_masked(amc_ctx* ctx, amc_ba_problem* problem, const uint8_t* point_const, const amc_ba_opts* options,
                             amc_ba_result* result) {
    return run("amc_bundle_adjust_masked", ctx, problem, point_const, options, result);
}

}  // extern "C"
