// bacov.hip — bundle-adjustment covariance on gfx950 (include/amc_bacov.h): DESIGN.md section 24.  The per-observation
// arithmetic is ba_core.h's, the plans are bacov_plan.h's; this file is the kernels and the C entry point.
//
// Work split (24.3, 24.4).  Every sum has one destination and a written order, so there are no atomics.  Formation: a
// lane per observation stores the Jacobian blocks; a lane per point inverts its block; a lane per (point, owner, column)
// stores W and V^-1 W; a wave per (image, entry) sums J_c^T J_c in 15.7's per-image order; a workgroup per destination
// block subtracts its points' terms in ascending point index.  The dense passes work on 64 x 64 tiles through LDS with
// one launch per panel step: an entry's updates arrive in ascending k because the steps do.  No MFMA: plain FP64
// multiplies and adds, contraction off.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "amc_internal.h"
#include "bacov_core.h"
#include "bacov_plan.h"
#include "../../include/amc_bacov.h"

using namespace amc;

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kKC = ba::kMaxParams;
constexpr int T = bacov::kTile;
constexpr int kPad = T + 2;  // LDS row stride of a tile in doubles

struct Status {
    int32_t fail, pad;
    int64_t fail_col;
    double min_ratio;
};

struct Dev {
    uint32_t nimg, ncam, npts, nobs, kc, m, ld, nslots;
    int32_t loss;
    double loss_scale, damping;
    const uint32_t *oimg, *opt, *ioff, *poff, *pobs, *icam, *coff, *cimg;
    const int32_t *cmodel, *icol, *ccol;
    const uint8_t* pvar;
    const double *oxy, *q, *t, *cp, *X;
    const uint32_t *ocol, *col_coord, *spo, *slot_owner, *slot_point, *dest_a, *dest_b, *dest_off, *pair_a, *pair_b;
    double *Jp, *Jc, *Jx, *Vinv, *W, *Y, *campart, *S, *Z, *Sig, *sdiag, *pcov;
    Status* st;
};

// ---- 24.3: evaluation and formation ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void bacov_eval_kernel(Dev d) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    if (o >= d.nobs) return;
    const uint32_t i = d.oimg[o], j = d.opt[o], c = d.icam[i];
    double r[2], Jp[12], Jc[2 * kKC], Jx[6];
    ba::observation(d.cmodel[c], d.cp + kKC * c, d.q + 4 * i, d.t + 3 * i, d.X + 3 * j, d.oxy + 2 * o, d.loss, d.loss_scale,
                    true, r, Jp, Jc, Jx);
    for (int k = 0; k < 12; ++k) d.Jp[12 * (size_t)o + k] = Jp[k];
    for (int a = 0; a < 2; ++a)
        for (uint32_t k = 0; k < d.kc; ++k) d.Jc[(size_t)2 * d.kc * o + d.kc * a + k] = Jc[kKC * a + k];
    for (int k = 0; k < 6; ++k) d.Jx[6 * (size_t)o + k] = Jx[k];
}

// V_j = sum J_x^T J_x + damping I over point order, inverted by the adjugate
__global__ __launch_bounds__(kBlock) void bacov_point_kernel(Dev d) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= d.npts || !d.pvar[j]) return;
    double V[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t k = d.poff[j]; k < d.poff[j + 1]; ++k) {
        const double* J = d.Jx + 6 * (size_t)d.pobs[k];
        V[0] = V[0] + (J[0] * J[0] + J[3] * J[3]);
        V[1] = V[1] + (J[0] * J[1] + J[3] * J[4]);
        V[2] = V[2] + (J[0] * J[2] + J[3] * J[5]);
        V[3] = V[3] + (J[1] * J[1] + J[4] * J[4]);
        V[4] = V[4] + (J[1] * J[2] + J[4] * J[5]);
        V[5] = V[5] + (J[2] * J[2] + J[5] * J[5]);
    }
    V[0] = V[0] + d.damping;
    V[3] = V[3] + d.damping;
    V[5] = V[5] + d.damping;
    double Vi[6];
    ba::sym3_inverse(V, Vi);
    for (int a = 0; a < 6; ++a) d.Vinv[6 * (size_t)j + a] = Vi[a];
}

// W_{j,owner} (3 x k) over the point's observations of that owner in point order, and Y = V_j^-1 W: a lane per column
__global__ __launch_bounds__(kBlock) void bacov_w_kernel(Dev d) {
    const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t s = tid / kKC;
    const uint32_t p = (uint32_t)(tid % kKC);
    if (s >= d.nslots) return;
    const uint32_t owner = d.slot_owner[s], j = d.slot_point[s];
    if (p >= d.ocol[owner + 1] - d.ocol[owner]) return;
    const uint32_t coord = d.col_coord[d.ocol[owner] + p];
    const bool is_img = owner < d.nimg;
    double w[3] = {0, 0, 0};
    for (uint32_t k = d.poff[j]; k < d.poff[j + 1]; ++k) {
        const uint32_t o = d.pobs[k], i = d.oimg[o];
        if (is_img ? i != owner : d.icam[i] != owner - d.nimg) continue;
        const double j0 = is_img ? d.Jp[12 * (size_t)o + coord] : d.Jc[(size_t)2 * d.kc * o + coord];
        const double j1 = is_img ? d.Jp[12 * (size_t)o + 6 + coord] : d.Jc[(size_t)2 * d.kc * o + d.kc + coord];
        const double* Jx = d.Jx + 6 * (size_t)o;
        for (int a = 0; a < 3; ++a) w[a] = w[a] + (Jx[a] * j0 + Jx[3 + a] * j1);
    }
    double y[3];
    ba::sym3_mul(d.Vinv + 6 * (size_t)j, w, y);
    for (int a = 0; a < 3; ++a) {
        d.W[(3 * s + a) * kKC + p] = w[a];
        d.Y[(3 * s + a) * kKC + p] = y[a];
    }
}

// B: entry (u, v), u >= v, of J_c^T J_c over the image's segment in 12.10's order.  Grid (171, nimg), one wave each.
__global__ __launch_bounds__(kWave) void bacov_b_kernel(Dev d) {
    const uint32_t i = blockIdx.y, c = d.icam[i];
    int u, v;
    bacov::tri_decode((int)blockIdx.x, u, v);
    const int32_t cu = u < 6 ? d.icol[6 * i + u] : d.ccol[kKC * c + (u - 6)];
    const int32_t cv = v < 6 ? d.icol[6 * i + v] : d.ccol[kKC * c + (v - 6)];
    if (cu < 0 || cv < 0) return;
    const uint32_t o0 = d.ioff[i], o1 = d.ioff[i + 1];
    double s = 0.0;
    for (uint32_t o = o0 + threadIdx.x; o < o1; o += kWave) {
        const double* jp = d.Jp + 12 * (size_t)o;
        const double* jc = d.Jc + (size_t)2 * d.kc * o;
        const double u0 = u < 6 ? jp[u] : jc[u - 6], u1 = u < 6 ? jp[6 + u] : jc[d.kc + (u - 6)];
        const double v0 = v < 6 ? jp[v] : jc[v - 6], v1 = v < 6 ? jp[6 + v] : jc[d.kc + (v - 6)];
        s = s + (u0 * v0 + u1 * v1);
    }
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) s = s + __shfl_xor(s, w);
    if (threadIdx.x != 0) return;
    if (v >= 6)
        d.campart[(size_t)bacov::kCamPairs * i + ((u - 6) * (u - 5) / 2 + (v - 6))] = s;
    else
        d.S[(size_t)cu * d.ld + cv] = s;
}

// a camera's block of B: its images' partials from 0.0 in ascending image index
__global__ __launch_bounds__(kBlock) void bacov_bcam_kernel(Dev d) {
    const uint32_t tid = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t c = tid / bacov::kCamPairs, e = tid % bacov::kCamPairs;
    if (c >= d.ncam) return;
    int a, b;
    bacov::tri_decode((int)e, a, b);
    const int32_t ca = d.ccol[kKC * c + a], cb = d.ccol[kKC * c + b];
    if (ca < 0 || cb < 0) return;
    double s = 0.0;
    for (uint32_t k = d.coff[c]; k < d.coff[c + 1]; ++k) s = s + d.campart[(size_t)bacov::kCamPairs * d.cimg[k] + e];
    d.S[(size_t)ca * d.ld + cb] = s;
}

// S = B - sum_j W_jA^T V_j^-1 W_jB: a workgroup per destination block, a lane per entry, the block's points in order
__global__ __launch_bounds__(kWave) void bacov_dest_kernel(Dev d) {
    const uint32_t blk = blockIdx.x;
    const uint32_t A = d.dest_a[blk], B = d.dest_b[blk];
    const uint32_t ra = d.ocol[A], rb = d.ocol[B], ka = d.ocol[A + 1] - ra, kb = d.ocol[B + 1] - rb;
    const uint32_t t0 = d.dest_off[blk], t1 = d.dest_off[blk + 1];
    for (uint32_t e = threadIdx.x; e < ka * kb; e += kWave) {
        const uint32_t p = e / kb, q = e % kb;
        if (A == B && q > p) continue;
        double* at = d.S + (size_t)(ra + p) * d.ld + (rb + q);
        double acc = *at;
        const auto term = [&](uint32_t t) {
            const double* y = d.Y + (size_t)3 * kKC * d.pair_a[t] + p;
            const double* w = d.W + (size_t)3 * kKC * d.pair_b[t] + q;
            return y[0] * w[0] + y[kKC] * w[kKC] + y[2 * kKC] * w[2 * kKC];
        };
        uint32_t t = t0;
        for (; t + 8 <= t1; t += 8) {  // eight terms' loads in flight, then the one chain in order
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = term(t + k);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc = acc - v[k];
        }
        for (; t < t1; ++t) acc = acc - term(t);
        *at = acc;
    }
}

// the padding's unit diagonal (rows m .. ld of S) and the diagonal of S for the pivot ratios
__global__ __launch_bounds__(kBlock) void bacov_diag_kernel(Dev d) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= d.ld) return;
    if (k >= d.m) d.S[(size_t)k * d.ld + k] = 1.0;
    d.sdiag[k] = d.S[(size_t)k * d.ld + k];
}

// ---- 24.4: Cholesky, one tile-wide panel per step ----------------------------------------------------------------------
// the diagonal tile of step kb: right-looking inside the tile, so an entry's chain goes on in ascending k
__global__ __launch_bounds__(kWave) void bacov_chol_diag_kernel(Dev d, uint32_t kb) {
    if (d.st->fail) return;
    __shared__ double A[T][kPad];
    const uint32_t tid = threadIdx.x, base = kb * T;
    for (int r = 0; r < T; ++r) A[r][tid] = d.S[(size_t)(base + r) * d.ld + base + tid];
    __syncthreads();
    double minr = d.st->min_ratio;
    for (uint32_t q = 0; q < (uint32_t)T; ++q) {
        const double piv = A[q][q];
        if (!(piv > 0.0) || !ap::finite(piv)) {  // (the same value in every lane: the whole workgroup leaves)
            if (tid == 0) {
                d.st->fail = 1;
                d.st->fail_col = (int64_t)(base + q);
                d.st->min_ratio = minr;
            }
            return;
        }
        const double l = ba::dsqrt(piv);
        if (base + q < d.m) {
            const double ratio = piv / d.sdiag[base + q];
            minr = ratio < minr ? ratio : minr;
        }
        __syncthreads();
        if (tid == q) A[q][q] = l;
        if (tid > q) A[tid][q] = A[tid][q] / l;
        __syncthreads();
        if (tid > q) {
            const double lp = A[tid][q];
            for (uint32_t c = q + 1; c <= tid; ++c) A[tid][c] = A[tid][c] - lp * A[c][q];
        }
        __syncthreads();
    }
    for (uint32_t r = 0; r < (uint32_t)T; ++r)
        if (tid <= r) d.S[(size_t)(base + r) * d.ld + base + tid] = A[r][tid];
    if (tid == 0) d.st->min_ratio = minr;
}

// the tiles below it: a lane per row, L_pq = (acc - sum_{k < q in the tile} L_pk L_qk) / L_qq
__global__ __launch_bounds__(kWave) void bacov_chol_panel_kernel(Dev d, uint32_t kb) {
    if (d.st->fail) return;
    __shared__ double Ld[T][kPad], R[T][kPad];
    const uint32_t tid = threadIdx.x, cbase = kb * T, rbase = (kb + 1 + blockIdx.x) * T;
    for (int r = 0; r < T; ++r) {
        Ld[r][tid] = d.S[(size_t)(cbase + r) * d.ld + cbase + tid];
        R[r][tid] = d.S[(size_t)(rbase + r) * d.ld + cbase + tid];
    }
    __syncthreads();
    for (int q = 0; q < T; ++q) {
        double v = R[tid][q];
        for (int k = 0; k < q; ++k) v = v - R[tid][k] * Ld[q][k];
        R[tid][q] = v / Ld[q][q];
    }
    __syncthreads();
    for (int r = 0; r < T; ++r) d.S[(size_t)(rbase + r) * d.ld + cbase + tid] = R[r][tid];
}

// 64 x 64 x 64 in a 256-lane workgroup, 4 x 4 entries per lane, k ascending: acc = acc -/+ a[k][row] * b[k][col]
template <bool kAdd>
__device__ __forceinline__ void tile_mac(const double (*a)[kPad], const double (*b)[kPad], int ty, int tx, double (&acc)[4][4]) {
    for (int k = 0; k < T; ++k) {
        double av[4], bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            av[i] = a[k][4 * ty + i];
            bv[i] = b[k][4 * tx + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = kAdd ? acc[i][j] + av[i] * bv[j] : acc[i][j] - av[i] * bv[j];
    }
}

// the trailing update of step kb: tile (ib, jb), kb < jb <= ib, loses L_ib,kb L_jb,kb^T
__global__ __launch_bounds__(kBlock) void bacov_chol_update_kernel(Dev d, uint32_t kb) {
    if (d.st->fail) return;
    if (blockIdx.y > blockIdx.x) return;
    __shared__ double Pa[T][kPad], Pb[T][kPad];  // [k][row]
    const uint32_t tid = threadIdx.x, ibase = (kb + 1 + blockIdx.x) * T, jbase = (kb + 1 + blockIdx.y) * T, kbase = kb * T;
    for (uint32_t e = tid; e < (uint32_t)(T * T); e += kBlock) {
        const uint32_t r = e / T, c = e % T;
        Pa[c][r] = d.S[(size_t)(ibase + r) * d.ld + kbase + c];
        Pb[c][r] = d.S[(size_t)(jbase + r) * d.ld + kbase + c];
    }
    __syncthreads();
    const int ty = tid / 16, tx = tid % 16;
    double acc[4][4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) acc[i][j] = d.S[(size_t)(ibase + 4 * ty + i) * d.ld + jbase + 4 * tx + j];
    tile_mac<false>(Pa, Pb, ty, tx, acc);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) d.S[(size_t)(ibase + 4 * ty + i) * d.ld + jbase + 4 * tx + j] = acc[i][j];
}

// ---- 24.5: Z = L^-1 by block rows, then Sigma = Z^T Z -------------------------------------------------------------------
// tile (ib, cb), cb <= ib: identity minus the products with the block rows above, then the solve inside the tile
__global__ __launch_bounds__(kBlock) void bacov_inv_row_kernel(Dev d, uint32_t ib) {
    if (d.st->fail) return;
    __shared__ double Pa[T][kPad], Pb[T][kPad];
    const uint32_t tid = threadIdx.x, cb = blockIdx.x, rbase = ib * T, cbase = cb * T;
    const int ty = tid / 16, tx = tid % 16;
    double acc[4][4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) acc[i][j] = (ib == cb && 4 * ty + i == 4 * tx + j) ? 1.0 : 0.0;
    for (uint32_t kt = cb; kt < ib; ++kt) {
        __syncthreads();
        for (uint32_t e = tid; e < (uint32_t)(T * T); e += kBlock) {
            const uint32_t r = e / T, c = e % T;
            Pa[c][r] = d.S[(size_t)(rbase + r) * d.ld + kt * T + c];  // L[p][k] as [k][p]
            Pb[r][c] = d.Z[(size_t)(kt * T + r) * d.ld + cbase + c];  // Z[k][c]
        }
        __syncthreads();
        tile_mac<false>(Pa, Pb, ty, tx, acc);
    }
    __syncthreads();
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) Pb[4 * ty + i][4 * tx + j] = acc[i][j];  // the tile [p][c]
    for (uint32_t e = tid; e < (uint32_t)(T * T); e += kBlock) {
        const uint32_t r = e / T, c = e % T;
        Pa[r][c] = d.S[(size_t)(rbase + r) * d.ld + rbase + c];  // the diagonal tile of L as [p][k]
    }
    __syncthreads();
    if (tid < (uint32_t)T) {
        for (int p = 0; p < T; ++p) {
            double v = Pb[p][tid];
            for (int k = 0; k < p; ++k) v = v - Pa[p][k] * Pb[k][tid];
            Pb[p][tid] = v / Pa[p][p];
        }
    }
    __syncthreads();
    for (uint32_t e = tid; e < (uint32_t)(T * T); e += kBlock) {
        const uint32_t r = e / T, c = e % T;
        d.Z[(size_t)(rbase + r) * d.ld + cbase + c] = Pb[r][c];
    }
}

// tile (ab, bb), bb <= ab, of Z^T Z and its mirror image; the block rows above ab hold zeros in column block ab
__global__ __launch_bounds__(kBlock) void bacov_ztz_kernel(Dev d) {
    if (d.st->fail) return;
    if (blockIdx.y > blockIdx.x) return;
    __shared__ double Pa[T][kPad], Pb[T][kPad];
    const uint32_t tid = threadIdx.x, ab = blockIdx.x, bb = blockIdx.y, nt = d.ld / T;
    const int ty = tid / 16, tx = tid % 16;
    double acc[4][4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (uint32_t kt = ab; kt < nt; ++kt) {
        __syncthreads();
        for (uint32_t e = tid; e < (uint32_t)(T * T); e += kBlock) {
            const uint32_t r = e / T, c = e % T;
            Pa[r][c] = d.Z[(size_t)(kt * T + r) * d.ld + ab * T + c];
            Pb[r][c] = d.Z[(size_t)(kt * T + r) * d.ld + bb * T + c];
        }
        __syncthreads();
        tile_mac<true>(Pa, Pb, ty, tx, acc);
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const size_t a = ab * T + 4 * ty + i, b = bb * T + 4 * tx + j;
            d.Sig[a * d.ld + b] = acc[i][j];
            if (ab != bb) d.Sig[b * d.ld + a] = acc[i][j];
        }
}

// ---- 24.6: point blocks ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void bacov_pointcov_kernel(Dev d) {
    if (d.st->fail) return;
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= d.npts || !d.pvar[j]) return;
    double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t s0 = d.spo[j], s1 = d.spo[j + 1];
    for (uint32_t sa = s0; sa < s1; ++sa) {
        const uint32_t ra = d.ocol[d.slot_owner[sa]], ka = d.ocol[d.slot_owner[sa] + 1] - ra;
        const double* wa = d.W + (size_t)3 * kKC * sa;
        for (uint32_t sb = s0; sb < s1; ++sb) {
            const uint32_t rb = d.ocol[d.slot_owner[sb]], kb = d.ocol[d.slot_owner[sb] + 1] - rb;
            const double* wb = d.W + (size_t)3 * kKC * sb;
            for (uint32_t p = 0; p < ka; ++p)
                for (uint32_t q = 0; q < kb; ++q) {
                    const double sig = d.Sig[(size_t)(ra + p) * d.ld + rb + q];
                    for (int a = 0; a < 3; ++a) {
                        const double ws = wa[a * kKC + p] * sig;
                        for (int b = 0; b < 3; ++b) M[3 * a + b] = M[3 * a + b] + ws * wb[b * kKC + q];
                    }
                }
        }
    }
    double out[9];
    bacov::point_cov_finish(d.Vinv + 6 * (size_t)j, M, out);
    for (int a = 0; a < 9; ++a) d.pcov[9 * (size_t)j + a] = out[a];
}

// ---- host side ---------------------------------------------------------------------------------------------------------
inline unsigned blocks_for(size_t n) { return (unsigned)std::max<size_t>((n + kBlock - 1) / kBlock, 1); }

void free_arrays(amc_bacov_result* r) {
    std::free(r->column_owner);
    std::free(r->column_coord);
    std::free(r->matrix);
    std::free(r->point_present);
    std::free(r->point_cov);
    r->column_owner = r->column_coord = nullptr;
    r->matrix = r->point_cov = nullptr;
    r->point_present = nullptr;
}

struct Events {
    hipEvent_t e[AMC_BACOV_PHASES + 1] = {};
    ~Events() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

int run(amc_ctx* ctx, const amc_ba_problem* pb, const uint8_t* point_const, const amc_bacov_opts* opts,
        amc_bacov_result* result) {
    const char* const fn = "amc_ba_covariance";
    const char* const hipchk_who = fn;
    if (!ctx || !pb || !opts || !result) return api_fail(AMC_E_INVALID, "%s: NULL argument", fn);
    std::memset(result, 0, sizeof *result);
    result->failed_column = -1;
    result->min_pivot_ratio = 1.0;
    const auto host_t0 = std::chrono::steady_clock::now();
    const amc_bacov_opts op = *opts;
    std::string bad = bacov::check_options(op);
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: invalid options: %s", fn, bad.c_str());
    bacov::Plan plan;
    try {
        bad = bacov::make_plan(*pb, point_const, &plan);
    } catch (const std::bad_alloc&) {
        return api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: %s", fn, bad.c_str());
    const size_t ncam = pb->num_cameras, nimg = pb->num_images, npts = pb->num_points, nobs = pb->num_observations;
    const size_t m = plan.m;
    if (m > AMC_BACOV_MAX_COLUMNS)
        return api_fail(AMC_E_INVALID, "%s: %zu variable columns (at most %d)", fn, m, AMC_BACOV_MAX_COLUMNS);
    result->num_columns = m;
    result->num_points = npts;
    result->success = 1;
    const bool want_points = op.want_points != 0, want_matrix = op.want_matrix != 0;
    result->column_owner = (uint32_t*)std::calloc(std::max<size_t>(m, 1), 4);
    result->column_coord = (uint32_t*)std::calloc(std::max<size_t>(m, 1), 4);
    if (want_matrix) result->matrix = (double*)std::calloc(std::max<size_t>(m * m, 1), 8);
    if (want_points) {
        result->point_present = (uint8_t*)std::calloc(std::max<size_t>(npts, 1), 1);
        result->point_cov = (double*)std::calloc(std::max<size_t>(9 * npts, 1), 8);
    }
    if (!result->column_owner || !result->column_coord || (want_matrix && !result->matrix) ||
        (want_points && (!result->point_present || !result->point_cov))) {
        free_arrays(result);
        return api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    struct Guard {  // an error from here on frees the result's arrays
        amc_bacov_result* r;
        bool armed = true;
        ~Guard() {
            if (armed) free_arrays(r);
        }
    } guard{result};
    if (m == 0) {  // nothing is variable in the reduced system: no device call (24.7)
        result->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count();
        guard.armed = false;
        return AMC_OK;
    }
    std::memcpy(result->column_owner, plan.col_owner.data(), m * 4);
    std::memcpy(result->column_coord, plan.col_coord.data(), m * 4);

    const uint32_t kc = plan.ba.kc;
    const size_t ld = (m + T - 1) / T * T, nt = ld / T;
    const size_t nslots = plan.slot_owner.size(), ndest = plan.dest_a.size(), npairs = plan.pair_a.size();
    const CtxView cv = ctx_view(ctx);
    HIPCHK(hipSetDevice(cv.device));
    hipStream_t st = cv.stream;
    StreamTimer timer(st);
    Events ev;
    HIPCHK(create_events(ev.e, AMC_BACOV_PHASES + 1));
    HIPCHK(timer.start());

    Dev d{};
    d.nimg = (uint32_t)nimg;
    d.ncam = (uint32_t)ncam;
    d.npts = (uint32_t)npts;
    d.nobs = (uint32_t)nobs;
    d.kc = kc;
    d.m = (uint32_t)m;
    d.ld = (uint32_t)ld;
    d.nslots = (uint32_t)nslots;
    d.loss = op.loss_function_type;
    d.loss_scale = op.loss_function_scale;
    d.damping = op.damping;
    uint32_t *d_oimg, *d_opt, *d_ioff, *d_poff, *d_pobs, *d_icam, *d_coff, *d_cimg, *d_ocol, *d_colcoord, *d_spo, *d_sown,
        *d_spt, *d_da, *d_db, *d_doff, *d_pa, *d_pb;
    int32_t *d_cmodel, *d_icol, *d_ccol;
    uint8_t* d_pvar;
    double *d_oxy, *d_q, *d_t, *d_cp, *d_X;
    DevBuf<void> mem;
    DevParts parts;
    parts.part(&d_oimg, nobs).part(&d_opt, nobs).part(&d_ioff, nimg + 1).part(&d_poff, npts + 1).part(&d_pobs, nobs)
        .part(&d_icam, nimg).part(&d_coff, ncam + 1).part(&d_cimg, nimg).part(&d_cmodel, ncam).part(&d_icol, 6 * nimg)
        .part(&d_ccol, kKC * ncam).part(&d_pvar, npts).part(&d_oxy, 2 * nobs).part(&d_q, 4 * nimg).part(&d_t, 3 * nimg)
        .part(&d_cp, kKC * ncam).part(&d_X, 3 * npts).part(&d_ocol, plan.nown + 1).part(&d_colcoord, m)
        .part(&d_spo, npts + 1).part(&d_sown, nslots).part(&d_spt, nslots).part(&d_da, ndest).part(&d_db, ndest)
        .part(&d_doff, ndest + 1).part(&d_pa, npairs).part(&d_pb, npairs)
        .part(&d.Jp, 12 * nobs).part(&d.Jc, (size_t)2 * kc * nobs).part(&d.Jx, 6 * nobs).part(&d.Vinv, 6 * npts)
        .part(&d.W, 3 * kKC * nslots).part(&d.Y, 3 * kKC * nslots).part(&d.campart, (size_t)bacov::kCamPairs * nimg)
        .part(&d.S, ld * ld).part(&d.Z, ld * ld).part(&d.Sig, ld * ld).part(&d.sdiag, ld).part(&d.pcov, 9 * npts)
        .part(&d.st, 1);
    {
        const hipError_t e = parts.carve(mem);
        if (e == hipErrorOutOfMemory) return api_fail(AMC_E_NOMEM, "%s: out of device memory", fn);
        HIPCHK(e);
    }
    d.oimg = d_oimg; d.opt = d_opt; d.ioff = d_ioff; d.poff = d_poff; d.pobs = d_pobs; d.icam = d_icam; d.coff = d_coff;
    d.cimg = d_cimg; d.cmodel = d_cmodel; d.icol = d_icol; d.ccol = d_ccol; d.pvar = d_pvar; d.oxy = d_oxy; d.q = d_q;
    d.t = d_t; d.cp = d_cp; d.X = d_X; d.ocol = d_ocol; d.col_coord = d_colcoord; d.spo = d_spo; d.slot_owner = d_sown;
    d.slot_point = d_spt; d.dest_a = d_da; d.dest_b = d_db; d.dest_off = d_doff; d.pair_a = d_pa; d.pair_b = d_pb;
    auto up = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    const bacov::Plan& p = plan;
    HIPCHK(up(d_oimg, p.ba.oimg.data(), nobs * 4));
    HIPCHK(up(d_opt, p.ba.opt.data(), nobs * 4));
    HIPCHK(up(d_ioff, p.ba.ioff.data(), (nimg + 1) * 4));
    HIPCHK(up(d_poff, p.ba.poff.data(), (npts + 1) * 4));
    HIPCHK(up(d_pobs, p.ba.pobs.data(), nobs * 4));
    HIPCHK(up(d_icam, pb->image_cameras, nimg * 4));
    HIPCHK(up(d_coff, p.ba.coff.data(), (ncam + 1) * 4));
    HIPCHK(up(d_cimg, p.ba.cimg.data(), nimg * 4));
    HIPCHK(up(d_cmodel, pb->camera_models, ncam * 4));
    HIPCHK(up(d_icol, p.icol.data(), 6 * nimg * 4));
    HIPCHK(up(d_ccol, p.ccol.data(), kKC * ncam * 4));
    HIPCHK(up(d_pvar, p.ba.pvar.data(), npts));
    HIPCHK(up(d_oxy, p.ba.oxy.data(), nobs * 16));
    HIPCHK(up(d_q, pb->qvec, nimg * 32));
    HIPCHK(up(d_t, pb->tvec, nimg * 24));
    HIPCHK(up(d_cp, p.ba.cparams.data(), ncam * kKC * 8));
    HIPCHK(up(d_X, pb->xyz, npts * 24));
    HIPCHK(up(d_ocol, p.ocol.data(), (p.nown + 1) * 4));
    HIPCHK(up(d_colcoord, p.col_coord.data(), m * 4));
    HIPCHK(up(d_spo, p.spo.data(), (npts + 1) * 4));
    HIPCHK(up(d_sown, p.slot_owner.data(), nslots * 4));
    HIPCHK(up(d_spt, p.slot_point.data(), nslots * 4));
    HIPCHK(up(d_da, p.dest_a.data(), ndest * 4));
    HIPCHK(up(d_db, p.dest_b.data(), ndest * 4));
    HIPCHK(up(d_doff, p.dest_off.data(), (ndest + 1) * 4));
    HIPCHK(up(d_pa, p.pair_a.data(), npairs * 4));
    HIPCHK(up(d_pb, p.pair_b.data(), npairs * 4));
    const Status st0{0, 0, -1, 1.0};
    HIPCHK(up(d.st, &st0, sizeof st0));
    HIPCHK(hipMemsetAsync(d.S, 0, ld * ld * 8, st));
    HIPCHK(hipMemsetAsync(d.Z, 0, ld * ld * 8, st));

#define BACOV_LAUNCH(kernel, grid, block, ...)                                   \
    do {                                                                         \
        hipLaunchKernelGGL(kernel, grid, dim3(block), 0, st, __VA_ARGS__);       \
        HIPCHK(hipGetLastError());                                               \
    } while (0)
    // evaluation
    HIPCHK(hipEventRecord(ev.e[0], st));
    if (nobs) BACOV_LAUNCH(bacov_eval_kernel, dim3(blocks_for(nobs)), kBlock, d);
    HIPCHK(hipEventRecord(ev.e[1], st));
    // formation
    if (npts) BACOV_LAUNCH(bacov_point_kernel, dim3(blocks_for(npts)), kBlock, d);
    if (nslots) BACOV_LAUNCH(bacov_w_kernel, dim3(blocks_for(nslots * kKC)), kBlock, d);
    for (size_t i0 = 0; i0 < nimg; i0 += 32768) {  // (the grid's y extent is 16 bits)
        Dev part = d;
        part.ioff += i0;
        part.icam += i0;
        part.icol += 6 * i0;
        part.campart += (size_t)bacov::kCamPairs * i0;
        BACOV_LAUNCH(bacov_b_kernel, dim3(bacov::kLocalPairs, (unsigned)std::min<size_t>(nimg - i0, 32768)), kWave, part);
    }
    if (plan.ba.camvar) BACOV_LAUNCH(bacov_bcam_kernel, dim3(blocks_for(ncam * bacov::kCamPairs)), kBlock, d);
    if (ndest) BACOV_LAUNCH(bacov_dest_kernel, dim3((unsigned)ndest), kWave, d);
    BACOV_LAUNCH(bacov_diag_kernel, dim3(blocks_for(ld)), kBlock, d);
    HIPCHK(hipEventRecord(ev.e[2], st));
    // factor
    for (uint32_t kb = 0; kb < nt; ++kb) {
        BACOV_LAUNCH(bacov_chol_diag_kernel, dim3(1), kWave, d, kb);
        const unsigned rest = (unsigned)(nt - kb - 1);
        if (rest) {
            BACOV_LAUNCH(bacov_chol_panel_kernel, dim3(rest), kWave, d, kb);
            BACOV_LAUNCH(bacov_chol_update_kernel, dim3(rest, rest), kBlock, d, kb);
        }
    }
    HIPCHK(hipEventRecord(ev.e[3], st));
    // inverse
    for (uint32_t ib = 0; ib < nt; ++ib) BACOV_LAUNCH(bacov_inv_row_kernel, dim3(ib + 1), kBlock, d, ib);
    BACOV_LAUNCH(bacov_ztz_kernel, dim3((unsigned)nt, (unsigned)nt), kBlock, d);
    HIPCHK(hipEventRecord(ev.e[4], st));
    // points
    if (want_points && npts) BACOV_LAUNCH(bacov_pointcov_kernel, dim3(blocks_for(npts)), kBlock, d);
    HIPCHK(hipEventRecord(ev.e[5], st));
#undef BACOV_LAUNCH
    Status hs{};
    HIPCHK(hipMemcpyAsync(&hs, d.st, sizeof hs, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    result->min_pivot_ratio = hs.min_ratio;
    if (hs.fail) {
        result->success = 0;
        result->failed_column = hs.fail_col;
        std::free(result->matrix);
        std::free(result->point_present);
        std::free(result->point_cov);
        result->matrix = result->point_cov = nullptr;
        result->point_present = nullptr;
    } else {
        if (want_matrix)
            HIPCHK(hipMemcpy2DAsync(result->matrix, m * 8, d.Sig, ld * 8, m * 8, m, hipMemcpyDeviceToHost, st));
        if (want_points && npts) {
            // (a constant point's entry of pcov is not written by any kernel and is not copied)
            std::vector<double> pc(9 * npts);
            HIPCHK(hipMemcpyAsync(pc.data(), d.pcov, 9 * npts * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            for (size_t j = 0; j < npts; ++j) {
                result->point_present[j] = plan.ba.pvar[j];
                if (plan.ba.pvar[j]) std::memcpy(result->point_cov + 9 * j, pc.data() + 9 * j, 72);
            }
        }
    }
    HIPCHK(timer.stop(result->device_ms));
    for (int k = 0; k < AMC_BACOV_PHASES; ++k) {
        float f = 0.f;
        HIPCHK(hipEventElapsedTime(&f, ev.e[k], ev.e[k + 1]));
        result->phase_ms[k] = f;
        result->kernel_ms += f;
    }
    result->copy_ms = result->device_ms - result->kernel_ms;
    result->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count() - result->device_ms;
    guard.armed = false;
    return AMC_OK;
}

}  // namespace

extern "C" {

void amc_bacov_opts_default(amc_bacov_opts* o) {
    if (!o) return;
    o->loss_function_type = AMC_BA_LOSS_TRIVIAL;
    o->want_points = 1;
    o->want_matrix = 1;
    o->reserved = 0;
    o->loss_function_scale = 1.0;
    o->damping = 1e-8;  // COLMAP's BACovarianceOptions::damping
}

int amc_ba_covariance(amc_ctx* ctx, const amc_ba_problem* problem, const uint8_t* point_const,
                      const amc_bacov_opts* options, amc_bacov_result* result) {
    return run(ctx, problem, point_const, options, result);
}

void amc_bacov_result_free(amc_bacov_result* r) {
    if (!r) return;
    free_arrays(r);
}

}  // extern "C"
