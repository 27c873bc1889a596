// ubench_ladder.hip - bottom-up ladder under the match kernel's scan loop.
//
// Each rung adds one ingredient of the scan loop match_mfma.hip had up to commit 4287819 (v_mfma_i32_32x32x32_i8) to a
// register-only int8 MFMA loop and reports ns per MFMA per SIMD (13.33 ns = one v_mfma_i32_32x32x32_i8 per 32 clk at
// the nominal 2.4 GHz), for both workgroup shapes that kernel knew; ladder16u_kernel<8, 2> is the loop it runs now:
//     <8 waves x 4 X tiles>  two waves per SIMD, 256 registers each
//     <4 waves x 8 X tiles>  one wave per SIMD, X fragments in AGPRs
//   rung 0  MFMAs only (A, B in registers; four dependent MFMAs per unit, units independent)
//   rung 1  + the four A-fragment ds_read_b128 per Y tile
//   rung 2  + the C-operand block (four more ds_read_b128 per Y tile; first MFMA of a unit takes it as C)
//   rung 3  + the 11 VALU per unit (the kernel's three asm blocks: 8 max ops and the 3-op key insertion), reads spread
//           over the phases
//   rung 4  the same with one insertion per TWO units of an X tile (32 outputs): 9.5 VALU per 16 outputs
//   LADDER_UNITS=1: rung 3 and rung 4 against the 16x16x64 loop with one insertion per 64- or 128-row unit
//           (ladder16u_kernel): behind one untimed pass over all rungs, three repetitions in one process, each
//           timing behind a full-length warm-up launch, the order of the rungs rotated between repetitions
//   The last lines printed, "register-only reference", are no rung of this ladder: v_mfma_i32_16x16x64_i8 on
//           register operands alone, the shape the guide's 3,944 TOPS was taken with (older outputs under profiles/
//           call that line "rung 4", before the merged-insertion rung took the number).
// Every rung 3 carries the kernel's 3-op key insertion (ladder_kernel, ladder2_kernel); ladder16_kernel keeps the 4-op
// compare / select insertion on purpose: it is the 8-output unit as it was measured and closed.
// Run under rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE for the
// pipe-busy fraction and the clock each rung holds.
//
//   hipcc --offload-arch=gfx950 -O3 -o tools/bin/ubench_ladder tools/ubench_ladder.hip && tools/bin/ubench_ladder
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

template <bool BA>
__device__ __forceinline__ void mfma_first(i32x16& d, const i32x4& a, const i32x4& b, const i32x16& c) {
    if constexpr (BA)
        asm volatile("v_mfma_i32_32x32x32_i8 %0, %1, %2, %3" : "=&v"(d) : "v"(a), "a"(b), "v"(c));
    else
        asm volatile("v_mfma_i32_32x32x32_i8 %0, %1, %2, %3" : "=&v"(d) : "v"(a), "v"(b), "v"(c));
}
template <bool BA>
__device__ __forceinline__ void mfma_acc(i32x16& d, const i32x4& a, const i32x4& b) {
    if constexpr (BA)
        asm volatile("v_mfma_i32_32x32x32_i8 %0, %1, %2, %0" : "+v"(d) : "v"(a), "a"(b));
    else
        asm volatile("v_mfma_i32_32x32x32_i8 %0, %1, %2, %0" : "+v"(d) : "v"(a), "v"(b));
}

// match_mfma.hip's insertion of a unit maximum into a lane's (best, second) keys: value << 7 | tile code, three
// instructions (the maximum is consumed).  The tile code is wave-uniform, a scalar operand.
__device__ __forceinline__ void key_insert(int& best, int& sec, int& m, int code) {
    asm volatile("v_lshl_or_b32 %2, %2, 7, %3\n\tv_med3_i32 %1, %0, %1, %2\n\tv_max_i32 %0, %0, %2"
                 : "+v"(best), "+v"(sec), "+v"(m) : "s"(code));
}

constexpr int kLds = 2 * 32768 + 4096;

template <int W, int XT, int LVL>
__global__ __launch_bounds__(64 * W) void ladder_kernel(int tiles, const int* __restrict__ seed, int* __restrict__ out) {
    constexpr bool BA = (W == 4);
    __shared__ __attribute__((aligned(16))) char smem[kLds];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    for (int i = tid; i < kLds / 4; i += 64 * W) reinterpret_cast<int*>(smem)[i] = seed[(i * 7 + blockIdx.x) & 4095];
    __syncthreads();
    i32x4 xf[XT][4];
#pragma unroll
    for (int xt = 0; xt < XT; ++xt)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int* p = seed + 4096 + ((tid * 16 + xt * 64 + s * 4) & 4095);  // (second half: the resident X side's bytes)
            if constexpr (BA)
                asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(xf[xt][s]) : "v"(p) : "memory");
            else
                xf[xt][s] = *reinterpret_cast<const i32x4*>(p);
        }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int best[XT], sec[XT], btile[XT];
#pragma unroll
    for (int xt = 0; xt < XT; ++xt) best[xt] = sec[xt] = btile[xt] = 0;
    struct YF { i32x4 f[4]; i32x16 ci; } y0, y1;
    auto load_part = [&](YF& y, int yt, int part) __attribute__((always_inline)) {
        const int row = (yt & 7) * 32 + l31;
        if (part < 4) {
            const int* rsb = reinterpret_cast<const int*>(smem + 65536) + (yt & 7) * 32 + 4 * lh;
            const i32x4 v = *reinterpret_cast<const i32x4*>(rsb + 8 * part);
#pragma unroll
            for (int e = 0; e < 4; ++e) y.ci[4 * part + e] = v[e];
        } else {
            const int s = part - 4, sw = (row >> 1) & 7;
            y.f[s] = *reinterpret_cast<const i32x4*>(smem + ((yt >> 3) & 1) * 32768 + row * 128 + (((2 * s + lh) ^ sw) * 16));
        }
    };
#pragma unroll
    for (int part = 0; part < 8; ++part) { load_part(y0, 0, part); load_part(y1, 1, part); }
    i32x16 acc[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[0][e] = acc[1][e] = 0;
    int pm[XT], ptile = 0;  // pending unit maxima (rung 4: the even tile's maximum waits here for the odd tile's)
#pragma unroll
    for (int xt = 0; xt < XT; ++xt) pm[xt] = 0;
    auto phase = [&](i32x16& an, const YF& y, int xtn, const i32x16& ac, int xtc, int tile, bool odd) __attribute__((always_inline)) {
        if (LVL >= 2) mfma_first<BA>(an, y.f[0], xf[xtn][0], y.ci); else mfma_acc<BA>(an, y.f[0], xf[xtn][0]);
        __builtin_amdgcn_sched_barrier(0);
        if (LVL >= 3) {
            // rung 4 inserts behind every second Y tile only (X tile XT - 1 of an odd tile goes in with the next even one)
            const int xi = (xtc + XT - 1) % XT;
            if (LVL == 3 || (xtc == 0 ? !odd : odd)) key_insert(best[xi], sec[xi], pm[xi], 126 - (ptile & 63));
            __builtin_amdgcn_sched_barrier(0);
        }
        mfma_acc<BA>(an, y.f[1], xf[xtn][1]);
        __builtin_amdgcn_sched_barrier(0);
        int t0 = 0, t1 = 0, t2 = 0, t3 = 0;
        if (LVL >= 3) {
            asm volatile("v_max3_i32 %0, %4, %5, %6\n\tv_max3_i32 %1, %7, %8, %9\n\tv_max3_i32 %2, %10, %11, %12\n\tv_max3_i32 %3, %13, %14, %15"
                         : "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
                         : "v"(ac[0]), "v"(ac[1]), "v"(ac[2]), "v"(ac[3]), "v"(ac[4]), "v"(ac[5]), "v"(ac[6]), "v"(ac[7]),
                           "v"(ac[8]), "v"(ac[9]), "v"(ac[10]), "v"(ac[11]));
            __builtin_amdgcn_sched_barrier(0);
        }
        mfma_acc<BA>(an, y.f[2], xf[xtn][2]);
        __builtin_amdgcn_sched_barrier(0);
        if (LVL >= 3) {
            int m4;
            if (LVL == 4 && odd)  // fold the even tile's maximum in: the last v_max becomes a v_max3
                asm volatile("v_max3_i32 %1, %5, %6, %7\n\tv_max3_i32 %0, %0, %3, %4\n\tv_max3_i32 %1, %9, %1, %8\n\tv_max3_i32 %2, %0, %1, %2"
                             : "+v"(t0), "=&v"(m4), "+v"(pm[xtc]) : "v"(t1), "v"(t2), "v"(ac[12]), "v"(ac[13]), "v"(ac[14]), "v"(ac[15]), "v"(t3));
            else
                asm volatile("v_max3_i32 %1, %5, %6, %7\n\tv_max3_i32 %0, %0, %3, %4\n\tv_max3_i32 %1, %9, %1, %8\n\tv_max_i32 %2, %0, %1"
                             : "+v"(t0), "=&v"(m4), "=&v"(pm[xtc]) : "v"(t1), "v"(t2), "v"(ac[12]), "v"(ac[13]), "v"(ac[14]), "v"(ac[15]), "v"(t3));
            ptile = tile;
            __builtin_amdgcn_sched_barrier(0);
        }
        mfma_acc<BA>(an, y.f[3], xf[xtn][3]);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto step = [&](YF& yc, YF& yn, int yt, bool odd) __attribute__((always_inline)) {
        constexpr int RPP = 16 / XT;
#pragma unroll
        for (int xt = 0; xt < XT; ++xt) {
            if (xt + 1 < XT) phase(acc[(xt + 1) & 1], yc, xt + 1, acc[xt & 1], xt, yt, odd);
            else phase(acc[0], yn, 0, acc[xt & 1], xt, yt, odd);
            if (xt < XT / 2) {
#pragma unroll
                for (int r = 0; r < RPP; ++r) {
                    const int part = xt * RPP + r;
                    if ((LVL >= 1 && part >= 4) || (LVL >= 2 && part < 4)) load_part(yn, yt + 1, part);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
#pragma unroll 1
    for (int yt = 0; yt < tiles; yt += 2) {
        step(y0, y1, yt, false);
        step(y1, y0, yt + 1, true);
    }
    int r = 0;
#pragma unroll
    for (int xt = 0; xt < XT; ++xt) r ^= best[xt] ^ sec[xt] ^ btile[xt] ^ pm[xt];
#pragma unroll
    for (int e = 0; e < 16; ++e) r ^= acc[0][e] ^ acc[1][e];
    if (r == 0x7fffffff) out[tid] = r;
}

// The same rungs with the units taken in PAIRS: the MFMAs of units u+2 and u+3 alternate (a0 b0 a1 b1 a2 b2 a3 b3), so
// no MFMA ever issues directly behind the one it depends on, while the VALU reduces units u and u+1 (four accumulator
// sets instead of two).  If the dependent back-to-back issue is what keeps the plain loop under the pipe's rate, this
// order shows it.
template <int W, int XT, int LVL>
__global__ __launch_bounds__(64 * W) void ladder2_kernel(int tiles, const int* __restrict__ seed, int* __restrict__ out) {
    constexpr bool BA = (W == 4);
    __shared__ __attribute__((aligned(16))) char smem[kLds];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    for (int i = tid; i < kLds / 4; i += 64 * W) reinterpret_cast<int*>(smem)[i] = seed[(i * 7 + blockIdx.x) & 4095];
    __syncthreads();
    i32x4 xf[XT][4];
#pragma unroll
    for (int xt = 0; xt < XT; ++xt)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int* p = seed + 4096 + ((tid * 16 + xt * 64 + s * 4) & 4095);  // (second half: the resident X side's bytes)
            if constexpr (BA)
                asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(xf[xt][s]) : "v"(p) : "memory");
            else
                xf[xt][s] = *reinterpret_cast<const i32x4*>(p);
        }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int best[XT], sec[XT], btile[XT];
#pragma unroll
    for (int xt = 0; xt < XT; ++xt) best[xt] = sec[xt] = btile[xt] = 0;
    struct YF { i32x4 f[4]; i32x16 ci; } y0, y1;
    auto load_part = [&](YF& y, int yt, int part) __attribute__((always_inline)) {
        const int row = (yt & 7) * 32 + l31;
        if (part < 4) {
            const int* rsb = reinterpret_cast<const int*>(smem + 65536) + (yt & 7) * 32 + 4 * lh;
            const i32x4 v = *reinterpret_cast<const i32x4*>(rsb + 8 * part);
#pragma unroll
            for (int e = 0; e < 4; ++e) y.ci[4 * part + e] = v[e];
        } else {
            const int s = part - 4, sw = (row >> 1) & 7;
            y.f[s] = *reinterpret_cast<const i32x4*>(smem + ((yt >> 3) & 1) * 32768 + row * 128 + (((2 * s + lh) ^ sw) * 16));
        }
    };
#pragma unroll
    for (int part = 0; part < 8; ++part) { load_part(y0, 0, part); load_part(y1, 1, part); }
    i32x16 acc[4];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[0][e] = acc[1][e] = acc[2][e] = acc[3][e] = 0;
    int pm[2] = {0, 0}, ptile = 0;
    auto ins = [&](int xi, int& m, int tile) __attribute__((always_inline)) {
        key_insert(best[xi], sec[xi], m, 126 - (tile & 63));
    };
    auto blkA = [&](const i32x16& ac, int& t0, int& t1, int& t2, int& t3) __attribute__((always_inline)) {
        asm volatile("v_max3_i32 %0, %4, %5, %6\n\tv_max3_i32 %1, %7, %8, %9\n\tv_max3_i32 %2, %10, %11, %12\n\tv_max3_i32 %3, %13, %14, %15"
                     : "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
                     : "v"(ac[0]), "v"(ac[1]), "v"(ac[2]), "v"(ac[3]), "v"(ac[4]), "v"(ac[5]), "v"(ac[6]), "v"(ac[7]),
                       "v"(ac[8]), "v"(ac[9]), "v"(ac[10]), "v"(ac[11]));
    };
    auto blkB = [&](const i32x16& ac, int& t0, int t1, int t2, int t3) __attribute__((always_inline)) {
        int m4;
        asm volatile("v_max3_i32 %1, %4, %5, %6\n\tv_max3_i32 %0, %0, %2, %3\n\tv_max3_i32 %1, %8, %1, %7\n\tv_max_i32 %0, %0, %1"
                     : "+v"(t0), "=&v"(m4) : "v"(t1), "v"(t2), "v"(ac[12]), "v"(ac[13]), "v"(ac[14]), "v"(ac[15]), "v"(t3));
    };
    // pair phase: accumulate units (xn, xn+1) of tile `yn_` into an0/an1, reduce units (xc, xc+1) from ac0/ac1
    auto pphase = [&](i32x16& an0, i32x16& an1, const YF& y, int xn, const i32x16& ac0, const i32x16& ac1, int xc, int tile)
                      __attribute__((always_inline)) {
        if (LVL >= 2) { mfma_first<BA>(an0, y.f[0], xf[xn][0], y.ci); mfma_first<BA>(an1, y.f[0], xf[xn + 1][0], y.ci); }
        else { mfma_acc<BA>(an0, y.f[0], xf[xn][0]); mfma_acc<BA>(an1, y.f[0], xf[xn + 1][0]); }
        __builtin_amdgcn_sched_barrier(0);
        if (LVL >= 3) {
            ins((xc + XT - 2) % XT, pm[0], ptile);
            ins((xc + XT - 1) % XT, pm[1], ptile);
            __builtin_amdgcn_sched_barrier(0);
        }
        mfma_acc<BA>(an0, y.f[1], xf[xn][1]);
        mfma_acc<BA>(an1, y.f[1], xf[xn + 1][1]);
        __builtin_amdgcn_sched_barrier(0);
        int a0 = 0, a1 = 0, a2 = 0, a3 = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
        if (LVL >= 3) {
            blkA(ac0, a0, a1, a2, a3);
            blkA(ac1, b0, b1, b2, b3);
            __builtin_amdgcn_sched_barrier(0);
        }
        mfma_acc<BA>(an0, y.f[2], xf[xn][2]);
        mfma_acc<BA>(an1, y.f[2], xf[xn + 1][2]);
        __builtin_amdgcn_sched_barrier(0);
        if (LVL >= 3) {
            blkB(ac0, a0, a1, a2, a3);
            blkB(ac1, b0, b1, b2, b3);
            pm[0] = a0; pm[1] = b0; ptile = tile;
            __builtin_amdgcn_sched_barrier(0);
        }
        mfma_acc<BA>(an0, y.f[3], xf[xn][3]);
        mfma_acc<BA>(an1, y.f[3], xf[xn + 1][3]);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto step = [&](YF& yc, YF& yn, int yt) __attribute__((always_inline)) {
        constexpr int NP = XT / 2;      // pair phases per tile
        constexpr int RPP = 8 / (NP > 1 ? NP / 2 : 1) > 8 ? 8 : 8 / (NP > 1 ? NP / 2 : 1);
#pragma unroll
        for (int pp = 0; pp < NP; ++pp) {
            const int xc = 2 * pp;
            i32x16& c0 = acc[(pp & 1) * 2];
            i32x16& c1 = acc[(pp & 1) * 2 + 1];
            i32x16& n0 = acc[((pp + 1) & 1) * 2];
            i32x16& n1 = acc[((pp + 1) & 1) * 2 + 1];
            if (pp + 1 < NP) pphase(n0, n1, yc, xc + 2, c0, c1, xc, yt);
            else pphase(n0, n1, yn, 0, c0, c1, xc, yt);
            if (pp < (NP > 1 ? NP / 2 : 1)) {
#pragma unroll
                for (int r = 0; r < RPP; ++r) {
                    const int part = pp * RPP + r;
                    if (part < 8 && ((LVL >= 1 && part >= 4) || (LVL >= 2 && part < 4))) load_part(yn, yt + 1, part);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
#pragma unroll 1
    for (int yt = 0; yt < tiles; yt += 2) {
        step(y0, y1, yt);
        step(y1, y0, yt + 1);
    }
    int r = pm[0] ^ pm[1];
#pragma unroll
    for (int xt = 0; xt < XT; ++xt) r ^= best[xt] ^ sec[xt] ^ btile[xt];
#pragma unroll
    for (int e = 0; e < 16; ++e) r ^= acc[0][e] ^ acc[1][e] ^ acc[2][e] ^ acc[3][e];
    if (r == 0x7fffffff) out[tid] = r;
}

// The scan loop re-tiled for v_mfma_i32_16x16x64_i8 (4 passes, 4 accumulator registers): a unit is one 16-row X tile
// against a PAIR of 16-row Y tiles (= the 32-row tile resolve_index recomputes), four MFMAs and 8 outputs per lane;
// VALU per unit: maximum of 8 (4 ops) + one insertion (4 ops).  Same LDS bytes per MAC as the 32x32x32 loop, a third
// more VALU per output.  LVL as above (0: MFMAs only ... 3: everything).
typedef int i32x4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void mfma16_first(i32x4v& d, const i32x4v& a, const i32x4v& b, const i32x4v& c) {
    asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %3" : "=&v"(d) : "v"(a), "v"(b), "v"(c));
}
__device__ __forceinline__ void mfma16_acc(i32x4v& d, const i32x4v& a, const i32x4v& b) {
    asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+v"(d) : "v"(a), "v"(b));
}
template <int W, int LVL>
__global__ __launch_bounds__(64 * W) void ladder16_kernel(int tiles, const int* __restrict__ seed, int* __restrict__ out) {
    constexpr int XT = 8;  // 16-row X tiles per wave (128 rows)
    __shared__ __attribute__((aligned(16))) char smem[kLds];
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
    for (int i = tid; i < kLds / 4; i += 64 * W) reinterpret_cast<int*>(smem)[i] = seed[(i * 7 + blockIdx.x) & 4095];
    __syncthreads();
    i32x4v xf[XT][2];
#pragma unroll
    for (int xt = 0; xt < XT; ++xt)
#pragma unroll
        for (int s = 0; s < 2; ++s) xf[xt][s] = *reinterpret_cast<const i32x4v*>(seed + 4096 + ((tid * 16 + xt * 64 + s * 4) & 4095));
    int best[XT], sec[XT], btile[XT];
#pragma unroll
    for (int xt = 0; xt < XT; ++xt) best[xt] = sec[xt] = btile[xt] = 0;
    struct YF { i32x4v f[2][2]; i32x4v ci[2]; } y0, y1;  // two 16-row tiles x two k halves; C blocks
    auto load_part = [&](YF& y, int yt, int part) __attribute__((always_inline)) {
        if (part < 2) {
            const int* rsb = reinterpret_cast<const int*>(smem + 65536) + (yt & 7) * 32 + part * 16 + 4 * lq;
            y.ci[part] = *reinterpret_cast<const i32x4v*>(rsb);
        } else {
            const int t = (part - 2) >> 1, s = (part - 2) & 1;
            const int row = (yt & 7) * 32 + t * 16 + l15, sw = (row >> 1) & 7;
            y.f[t][s] = *reinterpret_cast<const i32x4v*>(smem + ((yt >> 3) & 1) * 32768 + row * 128 + (((4 * s + lq) ^ sw) * 16));
        }
    };
#pragma unroll
    for (int part = 0; part < 6; ++part) { load_part(y0, 0, part); load_part(y1, 1, part); }
    i32x4v acc[2][2];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[0][0][e] = acc[0][1][e] = acc[1][0][e] = acc[1][1][e] = 0;
    int pm = 0, ptile = 0;
    auto phase = [&](i32x4v (&an)[2], const YF& y, int xtn, const i32x4v (&ac)[2], int xtc, int tile) __attribute__((always_inline)) {
        if (LVL >= 2) { mfma16_first(an[0], y.f[0][0], xf[xtn][0], y.ci[0]); mfma16_first(an[1], y.f[1][0], xf[xtn][0], y.ci[1]); }
        else { mfma16_acc(an[0], y.f[0][0], xf[xtn][0]); mfma16_acc(an[1], y.f[1][0], xf[xtn][0]); }
        __builtin_amdgcn_sched_barrier(0);
        if (LVL >= 3) {
            const int xi = (xtc + XT - 1) % XT;
            asm volatile("v_cmp_gt_i32 vcc, %3, %0\n\tv_med3_i32 %1, %0, %1, %3\n\tv_max_i32 %0, %0, %3\n\tv_cndmask_b32 %2, %2, %4, vcc"
                         : "+v"(best[xi]), "+v"(sec[xi]), "+v"(btile[xi]) : "v"(pm), "v"(ptile) : "vcc");
            __builtin_amdgcn_sched_barrier(0);
        }
        mfma16_acc(an[0], y.f[0][1], xf[xtn][1]);
        mfma16_acc(an[1], y.f[1][1], xf[xtn][1]);
        __builtin_amdgcn_sched_barrier(0);
        if (LVL >= 3) {
            int t0, t1;
            asm volatile("v_max3_i32 %0, %2, %3, %4\n\tv_max3_i32 %1, %5, %6, %7\n\tv_max3_i32 %0, %0, %8, %9\n\tv_max_i32 %0, %0, %1"
                         : "=&v"(t0), "=&v"(t1)
                         : "v"(ac[0][0]), "v"(ac[0][1]), "v"(ac[0][2]), "v"(ac[0][3]), "v"(ac[1][0]), "v"(ac[1][1]), "v"(ac[1][2]), "v"(ac[1][3]));
            pm = t0;
            ptile = tile;
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto step = [&](YF& yc, YF& yn, int yt) __attribute__((always_inline)) {
#pragma unroll
        for (int xt = 0; xt < XT; ++xt) {
            if (xt + 1 < XT) phase(acc[(xt + 1) & 1], yc, xt + 1, acc[xt & 1], xt, yt);
            else phase(acc[0], yn, 0, acc[xt & 1], xt, yt);
            if (xt < 6) {
                const int part = xt;
                if ((LVL >= 1 && part >= 2) || (LVL >= 2 && part < 2)) load_part(yn, yt + 1, part);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
#pragma unroll 1
    for (int yt = 0; yt < tiles; yt += 2) {
        step(y0, y1, yt);
        step(y1, y0, yt + 1);
    }
    int r = pm;
#pragma unroll
    for (int xt = 0; xt < XT; ++xt) r ^= best[xt] ^ sec[xt] ^ btile[xt];
#pragma unroll
    for (int e = 0; e < 4; ++e) r ^= acc[0][0][e] ^ acc[0][1][e] ^ acc[1][0][e] ^ acc[1][1][e];
    if (r == 0x7fffffff) out[tid] = r;
}

// The 16x16x64 loop with ONE insertion per unit of STEPS 32-row steps (STEPS = 2: 64-row blocks, 16 outputs per lane and
// unit, 11 VALU per 16 outputs; STEPS = 4: 128-row units, 9.5 per 16).  A lane owns one X row; per step its 8 outputs go
// to 4 max ops, the last of which folds the unit's carried partial maximum in, and the unit's last step is followed by
// the kernel's 3-op key insertion.  Y rows are dealt to MFMA rows so that a lane quarter's outputs of a unit are
// contiguous rows: row m of MFMA tile t is Y row (UR/4) * (m >> 2) + 4 t + (m & 3) of the unit (UR = 32 * STEPS rows), so
// the C operand of a tile is one ds_read_b128.  The A-fragment swizzle that keeps this read pattern conflict-free takes
// row bit 1 and the two bits that number the lane quarter's rows (not (row >> 1) & 7, which this pattern hits 4-way).
template <int W, int STEPS>
__global__ __launch_bounds__(64 * W) void ladder16u_kernel(int tiles, const int* __restrict__ seed, int* __restrict__ out) {
    constexpr int XT = 8, UR = 32 * STEPS, QB = STEPS == 2 ? 4 : 5;  // QB: the bit where the quarter's number starts
    __shared__ __attribute__((aligned(16))) char smem[kLds];
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
    for (int i = tid; i < kLds / 4; i += 64 * W) reinterpret_cast<int*>(smem)[i] = seed[(i * 7 + blockIdx.x) & 4095];
    __syncthreads();
    i32x4v xf[XT][2];
#pragma unroll
    for (int xt = 0; xt < XT; ++xt)
#pragma unroll
        for (int s = 0; s < 2; ++s) xf[xt][s] = *reinterpret_cast<const i32x4v*>(seed + 4096 + ((tid * 16 + xt * 64 + s * 4) & 4095));
    int best[XT], sec[XT], part[XT];
#pragma unroll
    for (int xt = 0; xt < XT; ++xt) best[xt] = sec[xt] = part[xt] = 0;
    struct YF { i32x4v f[2][2]; i32x4v ci[2]; } y0, y1;
    // step yt (32 rows' worth: MFMA tiles 2 sp, 2 sp + 1 of its unit; sp = yt % STEPS)
    auto load_part = [&](YF& y, int yt, int part_) __attribute__((always_inline)) {
        const int ubase = ((yt & 7) / STEPS) * UR, sp = yt % STEPS;  // unit's first row in the 256-row chunk
        if (part_ < 2) {
            const int t = 2 * sp + part_;
            y.ci[part_] = *reinterpret_cast<const i32x4v*>(reinterpret_cast<const int*>(smem + 65536) + ubase + (UR / 4) * lq + 4 * t);
        } else {
            const int t = 2 * sp + ((part_ - 2) >> 1), s = (part_ - 2) & 1;
            const int row = ubase + (UR / 4) * (l15 >> 2) + 4 * t + (l15 & 3);
            const int sw = ((row >> 1) & 1) | (((row >> QB) & 3) << 1);
            y.f[(part_ - 2) >> 1][s] = *reinterpret_cast<const i32x4v*>(smem + ((yt >> 3) & 1) * 32768 + row * 128 + (((4 * s + lq) ^ sw) * 16));
        }
    };
#pragma unroll
    for (int p = 0; p < 6; ++p) load_part(y0, 0, p);
    i32x4v acc[2][2];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[0][0][e] = acc[0][1][e] = acc[1][0][e] = acc[1][1][e] = 0;
    // sp: the step's place in its unit.  The maxima of a unit's last step are inserted one phase later (xi = xtc - 1).
    auto phase = [&](i32x4v (&an)[2], const YF& y, int xtn, const i32x4v (&ac)[2], int xtc, int code, int sp) __attribute__((always_inline)) {
        mfma16_first(an[0], y.f[0][0], xf[xtn][0], y.ci[0]);
        mfma16_first(an[1], y.f[1][0], xf[xtn][0], y.ci[1]);
        __builtin_amdgcn_sched_barrier(0);
        if (xtc == 0 ? sp == 0 : sp == STEPS - 1) {
            const int xi = (xtc + XT - 1) % XT;
            key_insert(best[xi], sec[xi], part[xi], code);
            __builtin_amdgcn_sched_barrier(0);
        }
        mfma16_acc(an[0], y.f[0][1], xf[xtn][1]);
        mfma16_acc(an[1], y.f[1][1], xf[xtn][1]);
        __builtin_amdgcn_sched_barrier(0);
        int t0, t1;
        if (sp == 0)
            asm volatile("v_max3_i32 %0, %3, %4, %5\n\tv_max3_i32 %1, %6, %7, %8\n\tv_max3_i32 %0, %0, %9, %10\n\tv_max_i32 %2, %0, %1"
                         : "=&v"(t0), "=&v"(t1), "=&v"(part[xtc])
                         : "v"(ac[0][0]), "v"(ac[0][1]), "v"(ac[0][2]), "v"(ac[0][3]), "v"(ac[1][0]), "v"(ac[1][1]), "v"(ac[1][2]), "v"(ac[1][3]));
        else
            asm volatile("v_max3_i32 %0, %3, %4, %5\n\tv_max3_i32 %1, %6, %7, %8\n\tv_max3_i32 %0, %0, %9, %10\n\tv_max3_i32 %2, %0, %1, %2"
                         : "=&v"(t0), "=&v"(t1), "+v"(part[xtc])
                         : "v"(ac[0][0]), "v"(ac[0][1]), "v"(ac[0][2]), "v"(ac[0][3]), "v"(ac[1][0]), "v"(ac[1][1]), "v"(ac[1][2]), "v"(ac[1][3]));
        __builtin_amdgcn_sched_barrier(0);
    };
    auto step = [&](YF& yc, YF& yn, int yt, int sp) __attribute__((always_inline)) {
        const int code = 126 - (((yt - 1) / STEPS) & 63);  // of the unit whose maxima are pending
#pragma unroll
        for (int xt = 0; xt < XT; ++xt) {
            if (xt + 1 < XT) phase(acc[(xt + 1) & 1], yc, xt + 1, acc[xt & 1], xt, code, sp);
            else phase(acc[0], yn, 0, acc[xt & 1], xt, code, sp);
            if (xt < 6) {
                load_part(yn, yt + 1, xt);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
#pragma unroll 1
    for (int yt = 0; yt < tiles; yt += STEPS) {
#pragma unroll
        for (int sp = 0; sp < STEPS; sp += 2) {
            step(y0, y1, yt + sp, sp);
            step(y1, y0, yt + sp + 1, sp + 1);
        }
    }
    int r = 0;
#pragma unroll
    for (int xt = 0; xt < XT; ++xt) r ^= best[xt] ^ sec[xt] ^ part[xt];
#pragma unroll
    for (int e = 0; e < 4; ++e) r ^= acc[0][0][e] ^ acc[0][1][e] ^ acc[1][0][e] ^ acc[1][1][e];
    if (r == 0x7fffffff) out[tid] = r;
}

template <int W, int LVL>
static void run16(const char* name, const int* d_seed, int* d_out, int cus);

// register-only v_mfma_i32_16x16x64_i8: 8 independent accumulators, W waves
template <int W>
__global__ __launch_bounds__(64 * W) void mfma16_kernel(int iters, const int* __restrict__ seed, int* __restrict__ out) {
    typedef int i32x4v __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x;
    i32x4v a = *reinterpret_cast<const i32x4v*>(seed + ((tid * 4) & 4095));
    i32x4v b = *reinterpret_cast<const i32x4v*>(seed + ((tid * 4 + 1024) & 4095));
    i32x4v acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = i32x4v{0, 0, 0, 0};
#pragma unroll 1
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[k], 0, 0, 0);
    }
    int r = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) r ^= acc[k][0] ^ acc[k][1] ^ acc[k][2] ^ acc[k][3];
    if (r == 0x7fffffff) out[tid] = r;
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); std::exit(1); } } while (0)

template <int W, int XT, int LVL, int PAIRED>
static void run(const char* name, const int* d_seed, int* d_out, int cus) {
    const int tiles = 8192;  // Y tiles per launch: XT * 4 MFMAs each
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    auto launch = [&](int t) {
        if (PAIRED) hipLaunchKernelGGL((ladder2_kernel<W, XT, LVL>), dim3(cus), dim3(64 * W), 0, 0, t, d_seed, d_out);
        else hipLaunchKernelGGL((ladder_kernel<W, XT, LVL>), dim3(cus), dim3(64 * W), 0, 0, t, d_seed, d_out);
    };
    launch(256);  // warm-up
    CHECK(hipDeviceSynchronize());
    float best = 1e30f;
    for (int rep = 0; rep < 3; ++rep) {
        CHECK(hipEventRecord(e0));
        launch(tiles);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float ms;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (ms < best) best = ms;
    }
    // per SIMD: waves per SIMD x tiles x XT x 4 MFMAs
    const double mfma_per_simd = (double)(W / 4) * tiles * XT * 4;
    const double ns = best * 1e6 / mfma_per_simd;
    std::printf("%-34s W%dx%d %s rung %d: %8.3f ms  %6.2f ns/MFMA/SIMD  = %.3f of nominal (13.33 ns)\n", name, W, XT,
                PAIRED ? "paired" : "chain ", LVL, best, ns, 13.3333 / ns);
}

template <int W, int LVL>
static void run16(const char* name, const int* d_seed, int* d_out, int cus) {
    const int tiles = 8192;  // 32-row Y tile pairs per launch: 8 X tiles x 4 MFMAs (16x16x64) each
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    hipLaunchKernelGGL((ladder16_kernel<W, LVL>), dim3(cus), dim3(64 * W), 0, 0, 256, d_seed, d_out);
    CHECK(hipDeviceSynchronize());
    float best = 1e30f;
    for (int rep = 0; rep < 3; ++rep) {
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL((ladder16_kernel<W, LVL>), dim3(cus), dim3(64 * W), 0, 0, tiles, d_seed, d_out);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float ms;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (ms < best) best = ms;
    }
    const double eq = (double)(W / 4) * tiles * 8 * 4 / 2;  // in 32x32x32-equivalents (half the MACs each)
    const double ns = best * 1e6 / eq;
    std::printf("%-34s W%d 16x16x64 rung %d: %8.3f ms  %6.2f ns/MFMA-equiv/SIMD = %.3f of nominal (13.33 ns)\n", name, W, LVL, best, ns, 13.3333 / ns);
}

// The unit rungs (LADDER_UNITS=1): one timing per call, four back-to-back launches of 8192 32-row Y steps behind a
// warm-up launch of the same length (a short one left the first timed rung of a process 1.2 - 1.7 ms slow), reported in
// the ladder's line format.  main() runs the rungs three times, starting each repetition at another rung, so that they
// share one box and one thermal state and none is always first.
template <class L>
static void measure(const char* name, int rep, L launch) {
    const int tiles = 8192, launches = 4;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    launch(tiles);  // warm-up
    CHECK(hipDeviceSynchronize());
    CHECK(hipEventRecord(e0));
    for (int i = 0; i < launches; ++i) launch(tiles);
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float ms;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
    // W = 8: two waves per SIMD, 16 32x32x32-equivalent MFMAs per wave and 32-row Y step (128 X rows)
    const double eq = 2.0 * tiles * launches * 16;
    const double ns = ms * 1e6 / eq;
    std::printf("%-46s rep %d: %8.3f ms  %6.2f ns/MFMA-equiv/SIMD = %.3f of nominal (13.33 ns)\n", name, rep, ms, ns, 13.3333 / ns);
}

int main() {
    int dev = 0, cus = 256;
    CHECK(hipGetDevice(&dev));
    CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    // operand data: the matrix pipe's power (hence the clock the chip holds) depends on what it multiplies.
    //   LADDER_DATA=0 random bytes (default) | 1 SIFT-like under the kernel's zero point (0x80 + small values)
    //   2 small positive bytes (what a zero point of 0 would feed) | 3 zeros | 4 all 0x80
    //   5 small - 36 (a per-image zero point z = max byte - 127 of extractor-like data: small magnitudes of either sign)
    //   6 small - 64
    //   7 the benchmark's bytes (bench.py, make_arena_torch(stats="l2")) under the kernel's zero point: 128-D rows, 60 %
    //     noisy copies of |N(0,1)|^3 prototypes and 40 % noise rows, L2-normalised, x 512, rounded, clamped to u8, ^ 0x80
    // LADDER_DATA_X: the same choice for the resident X side alone (default: what LADDER_DATA says) - the streamed Y side
    // (A operand, through LDS) and the X side (B operand, registers) may be encoded independently.
    const int mode = std::getenv("LADDER_DATA") ? std::atoi(std::getenv("LADDER_DATA")) : 0;
    const int mode_x = std::getenv("LADDER_DATA_X") ? std::atoi(std::getenv("LADDER_DATA_X")) : mode;
    std::vector<int> h(8192);
    // mode 7: 256 rows of 128 bytes (the first 128 rows feed the Y side, the others the X side)
    std::vector<unsigned char> bench_bytes(8192 * 4);
    {
        std::mt19937 gen(2024);
        std::normal_distribution<float> nd(0.0f, 1.0f);
        auto cube = [&] { const float v = std::fabs(nd(gen)); return v * v * v; };
        const int nproto = 32;
        std::vector<float> proto(nproto * 128), pmean(nproto);
        for (int p = 0; p < nproto; ++p) {
            float n2 = 0.0f, sum = 0.0f;
            for (int k = 0; k < 128; ++k) { proto[p * 128 + k] = cube(); n2 += proto[p * 128 + k] * proto[p * 128 + k]; }
            for (int k = 0; k < 128; ++k) { proto[p * 128 + k] /= std::sqrt(n2); sum += proto[p * 128 + k]; }
            pmean[p] = sum / 128.0f;
        }
        size_t high = 0;
        for (int r = 0; r < 256; ++r) {
            float d[128], n2 = 0.0f;
            const bool copy = (gen() % 10u) < 6u;
            const int p = (int)(gen() % (unsigned)nproto);
            for (int k = 0; k < 128; ++k) {
                d[k] = copy ? std::max(0.0f, proto[p * 128 + k] + nd(gen) * 0.08f * pmean[p]) : cube() * 0.1f;
                n2 += d[k] * d[k];
            }
            const float inv = 1.0f / std::max(std::sqrt(n2), 1e-12f);
            for (int k = 0; k < 128; ++k) {
                const float q = std::nearbyint(512.0f * d[k] * inv);
                const unsigned char u = (unsigned char)std::min(255.0f, std::max(0.0f, q));
                high += u >= 128;
                bench_bytes[r * 128 + k] = u ^ 0x80u;
            }
        }
        if (mode == 7 || mode_x == 7)
            std::printf("data mode 7: %.4f of the u8 bytes are >= 128 (before the zero point)\n", (double)high / (256.0 * 128.0));
    }
    unsigned s = 12345;
    auto rnd = [&] { s = s * 1664525u + 1013904223u; return s >> 8; };
    for (size_t i = 0; i < h.size(); ++i) {
        const int md = i < 4096 ? mode : mode_x;
        unsigned w = 0;
        for (int b = 0; b < 4; ++b) {
            unsigned byte;
            const unsigned r = rnd();
            const unsigned small = (r & 1) ? (r >> 1) % 12 : ((r >> 1) % 64);  // half near zero, half up to 63
            switch (md) {
                case 1: byte = 0x80u + small; break;
                case 2: byte = small; break;
                case 3: byte = 0; break;
                case 4: byte = 0x80u; break;
                case 5: byte = (small - 36u) & 255u; break;
                case 6: byte = (small - 64u) & 255u; break;
                case 7: byte = bench_bytes[i * 4 + b]; break;
                default: byte = r & 255u;
            }
            w |= byte << (8 * b);
        }
        h[i] = (int)w;
    }
    std::printf("data mode %d (Y side), %d (X side)\n", mode, mode_x);
    int *d_seed, *d_out;
    CHECK(hipMalloc(&d_seed, 8192 * sizeof(int) + 64));
    CHECK(hipMalloc(&d_out, 4096 * sizeof(int)));
    CHECK(hipMemcpy(d_seed, h.data(), 8192 * sizeof(int), hipMemcpyHostToDevice));
    std::printf("CUs %d\n", cus);
    if (std::getenv("LADDER_UNITS")) {  // the unit-width question: today's loop against one insertion per larger unit
        struct Rung { const char* name; void (*launch)(int, int, const int*, int*); };
        const Rung rungs[5] = {
            {"32x32x32 rung 3 (11 VALU per 16 outputs)", [](int t, int g, const int* sd, int* o) {
                hipLaunchKernelGGL((ladder_kernel<8, 4, 3>), dim3(g), dim3(512), 0, 0, t, sd, o); }},
            {"32x32x32 rung 4, insertion per 32 outputs", [](int t, int g, const int* sd, int* o) {
                hipLaunchKernelGGL((ladder_kernel<8, 4, 4>), dim3(g), dim3(512), 0, 0, t, sd, o); }},
            {"16x16x64, 8-output unit, 4-op insertion (old)", [](int t, int g, const int* sd, int* o) {
                hipLaunchKernelGGL((ladder16_kernel<8, 3>), dim3(g), dim3(512), 0, 0, t, sd, o); }},
            {"16x16x64, 64-row unit (11 VALU per 16)", [](int t, int g, const int* sd, int* o) {
                hipLaunchKernelGGL((ladder16u_kernel<8, 2>), dim3(g), dim3(512), 0, 0, t, sd, o); }},
            {"16x16x64, 128-row unit (9.5 VALU per 16)", [](int t, int g, const int* sd, int* o) {
                hipLaunchKernelGGL((ladder16u_kernel<8, 4>), dim3(g), dim3(512), 0, 0, t, sd, o); }},
        };
        // one untimed pass over all rungs first: the first ~100 ms of a process run at another clock than the rest
        for (int k = 0; k < 5; ++k)
            for (int i = 0; i < 5; ++i) rungs[k].launch(8192, cus, d_seed, d_out);
        CHECK(hipDeviceSynchronize());
        for (int rep = 0; rep < 3; ++rep)
            for (int k = 0; k < 5; ++k) {
                const Rung& r = rungs[(k + 2 * rep) % 5];  // repetitions start at rungs 0, 2, 4
                measure(r.name, rep, [&](int t) { r.launch(t, cus, d_seed, d_out); });
            }
        return 0;
    }
    if (std::getenv("LADDER_QUICK")) {  // the bare loop and the kernel's loop only (data-mode sweeps)
        run<8, 4, 0, 0>("MFMA only", d_seed, d_out, cus);
        run<8, 4, 2, 0>("+ C-operand block", d_seed, d_out, cus);
        run<8, 4, 3, 0>("+ 11 VALU per unit", d_seed, d_out, cus);
        run<4, 8, 3, 0>("+ 11 VALU per unit", d_seed, d_out, cus);
        return 0;
    }
    run<8, 4, 0, 0>("MFMA only", d_seed, d_out, cus);
    run<8, 4, 1, 0>("+ A-fragment ds_read_b128", d_seed, d_out, cus);
    run<8, 4, 2, 0>("+ C-operand block", d_seed, d_out, cus);
    run<8, 4, 3, 0>("+ 11 VALU per unit", d_seed, d_out, cus);
    run<8, 4, 4, 0>("+ insertion per two units (9.5)", d_seed, d_out, cus);
    run<4, 8, 0, 0>("MFMA only", d_seed, d_out, cus);
    run<4, 8, 1, 0>("+ A-fragment ds_read_b128", d_seed, d_out, cus);
    run<4, 8, 2, 0>("+ C-operand block", d_seed, d_out, cus);
    run<4, 8, 3, 0>("+ 11 VALU per unit", d_seed, d_out, cus);
    run<8, 4, 0, 1>("MFMA only", d_seed, d_out, cus);
    run<8, 4, 2, 1>("+ A fragments + C block", d_seed, d_out, cus);
    run<8, 4, 3, 1>("+ 11 VALU per unit", d_seed, d_out, cus);
    run<4, 8, 0, 1>("MFMA only", d_seed, d_out, cus);
    run<4, 8, 2, 1>("+ A fragments + C block", d_seed, d_out, cus);
    run<4, 8, 3, 1>("+ 11 VALU per unit", d_seed, d_out, cus);
    run16<8, 0>("MFMA only", d_seed, d_out, cus);
    run16<8, 1>("+ A-fragment ds_read_b128", d_seed, d_out, cus);
    run16<8, 2>("+ C-operand block", d_seed, d_out, cus);
    run16<8, 3>("+ 8 VALU per 8 outputs", d_seed, d_out, cus);
    run16<4, 0>("MFMA only", d_seed, d_out, cus);
    run16<4, 3>("+ reads + 8 VALU per 8 outputs", d_seed, d_out, cus);
    for (int w : {4, 8}) {
        hipEvent_t e0, e1;
        CHECK(hipEventCreate(&e0));
        CHECK(hipEventCreate(&e1));
        const int iters = 1 << 17;
        float best = 1e30f;
        for (int rep = 0; rep < 4; ++rep) {
            CHECK(hipEventRecord(e0));
            if (w == 4) hipLaunchKernelGGL((mfma16_kernel<4>), dim3(cus), dim3(256), 0, 0, rep ? iters : 64, d_seed, d_out);
            else hipLaunchKernelGGL((mfma16_kernel<8>), dim3(cus), dim3(512), 0, 0, rep ? iters : 64, d_seed, d_out);
            CHECK(hipEventRecord(e1));
            CHECK(hipEventSynchronize(e1));
            float ms;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            if (rep && ms < best) best = ms;
        }
        // a 16x16x64 MFMA is half a 32x32x32 one: report per 32x32x32-equivalent
        const double eq = (double)(w / 4) * iters * 8 / 2;
        const double ns = best * 1e6 / eq;
        std::printf("%-34s W%d register-only reference: %8.3f ms  %6.2f ns/MFMA-equiv/SIMD = %.3f of nominal\n", "16x16x64", w, best, ns, 13.3333 / ns);
    }
    return 0;
}
