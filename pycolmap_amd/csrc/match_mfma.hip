// match_mfma.hip — the hot kernel: one-way top-2 scan of 128-D u8 descriptor dot products on
// the int8 matrix cores (v_mfma_i32_16x16x64_i8).  gfx950 only.
//
// "One way" = COLMAP's FindBestMatchesOneWayBruteForce: for every row of
// image X, the best dot product against all rows of image Y (lowest index among ties) and the
// second-largest value with multiplicity.  The host runs it twice per pair:
//   MODE 0  X = image 1 (all rows)            , Y = image 2  -> accept bits, and the row table's 16-row X tiles that
//           hold a set bit: every reader of the row table tests the row's bit first (resolve_index* side 0,
//           select_candidates, finalize)
//   MODE 1  X = image 2 (candidate rows only) , Y = image 1  -> column table, lazily: only the
//           columns some accepted row points at (select_candidates_kernel), every one of them stored; the cross
//           check never looks at any other column, so results equal COLMAP's full transposed scan.
// The kernel reports the best VALUE, the 32-row TILE of Y that holds it, and the largest value
// OUTSIDE the best's unit, which is that tile (a lower bound of the second); resolve_index_kernel
// (match_common.hip) turns the tile into the exact lowest index and completes the second value
// by recomputing those 32 dot products, only for rows that can still pass COLMAP's acceptance
// tests (a larger second only ever rejects).
//
// Why this shape (measured on MI355X, tools/ubench_ladder.hip, profiles/scan16/, profiles/scan128/):
//   * the scan is bound by the package power budget; v_mfma_i32_16x16x64_i8 costs a quarter less energy per
//     MAC than v_mfma_i32_32x32x32_i8, the instruction this kernel used before;
//   * every 32-bit min/max/med3/max3/shift-or is HALF rate on gfx950 (~4.5 clk / wave64) and a wave has room for
//     about 14 of them per 8 MFMAs (16 outputs per lane); at ~2.0 GHz the loop is limited by vector issue (an MFMA
//     of this shape holds the SIMD's vector issue for 8 of its 16 clocks), so every VALU instruction saved counts.
// A values-only top-2 insertion per output does not fit that.  The scan therefore does less: it reduces a
// lane's 32 outputs of a UNIT to their maximum (16 x v_max3/v_max) and keeps the top two of those maxima plus the
// unit of the best: 19 VALU per 32 outputs = 9.5 per 16.  The row's exact second-largest value is completed by
// resolve_index_kernel from the winning tile (see `phase` below).  Everything else is moved off the VALU:
//   * zero point: the matrix core is signed, the arena holds a' = a - 128 (bytes ^ 0x80) and
//         sum a*b = sum a'*b' + 128*SX_i + 128*SY_j - 2^21        (SX, SY = byte sums, int32 exact)
//     The MFMA's A operand is the streamed Y tile and its B operand the resident X tile, so a
//     lane owns ONE X row and its accumulator registers are different Y rows: the Y term
//     128*SY_j is per register and rides in as the MFMA's C operand (four ints per MFMA, one ds_read_b128);
//     the X term is constant per lane, dropped during the scan and restored
//     (with the -2^21) when the row is decoded.  acc = v - 128*SX_i + 2^21, full int32 range:
//     ANY u8 data, any size.
//   * argmax: values only in the scan; the unit holding the best rides in the low bits of the value's key.
//
// Units.  v_mfma_i32_16x16x64_i8: lane l supplies row (l & 15) of A and of B, k bytes 16 (l >> 4) .. + 15 of the
// 64, and owns D rows 4 q + r (q = l >> 4, r = 0..3) of column (l & 15).  Which Y row is fed as A row m is the
// kernel's choice (each lane picks the LDS address it reads): within a 128-row BLOCK of Y, row m of MFMA tile
// t = 0..7 is Y row 32 (m >> 2) + 4 t + (m & 3).  Lane quarter q's 32 outputs of a block are then the contiguous
// rows 32 q .. 32 q + 31 - one unit, exactly the 32-row tile 4 block + q that resolve_index recomputes - and the C
// operand of a tile is four consecutive ints.  A block is scanned in four STEPS of two MFMA tiles each (32 rows'
// worth of fragments); the scan of an image ends with the last block that holds rows.
//
// Work items.  Every pair's X side is cut into
// SEGMENTS of 128 rows; the segments of all pairs that stream the same Y image are packed, four to
// an ITEM, by three small kernels (seg_count / seg_scan / seg_fill below) into 64-byte descriptors
// that carry every pointer a wave needs.  A workgroup pops an item, streams that Y image once
// through LDS, and its waves scan their own segments - which may belong to DIFFERENT pairs (they
// only share the Y stream).  So a 4,500-row image costs 36 segment-times, not 5 x 8; a 512-row pair
// fills a workgroup; and the reverse scan's candidate lists (known only on the
// device: the packing kernels read cand_cnt) are packed just as tightly.
//
// Shape.  One workgroup per item (dynamic queue; items in Y order so co-resident workgroups stream the same image out
// of L2; the next item's descriptor is fetched while the current one is scanned).  The queue's ticket is a RUN of up to
// R items - item t of R consecutive streamed images, which in an exhaustive job hold the same X segments: an item
// marked so in the run table keeps its X rows in the registers instead of fetching them again ("Runs" below; R = 1 and
// no table: a ticket is an item).  256 threads, a segment (eight resident 16-row X tiles) per wave, one wave per SIMD - and
// TWO such workgroups on every CU, each popping its own items, so that every SIMD still holds two waves.  They are
// independent: at an item boundary all four waves of a workgroup leave the loop together (they wait for the next
// item's chunks and X rows, decode, and meet at two barriers: 6.7 % of an item's clocks, profiles/boundary/), and
// the partner workgroup's wave then has the SIMD to itself instead of the matrix pipe of the whole CU standing idle.
// A chunk crossing's barrier joins four waves on four SIMDs.  Both workgroups must fit: at most 256 registers per lane
// (amdgpu_waves_per_eu pins it; MODE 0 compiles to 246 VGPRs, MODE 1 to 194, without scratch - check
// -Rpass-analysis=kernel-resource-usage after every change, profiles/scanloop/kernel_resource_usage.txt) and at most
// 80 KB of LDS (66 KB, ONE __shared__ object); launch_match_mfma asks the runtime.
// Taking the ticket two items ahead and warming the next item's X rows in L2 were both built and measured, and
// neither paid (profiles/boundary/README.md).
// Y streams through LDS in 128-row chunks (one block) by direct-to-LDS DMA, a ring of four buffers, a wave's four
// 1-KiB pieces of chunk c+3 issued one per step of chunk c, one barrier per chunk behind a counted wait; the prepared
// arena is pre-swizzled (arena_swizzle, amc_internal.h) so the linear DMA image is bank-conflict-free for
// ds_read_b128.  Each wave software-pipelines: the 4 MFMAs of (step, X tile) u+1 are interleaved with the
// VALU of u, two accumulator sets.
// The chunk loop.  Per chunk a wave issues 128 MFMAs and the 152 vector instructions of the top-2 work, and the vector
// pipe is what bounds it - so nothing else in the loop is a vector instruction, but for three adds per chunk
// (tools/scan_loop_census.py counts the assembly, tests/test_match_scan_loop_census_cpu.py holds it there):
//   * LDS reads: three lane bases carry the lane's part and the ring position and move to the next buffer in place,
//     once per chunk; step and tile are compile-time, so every ds_read_b128 is base + immediate;
//   * DMA: the global address is a scalar base advanced on the scalar unit plus the one lane offset lane * 16 (the
//     instruction's saddr form), the LDS address is m0;
//   * conditions: the loop is peeled by what is in flight - a STEADY loop for the chunks c with c + 3 < nchunks
//     (a fetch in every step, one fixed wait at the crossing), a DRAIN loop for the last up to three (no fetch, the
//     waits that fit) - and by whether the wave has rows: a wave without rows runs loops of its own that only issue
//     its DMA pieces, wait and meet the barriers.  Every wave of a workgroup executes the same number of s_barrier.
#include <cstdlib>

#include "amc_internal.h"
#include "scan_accept.h"

namespace amc {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const void gvoid_t;
typedef __attribute__((address_space(3))) void lvoid_t;

constexpr int kBN = 128;                // Y rows per LDS chunk: one block
constexpr int kYS = kBN / 32;           // 32-row steps per chunk
constexpr int kUR = 128;                // Y rows per block; arena_swizzle (amc_internal.h) is made for this width
constexpr int kSPB = kUR / 32;          // steps per block
constexpr int kChunkBytes = kBN * kDim; // 16 KiB
constexpr int kW = kSegsPerItem;        // waves per workgroup: a segment each
constexpr int kWGPerCU = 2;             // workgroups that share a CU, one wave of each on every SIMD
constexpr int kXT = kSegRows / 16;      // resident 16-row X tiles per wave
constexpr int kKeyShift = 7, kKeyCarried = 127;
// run table entries (launch_build_runs): an item index, with kRunSameX if the item's four X segments are those of the
// run's previous item; kRunNone where a streamed image has no such item
constexpr uint32_t kRunSameX = 0x80000000u, kRunNone = 0xFFFFFFFFu;

// single LDS object (a second __shared__ object de-pipelines the DMA waits).  A ring of FOUR chunk buffers: while
// chunk c is scanned, chunks c+1 and c+2 have landed (or are landing) and chunk c+3 is being fetched into the buffer
// chunk c-1 left - so its DMA pieces need not wait for a barrier and are issued one per step instead of all at the
// chunk boundary, where they stalled the wave's MFMA stream (2.7 % of the scan).  Three chunks ahead of 128 rows each
// is the prefetch distance in rows that two chunks of 256 were.
constexpr int kNB = 4;
constexpr int kOffRs = 0;                        // kNB x rs128 chunks (kBN ints each)
constexpr int kOffQ = kOffRs + kNB * kBN * 4;    // queue slot, copy-part slot
constexpr int kOffB = kOffQ + 16;                // kNB x descriptor chunks
constexpr int kLdsBytes = kOffB + kNB * kChunkBytes;
static_assert(kRowPad % kBN == 0, "a chunk divides the row padding: every chunk that holds a row lies inside the padded image");
static_assert(kUR == 128 && kSPB == 4 && kBN == kUR, "a lane quarter's rows of a block are one 32-row tile; the loop body is one block, which is one chunk");
static_assert(kRowPad % kSegRows == 0 && kSegRows % 32 == 0, "segments tile the padded rows");
static_assert((kNB & (kNB - 1)) == 0, "the ring position is taken modulo kNB with a mask");
static_assert(kWGPerCU * kLdsBytes <= 160 * 1024, "LDS of one CU holds two workgroups");
static_assert(kW == 4, "one wave of a workgroup per SIMD");
static_assert(sizeof(SegDesc) == 64, "a descriptor is 16 dwords: one per lane of a quarter wave");

// dword positions of the SegDesc fields (a wave holds its descriptor in ONE register: lane l < 16 has dword l)
enum : int { kDXprep = 0, kDXrs = 2, kDOut = 4, kDList = 6, kDYprep = 8, kDYrs = 10, kDCnt = 12, kDAccword = 13,
             kDYrows = 14 };

// The MFMAs and the VALU that reads their results are inline asm: hipcc pattern-matches v_max3 only some of the
// time, selects the tied form for an MFMA with a C operand (and then copies the C registers into the accumulator
// first, on the matrix pipe's critical path), and pads dependent asm statements with s_nops it cannot know to be
// needless.  hipcc does not pad hazards for inline asm either, so the kernel is structured so that an accumulator
// is only ever read by the VALU after four further MFMAs have issued behind the one that completed it (see `phase`);
// sched_barriers pin that order.
// First MFMA of an accumulator: C operand = four of the Y rows' 128*SY, destination = a free accumulator (early
// clobber).  Operands come from LDS reads (the waitcnt pass tracks asm operands); the result is next read by the
// dependent MFMA (same destination as C operand: no wait states needed).
__device__ __forceinline__ void mfma_first(i32x4& d, const i32x4& a, const i32x4& b, const i32x4& c) {
    asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %3" : "=&v"(d) : "v"(a), "v"(b), "v"(c));
}
// The second MFMA (k bytes 64..127) accumulates in place.
__device__ __forceinline__ void mfma_acc(i32x4& d, const i32x4& a, const i32x4& b) {
    asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+v"(d) : "v"(a), "v"(b));
}

struct YFrag {
    i32x4 f[2][2];  // one step: two MFMA tiles x two 64-deep k halves (MFMA A operand)
    i32x4 ci[2];    // 128*SY_j for this lane's four Y rows of either tile (MFMA C operand)
};

#ifdef AMC_SCAN_STAMPS
// Diagnostic build only (tools/scan_stamps.hip includes this file with the macro; libamc.so is compiled without it and
// holds none of this): s_memtime stamps around the places where a wave's MFMA stream stops, summed per wave in scalar
// registers and stored - running sums, lane 0 - behind every item.  Per (MODE, workgroup, wave) sixteen dwords, over the
// items that had a successor in the same workgroup:
//   [0] clocks from arriving at a chunk crossing's s_waitcnt to leaving its s_barrier   [1] clocks from the
//   __syncthreads() that ends an item's scan to the first MFMA of the next item   [2] clocks from an item's first MFMA
//   to the next item's   [3] such items   [4] those of them this wave had rows in
// for the workgroup's last item: [5] as [0]   [6] first MFMA to the end of the epilogue   [7] 1
// and of [1] and [3] the part of the successors that kept the X rows (kRunSameX): [8] clocks   [9] items
// [1] split: [10] clocks from that __syncthreads() to arriving at the next item's top wait (the next item's loads issued,
// this item decoded and stored)   [11] clocks in that wait and its barrier (what is left of the loads' round trips, and
// the other waves); the rest of [1] is the way to the first MFMA.  [12], [13]: [10] and [11] of the successors that kept
// the X rows
constexpr int kStampMaxWG = 1024, kStampDwords = 16;
__device__ uint32_t g_scan_stamps[2 * kStampMaxWG * kSegsPerItem * kStampDwords];
#define AMC_STAMP() ((uint32_t)__builtin_amdgcn_s_memtime())
#endif

// The previous batch's matches on their way to the host (CopyJob, amc_internal.h).  The runtime's own copy kernel
// covers the buffer with its grid and takes every CU while PCIe moves 400 MB (10 ms, and the scan behind it waits:
// kernel trace of the dense set, 19 ms of 292 per call); a small copy kernel on a second stream shares a hardware queue
// with the scan's stream more often than not.  So the copy rides in the scan's own launch: the first `parts`
// workgroups to arrive take one part each - 256 lanes with four 16-byte loads in flight per lane, sixteen such
// workgroups saturate PCIe - and then scan like the others; the scan loses parts x 10 ms of one workgroup's time.
// Compiled as ONE general function of (tid, nthreads).  `used` keeps the compiler from specialising it for its
// single caller's thread count (which also moves that kernel's register allocation); the assumption states the
// ranges it may rely on.
__device__ __noinline__ __attribute__((used)) void copy_part(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                             unsigned long long b, unsigned long long e, int tid,
                                                             int nthreads) {
    __builtin_assume(tid >= 0 && tid < 1024 && nthreads >= 256 && nthreads <= 512);
    unsigned long long i = b + (unsigned long long)tid;
    const unsigned long long st = (unsigned long long)nthreads;
    for (; i + 3 * st < e; i += 4 * st) {
        const uint4 v0 = src[i], v1 = src[i + st], v2 = src[i + 2 * st], v3 = src[i + 3 * st];
        dst[i] = v0; dst[i + st] = v1; dst[i + 2 * st] = v2; dst[i + 3 * st] = v3;
    }
    for (; i < e; i += st) dst[i] = src[i];
}

// Two waves per SIMD, pinned: a 256-thread bound alone lets the compiler plan for one wave per SIMD and 512 registers,
// and then only one workgroup fits a CU (launch_match_mfma checks the occupancy it gets).
template <int MODE>
__global__ __launch_bounds__(64 * kW) __attribute__((amdgpu_waves_per_eu(kWGPerCU, kWGPerCU)))
void match_mfma_kernel(const SegDesc* __restrict__ segs, const uint32_t* __restrict__ nruns_p,
                       uint32_t* __restrict__ queue_head, uint32_t* __restrict__ accmask,
                       const ScanAccept* __restrict__ accept, CopyJob job, uint32_t* __restrict__ copy_head,
                       const uint32_t* __restrict__ run_items, int run_len) {
    static_assert(kChunkBytes / 1024 == kW * kYS, "a chunk splits into 1 KiB DMA pieces, one per wave and step");
    static_assert(kBN * 4 == 512, "a chunk's rs128 block is half a wave's DMA");
    __shared__ __attribute__((aligned(16))) char smem[kLdsBytes];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    volatile uint32_t* s_q = reinterpret_cast<volatile uint32_t*>(smem + kOffQ);
    if constexpr (MODE == 0) {
        if (job.parts) {  // (wave-uniform: a kernel argument)
            // (the slot lives in smem: with a second LDS object in the kernel the compiler orders every LDS read of
            // the scan behind the pending DMA with an s_waitcnt vmcnt(0), one per step)
            volatile uint32_t* s_part = reinterpret_cast<volatile uint32_t*>(smem + kOffQ + 4);
            if (tid == 0) *s_part = atomicAdd(copy_head, 1u);
            __syncthreads();
            const uint32_t part = *s_part;
            if (part < job.parts)
                copy_part(static_cast<const uint4*>(job.src), static_cast<uint4*>(job.dst), job.n16 * part / job.parts,
                          job.n16 * (part + 1) / job.parts, tid, 64 * kW);
        }
    }
    const uint32_t nruns = *nruns_p;  // (without a run table: the items, every one a run of its own)
    const ScanAccept sa = *accept;  // twelve scalar registers for the whole kernel (re-read per row block it is four dependent scalar-cache round trips per X tile)

    // the entries of run r, one per lane: lanes run_len.. hold "none", and so does every lane of a run past the end
    auto load_run = [&](uint32_t r) -> uint32_t {
        uint32_t v = kRunNone;
        if (r < nruns) {
            if (run_items) {  // (wave-uniform: a kernel argument)
                if (lane < run_len) v = run_items[(size_t)r * run_len + lane];
            } else if (lane == 0) {
                v = r;
            }
        }
        return v;
    };
    // the first entry of a run behind position `after` (-1: from its start) that is an item: its position, or -1
    auto next_entry = [&](uint32_t rv, int after) -> int {
        const unsigned long long m = __ballot(rv != kRunNone) & (~0ull << (after + 1));
        return m ? __builtin_ctzll(m) : -1;
    };
    // the wave's descriptor of the item of run entry e, one dword per lane (lanes 16.. hold 0)
    auto load_desc = [&](uint32_t e) -> int {
        int v = 0;
        if (e != kRunNone && lane < 16)
            v = reinterpret_cast<const int*>(segs + (size_t)(e & ~kRunSameX) * kSegsPerItem + wid)[lane];
        return v;
    };
    auto dword = [&](int dv, int f) -> int { return __builtin_amdgcn_readlane(dv, f); };
    auto dptr = [&](int dv, int f) -> const char* {
        const uint64_t lo = (uint32_t)__builtin_amdgcn_readlane(dv, f);
        const uint64_t hi = (uint32_t)__builtin_amdgcn_readlane(dv, f + 1);
        return reinterpret_cast<const char*>(lo | (hi << 32));
    };

    // chunk c of the Y image (prep / rs128 base pointers) -> LDS buffer `buf`, in 1 KiB pieces dealt to the waves; a
    // wave owns kPW pieces of a chunk, wave 0 also its rs128 block.  A DMA instruction's global address is a scalar
    // base, wave-uniform and computed on the scalar unit, plus ONE 32-bit lane offset that never changes, lane * 16
    // (the instruction's `saddr` form: written as base + zero-extended offset the compiler selects it); its LDS
    // address is m0 + lane * 16.  No vector instruction forms an address.
    constexpr int kPW = kChunkBytes / 1024 / kW;
    uint32_t lane16 = (uint32_t)lane * 16u;
    // (an empty asm in front of every use: the offset stays ONE 32-bit register, extended where it is used; hoisted, the
    // extension makes it a 64-bit lane address and every DMA instruction a 64-bit vector add)
    auto lane_off = [&]() __attribute__((always_inline)) -> uint32_t {
        asm volatile("" : "+v"(lane16));
        return lane16;
    };
    auto stage_piece = [&](const char* yprep, int c, int buf, int ps) __attribute__((always_inline)) {
        const int piece = ps * kW + wid;
        const char* src = yprep + ((size_t)c * kChunkBytes + piece * 1024);
        __builtin_amdgcn_global_load_lds((gvoid_t*)(src + lane_off()),
                                         (lvoid_t*)(smem + kOffB + buf * kChunkBytes + piece * 1024), 16, 0, 0);
    };
    auto stage_rs = [&](const char* yrs, int c, int buf) __attribute__((always_inline)) {
        const char* src = yrs + (size_t)c * kBN * 4;
        if (wid == 0 && lane < kBN / 4)  // rs128 of this chunk's rows: 512 B, the lower half of the wave
            __builtin_amdgcn_global_load_lds((gvoid_t*)(src + lane_off()), (lvoid_t*)(smem + kOffRs + buf * kBN * 4), 16, 0,
                                             0);
    };
    auto stage = [&](const char* yprep, const char* yrs, int c, int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int ps = 0; ps < kPW; ++ps) stage_piece(yprep, c, buf, ps);
        stage_rs(yrs, c, buf);
    };
    // an item starts with the chunks 0 .. kNB - 2 of its Y image in flight, as many as hold rows (dv: its descriptor)
    auto stage_head = [&](int dv) __attribute__((always_inline)) {
        const char* yprep = dptr(dv, kDYprep);
        const char* yrs = dptr(dv, kDYrs);
        const int yrows = dword(dv, kDYrows);
        stage(yprep, yrs, 0, 0);
#pragma unroll
        for (int c = 1; c < kNB - 1; ++c)
            if (yrows > c * kBN) stage(yprep, yrs, c, c);
    };

    // A-operand fragments + C blocks of step `ys` of the chunk the lane bases point at, as six 16-byte reads: parts 0,
    // 1 = the C blocks (needed first), 2..5 = the two tiles' two k halves.  The scan spreads them over the phases of the
    // previous step, one behind each phase's last MFMA, so they never pile up in one MFMA shadow.
    // This lane's A row m = l15 of tile t of block b is row b*128 + 32 (m >> 2) + 4 t + (m & 3) of the chunk; its
    // swizzle does not depend on b and t (arena_swizzle takes row bits 1, 5 and 6).
    const int yrow_lane = (kUR / 4) * (l15 >> 2) + (l15 & 3);
    const int ysw_lane = arena_swizzle(yrow_lane);
    // Three lane bases: the byte offsets of the two k halves' slots and of the C block in the ring buffer being read.
    // They carry the lane's part AND the ring position (once per chunk the scan adds a wave-uniform buffer stride to
    // them in place, `advance`); the step and the tile are compile-time, so every ds_read_b128 is base + immediate.
    int yb0 = kOffB + yrow_lane * kDim + ((lq ^ ysw_lane) * 16);
    int yb1 = kOffB + yrow_lane * kDim + (((4 + lq) ^ ysw_lane) * 16);
    int cbs = kOffRs + (kUR / 4) * lq * 4;
    auto load_y_part = [&](YFrag& y, int ys, int part) __attribute__((always_inline)) {
        if (part < 2) {
            // accumulator register r of tile t <-> Y row 32 lq + 4 t + r of the block (the -2^21 lives in xterm)
            y.ci[part] = *reinterpret_cast<const i32x4*>(smem + cbs + (8 * ys * 4 + 16 * part));
        } else {
            const int tt = (part - 2) >> 1, s = (part - 2) & 1;  // tile 2 ys + tt
            y.f[tt][s] = *reinterpret_cast<const i32x4*>(smem + (s ? yb1 : yb0) + (8 * ys + tt * 4) * kDim);
        }
    };
    auto load_y = [&](YFrag& y, int ys) __attribute__((always_inline)) {
#pragma unroll
        for (int part = 0; part < 6; ++part) load_y_part(y, ys, part);
    };
    // the bases move from ring buffer cb to the next one (three VALU instructions per chunk; asm, so that the compiler
    // keeps them in place instead of holding one set of bases per buffer)
    auto advance = [&](int cb) __attribute__((always_inline)) {
        const int k = cb == kNB - 1 ? -(kNB - 1) : 1;
        asm volatile("v_add_u32 %0, %3, %0\n\tv_add_u32 %1, %3, %1\n\tv_add_u32 %2, %4, %2"
                     : "+v"(yb0), "+v"(yb1), "+v"(cbs) : "s"(k * kChunkBytes), "s"(k * kBN * 4));
    };

    // resident X state: B-operand fragments, one (best, second, block) per lane and X tile; part = the running
    // maximum of the unit being scanned
    i32x4 xf[kXT][2];
    int best[kXT], sec[kXT], btile[kXT], xterm[kXT], part[kXT];
    auto load_x = [&](int dv) __attribute__((always_inline)) {
        const int cnt = dword(dv, kDCnt);
        const char* xprep = dptr(dv, kDXprep);
        const int* xrs = reinterpret_cast<const int*>(dptr(dv, kDXrs));
#pragma unroll
        for (int xt = 0; xt < kXT; ++xt) {
            const int kl = xt * 16 + l15;  // row within the segment
            int row;
            if (MODE == 0) {
                row = kl;  // xprep / xrs point at the segment's first row; rows past the image's end are zero padding
            } else {
                // candidate rows; a segment's tail repeats its last row (results never stored), an empty one reads row 0
                const uint32_t* list = reinterpret_cast<const uint32_t*>(dptr(dv, kDList));
                row = cnt > 0 ? (int)list[min(kl, cnt - 1)] : 0;
            }
            const char* rp = xprep + (size_t)row * kDim;
            const int sw = arena_swizzle(row);
#pragma unroll
            for (int s = 0; s < 2; ++s) xf[xt][s] = *reinterpret_cast<const i32x4*>(rp + (((4 * s + lq) ^ sw) * 16));
            // acc = sum a'b' + 128*SY_j = v - (128*SX_i - 2^21)
            xterm[xt] = xrs[row] - (1 << 21);
            // COLMAP's floor best = second = 0  <=>  acc = -xterm
            best[xt] = ((-xterm[xt]) << kKeyShift) | kKeyCarried;  // a key: value << 7 | block code (see `insert`)
            sec[xt] = best[xt];
            btile[xt] = -1;
        }
    };
    // an item whose X rows are the ones this wave already holds (a run entry with kRunSameX): xf and xterm stay, the
    // top-2 state starts over as load_x starts it
    auto reset_x = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int xt = 0; xt < kXT; ++xt) {
            best[xt] = ((-xterm[xt]) << kKeyShift) | kKeyCarried;
            sec[xt] = best[xt];
            btile[xt] = -1;
        }
    };

#ifdef AMC_SCAN_STAMPS
    uint32_t st_a = 0, st_first = 0, st_end = 0, st_sum[5] = {0, 0, 0, 0, 0}, st_kept[2] = {0, 0};
    uint32_t st_w0 = 0, st_w1 = 0, st_split[4] = {0, 0, 0, 0};
    bool st_prev = false, st_prev_active = false, st_keep_x = false;
    uint32_t* const st_slot = g_scan_stamps + ((size_t)(MODE * kStampMaxWG + min((int)blockIdx.x, kStampMaxWG - 1)) * kW + wid) * kStampDwords;
#endif
    // Runs.  A ticket is a run: up to run_len items that follow each other in this workgroup, item t of consecutive
    // streamed images, so that an entry marked kRunSameX finds its X rows in the registers.  The workgroup holds the
    // entries of its run (rv), of its next run (rvn) and - in flight from the first item of a run on - of the run after
    // that (rvn2): the next item's descriptor can then always be fetched at the top of an item, whichever run it is in.
    // Without a table a ticket IS its entry, nothing is in flight for it and the queue is one ticket ahead, not two:
    // the items are handed out exactly as they were before there were runs (a reverse scan has one or two items per
    // workgroup, and a workgroup that holds a second ticket while another idles is what it cannot afford).
    const bool table = MODE == 0 && run_items != nullptr;  // (wave-uniform)
    uint32_t rv = kRunNone, rvn, rvn2 = kRunNone;
    if (tid == 0) *s_q = atomicAdd(queue_head, 1u);
    __syncthreads();
    rvn = load_run(*s_q);
    if (table) {
        __syncthreads();
        if (tid == 0) *s_q = atomicAdd(queue_head, 1u);
        __syncthreads();
        rvn2 = load_run(*s_q);
    }
    int kpos = next_entry(rvn, -1);  // (a run of the table holds an item; a ticket past the end holds none)
    uint32_t e = kpos >= 0 ? (uint32_t)__builtin_amdgcn_readlane((int)rvn, kpos) : kRunNone;
    bool first = true;  // this item starts a run: the entries move up and a ticket is taken
    int dv = load_desc(e);
    if (e != kRunNone) {
        stage_head(dv);
        if (dword(dv, kDCnt) > 0) load_x(dv);
    }
    __syncthreads();  // everyone has read the slot before it is rewritten

    while (e != kRunNone) {
        // chunks 0 .. 2 of this item's Y image are on their way and the X fragments are being loaded (issued by
        // the previous iteration or the prologue)
        const char* yprep = dptr(dv, kDYprep);  // the same in every descriptor of the item
        const char* yrs = dptr(dv, kDYrs);
        // Only the chunks that hold rows: what follows them is the image's zero padding (rows_pad is a multiple of
        // 256) - a zero row can never become a best nor raise a second, so a chunk of nothing else is neither
        // fetched nor scanned (an image of 4,000 rows paid for 4,096; n ~ U[2000, 6000]: 2.4 % of the scan; ending
        // at a 128-row chunk leaves 64 padded rows per image on average).
        const int nchunks = (dword(dv, kDYrows) + kBN - 1) / kBN;
        const bool active = dword(dv, kDCnt) > 0;  // wave-uniform
        if (first && tid == 0) *s_q = atomicAdd(queue_head, 1u);  // the run after the next (no table: the next item), behind the loads already in flight

        i32x4 acc[2][2];
        // 19 VALU for 32 outputs: the scan only keeps, per lane, the top two of the per-unit
        // MAXIMA (16 v_max3/v_max for the maximum of the unit's 32 outputs, then one insertion)
        // and the block of the best.  The second-largest VALUE of the whole row is either the
        // maximum of another unit - which the running `sec` then holds, ties included - or
        // sits inside the winning tile, where resolve_index_kernel recomputes the 32 dot
        // products anyway to find the index: it takes the second of those 32 as well and the
        // row's second is the larger of the two.
        // Insertion of a unit maximum (part[xt], consumed) into a lane's (best, second) state, in place.
        // Three instructions: the state holds KEYS, value << 7 | code, code = 126 - (block mod 64) (64 blocks = 8,192 rows).  The accumulators stay
        // below 2^24 in magnitude (|sum a'b'| <= 2^21, 128 SY < 2^22), so a key fits 32 bits; a larger value is a
        // larger key, equal values are ordered first block first (strict '>' of the reference scan), and the second
        // largest key carries the second largest value, equal ones included.  Every 64 blocks (and at the end of the
        // item) `flush` moves the block of a best found since the last flush to btile and marks the key "carried"
        // (code 127: it beats equal values of later blocks).  The block code is wave-uniform: a scalar operand.
        auto insert = [&](int xt, int code) __attribute__((always_inline)) {
            asm volatile(
                "v_lshl_or_b32 %2, %2, 7, %3\n\t"
                "v_med3_i32 %1, %0, %1, %2\n\t"  // sec <= best always: the new second of the maxima
                "v_max_i32 %0, %0, %2"
                : "+v"(best[xt]), "+v"(sec[xt]), "+v"(part[xt])
                : "s"(code));
        };
        auto flush = [&](int sb) __attribute__((always_inline)) {  // sb: the 64-block group that ends here
#pragma unroll
            for (int xt = 0; xt < kXT; ++xt) {
                const int c = best[xt] & 127;
                btile[xt] = c != kKeyCarried ? sb * 64 + (126 - c) : btile[xt];
                best[xt] |= kKeyCarried;
            }
        };
        // One phase = the 4 MFMAs of the NEXT (step, X tile) into `an` - two tiles x two k halves - with the VALU
        // of the CURRENT one (reading `ac`, completed by the previous phase) behind them: four max ops that fold
        // the step's 8 outputs into part[xtc] (the unit's first step starts it, sp == 0), and behind a unit's last
        // step the insertion of the finished maximum, deferred by one phase (X tile xtc - 1; the last X tile's goes
        // in with the first phase of the next step).  Interleaved, the matrix pipe stays fed; "the MFMAs, then the
        // VALU" leaves it idle whenever every wave of the SIMD is in its VALU stretch.
        // gb: the block this step belongs to, counted from the image's first.
        auto phase = [&](i32x4 (&an)[2], const YFrag& y, int xtn, const i32x4 (&ac)[2], int xtc, int sp, int gb)
                         __attribute__((always_inline)) {
            mfma_first(an[0], y.f[0][0], xf[xtn][0], y.ci[0]);
            mfma_first(an[1], y.f[1][0], xf[xtn][0], y.ci[1]);
            __builtin_amdgcn_sched_barrier(0);
            if (xtc == 0 ? sp == 0 : sp == kSPB - 1) {
                insert((xtc + kXT - 1) % kXT, 126 - ((xtc == 0 ? gb - 1 : gb) & 63));
                // the last unit of a 64-block group has just gone in: settle the blocks before the next group reuses the codes
                if (xtc == 0 && gb != 0 && (gb & 63) == 0) flush((gb >> 6) - 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            mfma_acc(an[0], y.f[0][1], xf[xtn][1]);
            mfma_acc(an[1], y.f[1][1], xf[xtn][1]);
            __builtin_amdgcn_sched_barrier(0);
            // `ac` is read here: four MFMAs have issued since the one that completed it.  One asm block (hipcc pads
            // dependent asm statements with s_nops it cannot know to be needless)
            int t0, t1;
            if (sp == 0)
                asm volatile(
                    "v_max3_i32 %0, %3, %4, %5\n\t"
                    "v_max3_i32 %1, %6, %7, %8\n\t"
                    "v_max3_i32 %0, %0, %9, %10\n\t"
                    "v_max_i32 %2, %0, %1"
                    : "=&v"(t0), "=&v"(t1), "=&v"(part[xtc])
                    : "v"(ac[0][0]), "v"(ac[0][1]), "v"(ac[0][2]), "v"(ac[0][3]), "v"(ac[1][0]), "v"(ac[1][1]),
                      "v"(ac[1][2]), "v"(ac[1][3]));
            else
                asm volatile(
                    "v_max3_i32 %0, %3, %4, %5\n\t"
                    "v_max3_i32 %1, %6, %7, %8\n\t"
                    "v_max3_i32 %0, %0, %9, %10\n\t"
                    "v_max3_i32 %2, %0, %1, %2"  // the unit's earlier steps folded in
                    : "=&v"(t0), "=&v"(t1), "+v"(part[xtc])
                    : "v"(ac[0][0]), "v"(ac[0][1]), "v"(ac[0][2]), "v"(ac[0][3]), "v"(ac[1][0]), "v"(ac[1][1]),
                      "v"(ac[1][2]), "v"(ac[1][3]));
            __builtin_amdgcn_sched_barrier(0);
        };

        // ---- software-pipelined scan over all of Y -----------------------------------
        // (step, xt = 0..kXT-1) in order; acc[0] holds even xt, acc[1] odd xt.  Each phase
        // issues the MFMAs of the NEXT one, then runs the VALU of the current one.
        YFrag y0, y1;
#ifdef AMC_SCAN_STAMPS
        st_w0 = AMC_STAMP();
#endif
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // chunk 0 and this item's X rows landed
        __syncthreads();
#ifdef AMC_SCAN_STAMPS
        st_w1 = AMC_STAMP();
#endif
        if (first) {  // (everything this wave loaded has landed)
            rv = rvn;
            if (table) {
                rvn = rvn2;
                rvn2 = load_run(*s_q);  // in flight during the scan
            } else {
                rvn = load_run(*s_q);  // (no load: the ticket itself)
            }
        }
        // the next item: the run's next entry, or the next run's first
        int kn = next_entry(rv, kpos);
        const bool same_run = kn >= 0;
        if (!same_run) kn = next_entry(rvn, -1);
        const uint32_t en = kn < 0 ? kRunNone : (uint32_t)__builtin_amdgcn_readlane((int)(same_run ? rv : rvn), kn);
        const bool keep_x = MODE == 0 && same_run && (en & kRunSameX) != 0;
        const int dvn = load_desc(en);  // in flight during the scan
#ifdef AMC_SCAN_STAMPS
        {
            const uint32_t now = AMC_STAMP();
            if (st_prev) {  // the item before this one is complete: its crossings, its boundary, its period
                st_sum[0] += st_a;
                st_sum[1] += now - st_end;
                st_sum[2] += now - st_first;
                st_sum[3] += 1;
                st_sum[4] += st_prev_active ? 1 : 0;
                st_split[0] += st_w0 - st_end;
                st_split[1] += st_w1 - st_w0;
                if (st_keep_x) {  // this item kept the X rows of the one before
                    st_kept[0] += now - st_end;
                    st_kept[1] += 1;
                    st_split[2] += st_w0 - st_end;
                    st_split[3] += st_w1 - st_w0;
                }
                if (lane == 0) {
#pragma unroll
                    for (int k = 0; k < 5; ++k) st_slot[k] = st_sum[k];
                    st_slot[8] = st_kept[0];
                    st_slot[9] = st_kept[1];
#pragma unroll
                    for (int k = 0; k < 4; ++k) st_slot[10 + k] = st_split[k];
                }
            }
            st_a = 0;
            st_first = now;
        }
#endif
        // The sched_barriers pin the interleaving.  An accumulator is read (by inline asm, which
        // hipcc does not hazard-check) only after FOUR further MFMAs have issued behind the one
        // that completed it - the matrix pipe runs MFMAs in order, 16 clk each (4 passes), so two of them
        // have run to their end since: well over the 7 wait states a 4-pass MFMA's result needs before a VALU read
        // (two further MFMAs would do; the rule the 8-pass instruction needed, 11 states, held with two as well).
        //
        // The chunk loop is peeled by what is in flight.  STEADY chunks, c + 3 < nchunks: every step issues this wave's
        // piece of chunk c + 3 into the buffer chunk c - 1 left (never bunched), and the crossing to chunk c + 1 waits
        // with the one count that fits.  DRAIN, the last up to three chunks: nothing is fetched, the crossing's count
        // depends on how many chunks remain, and the last chunk has no crossing.  The ring position cb = c % kNB is a
        // scalar; where the DMA goes and by how much the read bases move are computed from it on the scalar unit.
        static_assert(kPW == kYS, "one DMA piece per wave and step");
        static_assert(kNB == 4, "the counted waits below are written out for three chunks ahead");
        // Chunk c + 1 must have landed.  Loads return in the order they were issued, and behind this wave's pieces of
        // chunk c + 1 it has issued its kPW pieces (wave 0: + 1 rs128 block) of every later chunk that exists, c + 2
        // and c + 3: so many may stay in flight and no more.  (At the first crossing chunks 1 and 2 have landed with
        // the item's X rows; fewer pieces are in flight than the count allows.)  rem: chunks behind chunk c, >= 1.
        auto crossing = [&](bool steady, int rem) __attribute__((always_inline)) {
#ifdef AMC_SCAN_STAMPS
            const uint32_t st_t = AMC_STAMP();
#endif
            if (steady) {
                if (wid == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * kPW + 2) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * kPW) : "memory");
            } else if (rem >= 2) {
                if (wid == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kPW + 1) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kPW) : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // nothing further to fetch
            }
            // a bare barrier: __syncthreads() is a fence and would drain the pieces just issued (vmcnt(0)).
            // Nothing is stored to LDS here by a wave itself; the DMA'd bytes are ordered by the waits above.
            asm volatile("s_barrier" ::: "memory");
#ifdef AMC_SCAN_STAMPS
            st_a += AMC_STAMP() - st_t;
#endif
        };
        // this wave's piece `ys` of chunk c + 3 (wave 0: with step 0 its rs128 block), into ring buffer (cb + 3) % kNB
        auto fetch = [&](int c, int cb, int ys) __attribute__((always_inline)) {
            const int fb = (cb + kNB - 1) & (kNB - 1);
            stage_piece(yprep, c + kNB - 1, fb, ys);
            if (ys == 0) stage_rs(yrs, c + kNB - 1, fb);
        };
        int c = 0, cb = 0;
        if (active) {
            load_y(y0, 0);
            mfma_first(acc[0][0], y0.f[0][0], xf[0][0], y0.ci[0]);
            mfma_first(acc[0][1], y0.f[1][0], xf[0][0], y0.ci[1]);
            mfma_acc(acc[0][0], y0.f[0][1], xf[0][1]);
            mfma_acc(acc[0][1], y0.f[1][1], xf[0][1]);
            // the first phase inserts a pending maximum: one below every accumulator, its key is below every floor key
            part[kXT - 1] = -(1 << 24);
            __builtin_amdgcn_sched_barrier(0);
            // one step = 32 rows' worth of Y held in `yc`; prefetches the next step into `yn`.  ys = the step of the
            // chunk, 0 .. kYS - 1, `steady` as above: both compile-time.  The chunk's last step crosses to the next
            // chunk, moves the read bases there and prefetches its first step; behind the image's last chunk that reads
            // a buffer nobody needs (result unused), to stay branch-free.
            auto step = [&](YFrag& yc, YFrag& yn, int ys, bool steady) __attribute__((always_inline)) {
                if (steady) fetch(c, cb, ys);
                if (ys == kYS - 1) {
                    const int rem = nchunks - 1 - c;
                    if (steady || rem >= 1) crossing(steady, rem);
                    advance(cb);
                }
                const int nys = ys == kYS - 1 ? 0 : ys + 1;
#pragma unroll
                for (int xt = 0; xt < kXT; ++xt) {  // sp = ys, gb = c: a chunk is one block
                    if (xt + 1 < kXT)
                        phase(acc[(xt + 1) & 1], yc, xt + 1, acc[xt & 1], xt, ys, c);
                    else
                        phase(acc[0], yn, 0, acc[xt & 1], xt, ys, c);
                    if (xt < 6) {
                        load_y_part(yn, nys, xt);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            };
#pragma unroll 1
            for (; c + kNB - 1 < nchunks; ++c, cb = (cb + 1) & (kNB - 1)) {
                step(y0, y1, 0, true);
                step(y1, y0, 1, true);
                step(y0, y1, 2, true);
                step(y1, y0, 3, true);
            }
#pragma unroll 1
            for (; c < nchunks; ++c, cb = (cb + 1) & (kNB - 1)) {
                step(y0, y1, 0, false);
                step(y1, y0, 1, false);
                step(y0, y1, 2, false);
                step(y1, y0, 3, false);
            }
            // the read bases back to ring buffer 0 for the next item (every chunk moved them on by one)
            yb0 -= cb * kChunkBytes;
            yb1 -= cb * kChunkBytes;
            cbs -= cb * kBN * 4;
            const int lastb = nchunks - 1;
            insert(kXT - 1, 126 - (lastb & 63));  // the last unit's maximum is still pending
            flush(lastb >> 6);
#pragma unroll
            for (int xt = 0; xt < kXT; ++xt) {  // keys -> values
                best[xt] >>= kKeyShift;
                sec[xt] >>= kKeyShift;
            }
        } else {
            // a wave without rows only feeds the ring: its pieces of every chunk, the same waits, the same barriers
#pragma unroll 1
            for (; c + kNB - 1 < nchunks; ++c, cb = (cb + 1) & (kNB - 1)) {
#pragma unroll
                for (int ys = 0; ys < kYS; ++ys) fetch(c, cb, ys);
                crossing(true, kNB - 1);
            }
#pragma unroll 1
            for (; c + 1 < nchunks; ++c) crossing(false, nchunks - 1 - c);
        }
        __syncthreads();  // everyone is done with the LDS chunk buffers (and has read the queue slot)
#ifdef AMC_SCAN_STAMPS
        st_end = AMC_STAMP();
        st_prev = true;
        st_prev_active = active;
#endif

        // ---- item done.  Start the next one's loads, then decode and store this one under them ----
        int eb[kXT], es[kXT], et[kXT], ex[kXT];
#pragma unroll
        for (int xt = 0; xt < kXT; ++xt) {
            // (asm: hipcc otherwise sinks these copies into the scan loop, 3 x kXT moves per step)
            asm volatile("v_mov_b32 %0, %1" : "=v"(eb[xt]) : "v"(best[xt]));
            asm volatile("v_mov_b32 %0, %1" : "=v"(es[xt]) : "v"(sec[xt]));
            asm volatile("v_mov_b32 %0, %1" : "=v"(et[xt]) : "v"(btile[xt]));
            ex[xt] = xterm[xt];
        }
        if (en != kRunNone) {
            stage_head(dvn);
            if (dword(dvn, kDCnt) > 0) {
                if (keep_x) reset_x();
                else load_x(dvn);
            }
        }
        if (active) {
            const int cnt = dword(dv, kDCnt);
            // Merge the four lane quarters (they saw different Y rows of every block; equal values keep the lower tile)
            // and decode, TWO X tiles' worth of instructions instead of eight: the merge is a reduce-scatter, not a
            // butterfly.  v_permlane32_swap exchanges the upper half of one register with the lower half of another:
            // applied to the states of the X tiles xt and xt + 4 it leaves, in the lower 32 lanes, both halves' states
            // of tile xt side by side and in the upper 32 lanes those of tile xt + 4 - one merge serves two tiles.
            // v_permlane16_swap does the same with 16-lane rows for the pairs that are left.  Behind both rounds two
            // register sets hold all 128 rows of the segment, one row per lane: set k, lane quarter q = X tile
            // 2 k + (q & 1) + 4 (q >> 1), and the decode, the acceptance test and the store run twice, in all lanes,
            // where they ran eight times in sixteen.  (The epilogue runs against the partner workgroup's scan on the
            // same SIMD: its cost is its instruction count.  profiles/headfetch/README.md.)
            // A lane's tile: the quarter's own of its block's four (-1 while nothing beat the floor)
            int mb[kXT], ms[kXT], mt[kXT];
#pragma unroll
            for (int xt = 0; xt < kXT; ++xt) {
                mb[xt] = eb[xt];
                ms[xt] = es[xt];
                mt[xt] = et[xt] < 0 ? -1 : et[xt] * kSPB + lq;
            }
            auto merge = [&](int a, int o) __attribute__((always_inline)) {  // state o into state a
                const int b = mb[a], t = mt[a], ob = mb[o], ot = mt[o];
                const bool ow = (ob > b) || (ob == b && (unsigned)ot < (unsigned)t);
                ms[a] = max(max(ms[a], ms[o]), ow ? b : ob);
                mt[a] = ow ? ot : t;
                mb[a] = ow ? ob : b;
            };
            auto swap32 = [&](int& x, int& y) __attribute__((always_inline)) {
                const auto r = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)y, false, false);
                x = (int)r[0];
                y = (int)r[1];
            };
            auto swap16 = [&](int& x, int& y) __attribute__((always_inline)) {
                const auto r = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)y, false, false);
                x = (int)r[0];
                y = (int)r[1];
            };
            static_assert(kXT == 8, "two rounds of pairing leave two register sets");
#pragma unroll
            for (int xt = 0; xt < 4; ++xt) {  // lanes 0..31: tile xt, quarters q and q + 2; lanes 32..63: tile xt + 4
                swap32(mb[xt], mb[xt + 4]);
                swap32(ms[xt], ms[xt + 4]);
                swap32(mt[xt], mt[xt + 4]);
                merge(xt, xt + 4);
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {  // rows of 16 lanes: tiles 2k, 2k + 1, 2k + 4, 2k + 5
                swap16(mb[2 * k], mb[2 * k + 1]);
                swap16(ms[2 * k], ms[2 * k + 1]);
                swap16(mt[2 * k], mt[2 * k + 1]);
                merge(2 * k, 2 * k + 1);
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int xtl = 2 * k + (lq & 1) + 4 * (lq >> 1);  // this lane's X tile
                const int kl = xtl * 16 + l15;
                const int exl = (lq & 2) ? ((lq & 1) ? ex[2 * k + 5] : ex[2 * k + 4]) : ((lq & 1) ? ex[2 * k + 1] : ex[2 * k]);
                const int b = mb[2 * k], s = ms[2 * k], t = mt[2 * k];
                bool acc_bit = false;
                const bool live = kl < cnt;
                Top2 o;
                o.best_v = (uint32_t)(b + exl);
                o.best_idx = o.best_v ? (uint32_t)t : 0xFFFFFFFFu;  // TILE of the best
                o.second_v = (uint32_t)(s + exl);
                o.pad = 0;
                // a larger second only ever rejects: rows failing now can be forgotten
                // (scan_accept.h: thresholds instead of acos; a superset of what the exact tests keep)
                if (MODE == 0) acc_bit = live && scan_may_accept(sa, o.best_v, o.second_v);
                // (16 bits per lane quarter: the rows of its X tile)
                const unsigned long long bits = MODE == 0 ? (unsigned long long)__ballot(acc_bit) : 0ull;
                // MODE 0 stores what is read: every reader of the row table tests the row's accept bit first
                // (resolve_index* side 0, select_candidates, finalize), so a row the scan rejects here is never looked
                // at.  The unit is the X tile - 16 rows, 256 contiguous bytes - stored whole if any of its rows is
                // accepted: on a sparse set (a few accepted rows per pair) next to nothing is written, 8 GB per
                // headline step less, and on a dense one (a third of the rows accepted) the stores stay the full lines
                // they were - 16-byte records scattered one in three cost the scan 0.8 % there.  MODE 1 stores every
                // candidate row: finalize reads cols[j] without a mask.
                const bool tile_any = MODE == 0 && ((uint32_t)(bits >> (16 * lq)) & 0xFFFFu) != 0;
                if (live && (MODE == 1 || tile_any)) {
                    Top2* out = reinterpret_cast<Top2*>(const_cast<char*>(dptr(dv, kDOut)));
                    int row = kl;  // MODE 0: `out` points at the segment's first row
                    if (MODE == 1) row = (int)reinterpret_cast<const uint32_t*>(dptr(dv, kDList))[kl];
                    out[row] = o;
                }
                if (MODE == 0) {  // accept bits of 32 rows = two X tiles: the lower quarters' and the upper quarters'
                    // a word without a bit stays as the batch's memset left it (enqueue_scan zeroes the mask)
                    const uint32_t w_lo = (uint32_t)bits, w_hi = (uint32_t)(bits >> 32);
                    if (lane == 0 && w_lo != 0) accmask[(uint32_t)dword(dv, kDAccword) + k] = w_lo;
                    if (lane == 0 && w_hi != 0) accmask[(uint32_t)dword(dv, kDAccword) + k + 2] = w_hi;
                }
            }
        }
#ifdef AMC_SCAN_STAMPS
        if (en == kRunNone && lane == 0) {  // the workgroup's last item
            st_slot[5] = st_a;
            st_slot[6] = AMC_STAMP() - st_first;
            st_slot[7] = 1;
        }
#endif
#ifdef AMC_SCAN_STAMPS
        st_keep_x = keep_x;
#endif
        e = en;
        kpos = kn;
        first = !same_run;
        dv = dvn;
    }
}

// ---------------------------------------------------------------------------------------------------
// Packing the segments of a launch into items (three tiny kernels, all on the match stream).
// `order` lists the launch's pairs sorted by the streamed image; `grp_start` (host-built, ngroups + 1
// entries) cuts it where that image changes.  A pair contributes ceil(rows / 128) segments - rows = image 1's
// rows (mode 0) or the pair's candidate count (mode 1, known only here) - none if the streamed image is empty.
// Items never mix streamed images: every group is padded to a multiple of 4 segments with null descriptors
// (cnt = 0, but a valid Y stream, so any wave can read it from its own descriptor).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pair_segments(int mode, const ImageDev* imgs, const PairDev& p, uint32_t pi,
                                                  const uint32_t* cand_cnt, uint32_t* nrows_out) {
    const uint32_t nx = mode == 0 ? imgs[p.slot1].rows : cand_cnt[pi];
    const uint32_t ny = imgs[mode == 0 ? p.slot2 : p.slot1].rows;
    *nrows_out = nx;
    return ny ? (nx + kSegRows - 1) / kSegRows : 0u;
}

// one 256-thread block per group: seg_base[i] = segments of the group before pair order[i]; group totals
__global__ __launch_bounds__(256) void seg_count_kernel(int mode, const ImageDev* __restrict__ imgs,
                                                        const PairDev* __restrict__ pairs,
                                                        const uint32_t* __restrict__ order,
                                                        const uint32_t* __restrict__ grp_start,
                                                        const uint32_t* __restrict__ cand_cnt,
                                                        uint32_t* __restrict__ seg_base, uint32_t* __restrict__ grp_segs) {
    __shared__ uint32_t wsum[4];
    const uint32_t g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint32_t i0 = grp_start[g], i1 = grp_start[g + 1];
    uint32_t running = 0;
    for (uint32_t base = i0; base < i1; base += 256) {
        const uint32_t i = base + tid;
        uint32_t s = 0, nr;
        if (i < i1) {
            const uint32_t pi = order[i];
            s = pair_segments(mode, imgs, pairs[pi], pi, cand_cnt, &nr);
        }
        uint32_t inc = s;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const uint32_t o = __shfl_up(inc, m);
            if (lane >= (uint32_t)m) inc += o;
        }
        if (lane == 63) wsum[wid] = inc;
        __syncthreads();
        uint32_t wbase = 0, total = 0;
        for (uint32_t k = 0; k < 4; ++k) {
            if (k < wid) wbase += wsum[k];
            total += wsum[k];
        }
        if (i < i1) seg_base[i] = running + wbase + inc - s;
        running += total;
        __syncthreads();
    }
    if (tid == 0) grp_segs[g] = running;
}

// one block: grp_item_base = exclusive scan of ceil(grp_segs / 4); the launch's item count
__global__ __launch_bounds__(1024) void seg_scan_kernel(const uint32_t* __restrict__ grp_segs, uint32_t ngroups,
                                                        uint32_t* __restrict__ grp_item_base,
                                                        uint32_t* __restrict__ nitems_out) {
    __shared__ uint32_t wsum[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    uint32_t running = 0;
    for (uint32_t base = 0; base < ngroups; base += 1024) {
        const uint32_t g = base + tid;
        const uint32_t s = g < ngroups ? (grp_segs[g] + kSegsPerItem - 1) / kSegsPerItem : 0u;
        uint32_t inc = s;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const uint32_t o = __shfl_up(inc, m);
            if (lane >= (uint32_t)m) inc += o;
        }
        if (lane == 63) wsum[wid] = inc;
        __syncthreads();
        uint32_t wbase = 0, total = 0;
        for (uint32_t k = 0; k < 16; ++k) {
            if (k < wid) wbase += wsum[k];
            total += wsum[k];
        }
        if (g < ngroups) grp_item_base[g] = running + wbase + inc - s;
        running += total;
        __syncthreads();
    }
    if (tid == 0) *nitems_out = running;
}

// kFillY 256-thread blocks per group: a wave per pair in turn writes the pair's descriptors (lane = segment);
// the group's first block pads its last item.  (One block per group left the 500 groups of an exhaustive launch
// to 500 blocks: 2 ms per launch on the dense set.)
constexpr uint32_t kFillY = 8;
__global__ __launch_bounds__(256) void seg_fill_kernel(int mode, const ImageDev* __restrict__ imgs,
                                                       const PairDev* __restrict__ pairs,
                                                       const uint32_t* __restrict__ order,
                                                       const uint32_t* __restrict__ grp_start,
                                                       const uint32_t* __restrict__ cand_cnt,
                                                       const uint32_t* __restrict__ candbuf,
                                                       const uint32_t* __restrict__ seg_base,
                                                       const uint32_t* __restrict__ grp_segs,
                                                       const uint32_t* __restrict__ grp_item_base,
                                                       Top2* __restrict__ outbuf, SegDesc* __restrict__ segs) {
    const uint32_t g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = blockIdx.y * 4 + (tid >> 6);
    const uint32_t i0 = grp_start[g], i1 = grp_start[g + 1];
    if (i0 >= i1) return;
    const uint32_t total = grp_segs[g];
    if (total == 0) return;
    SegDesc* gs = segs + (size_t)grp_item_base[g] * kSegsPerItem;
    // the group's streamed image (the same for all of its pairs)
    const PairDev p0 = pairs[order[i0]];
    const ImageDev Y = imgs[mode == 0 ? p0.slot2 : p0.slot1];
    for (uint32_t i = i0 + wid; i < i1; i += 4 * kFillY) {
        const uint32_t pi = order[i];
        const PairDev p = pairs[pi];
        uint32_t nx;
        const uint32_t ns = pair_segments(mode, imgs, p, pi, cand_cnt, &nx);
        const ImageDev X = imgs[mode == 0 ? p.slot1 : p.slot2];
        const uint32_t sb = seg_base[i];
        for (uint32_t k = lane; k < ns; k += 64) {
            const uint32_t row0 = k * kSegRows;
            SegDesc d;
            d.yprep = Y.prep;
            d.yrs = Y.rs128;
            d.yrows = Y.rows;
            d.cnt = min(nx - row0, (uint32_t)kSegRows);
            d.pad_ = 0;
            if (mode == 0) {
                d.xprep = X.prep + (size_t)row0 * kDim;
                d.xrs = X.rs128 + row0;
                d.out = outbuf + p.row_off + row0;
                d.list = nullptr;
                d.accword = (uint32_t)((p.row_off + row0) >> 5);
            } else {
                d.xprep = X.prep;
                d.xrs = X.rs128;
                d.out = outbuf + p.col_off;  // rows scattered by their index
                d.list = candbuf + p.col_off + row0;
                d.accword = 0;
            }
            gs[sb + k] = d;
        }
    }
    const uint32_t padded = (total + kSegsPerItem - 1) / kSegsPerItem * kSegsPerItem;
    if (blockIdx.y == 0 && tid < padded - total) {
        SegDesc d;
        d.xprep = Y.prep;  // any mapped rows: a null segment's results are never stored
        d.xrs = Y.rs128;
        d.out = nullptr;
        d.list = nullptr;
        d.yprep = Y.prep;
        d.yrs = Y.rs128;
        d.cnt = 0;
        d.accword = 0;
        d.yrows = Y.rows;
        d.pad_ = 0;
        gs[total + tid] = d;
    }
}

hipError_t launch_build_segments(int mode, const ImageDev* imgs, const PairDev* pairs, const uint32_t* order,
                                 const uint32_t* grp_start, uint32_t ngroups, const uint32_t* cand_cnt,
                                 const uint32_t* candbuf, Top2* outbuf, uint32_t* seg_base, uint32_t* grp_segs,
                                 uint32_t* grp_item_base, SegDesc* segs, uint32_t* nitems_dev, hipStream_t s) {
    if (ngroups == 0) return memset_async(nitems_dev, 0, sizeof(uint32_t), s);
    hipLaunchKernelGGL(seg_count_kernel, dim3(ngroups), dim3(256), 0, s, mode, imgs, pairs, order, grp_start,
                       cand_cnt, seg_base, grp_segs);
    hipLaunchKernelGGL(seg_scan_kernel, dim3(1), dim3(1024), 0, s, grp_segs, ngroups, grp_item_base, nitems_dev);
    hipLaunchKernelGGL(seg_fill_kernel, dim3(ngroups, kFillY), dim3(256), 0, s, mode, imgs, pairs, order, grp_start,
                       cand_cnt, candbuf, seg_base, grp_segs, grp_item_base, outbuf, segs);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Runs (forward scan only).  In an exhaustive job item t of streamed image j and item t of image j + 1 hold the same
// four X segments, for every X image below j - and a workgroup that scans them one after the other fetches those 64 KB
// once.  The groups of the forward order are taken in BLOCKS of R consecutive groups; run (block, t) lists item t of
// each group of the block that has one, in group order, "none" (kRunNone) elsewhere: run_items[nruns x R].  The order
// only makes shared rows frequent.  Whether an entry may keep the X rows of the entry before it is read off the
// descriptors themselves: kRunSameX is set where xprep, xrs and cnt agree in all four descriptors of the two items and
// neither has a candidate list - whatever the pair list looks like, a wrong order costs speed and never a result.
// The launch's LAST block (of kRunTailBlocks or more) is written as runs of one item each, in item order: a run is
// what a workgroup can be left alone with when the queue is empty, and the launch ends on items as it did before.
// ---------------------------------------------------------------------------------------------------
constexpr uint32_t kRunTailBlocks = 8;
__device__ __forceinline__ bool run_block_is_single(uint32_t b, uint32_t nblocks) {
    return nblocks >= kRunTailBlocks && b + 1 == nblocks;
}
// one block: run_base = exclusive scan, over the blocks, of the largest item count among a block's groups; the total
__global__ __launch_bounds__(1024) void run_scan_kernel(const uint32_t* __restrict__ grp_segs, uint32_t ngroups, uint32_t R,
                                                        uint32_t* __restrict__ run_base, uint32_t* __restrict__ nruns_out) {
    __shared__ uint32_t wsum[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint32_t nblocks = (ngroups + R - 1) / R;
    uint32_t running = 0;
    for (uint32_t base = 0; base < nblocks; base += 1024) {
        const uint32_t b = base + tid;
        uint32_t s = 0;
        if (b < nblocks)
            for (uint32_t g = b * R; g < min(b * R + R, ngroups); ++g) {
                const uint32_t n = (grp_segs[g] + kSegsPerItem - 1) / kSegsPerItem;
                s = run_block_is_single(b, nblocks) ? s + n : max(s, n);
            }
        uint32_t inc = s;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const uint32_t o = __shfl_up(inc, m);
            if (lane >= (uint32_t)m) inc += o;
        }
        if (lane == 63) wsum[wid] = inc;
        __syncthreads();
        uint32_t wbase = 0, total = 0;
        for (uint32_t k = 0; k < 16; ++k) {
            if (k < wid) wbase += wsum[k];
            total += wsum[k];
        }
        if (b < nblocks) run_base[b] = running + wbase + inc - s;
        running += total;
        __syncthreads();
    }
    if (tid == 0) *nruns_out = running;
}

// the X side of two items is the same rows, segment for segment (and read as rows, not through a candidate list)
__device__ __forceinline__ bool items_share_x(const SegDesc* __restrict__ a, const SegDesc* __restrict__ b) {
    bool same = true;
    for (int w = 0; w < kSegsPerItem; ++w)
        same = same && a[w].xprep == b[w].xprep && a[w].xrs == b[w].xrs && a[w].cnt == b[w].cnt && a[w].list == nullptr &&
               b[w].list == nullptr;
    return same;
}

// kFillY 256-thread blocks per block of R groups (behind seg_fill_kernel: it reads the descriptors)
constexpr uint32_t kRunMax = 8;
__global__ __launch_bounds__(256) void run_fill_kernel(const SegDesc* __restrict__ segs, const uint32_t* __restrict__ grp_segs,
                                                       const uint32_t* __restrict__ grp_item_base, uint32_t ngroups,
                                                       uint32_t R, const uint32_t* __restrict__ run_base,
                                                       uint32_t* __restrict__ run_items) {
    __shared__ uint32_t s_items[kRunMax], s_base[kRunMax];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (tid < R) {
        const uint32_t g = b * R + tid;
        s_items[tid] = g < ngroups ? (grp_segs[g] + kSegsPerItem - 1) / kSegsPerItem : 0u;
        s_base[tid] = g < ngroups ? grp_item_base[g] : 0u;
    }
    __syncthreads();
    uint32_t m = 0;
    for (uint32_t p = 0; p < R; ++p) m = max(m, s_items[p]);
    uint32_t* out = run_items + (size_t)run_base[b] * R;
    if (run_block_is_single(b, gridDim.x)) {  // a run per item, group after group
        uint32_t total = 0;
        for (uint32_t p = 0; p < R; ++p) total += s_items[p];
        for (uint32_t idx = blockIdx.y * 256 + tid; idx < total * R; idx += 256 * gridDim.y) {
            uint32_t t = idx / R, p = 0;
            const uint32_t pos = idx - t * R;
            while (t >= s_items[p]) t -= s_items[p++];  // (t < total: p stays below R)
            out[idx] = pos == 0 ? s_base[p] + t : kRunNone;
        }
        return;
    }
    for (uint32_t idx = blockIdx.y * 256 + tid; idx < m * R; idx += 256 * gridDim.y) {
        const uint32_t t = idx / R, p = idx - t * R;
        uint32_t entry = kRunNone;
        if (t < s_items[p]) {
            entry = s_base[p] + t;
            int pp = (int)p - 1;  // the run's previous entry that is an item
            while (pp >= 0 && t >= s_items[pp]) --pp;
            if (pp >= 0 && items_share_x(segs + (size_t)entry * kSegsPerItem, segs + (size_t)(s_base[pp] + t) * kSegsPerItem))
                entry |= kRunSameX;
        }
        out[idx] = entry;
    }
}

hipError_t launch_build_runs(const SegDesc* segs, const uint32_t* grp_segs, const uint32_t* grp_item_base, uint32_t ngroups,
                             uint32_t R, uint32_t* run_base, uint32_t* run_items, uint32_t* nruns_dev, hipStream_t s) {
    if (R < 2 || R > kRunMax) return hipErrorInvalidValue;
    if (ngroups == 0) return memset_async(nruns_dev, 0, sizeof(uint32_t), s);
    const uint32_t nblocks = (ngroups + R - 1) / R;
    hipLaunchKernelGGL(run_scan_kernel, dim3(1), dim3(1024), 0, s, grp_segs, ngroups, R, run_base, nruns_dev);
    hipLaunchKernelGGL(run_fill_kernel, dim3(nblocks, kFillY), dim3(256), 0, s, segs, grp_segs, grp_item_base, ngroups, R,
                       run_base, run_items);
    return hipGetLastError();
}

hipError_t launch_match_mfma(int mode, const SegDesc* segs, const uint32_t* nitems_dev, uint32_t max_items,
                             uint32_t* queue_head, uint32_t* accmask, const ScanAccept* accept_dev, hipStream_t s,
                             const CopyJob& job_in, uint32_t* copy_head, const uint32_t* run_items, uint32_t run_len,
                             const uint32_t* nruns_dev) {
    if (run_items && (mode != 0 || run_len < 2 || run_len > kRunMax || !nruns_dev)) return hipErrorInvalidValue;
    const uint32_t* const ntickets = run_items ? nruns_dev : nitems_dev;
    const int rl = run_items ? (int)run_len : 1;
    if (max_items == 0) return hipSuccess;  // (the caller checks: a job is only handed to a launch that happens)
    CopyJob job = (mode == 0 && copy_head) ? job_in : CopyJob();
    // The persistent workgroups pop from these two counters: nothing is launched unless both were reset.
    hipError_t e = job.parts ? memset_async(copy_head, 0, sizeof(uint32_t), s) : hipSuccess;
    if (e != hipSuccess) return e;
    int dev = 0, cus = 256;
    if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    // Two workgroups per CU, and the kernels must really fit that way (registers, LDS): asked of the runtime once.
    // One per CU would run on half the machine's register file without anyone noticing - it is an error instead.
    static const hipError_t occupancy = [] {
        int n0 = 0, n1 = 0;
        hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n0, match_mfma_kernel<0>, 64 * kW, 0);
        if (oe == hipSuccess) oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n1, match_mfma_kernel<1>, 64 * kW, 0);
        if (oe != hipSuccess) return oe;
        return n0 >= kWGPerCU && n1 >= kWGPerCU ? hipSuccess : hipErrorLaunchOutOfResources;
    }();
    if (occupancy != hipSuccess) return occupancy;
    int wgs = kWGPerCU * cus;
    // AMC_SCAN_GRID (A/B hook, read once) caps the number of WORKGROUPS (two of them fill a CU): fewer than 2 per CU -
    // the CUs left over stay free for whatever else is in flight (round 6's question: does a power-bound scan lose
    // less than its share of CUs?  DESIGN.md section 6)
    static const int grid_cap = [] {
        const char* e = std::getenv("AMC_SCAN_GRID");
        return e ? std::atoi(e) : 0;
    }();
    if (grid_cap > 0 && grid_cap < wgs) wgs = grid_cap;
    const uint32_t grid = max_items < (uint32_t)wgs ? max_items : (uint32_t)wgs;
    if (job.parts > grid) job.parts = grid;  // every part needs a workgroup
    if ((e = memset_async(queue_head, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
    if (mode == 0)
        hipLaunchKernelGGL((match_mfma_kernel<0>), dim3(grid), dim3(64 * kW), 0, s, segs, ntickets, queue_head,
                           accmask, accept_dev, job, copy_head, run_items, rl);
    else
        hipLaunchKernelGGL((match_mfma_kernel<1>), dim3(grid), dim3(64 * kW), 0, s, segs, ntickets, queue_head,
                           accmask, accept_dev, job, copy_head, run_items, rl);
    return hipGetLastError();
}

}  // namespace amc
