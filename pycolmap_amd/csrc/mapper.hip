// mapper.hip — the two image-level statistics of COLMAP 3.9.1's IncrementalMapper on gfx950 (include/amc_mapper.h),
// as DESIGN.md section 20 restates them.
//
// amc_image_visibility (20.1, 20.5): a wave per candidate image, the lanes over its points2D in rounds of 64.  A lane
// walks its point2D's correspondences, looks each up in the table of the graph images' point3D ids and, when one carries
// a point, stores a 1 into the wave's byte map of the finest pyramid level in LDS (64 x 64 cells; lanes that hit one
// cell store the same value, so no atomics).  The five coarser levels are ORs of 2 x 2 children, built level by level
// in LDS; every level's occupied cells are counted and weighted by the level's cell count.  Integers only.
//
// amc_shared_point_angles (20.3, 20.5): a lane per image computes the projection centre (16.2); then a wave per pair,
// the lanes over its shared points: each computes 11.4's angle and keeps it as a 64-bit key whose unsigned order is
// 20.3's total order of doubles (NaN last); the element of the pair's rank is then found bit by bit from the top, 64
// counting passes over the keys.  A lane reads back only the keys it wrote itself.  No atomics, no LDS.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "amc_internal.h"
#include "filter_core.h"
#include "../../include/amc_mapper.h"

using namespace amc;

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kFine = 64;  // the finest level's cells per side: 2^AMC_MAPPER_PYRAMID_LEVELS
// a wave's byte maps, finest first: 64^2 + 32^2 + 16^2 + 8^2 + 4^2 + 2^2 bytes
constexpr int kMapBytes = 4096 + 1024 + 256 + 64 + 16 + 4;
constexpr int kMapWords = kMapBytes / 4;
constexpr long long kDefaultBatchImages = 1 << 16, kDefaultBatchPairs = 1 << 16;
constexpr uint64_t kNaNKey = ~0ull;

unsigned blocks_for(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// ---- amc_image_visibility ------------------------------------------------------------------------------------------------

struct VisDev {
    const uint64_t* ipoff;  // graph images + 1
    const uint64_t* table;  // per graph point2D: its point3D id or AMC_MAPPER_NO_POINT3D
    const uint32_t *cw, *ch;
    const uint64_t* cpoff;  // candidates + 1
    const double* xy;
    const uint64_t* coff;   // candidate points2D + 1
    const uint32_t *cimg, *cp2;
    uint32_t *nobs, *nvis;
    uint64_t* score;
    uint32_t first, last;   // the launch's candidates
};

// 20.1's cell of a coordinate along an axis of the given extent: trunc(64 x / extent) clipped to 0 .. 63; a quotient
// that is negative or NaN goes to cell 0 (COLMAP's conversion of it is undefined)
__device__ __forceinline__ uint32_t vis_cell(double x, double extent) {
    const double v = (double)kFine * x / extent;
    if (!(v >= 1.0)) return 0;
    if (v >= (double)kFine) return kFine - 1;
    return (uint32_t)v;
}

// dst (side x side bytes) = OR of src's 2 x 2 children (2 side x 2 side bytes); returns this lane's occupied cells
__device__ __forceinline__ uint32_t vis_coarsen(const uint8_t* src, uint8_t* dst, uint32_t side, uint32_t lane) {
    uint32_t n = 0;
    for (uint32_t i = lane; i < side * side; i += kWave) {
        const uint32_t r = i / side, c = i % side;
        const uint8_t* s = src + (2 * r) * (2 * side) + 2 * c;
        const uint8_t v = (s[0] | s[1] | s[2 * side] | s[2 * side + 1]) ? 1 : 0;
        dst[i] = v;
        n += v;
    }
    return n;
}

// every wave of the block takes every barrier: a wave without a candidate only skips the work between them
__global__ __launch_bounds__(kBlock) void visibility_kernel(VisDev d) {
    __shared__ uint32_t lds[kWavesPerBlock][kMapWords];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint64_t c = (uint64_t)d.first + (uint64_t)blockIdx.x * kWavesPerBlock + wave;
    const bool live = c < d.last;
    uint32_t* w32 = lds[wave];
    uint8_t* l5 = reinterpret_cast<uint8_t*>(w32);
    uint8_t* l4 = l5 + 4096;
    uint8_t* l3 = l4 + 1024;
    uint8_t* l2 = l3 + 256;
    uint8_t* l1 = l2 + 64;
    uint8_t* l0 = l1 + 16;
    for (uint32_t i = lane; i < kFine * kFine / 4; i += kWave) w32[i] = 0;
    __syncthreads();
    uint32_t nobs = 0, nvis = 0;
    if (live) {
        const uint64_t p0 = d.cpoff[c], p1 = d.cpoff[c + 1];
        const double W = (double)d.cw[c], H = (double)d.ch[c];
        for (uint64_t j = p0 + lane; j < p1; j += kWave) {
            const uint64_t k0 = d.coff[j], k1 = d.coff[j + 1];
            bool vis = false;
            for (uint64_t k = k0; k < k1 && !vis; ++k) vis = d.table[d.ipoff[d.cimg[k]] + d.cp2[k]] != AMC_MAPPER_NO_POINT3D;
            nobs += k1 > k0 ? 1u : 0u;
            if (vis) {
                nvis += 1;
                l5[vis_cell(d.xy[2 * j + 1], H) * kFine + vis_cell(d.xy[2 * j], W)] = 1;
            }
        }
    }
    __syncthreads();
    // a level's occupied cells times its cell count, finest first; the bytes are 0 or 1, so popcount counts them
    uint32_t cells = 0;
    for (uint32_t i = lane; i < kFine * kFine / 4; i += kWave) cells += __popc(w32[i]);
    uint32_t score = cells * 4096u;
    score += vis_coarsen(l5, l4, 32, lane) * 1024u;
    __syncthreads();
    score += vis_coarsen(l4, l3, 16, lane) * 256u;
    __syncthreads();
    score += vis_coarsen(l3, l2, 8, lane) * 64u;
    __syncthreads();
    score += vis_coarsen(l2, l1, 4, lane) * 16u;
    __syncthreads();
    score += vis_coarsen(l1, l0, 2, lane) * 4u;
    for (int m = kWave / 2; m >= 1; m >>= 1) {  // integer sums: their order is free
        nobs += __shfl_xor(nobs, m);
        nvis += __shfl_xor(nvis, m);
        score += __shfl_xor(score, m);
    }
    if (live && lane == 0) {
        d.nobs[c] = nobs;
        d.nvis[c] = nvis;
        d.score[c] = score;  // at most AMC_MAPPER_MAX_SCORE < 2^32
    }
}

std::string check_visibility(const amc_visibility_problem& pb) {
    const size_t ng = pb.num_graph_images, nc = pb.num_candidates;
    if (!pb.image_point_offsets || !pb.cand_point_offsets || !pb.corr_offsets) return "NULL offsets";
    if (nc && (!pb.cand_width || !pb.cand_height)) return "NULL candidate sizes";
    if (pb.image_point_offsets[0] != 0 || pb.cand_point_offsets[0] != 0 || pb.corr_offsets[0] != 0) return "offsets that do not start at 0";
    for (size_t g = 0; g < ng; ++g)
        if (pb.image_point_offsets[g + 1] < pb.image_point_offsets[g]) return "image_point_offsets decreases at image " + std::to_string(g);
    if (pb.image_point_offsets[ng] && !pb.point2D_point3D) return "NULL point2D_point3D";
    for (size_t c = 0; c < nc; ++c) {
        if (pb.cand_point_offsets[c + 1] < pb.cand_point_offsets[c]) return "cand_point_offsets decreases at candidate " + std::to_string(c);
        if (pb.cand_point_offsets[c + 1] - pb.cand_point_offsets[c] > UINT32_MAX) return "candidate " + std::to_string(c) + " has 2^32 or more points2D";
    }
    const uint64_t np = pb.cand_point_offsets[nc];
    if (np && !pb.cand_xy) return "NULL cand_xy";
    for (uint64_t j = 0; j < np; ++j)
        if (pb.corr_offsets[j + 1] < pb.corr_offsets[j]) return "corr_offsets decreases at point2D " + std::to_string(j);
    const uint64_t nk = pb.corr_offsets[np];
    if (nk && (!pb.corr_image || !pb.corr_point2D)) return "NULL correspondences";
    for (uint64_t k = 0; k < nk; ++k) {
        const uint32_t g = pb.corr_image[k];
        if (g >= ng) return "correspondence " + std::to_string(k) + " names graph image " + std::to_string(g) + " of " + std::to_string(ng);
        if (pb.corr_point2D[k] >= pb.image_point_offsets[g + 1] - pb.image_point_offsets[g])
            return "correspondence " + std::to_string(k) + " names point2D " + std::to_string(pb.corr_point2D[k]) + " of graph image " + std::to_string(g) +
                   ", which has " + std::to_string(pb.image_point_offsets[g + 1] - pb.image_point_offsets[g]);
    }
    return "";
}

void free_visibility(amc_visibility_result* r) {
    std::free(r->num_observations);
    std::free(r->num_visible_points3D);
    std::free(r->score);
    r->num_observations = nullptr;
    r->num_visible_points3D = nullptr;
    r->score = nullptr;
}

int visibility_device(amc_ctx* ctx, const amc_visibility_problem& pb, uint64_t batch, amc_visibility_result* result) {
    static const char* const hipchk_who = "amc_image_visibility";
    const size_t ng = pb.num_graph_images, nc = pb.num_candidates;
    const uint64_t nt = pb.image_point_offsets[ng], np = pb.cand_point_offsets[nc], nk = pb.corr_offsets[np];
    const CtxView cv = ctx_view(ctx);
    HIPCHK(hipSetDevice(cv.device));
    hipStream_t st = cv.stream;
    uint64_t *d_ipoff, *d_table, *d_cpoff, *d_coff;
    uint32_t *d_cw, *d_ch, *d_cimg, *d_cp2;
    double* d_xy;
    VisDev d{};
    DevBuf<void> mem;  // the call's working set: allocated here, freed on return
    DevParts parts;
    parts.part(&d_ipoff, ng + 1).part(&d_table, nt).part(&d_cw, nc).part(&d_ch, nc).part(&d_cpoff, nc + 1).part(&d_xy, 2 * np)
        .part(&d_coff, np + 1).part(&d_cimg, nk).part(&d_cp2, nk).part(&d.nobs, nc).part(&d.nvis, nc).part(&d.score, nc);
    {
        const auto t0 = std::chrono::steady_clock::now();
        const hipError_t e = parts.carve(mem);
        if (e == hipErrorOutOfMemory) return api_fail(AMC_E_NOMEM, "%s: out of device memory", hipchk_who);
        HIPCHK(e);
        result->alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    // an early return must not leave copies in flight that read the caller's arrays or write the result's
    struct Drain {
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{st};
    StreamTimer timer(st), copies(st);
    HIPCHK(timer.start());
    auto up = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    auto down = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
    HIPCHK(copies.span_begin());
    HIPCHK(up(d_ipoff, pb.image_point_offsets, (ng + 1) * 8));
    HIPCHK(up(d_table, pb.point2D_point3D, nt * 8));
    HIPCHK(up(d_cw, pb.cand_width, nc * 4));
    HIPCHK(up(d_ch, pb.cand_height, nc * 4));
    HIPCHK(up(d_cpoff, pb.cand_point_offsets, (nc + 1) * 8));
    HIPCHK(up(d_xy, pb.cand_xy, np * 16));
    HIPCHK(up(d_coff, pb.corr_offsets, (np + 1) * 8));
    HIPCHK(up(d_cimg, pb.corr_image, nk * 4));
    HIPCHK(up(d_cp2, pb.corr_point2D, nk * 4));
    HIPCHK(copies.span_end());
    d.ipoff = d_ipoff;
    d.table = d_table;
    d.cw = d_cw;
    d.ch = d_ch;
    d.cpoff = d_cpoff;
    d.xy = d_xy;
    d.coff = d_coff;
    d.cimg = d_cimg;
    d.cp2 = d_cp2;
    HIPCHK(timer.span_begin());
    for (uint64_t first = 0; first < nc; first += batch) {
        d.first = (uint32_t)first;
        d.last = (uint32_t)std::min<uint64_t>(nc, first + batch);
        hipLaunchKernelGGL(visibility_kernel, dim3((d.last - d.first + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, st, d);
        HIPCHK(hipGetLastError());
        result->num_batches += 1;
    }
    HIPCHK(timer.span_end());
    HIPCHK(copies.span_begin());
    HIPCHK(down(result->num_observations, d.nobs, nc * 4));
    HIPCHK(down(result->num_visible_points3D, d.nvis, nc * 4));
    HIPCHK(down(result->score, d.score, nc * 8));
    HIPCHK(copies.span_end());
    HIPCHK(timer.stop(result->device_ms));
    HIPCHK(timer.spans(result->kernel_ms));
    HIPCHK(copies.spans(result->copy_ms));
    return AMC_OK;
}

int run_visibility(amc_ctx* ctx, const amc_visibility_problem* pb, amc_visibility_result* result) {
    const char* fn = "amc_image_visibility";
    const auto host_t0 = std::chrono::steady_clock::now();
    if (result) std::memset(result, 0, sizeof *result);
    if (!ctx || !pb || !result) return api_fail(AMC_E_INVALID, "%s: NULL argument", fn);
    // (the test hook is read before anything can fail, once per call)
    const uint64_t batch = (uint64_t)env_int("AMC_MAPPER_BATCH_IMAGES", kDefaultBatchImages, 1, kDefaultBatchImages);
    const std::string bad = check_visibility(*pb);
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: %s", fn, bad.c_str());
    const size_t nc = pb->num_candidates;
    if (nc > UINT32_MAX) return api_fail(AMC_E_INVALID, "%s: 2^32 or more candidates", fn);
    result->num_candidates = nc;
    result->max_score = AMC_MAPPER_MAX_SCORE;
    result->num_observations = (uint32_t*)std::calloc(std::max<size_t>(nc, 1), 4);
    result->num_visible_points3D = (uint32_t*)std::calloc(std::max<size_t>(nc, 1), 4);
    result->score = (uint64_t*)std::calloc(std::max<size_t>(nc, 1), 8);
    if (!result->num_observations || !result->num_visible_points3D || !result->score) {
        free_visibility(result);
        return api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    const int rc = nc ? visibility_device(ctx, *pb, batch, result) : AMC_OK;
    if (rc != AMC_OK) {
        free_visibility(result);
        return rc;
    }
    result->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count() - result->device_ms;
    return AMC_OK;
}

// ---- amc_shared_point_angles ---------------------------------------------------------------------------------------------

struct AngDev {
    uint32_t nimg;
    const double *q, *t;
    double* centre;        // 3 per image
    const double* xyz;
    const uint32_t* pimg;  // 2 per pair
    const uint64_t* poff;  // pairs + 1
    const uint32_t* pts;
    const uint32_t* rank;  // per pair
    uint64_t* keys;        // per shared point
    double* out;           // per pair
    uint32_t first, last;  // the launch's pairs
};

__global__ __launch_bounds__(kBlock) void centre_kernel(AngDev d) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= d.nimg) return;
    double C[3];
    filt::projection_centre(d.q + 4 * (size_t)i, d.t + 3 * (size_t)i, C);
    for (int k = 0; k < 3; ++k) d.centre[3 * (size_t)i + k] = C[k];
}

// 20.3's total order as the unsigned order of a key: -inf < ... < -0 < +0 < ... < +inf < NaN, every NaN one key
__device__ __forceinline__ uint64_t angle_key(double a) {
    if (a != a) return kNaNKey;
    const uint64_t u = (uint64_t)__double_as_longlong(a);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __forceinline__ double key_angle(uint64_t k) {
    if (k == kNaNKey) return __longlong_as_double(0x7ff8000000000000ll);
    return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

// a wave per pair of the launch
__global__ __launch_bounds__(kBlock) void pair_angle_kernel(AngDev d) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t p = (uint64_t)d.first + ((uint64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;
    if (p >= d.last) return;  // (the whole wave)
    const uint64_t k0 = d.poff[p], k1 = d.poff[p + 1];
    double c1[3], c2[3];
    for (int i = 0; i < 3; ++i) {
        c1[i] = d.centre[3 * (size_t)d.pimg[2 * p] + i];
        c2[i] = d.centre[3 * (size_t)d.pimg[2 * p + 1] + i];
    }
    // the keys: this lane's first in a register, the others in memory, where only this lane reads them again
    uint64_t key0 = 0;
    const bool has0 = k0 + lane < k1;
    for (uint64_t k = k0 + lane; k < k1; k += kWave) {
        const uint64_t key = angle_key(tri::tri_angle(c1, c2, d.xyz + 3 * (size_t)d.pts[k]));
        if (k == k0 + lane) key0 = key;
        else d.keys[k] = key;
    }
    // the key of the given rank, bit by bit from the top: among the keys that agree with the prefix above bit b, those
    // with bit b clear come first
    uint32_t r = d.rank[p];
    uint64_t prefix = 0;
    for (int b = 63; b >= 0; --b) {
        const uint64_t above = b == 63 ? 0ull : ~0ull << (b + 1);
        uint32_t n = (has0 && (key0 & above) == prefix && !((key0 >> b) & 1)) ? 1u : 0u;
        for (uint64_t k = k0 + lane + kWave; k < k1; k += kWave) {
            const uint64_t key = d.keys[k];
            n += ((key & above) == prefix && !((key >> b) & 1)) ? 1u : 0u;
        }
        for (int m = kWave / 2; m >= 1; m >>= 1) n += __shfl_xor(n, m);  // an integer sum: its order is free
        if (r >= n) {
            r -= n;
            prefix |= 1ull << b;
        }
    }
    if (lane == 0) d.out[p] = key_angle(prefix);
}

std::string check_angles(const amc_pair_angle_problem& pb, const amc_pair_angle_opts& op) {
    if (!(op.percentile >= 0.0 && op.percentile <= 100.0)) return "a percentile outside 0 .. 100";
    const size_t ni = pb.num_images, npt = pb.num_points, np = pb.num_pairs;
    if (!pb.pair_offsets) return "NULL pair_offsets";
    if (ni && (!pb.qvec || !pb.tvec)) return "NULL poses";
    if (npt && !pb.point_xyz) return "NULL point_xyz";
    if (ni > UINT32_MAX || npt > UINT32_MAX || np > UINT32_MAX) return "2^32 or more images, points or pairs";
    if (np && !pb.pair_images) return "NULL pair_images";
    if (pb.pair_offsets[0] != 0) return "pair_offsets does not start at 0";
    for (size_t p = 0; p < np; ++p) {
        if (pb.pair_offsets[p + 1] <= pb.pair_offsets[p]) return "pair " + std::to_string(p) + " has no shared points (or pair_offsets decreases)";
        if (pb.pair_offsets[p + 1] - pb.pair_offsets[p] > AMC_MAPPER_MAX_PAIR_POINTS)
            return "pair " + std::to_string(p) + " has " + std::to_string(pb.pair_offsets[p + 1] - pb.pair_offsets[p]) +
                   " shared points, more than " + std::to_string(AMC_MAPPER_MAX_PAIR_POINTS) + " (AMC_MAPPER_MAX_PAIR_POINTS)";
        if (pb.pair_images[2 * p] >= ni || pb.pair_images[2 * p + 1] >= ni) return "pair " + std::to_string(p) + " names an image out of range";
    }
    const uint64_t ns = pb.pair_offsets[np];
    if (ns && !pb.shared_points) return "NULL shared_points";
    for (uint64_t k = 0; k < ns; ++k)
        if (pb.shared_points[k] >= npt) return "shared point " + std::to_string(k) + " names point " + std::to_string(pb.shared_points[k]) + " of " + std::to_string(npt);
    return "";
}

int angles_device(amc_ctx* ctx, const amc_pair_angle_problem& pb, const std::vector<uint32_t>& rank, uint64_t batch,
                  amc_pair_angle_result* result) {
    static const char* const hipchk_who = "amc_shared_point_angles";
    const size_t ni = pb.num_images, npt = pb.num_points, np = pb.num_pairs;
    const uint64_t ns = pb.pair_offsets[np];
    const CtxView cv = ctx_view(ctx);
    HIPCHK(hipSetDevice(cv.device));
    hipStream_t st = cv.stream;
    double *d_q, *d_t, *d_xyz;
    uint32_t *d_pimg, *d_pts, *d_rank;
    uint64_t* d_poff;
    AngDev d{};
    DevBuf<void> mem;
    DevParts parts;
    parts.part(&d_q, 4 * ni).part(&d_t, 3 * ni).part(&d.centre, 3 * ni).part(&d_xyz, 3 * npt).part(&d_pimg, 2 * np).part(&d_poff, np + 1)
        .part(&d_pts, ns).part(&d_rank, np).part(&d.keys, ns).part(&d.out, np);
    {
        const auto t0 = std::chrono::steady_clock::now();
        const hipError_t e = parts.carve(mem);
        if (e == hipErrorOutOfMemory) return api_fail(AMC_E_NOMEM, "%s: out of device memory", hipchk_who);
        HIPCHK(e);
        result->alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    struct Drain {
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{st};
    StreamTimer timer(st), copies(st);
    HIPCHK(timer.start());
    auto up = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    HIPCHK(copies.span_begin());
    HIPCHK(up(d_q, pb.qvec, ni * 32));
    HIPCHK(up(d_t, pb.tvec, ni * 24));
    HIPCHK(up(d_xyz, pb.point_xyz, npt * 24));
    HIPCHK(up(d_pimg, pb.pair_images, np * 8));
    HIPCHK(up(d_poff, pb.pair_offsets, (np + 1) * 8));
    HIPCHK(up(d_pts, pb.shared_points, ns * 4));
    HIPCHK(up(d_rank, rank.data(), np * 4));
    HIPCHK(copies.span_end());
    d.nimg = (uint32_t)ni;
    d.q = d_q;
    d.t = d_t;
    d.xyz = d_xyz;
    d.pimg = d_pimg;
    d.poff = d_poff;
    d.pts = d_pts;
    d.rank = d_rank;
    HIPCHK(timer.span_begin());
    hipLaunchKernelGGL(centre_kernel, dim3(blocks_for(ni)), dim3(kBlock), 0, st, d);
    HIPCHK(hipGetLastError());
    for (uint64_t first = 0; first < np; first += batch) {
        d.first = (uint32_t)first;
        d.last = (uint32_t)std::min<uint64_t>(np, first + batch);
        hipLaunchKernelGGL(pair_angle_kernel, dim3(blocks_for((size_t)(d.last - d.first) * kWave)), dim3(kBlock), 0, st, d);
        HIPCHK(hipGetLastError());
        result->num_batches += 1;
    }
    HIPCHK(timer.span_end());
    HIPCHK(copies.span_begin());
    HIPCHK(hipMemcpyAsync(result->angle, d.out, np * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(copies.span_end());
    HIPCHK(timer.stop(result->device_ms));
    HIPCHK(timer.spans(result->kernel_ms));
    HIPCHK(copies.spans(result->copy_ms));
    return AMC_OK;
}

int run_angles(amc_ctx* ctx, const amc_pair_angle_problem* pb, const amc_pair_angle_opts* options, amc_pair_angle_result* result) {
    const char* fn = "amc_shared_point_angles";
    const auto host_t0 = std::chrono::steady_clock::now();
    if (result) std::memset(result, 0, sizeof *result);
    if (!ctx || !pb || !result) return api_fail(AMC_E_INVALID, "%s: NULL argument", fn);
    amc_pair_angle_opts op;
    amc_pair_angle_opts_default(&op);
    if (options) op = *options;
    const uint64_t batch = (uint64_t)env_int("AMC_MAPPER_BATCH_PAIRS", kDefaultBatchPairs, 1, kDefaultBatchPairs);
    const std::string bad = check_angles(*pb, op);
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: %s", fn, bad.c_str());
    const size_t np = pb->num_pairs;
    result->num_pairs = np;
    result->angle = (double*)std::calloc(std::max<size_t>(np, 1), 8);
    if (!result->angle) return api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    int rc = AMC_OK;
    try {
        // Percentile's index, as COLMAP computes it: round(p / 100 * (n - 1)), half away from zero, clamped to 0 .. n - 1
        std::vector<uint32_t> rank(std::max<size_t>(np, 1), 0);
        for (size_t p = 0; p < np; ++p) {
            const uint64_t n = pb->pair_offsets[p + 1] - pb->pair_offsets[p];
            const double idx = std::round(op.percentile / 100 * (double)(n - 1));
            rank[p] = (uint32_t)std::max(0.0, std::min((double)(n - 1), idx));
        }
        rc = np ? angles_device(ctx, *pb, rank, batch, result) : AMC_OK;
    } catch (const std::bad_alloc&) {
        rc = api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    if (rc != AMC_OK) {
        std::free(result->angle);
        result->angle = nullptr;
        return rc;
    }
    result->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count() - result->device_ms;
    return AMC_OK;
}

}  // namespace

extern "C" {

int amc_image_visibility(amc_ctx* ctx, const amc_visibility_problem* problem, amc_visibility_result* result) {
    return run_visibility(ctx, problem, result);
}

void amc_visibility_result_free(amc_visibility_result* r) {
    if (!r) return;
    free_visibility(r);
}

void amc_pair_angle_opts_default(amc_pair_angle_opts* o) {
    if (!o) return;
    o->percentile = 75.0;  // FindLocalBundle's Percentile(tri_angles, 75)
}

int amc_shared_point_angles(amc_ctx* ctx, const amc_pair_angle_problem* problem, const amc_pair_angle_opts* options,
                            amc_pair_angle_result* result) {
    return run_angles(ctx, problem, options, result);
}

void amc_pair_angle_result_free(amc_pair_angle_result* r) {
    if (!r) return;
    std::free(r->angle);
    r->angle = nullptr;
}

}  // extern "C"
