// patchmatch.hip — PatchMatch stereo on gfx950 (include/amc_patchmatch.h), the restatement of DESIGN.md section 22.  The
// arithmetic is patchmatch_core.h's, shared with tests/patchmatch_ref: the two are bit-identical.
//
// Work split (22.8).  A sweep is one launch over every problem of the batch.  A wave (a workgroup of 64 lanes) takes
// one line of one problem and walks it pixel by pixel, carrying the predecessor in registers.  At a pixel
//   - the 64 lanes fill the reference window's values and bilateral weights in LDS, a sample each per round;
//   - lane l takes the (hypothesis, source) pairs l, l + 64, ...: each sums its window sequentially in row-major order,
//     which is the reference's loop, and leaves its cost (and forward-backward error) in LDS;
//   - lane s takes source s's forward message, selection probability and sampling weight;
//   - every lane then runs the draws and the arg-min over the LDS arrays: wave-uniform, in the reference's order.
// No atomics; a wave writes the state of its own line only.  The initialisation, the final costs and the filter take a
// lane per pixel (and source).
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "amc_internal.h"
#include "patchmatch_core.h"
#include "../../include/amc_patchmatch.h"

using namespace amc;

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr long long kDefaultBatchBytes = 1ll << 30;  // state bytes of the problems of one launch
constexpr uint32_t kMaxBatchProblems = 32768;        // gridDim.y
constexpr uint64_t kNoMap = AMC_PATCHMATCH_NO_MAP;

struct ImgD {
    uint64_t off;      // into the pixel bytes
    uint64_t map_off;  // into the input maps, or kNoMap
    int32_t w, h;
    pm::Cam k;
};
struct ProbD {
    uint32_t ref, nsrc;
    uint64_t src0;  // its first SrcD
    uint64_t pix0;  // its first pixel in the state arrays
    uint64_t sel0;  // its first value in the per-source arrays ([source][h][w])
    float dmin, dmax;
};
struct SrcD {
    pm::Rel rel;
    uint32_t img;
};
struct Dev {
    pm::Params p;
    const uint8_t* pixels;
    const ImgD* img;
    const ProbD* prob;
    const SrcD* src;
    const float *in_depth, *in_normal;
    float *depth, *normal, *sel, *cost, *fb;
    uint8_t* cnt;
    uint32_t prob0, prob1;  // the launch's problems
    uint32_t sweep;
};

__device__ __forceinline__ pm::View view_of(const Dev& d, const ImgD& im) {
    pm::View v;
    v.px = d.pixels + im.off;
    v.w = im.w;
    v.h = im.h;
    v.k = im.k;
    return v;
}

// 22.4: the state before the first sweep
__global__ __launch_bounds__(kBlock) void pm_init_kernel(Dev d) {
    const uint32_t pi = d.prob0 + blockIdx.y;
    if (pi >= d.prob1) return;
    const ProbD pb = d.prob[pi];
    const ImgD im = d.img[pb.ref];
    const uint64_t hw = (uint64_t)im.w * (uint64_t)im.h;
    const uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= hw) return;
    const int row = (int)(idx / (uint64_t)im.w), col = (int)(idx % (uint64_t)im.w);
    float ray[3], depth, n[3];
    pm::pixel_ray(im.k, row, col, ray);
    bool given = false;
    if (d.p.geom && d.in_depth && im.map_off != kNoMap) {
        depth = d.in_depth[im.map_off + idx];
        const float* nm = d.in_normal + 3 * im.map_off;
        n[0] = nm[idx];
        n[1] = nm[hw + idx];
        n[2] = nm[2 * hw + idx];
        given = depth >= pb.dmin && depth <= pb.dmax && pm::face_camera(ray, n);
    }
    if (!given) pm::random_hyp(pm::rng_at(d.p.seed, pb.ref, (uint32_t)row, (uint32_t)col, pm::kSweepInit), 0, ray, pb.dmin, pb.dmax, depth, n);
    d.depth[pb.pix0 + idx] = depth;
    float* nm = d.normal + 3 * pb.pix0;
    nm[idx] = n[0];
    nm[hw + idx] = n[1];
    nm[2 * hw + idx] = n[2];
    for (uint32_t s = 0; s < pb.nsrc; ++s) d.sel[pb.sel0 + (uint64_t)s * hw + idx] = 0.5f;
}

// the window of the current pixel in LDS; offs holds the samples' nominal offsets, which do not depend on the pixel
struct LdsWindow {
    const float *val, *wgt;
    const uint32_t* offs;
    int row, col, w, h;
    __device__ __forceinline__ void get(int i, float& x, float& y, float& v, float& wt) const {
        const uint32_t o = offs[i];
        const int rr = pm::clampi(row + (int)(o >> 16) - 128, 0, h - 1), cc = pm::clampi(col + (int)(o & 0xffffu) - 128, 0, w - 1);
        x = (float)cc + 0.5f;
        y = (float)rr + 0.5f;
        v = val[i];
        wt = wgt[i];
    }
};

// 22.4 - 22.5: one sweep; blockIdx.x = the line, blockIdx.y = the problem
__global__ __launch_bounds__(kWave) void pm_sweep_kernel(Dev d) {
    extern __shared__ float lds[];
    const uint32_t pi = d.prob0 + blockIdx.y;
    if (pi >= d.prob1) return;
    const ProbD pb = d.prob[pi];
    const ImgD im = d.img[pb.ref];
    const int dir = (int)(d.sweep & 3u), iter = (int)(d.sweep >> 2);
    const bool vertical = dir == 0 || dir == 2;  // down, up: a line is a column
    const int lines = vertical ? im.w : im.h, len = vertical ? im.h : im.w;
    if ((int)blockIdx.x >= lines) return;
    const int line = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int S = (int)pb.nsrc, count = d.p.side * d.p.side;
    const uint64_t hw = (uint64_t)im.w * (uint64_t)im.h;
    float* l_val = lds;
    float* l_wgt = l_val + count;
    uint32_t* l_off = reinterpret_cast<uint32_t*>(l_wgt + count);
    float* l_cost = reinterpret_cast<float*>(l_off + count);
    float* l_geo = l_cost + pm::kNumHyps * pm::kMaxSources;
    float* l_wsrc = l_geo + pm::kNumHyps * pm::kMaxSources;
    float* l_fwd = l_wsrc + pm::kMaxSources;
    for (int i = lane; i < count; i += kWave) {
        const int dr = (i / d.p.side - d.p.half) * d.p.step, dc = (i % d.p.side - d.p.half) * d.p.step;
        l_off[i] = ((uint32_t)(dr + 128) << 16) | (uint32_t)(dc + 128);
    }
    if (lane < pm::kMaxSources) l_fwd[lane] = 0.5f;
    __syncthreads();
    const pm::View ref = view_of(d, im);
    float* dep = d.depth + pb.pix0;
    float* nm = d.normal + 3 * pb.pix0;
    int prow = 0, pcol = 0;
    float pdepth = 0.0f, pn[3] = {0.0f, 0.0f, -1.0f};
    for (int k = 0; k < len; ++k) {
        const int pos = (dir == 0 || dir == 1) ? k : len - 1 - k;
        const int row = vertical ? pos : line, col = vertical ? line : pos;
        const uint64_t idx = (uint64_t)row * (uint64_t)im.w + (uint64_t)col;
        const float depth = dep[idx];
        const float n[3] = {nm[idx], nm[hw + idx], nm[2 * hw + idx]};
        const pm::Rng g = pm::rng_at(d.p.seed, pb.ref, (uint32_t)row, (uint32_t)col, d.sweep);
        pm::Hyps H;
        pm::make_hyps(im.k, g, iter, pb.dmin, pb.dmax, row, col, depth, n, k > 0, prow, pcol, pdepth, pn, H);
        for (int i = lane; i < count; i += kWave) {
            float x, y, v, w;
            pm::window_sample(d.p, ref, row, col, i, x, y, v, w);
            l_val[i] = v;
            l_wgt[i] = w;
        }
        __syncthreads();
        const LdsWindow win{l_val, l_wgt, l_off, row, col, im.w, im.h};
        for (int q = lane; q < pm::kNumHyps * S; q += kWave) {
            const int h = q / S, s = q % S;
            const SrcD& sd = d.src[pb.src0 + (uint64_t)s];
            const ImgD sim = d.img[sd.img];
            const pm::View sv = view_of(d, sim);
            float hn[3], hd = 0.0f;  // (a select over h keeps H in registers)
#pragma unroll
            for (int j = 0; j < pm::kNumHyps; ++j)
                if (j == h) {
                    hd = H.depth[j];
                    hn[0] = H.n[j][0];
                    hn[1] = H.n[j][1];
                    hn[2] = H.n[j][2];
                }
            l_cost[q] = pm::ncc_cost(d.p, im.k, sv, sd.rel, row, col, hd, hn, win);
            if (d.p.geom) {
                float e = d.p.geom_max;
                if (d.in_depth && sim.map_off != kNoMap)
                    e = pm::fb_error(im.k, sim.k, sim.w, sim.h, d.in_depth + sim.map_off, sd.rel, row, col, hd, d.p.geom_max);
                l_geo[q] = e;
            }
        }
        __syncthreads();
        if (lane < S) {
            float ray[3];
            pm::pixel_ray(im.k, row, col, ray);
            const float X[3] = {depth * ray[0], depth * ray[1], depth};
            float* selp = d.sel + pb.sel0 + (uint64_t)lane * hw + idx;
            float fwd = l_fwd[lane], sel = *selp;
            l_wsrc[lane] = pm::source_weight(d.p, l_cost[lane], X, n, d.src[pb.src0 + (uint64_t)lane].rel.C, fwd, sel);
            l_fwd[lane] = fwd;
            *selp = sel;
        }
        __syncthreads();
        const int best = pm::pick_hypothesis(d.p, S, l_wsrc, l_cost, l_geo, g, pm::kDrawSamples);
        prow = row;
        pcol = col;
#pragma unroll
        for (int j = 0; j < pm::kNumHyps; ++j)
            if (j == best) {
                pdepth = H.depth[j];
                pn[0] = H.n[j][0];
                pn[1] = H.n[j][1];
                pn[2] = H.n[j][2];
            }
        if (lane == 0) {
            dep[idx] = pdepth;
            nm[idx] = pn[0];
            nm[hw + idx] = pn[1];
            nm[2 * hw + idx] = pn[2];
        }
        __syncthreads();
    }
}

// 22.7: the state's cost (and forward-backward error) in every source; blockIdx.z = the source
__global__ __launch_bounds__(kBlock) void pm_cost_kernel(Dev d) {
    const uint32_t pi = d.prob0 + blockIdx.y;
    if (pi >= d.prob1) return;
    const ProbD pb = d.prob[pi];
    if (blockIdx.z >= pb.nsrc) return;
    const ImgD im = d.img[pb.ref];
    const uint64_t hw = (uint64_t)im.w * (uint64_t)im.h;
    const uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= hw) return;
    const int row = (int)(idx / (uint64_t)im.w), col = (int)(idx % (uint64_t)im.w);
    const SrcD& sd = d.src[pb.src0 + blockIdx.z];
    const ImgD sim = d.img[sd.img];
    const pm::View ref = view_of(d, im), sv = view_of(d, sim);
    const float depth = d.depth[pb.pix0 + idx];
    const float* nm = d.normal + 3 * pb.pix0;
    const float n[3] = {nm[idx], nm[hw + idx], nm[2 * hw + idx]};
    const pm::DirectWindow win{&d.p, &ref, row, col};
    const uint64_t at = pb.sel0 + (uint64_t)blockIdx.z * hw + idx;
    d.cost[at] = pm::ncc_cost(d.p, im.k, sv, sd.rel, row, col, depth, n, win);
    if (d.p.geom) {
        float e = 3.0e38f;
        if (d.in_depth && sim.map_off != kNoMap) e = pm::fb_error(im.k, sim.k, sim.w, sim.h, d.in_depth + sim.map_off, sd.rel, row, col, depth, 3.0e38f);
        d.fb[at] = e;
    }
}

// 22.7: the filter, a lane per pixel, the sources in order
__global__ __launch_bounds__(kBlock) void pm_filter_kernel(Dev d) {
    const uint32_t pi = d.prob0 + blockIdx.y;
    if (pi >= d.prob1) return;
    const ProbD pb = d.prob[pi];
    const ImgD im = d.img[pb.ref];
    const uint64_t hw = (uint64_t)im.w * (uint64_t)im.h;
    const uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= hw) return;
    const int row = (int)(idx / (uint64_t)im.w), col = (int)(idx % (uint64_t)im.w);
    float ray[3];
    pm::pixel_ray(im.k, row, col, ray);
    const float depth = d.depth[pb.pix0 + idx];
    const float X[3] = {depth * ray[0], depth * ray[1], depth};
    int count = 0;
    for (uint32_t s = 0; s < pb.nsrc; ++s) {
        const uint64_t at = pb.sel0 + (uint64_t)s * hw + idx;
        bool ok = d.sel[at] >= pm::kFilterMinSelProb && 1.0f - d.cost[at] >= d.p.filter_min_ncc &&
                  pm::cos_tri_angle(X, d.src[pb.src0 + s].rel.C) <= d.p.cos_filter_tri;
        if (d.p.geom) ok = ok && d.fb[at] <= d.p.filter_geom_max;
        count += ok ? 1 : 0;
    }
    d.cnt[pb.pix0 + idx] = (uint8_t)(count > 255 ? 255 : count);
    if (count < d.p.filter_min_num) {
        float* nm = d.normal + 3 * pb.pix0;
        d.depth[pb.pix0 + idx] = 0.0f;
        nm[idx] = 0.0f;
        nm[hw + idx] = 0.0f;
        nm[2 * hw + idx] = 0.0f;
    }
}

// What is wrong with the call, or the empty string.  Nothing is read through an offset or an index before it has been
// checked.
std::string check_call(const amc_patch_match_opts& o, const amc_patch_match_problem& pb) {
    const size_t ni = pb.num_images, np = pb.num_problems;
    if (o.window_radius < 1 || o.window_radius > AMC_PATCHMATCH_MAX_WINDOW_RADIUS) return "window_radius is not in 1 .. 32";
    if (o.window_step < 1 || o.window_step > o.window_radius) return "window_step is not in 1 .. window_radius";
    if (o.num_samples < 1 || o.num_samples > 4096) return "num_samples is not in 1 .. 4096";
    if (o.num_iterations < 0 || o.num_iterations > (1 << 20)) return "num_iterations is negative or over 2^20";
    if (!(o.sigma_color > 0.0) || !(o.ncc_sigma > 0.0) || !(o.incident_angle_sigma > 0.0)) return "a sigma is not positive";
    if (!(o.min_triangulation_angle >= 0.0 && o.min_triangulation_angle < 180.0) ||
        !(o.filter_min_triangulation_angle >= 0.0 && o.filter_min_triangulation_angle < 180.0))
        return "a triangulation angle is not in [0, 180)";
    if (!(o.geom_consistency_regularizer >= 0.0) || !(o.geom_consistency_max_cost >= 0.0) || !(o.filter_geom_consistency_max_cost >= 0.0))
        return "a geometric-consistency option is negative";
    if (!(o.filter_min_ncc >= -1.0 && o.filter_min_ncc <= 1.0)) return "filter_min_ncc is not in [-1, 1]";
    if (o.filter_min_num_consistent < 0) return "filter_min_num_consistent is negative";
    if (ni > 0x7fffffffu || np > 0x7fffffffu) return "too many images or problems for 32-bit indices";
    if (ni && (!pb.pixels || !pb.pixel_offsets || !pb.widths || !pb.heights || !pb.K || !pb.R || !pb.t)) return "NULL image array";
    if (np && (!pb.ref_images || !pb.src_offsets || !pb.src_images || !pb.depth_ranges)) return "NULL problem array";
    const int maps = (pb.in_depth != nullptr) + (pb.in_normal != nullptr) + (pb.in_map_offsets != nullptr);
    if (maps != 0 && maps != 3) return "in_depth, in_normal and in_map_offsets are not given together";
    for (size_t i = 0; i < ni; ++i) {
        if (pb.widths[i] < 1 || pb.heights[i] < 1) return "image " + std::to_string(i) + " has no pixels";
        if ((uint64_t)pb.widths[i] * (uint64_t)pb.heights[i] > AMC_PATCHMATCH_MAX_PIXELS)
            return "image " + std::to_string(i) + " has more than 2^31 pixels (AMC_PATCHMATCH_MAX_PIXELS)";
    }
    if (!np) return std::string();
    if (pb.src_offsets[0] != 0) return "src_offsets does not start at 0";
    for (size_t p = 0; p < np; ++p) {
        if (pb.src_offsets[p + 1] < pb.src_offsets[p]) return "src_offsets decreases at problem " + std::to_string(p);
        const uint64_t s = pb.src_offsets[p + 1] - pb.src_offsets[p];
        if (s < 1 || s > AMC_PATCHMATCH_MAX_SOURCES)
            return "problem " + std::to_string(p) + " has " + std::to_string(s) + " sources, not 1 .. " + std::to_string(AMC_PATCHMATCH_MAX_SOURCES) +
                   " (AMC_PATCHMATCH_MAX_SOURCES)";
        if (pb.ref_images[p] >= ni) return "problem " + std::to_string(p) + " names a reference image out of range";
        const double lo = pb.depth_ranges[2 * p], hi = pb.depth_ranges[2 * p + 1];
        if (!(lo > 0.0) || !(hi >= lo) || !(hi < 1e30) || !((float)lo > 0.0f))
            return "problem " + std::to_string(p) + " has a depth range that is not 0 < min <= max";
    }
    for (uint64_t k = 0; k < pb.src_offsets[np]; ++k)
        if (pb.src_images[k] >= ni) return "source " + std::to_string(k) + " names an image out of range";
    return std::string();
}

void free_arrays(amc_patch_match_result* r) {
    std::free(r->map_offsets);
    std::free(r->cost_offsets);
    std::free(r->depth);
    std::free(r->normal);
    std::free(r->num_consistent);
    std::free(r->costs);
    r->map_offsets = r->cost_offsets = nullptr;
    r->depth = r->normal = r->costs = nullptr;
    r->num_consistent = nullptr;
}

pm::Options core_options(const amc_patch_match_opts& o) {
    pm::Options c;
    c.window_radius = o.window_radius;
    c.window_step = o.window_step;
    c.num_samples = o.num_samples;
    c.geom = o.geom_consistency;
    c.filter = o.filter;
    c.filter_min_num = o.filter_min_num_consistent;
    c.sigma_spatial = o.sigma_spatial;
    c.sigma_color = o.sigma_color;
    c.ncc_sigma = o.ncc_sigma;
    c.min_tri_deg = o.min_triangulation_angle;
    c.incident_sigma = o.incident_angle_sigma;
    c.geom_reg = o.geom_consistency_regularizer;
    c.geom_max = o.geom_consistency_max_cost;
    c.filter_min_ncc = o.filter_min_ncc;
    c.filter_min_tri_deg = o.filter_min_triangulation_angle;
    c.filter_geom_max = o.filter_geom_consistency_max_cost;
    c.seed = o.seed;
    return c;
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

int run_device(amc_ctx* ctx, const amc_patch_match_problem& pb, const amc_patch_match_opts& op, uint64_t batch_bytes,
               amc_patch_match_result* result) {
    static const char* const hipchk_who = "amc_patch_match";
    const size_t ni = pb.num_images, np = pb.num_problems;
    const uint64_t nsrc = pb.src_offsets[np], npix = result->num_pixels, nsel = result->num_costs;
    // the host's tables
    std::vector<ImgD> img(ni);
    uint64_t nbytes = 0, nmap = 0;
    for (size_t i = 0; i < ni; ++i) {
        const uint64_t hw = (uint64_t)pb.widths[i] * (uint64_t)pb.heights[i];
        img[i].off = pb.pixel_offsets[i];
        img[i].map_off = pb.in_map_offsets ? pb.in_map_offsets[i] : kNoMap;
        img[i].w = pb.widths[i];
        img[i].h = pb.heights[i];
        img[i].k = pm::Cam{(float)pb.K[4 * i], (float)pb.K[4 * i + 1], (float)pb.K[4 * i + 2], (float)pb.K[4 * i + 3]};
        nbytes = std::max(nbytes, img[i].off + hw);
        if (img[i].map_off != kNoMap) nmap = std::max(nmap, img[i].map_off + hw);
    }
    std::vector<ProbD> prob(np);
    std::vector<SrcD> src(nsrc);
    std::vector<uint64_t> state_bytes(np + 1, 0);  // a CSR for split_batches
    for (size_t p = 0; p < np; ++p) {
        const uint32_t r = pb.ref_images[p];
        ProbD& q = prob[p];
        q.ref = r;
        q.nsrc = (uint32_t)(pb.src_offsets[p + 1] - pb.src_offsets[p]);
        q.src0 = pb.src_offsets[p];
        q.pix0 = result->map_offsets[p];
        q.sel0 = result->cost_offsets[p];
        q.dmin = (float)pb.depth_ranges[2 * p];
        q.dmax = (float)pb.depth_ranges[2 * p + 1];
        if (q.dmax < q.dmin) q.dmax = q.dmin;
        for (uint64_t k = pb.src_offsets[p]; k < pb.src_offsets[p + 1]; ++k) {
            const uint32_t s = pb.src_images[k];
            src[k].rel = pm::make_rel(pb.R + 9 * (size_t)r, pb.t + 3 * (size_t)r, pb.R + 9 * (size_t)s, pb.t + 3 * (size_t)s);
            src[k].img = s;
        }
        state_bytes[p + 1] = state_bytes[p] + (result->map_offsets[p + 1] - result->map_offsets[p]) * (16 + 4 * (uint64_t)q.nsrc);
    }
    const Batches batches = split_batches(state_bytes.data(), np, kMaxBatchProblems, batch_bytes);

    const CtxView cv = ctx_view(ctx);
    HIPCHK(hipSetDevice(cv.device));
    hipStream_t st = cv.stream;
    Dev d{};
    d.p = pm::make_params(core_options(op));
    uint8_t* d_pixels;
    ImgD* d_img;
    ProbD* d_prob;
    SrcD* d_src;
    float *d_in_depth, *d_in_normal;
    const bool final_costs = op.filter || op.want_costs;
    DevBuf<void> mem;  // the call's working set: allocated here, freed on return
    DevParts parts;
    parts.part(&d_pixels, nbytes).part(&d_img, ni).part(&d_prob, np).part(&d_src, nsrc).part(&d_in_depth, nmap).part(&d_in_normal, 3 * nmap)
        .part(&d.depth, npix).part(&d.normal, 3 * npix).part(&d.sel, nsel).part(&d.cost, final_costs ? nsel : 0)
        .part(&d.fb, final_costs && op.geom_consistency ? nsel : 0).part(&d.cnt, npix);
    {
        const auto t0 = std::chrono::steady_clock::now();
        const hipError_t e = parts.carve(mem);
        if (e == hipErrorOutOfMemory) return api_fail(AMC_E_NOMEM, "%s: out of device memory", hipchk_who);
        HIPCHK(e);
        result->alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    // an early return must not leave copies in flight that read the tables or write the result's arrays
    struct Drain {
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{st};
    StreamTimer timer(st), copies(st);
    HIPCHK(timer.start());
    auto up = [&](void* dst, const void* s, size_t bytes) { return bytes ? hipMemcpyAsync(dst, s, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
    auto down = [&](void* dst, const void* s, size_t bytes) { return bytes ? hipMemcpyAsync(dst, s, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
    HIPCHK(copies.span_begin());
    HIPCHK(up(d_pixels, pb.pixels, nbytes));
    HIPCHK(up(d_img, img.data(), ni * sizeof(ImgD)));
    HIPCHK(up(d_prob, prob.data(), np * sizeof(ProbD)));
    HIPCHK(up(d_src, src.data(), nsrc * sizeof(SrcD)));
    HIPCHK(up(d_in_depth, pb.in_depth, nmap * 4));
    HIPCHK(up(d_in_normal, pb.in_normal, nmap * 12));
    HIPCHK(hipMemsetAsync(d.cnt, 0, std::max<uint64_t>(npix, 1), st));
    HIPCHK(copies.span_end());
    d.pixels = d_pixels;
    d.img = d_img;
    d.prob = d_prob;
    d.src = d_src;
    d.in_depth = nmap ? d_in_depth : nullptr;
    d.in_normal = nmap ? d_in_normal : nullptr;
    const int count = d.p.side * d.p.side;
    const size_t lds_bytes = ((size_t)3 * count + 2 * pm::kNumHyps * pm::kMaxSources + 2 * pm::kMaxSources) * 4;
    HIPCHK(timer.span_begin());
    for (size_t b = 0; b < batches.count(); ++b) {
        d.prob0 = (uint32_t)batches.start[b];
        d.prob1 = (uint32_t)batches.start[b + 1];
        uint64_t most_pix = 0;
        int most_w = 0, most_h = 0;
        uint32_t most_src = 0;
        for (uint32_t p = d.prob0; p < d.prob1; ++p) {
            const ImgD& im = img[prob[p].ref];
            most_pix = std::max(most_pix, (uint64_t)im.w * (uint64_t)im.h);
            most_w = std::max(most_w, im.w);
            most_h = std::max(most_h, im.h);
            most_src = std::max(most_src, prob[p].nsrc);
        }
        const unsigned nb = d.prob1 - d.prob0;
        hipLaunchKernelGGL(pm_init_kernel, dim3(blocks_for(most_pix), nb), dim3(kBlock), 0, st, d);
        HIPCHK(hipGetLastError());
        result->num_launches += 1;
        for (int sweep = 0; sweep < 4 * op.num_iterations; ++sweep) {
            d.sweep = (uint32_t)sweep;
            const int lines = (sweep & 1) ? most_h : most_w;  // down / up: a line per column
            hipLaunchKernelGGL(pm_sweep_kernel, dim3((unsigned)lines, nb), dim3(kWave), lds_bytes, st, d);
            HIPCHK(hipGetLastError());
            result->num_launches += 1;
        }
        if (final_costs) {
            hipLaunchKernelGGL(pm_cost_kernel, dim3(blocks_for(most_pix), nb, most_src), dim3(kBlock), 0, st, d);
            HIPCHK(hipGetLastError());
            result->num_launches += 1;
        }
        if (op.filter) {
            hipLaunchKernelGGL(pm_filter_kernel, dim3(blocks_for(most_pix), nb), dim3(kBlock), 0, st, d);
            HIPCHK(hipGetLastError());
            result->num_launches += 1;
        }
        result->num_batches += 1;
    }
    HIPCHK(timer.span_end());
    HIPCHK(copies.span_begin());
    HIPCHK(down(result->depth, d.depth, npix * 4));
    HIPCHK(down(result->normal, d.normal, npix * 12));
    HIPCHK(down(result->num_consistent, d.cnt, npix));
    if (op.want_costs) HIPCHK(down(result->costs, d.cost, nsel * 4));
    HIPCHK(copies.span_end());
    HIPCHK(timer.stop(result->device_ms));
    HIPCHK(timer.spans(result->kernel_ms));
    HIPCHK(copies.spans(result->copy_ms));
    return AMC_OK;
}

int run(amc_ctx* ctx, const amc_patch_match_opts* opts, const amc_patch_match_problem* pb, amc_patch_match_result* result) {
    const char* fn = "amc_patch_match";
    const auto host_t0 = std::chrono::steady_clock::now();
    if (result) std::memset(result, 0, sizeof *result);
    if (!ctx || !pb || !result) return api_fail(AMC_E_INVALID, "%s: NULL argument", fn);
    amc_patch_match_opts op;
    amc_patch_match_opts_default(&op);
    if (opts) op = *opts;
    // (the test hook is read before anything can fail, once per call)
    const uint64_t batch_bytes = (uint64_t)env_int("AMC_PATCHMATCH_BATCH_BYTES", kDefaultBatchBytes, 1, 1ll << 40);
    const std::string bad = check_call(op, *pb);
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: %s", fn, bad.c_str());
    const size_t np = pb->num_problems;
    result->num_problems = np;
    result->map_offsets = (uint64_t*)std::calloc(np + 1, 8);
    result->cost_offsets = (uint64_t*)std::calloc(np + 1, 8);
    if (!result->map_offsets || !result->cost_offsets) {
        free_arrays(result);
        return api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    for (size_t p = 0; p < np; ++p) {
        const uint32_t r = pb->ref_images[p];
        const uint64_t hw = (uint64_t)pb->widths[r] * (uint64_t)pb->heights[r];
        result->map_offsets[p + 1] = result->map_offsets[p] + hw;
        result->cost_offsets[p + 1] = result->cost_offsets[p] + hw * (pb->src_offsets[p + 1] - pb->src_offsets[p]);
    }
    const uint64_t npix = result->num_pixels = result->map_offsets[np];
    const uint64_t ncost = result->num_costs = result->cost_offsets[np];
    result->depth = (float*)std::calloc(std::max<uint64_t>(npix, 1), 4);
    result->normal = (float*)std::calloc(std::max<uint64_t>(npix, 1) * 3, 4);
    result->num_consistent = (uint8_t*)std::calloc(std::max<uint64_t>(npix, 1), 1);
    if (op.want_costs) result->costs = (float*)std::calloc(std::max<uint64_t>(ncost, 1), 4);
    if (!result->depth || !result->normal || !result->num_consistent || (op.want_costs && !result->costs)) {
        free_arrays(result);
        return api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    int rc = AMC_OK;
    try {
        if (np) rc = run_device(ctx, *pb, op, batch_bytes, result);
    } catch (const std::bad_alloc&) {
        rc = api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    if (rc != AMC_OK) {
        free_arrays(result);
        return rc;
    }
    result->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count() - result->device_ms;
    return AMC_OK;
}

}  // namespace

extern "C" {

void amc_patch_match_opts_default(amc_patch_match_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->window_radius = 5;
    o->window_step = 1;
    o->num_samples = 15;
    o->num_iterations = 5;
    o->filter_min_num_consistent = 2;
    o->sigma_spatial = -1.0;
    o->sigma_color = 0.2;
    o->ncc_sigma = 0.6;
    o->min_triangulation_angle = 1.0;
    o->incident_angle_sigma = 0.9;
    o->geom_consistency_regularizer = 0.3;
    o->geom_consistency_max_cost = 3.0;
    o->filter_min_ncc = 0.1;
    o->filter_min_triangulation_angle = 3.0;
    o->filter_geom_consistency_max_cost = 1.0;
}

int amc_patch_match(amc_ctx* ctx, const amc_patch_match_opts* opts, const amc_patch_match_problem* problem, amc_patch_match_result* result) {
    return run(ctx, opts, problem, result);
}

void amc_patch_match_result_free(amc_patch_match_result* r) {
    if (!r) return;
    free_arrays(r);
}

}  // extern "C"
