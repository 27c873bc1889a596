// fusion.hip — stereo fusion on gfx950 (include/amc_fusion.h), the restatement of DESIGN.md section 23.  The arithmetic
// is fusion_core.h's, shared with tests/fusion_ref: the two are bit-identical.
//
// Work split (23.6).  The maps, the images and the claim cells stay on the device for the whole call.  Step i is
//   - one launch that flags image i's seeds (a lane per pixel); the host turns the flags into the seed list;
//   - per batch of seeds one cluster launch: a wave (a workgroup of 64 lanes) per seed.  The lanes take the children of
//     a node, one neighbour each: project, gather depth and normal, run the three tests, ballot.  The walk itself is
//     wave-uniform: a stack of (member, mask of the children still to visit) in LDS, the highest neighbour first.  The
//     members live in LDS; the medians and the visibility set are found by rank counting across the lanes;
//   - the host reads one word per seed, numbers the points, and one gather launch packs them for the download.
// No atomics: a claim cell holds step + 1, every writer of a step stores the same value, and a value of the running
// step does not count as a claim (fu::claimed).
#include <cfloat>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "amc_internal.h"
#include "fusion_core.h"
#include "../../include/amc_fusion.h"

using namespace amc;

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kMaxC = AMC_FUSION_MAX_CLUSTER;
constexpr int kMaxTD = AMC_FUSION_MAX_TRAVERSAL_DEPTH;
constexpr long long kDefaultBatchSeeds = 1ll << 16;
constexpr uint64_t kNoMap = AMC_FUSION_NO_MAP;
// the word per seed that the host reads
constexpr uint32_t kInfoValid = 1u << 30, kInfoTruncated = 1u << 31;
constexpr int kInfoVisShift = 10;

struct ImgF {
    fu::Cam cam;
    uint64_t rgb_off;  // into the rgb bytes
    uint64_t map_off;  // into the depth maps and the claim cells (times 3: the normal maps), or kNoMap
    uint64_t nb0;      // its first neighbour
    int32_t w, h;
    uint32_t nnb, pad;
};
struct Dev {
    fu::Params p;
    const ImgF* img;
    const uint8_t* rgb;
    const float *depth, *normal;
    const uint32_t* nb;
    uint32_t* claims;
    uint32_t step, num_seeds;  // the launch's image and seeds
    const uint32_t* seeds;     // their pixels
    uint32_t vis_stride;       // min(kMaxC, images)
    // per seed of the launch
    float* rec;                // x y z nx ny nz
    uint32_t *color, *info, *vis;
    uint8_t* flags;            // per pixel of image `step`: a seed
};
struct Gather {
    uint32_t num_points, vis_stride;
    const uint32_t* slot;      // the point's seed in the launch
    const uint32_t* vis_off;   // num_points + 1, within the launch
    const float* rec;
    const uint32_t *color, *vis;
    float *xyz, *normal;
    uint32_t *out_color, *out_vis;
};

// 23.4: image `step`'s pixels with a depth that no earlier step claimed
__global__ __launch_bounds__(kBlock) void fusion_seed_kernel(Dev d) {
    const ImgF& im = d.img[d.step];
    const uint64_t hw = (uint64_t)im.w * (uint64_t)im.h;
    const uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= hw) return;
    const float z = d.depth[im.map_off + idx];
    d.flags[idx] = (z > 0.0f && !fu::claimed(d.claims[im.map_off + idx], d.step)) ? 1 : 0;
}

__device__ __forceinline__ int wave_sum(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// 23.2 - 23.3: one seed's cluster and its point; blockIdx.x = the seed
__global__ __launch_bounds__(kWave) void fusion_cluster_kernel(Dev d) {
    __shared__ float mX[3][kMaxC], mN[3][kMaxC];
    __shared__ uint32_t mC[3][kMaxC], mImg[kMaxC], mPix[kMaxC], mFirst[kMaxC];
    __shared__ unsigned long long fMask[kMaxTD];
    __shared__ uint32_t fMember[kMaxTD], fDepth[kMaxTD];
    __shared__ float selF[2][6];
    __shared__ uint32_t selC[2][3];
    const uint32_t slot = blockIdx.x;
    if (slot >= d.num_seeds) return;
    const int lane = (int)threadIdx.x;
    const uint32_t step = d.step;
    const ImgF& si = d.img[step];
    const uint32_t spix = d.seeds[slot];
    const float su = (float)(spix % (uint32_t)si.w) + 0.5f, sv = (float)(spix / (uint32_t)si.w) + 0.5f;
    float Xs[3], Ns[3];
    {
        const uint64_t hw = (uint64_t)si.w * (uint64_t)si.h;
        const float* nm = d.normal + 3 * si.map_off;
        fu::lift(si.cam, su, sv, d.depth[si.map_off + spix], Xs);
        fu::world_normal(si.cam, nm[spix], nm[hw + spix], nm[2 * hw + spix], Ns);
        if (lane < 3) {
            mX[lane][0] = Xs[lane];
            mN[lane][0] = Ns[lane];
            mC[lane][0] = d.rgb[si.rgb_off + 3 * (uint64_t)spix + lane];
        }
        if (lane == 0) {
            mImg[0] = step;
            mPix[0] = spix;
        }
    }
    __syncthreads();

    int count = 1, sp = 0;  // members, stack frames
    // the children of a member in image a with point X that pass the tests that do not depend on the walk: bit k = a's
    // neighbour k
    auto children = [&](uint32_t a, const float X[3]) -> unsigned long long {
        const ImgF& ia = d.img[a];
        bool ok = false;
        if ((uint32_t)lane < ia.nnb) {
            const uint32_t b = d.nb[ia.nb0 + lane];
            const ImgF& ib = d.img[b];
            float p[3];
            int r, c;
            fu::project(ib.cam, X, p);
            if (b > step && ib.map_off != kNoMap && fu::pixel_of(p, ib.w, ib.h, r, c)) {
                const uint64_t hw = (uint64_t)ib.w * (uint64_t)ib.h, idx = (uint64_t)r * (uint64_t)ib.w + (uint64_t)c;
                const float zb = d.depth[ib.map_off + idx];
                if (zb > 0.0f) {
                    float ps[3], Nb[3], Xc[3];
                    fu::project(ib.cam, Xs, ps);
                    const float* nm = d.normal + 3 * ib.map_off;
                    fu::world_normal(ib.cam, nm[idx], nm[hw + idx], nm[2 * hw + idx], Nb);
                    fu::lift(ib.cam, (float)c + 0.5f, (float)r + 0.5f, zb, Xc);
                    ok = fu::depth_ok(d.p, ps[2], zb) && fu::normal_ok(d.p, Ns, Nb) && fu::reproj_ok(d.p, si.cam, Xc, su, sv);
                }
            }
        }
        return __ballot(ok);
    };

    bool truncated = false;
    if (1 < d.p.max_traversal_depth && d.p.limit > 1) {
        const unsigned long long m = children(step, Xs);
        if (m) {
            if (lane == 0) {
                fMask[0] = m;
                fMember[0] = 0;
                fDepth[0] = 0;
            }
            sp = 1;
        }
    }
    __syncthreads();
    while (sp > 0) {
        const unsigned long long mask = fMask[sp - 1];
        if (!mask) {
            --sp;
            continue;
        }
        const int k = 63 - __clzll((long long)mask);
        const uint32_t parent = fMember[sp - 1], depth = fDepth[sp - 1];
        __syncthreads();  // every lane has read the frame
        if (lane == 0) fMask[sp - 1] = mask & ~(1ull << k);
        const uint32_t a = mImg[parent];
        const float X[3] = {mX[0][parent], mX[1][parent], mX[2][parent]};
        const uint32_t b = d.nb[d.img[a].nb0 + (uint32_t)k];
        const ImgF& ib = d.img[b];
        float p[3];
        int r = 0, c = 0;
        fu::project(ib.cam, X, p);
        const bool inside = fu::pixel_of(p, ib.w, ib.h, r, c);  // (it was when the mask was made)
        const uint64_t hw = (uint64_t)ib.w * (uint64_t)ib.h, idx = (uint64_t)r * (uint64_t)ib.w + (uint64_t)c;
        bool take = inside && !fu::claimed(d.claims[ib.map_off + (inside ? idx : 0)], step);
        if (take) {  // already a member?
            bool mine = false;
            for (int m = lane; m < count; m += kWave) mine = mine || (mImg[m] == b && mPix[m] == (uint32_t)idx);
            take = __ballot(mine) == 0ull;
        }
        if (take && count == d.p.limit) {  // (only while probing: the library's bound cut this cluster short)
            truncated = true;
            break;
        }
        if (take) {
            const float zb = d.depth[ib.map_off + idx];
            const float* nm = d.normal + 3 * ib.map_off;
            float Xc[3], Nb[3];
            fu::lift(ib.cam, (float)c + 0.5f, (float)r + 0.5f, zb, Xc);
            fu::world_normal(ib.cam, nm[idx], nm[hw + idx], nm[2 * hw + idx], Nb);
            if (lane < 3) {
                mX[lane][count] = Xc[lane];
                mN[lane][count] = Nb[lane];
                mC[lane][count] = d.rgb[ib.rgb_off + 3 * idx + lane];
            }
            if (lane == 0) {
                mImg[count] = b;
                mPix[count] = (uint32_t)idx;
                d.claims[ib.map_off + idx] = step + 1u;
            }
            ++count;
            if (count == d.p.limit && !d.p.probe) break;
            if ((int)depth + 2 < d.p.max_traversal_depth) {  // the new member is at depth + 1
                const unsigned long long m = children(b, Xc);
                if (m) {
                    if (lane == 0) {
                        fMask[sp] = m;
                        fMember[sp] = (uint32_t)(count - 1);
                        fDepth[sp] = depth + 1u;
                    }
                    ++sp;
                }
            }
        }
        __syncthreads();
    }
    __syncthreads();

    // 23.3: the medians by rank counting; the two middle ranks
    const int rlo = (count - 1) / 2, rhi = count / 2;
    for (int e = lane; e < count; e += kWave) {
        for (int ch = 0; ch < 9; ++ch) {
            const float* fa = ch < 3 ? mX[ch] : mN[ch < 6 ? ch - 3 : 0];
            const uint32_t* ca = mC[ch < 6 ? 0 : ch - 6];
            const uint32_t ke = ch < 6 ? fu::order_key(fa[e]) : ca[e];
            int rank = 0;
            for (int j = 0; j < count; ++j) {
                const uint32_t kj = ch < 6 ? fu::order_key(fa[j]) : ca[j];
                rank += (kj < ke || (kj == ke && j < e)) ? 1 : 0;
            }
            if (ch < 6) {
                if (rank == rlo) selF[0][ch] = fa[e];
                if (rank == rhi) selF[1][ch] = fa[e];
            } else {
                if (rank == rlo) selC[0][ch - 6] = ca[e];
                if (rank == rhi) selC[1][ch - 6] = ca[e];
            }
        }
        // the first member of its image
        bool first = true;
        for (int j = 0; j < e; ++j) first = first && mImg[j] != mImg[e];
        mFirst[e] = first ? 1u : 0u;
    }
    __syncthreads();
    int nvis = 0;
    for (int e = lane; e < count; e += kWave) {
        if (!mFirst[e]) continue;
        int rank = 0;
        for (int j = 0; j < count; ++j) rank += (mFirst[j] && mImg[j] < mImg[e]) ? 1 : 0;
        d.vis[(uint64_t)slot * d.vis_stride + (uint32_t)rank] = mImg[e];  // rank < the images from `step` on <= vis_stride
        ++nvis;
    }
    nvis = wave_sum(nvis);
    if (lane == 0) {
        const bool odd = (count & 1) != 0;
        float X[3], N[3];
        for (int k = 0; k < 3; ++k) {
            X[k] = fu::median_of(selF[0][k], selF[1][k], odd);
            N[k] = fu::median_of(selF[0][3 + k], selF[1][3 + k], odd);
        }
        fu::normalise(N);
        float* rec = d.rec + 6 * (uint64_t)slot;
        for (int k = 0; k < 3; ++k) {
            rec[k] = X[k];
            rec[3 + k] = N[k];
        }
        d.color[slot] = fu::median_of_u8(selC[0][0], selC[1][0]) | (fu::median_of_u8(selC[0][1], selC[1][1]) << 8) |
                        (fu::median_of_u8(selC[0][2], selC[1][2]) << 16);
        const bool valid = count >= d.p.min_num_pixels && fu::in_box(d.p, X);
        d.info[slot] = (uint32_t)count | ((uint32_t)nvis << kInfoVisShift) | (valid ? kInfoValid : 0u) | (truncated ? kInfoTruncated : 0u);
    }
}

// the launch's points, packed in seed order
__global__ __launch_bounds__(kBlock) void fusion_gather_kernel(Gather g) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= g.num_points) return;
    const uint32_t slot = g.slot[p];
    for (int k = 0; k < 3; ++k) {
        g.xyz[3 * (uint64_t)p + k] = g.rec[6 * (uint64_t)slot + k];
        g.normal[3 * (uint64_t)p + k] = g.rec[6 * (uint64_t)slot + 3 + k];
    }
    g.out_color[p] = g.color[slot];
    const uint32_t v0 = g.vis_off[p], v1 = g.vis_off[p + 1];
    for (uint32_t v = v0; v < v1; ++v) g.out_vis[v] = g.vis[(uint64_t)slot * g.vis_stride + (v - v0)];
}

// What is wrong with the call, or the empty string.  Nothing is read through an offset or an index before it has been
// checked.
std::string check_call(const amc_fusion_opts& o, const amc_fusion_problem& pb) {
    const size_t n = pb.num_images;
    if (o.min_num_pixels < 0) return "min_num_pixels is negative";
    if (o.max_num_pixels < 1 || o.max_num_pixels < o.min_num_pixels) return "max_num_pixels is not at least 1 and min_num_pixels";
    if (o.max_traversal_depth < 1 || o.max_traversal_depth > AMC_FUSION_MAX_TRAVERSAL_DEPTH)
        return "max_traversal_depth is not in 1 .. " + std::to_string(AMC_FUSION_MAX_TRAVERSAL_DEPTH) + " (AMC_FUSION_MAX_TRAVERSAL_DEPTH)";
    if (!(o.max_reproj_error >= 0.0) || !(o.max_depth_error >= 0.0) || !(o.max_normal_error >= 0.0)) return "an error bound is negative";
    for (int k = 0; k < 6; ++k)
        if (o.bounding_box[k] != o.bounding_box[k]) return "bounding_box holds a value that is not a number";
    if (n > 0x7fffffffu) return "too many images for 32-bit indices";
    if (!n) return std::string();
    if (!pb.rgb || !pb.rgb_offsets || !pb.widths || !pb.heights || !pb.K || !pb.R || !pb.t) return "NULL image array";
    if (!pb.depth || !pb.normal || !pb.map_offsets) return "NULL map array";
    if (!pb.nb_offsets || !pb.nb_images) return "NULL neighbour array";
    for (size_t i = 0; i < n; ++i) {
        if (pb.widths[i] < 1 || pb.heights[i] < 1) return "image " + std::to_string(i) + " has no pixels";
        if ((uint64_t)pb.widths[i] * (uint64_t)pb.heights[i] > AMC_FUSION_MAX_PIXELS)
            return "image " + std::to_string(i) + " has more than 2^31 pixels (AMC_FUSION_MAX_PIXELS)";
    }
    if (pb.nb_offsets[0] != 0) return "nb_offsets does not start at 0";
    for (size_t i = 0; i < n; ++i) {
        if (pb.nb_offsets[i + 1] < pb.nb_offsets[i]) return "nb_offsets decreases at image " + std::to_string(i);
        const uint64_t k = pb.nb_offsets[i + 1] - pb.nb_offsets[i];
        if (k > AMC_FUSION_MAX_NEIGHBOURS)
            return "image " + std::to_string(i) + " has " + std::to_string(k) + " neighbours, more than " + std::to_string(AMC_FUSION_MAX_NEIGHBOURS) +
                   " (AMC_FUSION_MAX_NEIGHBOURS)";
    }
    for (uint64_t k = 0; k < pb.nb_offsets[n]; ++k)
        if (pb.nb_images[k] >= n) return "neighbour " + std::to_string(k) + " names an image out of range";
    return std::string();
}

// the call's output while it grows
struct Points {
    std::vector<float> xyz, normal;
    std::vector<uint32_t> color, seed_image, seed_pixel, num_fused, vis;
    std::vector<uint64_t> vis_off{0};
};

void free_arrays(amc_fusion_result* r) {
    std::free(r->xyz);
    std::free(r->normal);
    std::free(r->color);
    std::free(r->seed_image);
    std::free(r->seed_pixel);
    std::free(r->num_fused);
    std::free(r->vis_offsets);
    std::free(r->vis_images);
    r->xyz = r->normal = nullptr;
    r->color = nullptr;
    r->seed_image = r->seed_pixel = r->num_fused = r->vis_images = nullptr;
    r->vis_offsets = nullptr;
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

int run_device(amc_ctx* ctx, const amc_fusion_problem& pb, const amc_fusion_opts& op, uint64_t batch_seeds, Points& out,
               amc_fusion_result* result) {
    static const char* const hipchk_who = "amc_fuse_depth_maps";
    const size_t n = pb.num_images;
    const uint64_t nnb = pb.nb_offsets[n];
    std::vector<ImgF> img(n);
    uint64_t nbytes = 0, nmap = 0, most_pix = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t hw = (uint64_t)pb.widths[i] * (uint64_t)pb.heights[i];
        ImgF& im = img[i];
        im.cam = fu::make_cam(pb.K + 4 * i, pb.R + 9 * i, pb.t + 3 * i);
        im.rgb_off = pb.rgb_offsets[i];
        im.map_off = pb.map_offsets[i];
        im.nb0 = pb.nb_offsets[i];
        im.w = pb.widths[i];
        im.h = pb.heights[i];
        im.nnb = (uint32_t)(pb.nb_offsets[i + 1] - pb.nb_offsets[i]);
        im.pad = 0;
        nbytes = std::max(nbytes, im.rgb_off + 3 * hw);
        if (im.map_off != kNoMap) {
            nmap = std::max(nmap, im.map_off + hw);
            most_pix = std::max(most_pix, hw);
        }
    }
    if (!nmap) return AMC_OK;  // no image has maps: no seeds
    const uint64_t batch = std::min<uint64_t>(batch_seeds, most_pix);
    const uint32_t vis_stride = (uint32_t)std::min<uint64_t>(kMaxC, n);

    const CtxView cv = ctx_view(ctx);
    HIPCHK(hipSetDevice(cv.device));
    hipStream_t st = cv.stream;
    Dev d{};
    double box[6];
    for (int k = 0; k < 6; ++k) box[k] = op.bounding_box[k];
    d.p = fu::make_params(op.min_num_pixels, op.max_num_pixels, kMaxC, op.max_traversal_depth, op.max_reproj_error, op.max_depth_error,
                          op.max_normal_error, box);
    d.vis_stride = vis_stride;
    uint8_t* d_rgb;
    ImgF* d_img;
    float *d_depth, *d_normal;
    uint32_t *d_nb, *d_seeds, *d_slot, *d_voff, *d_out_color, *d_out_vis;
    float *d_out_xyz, *d_out_normal;
    DevBuf<void> mem;  // the call's working set: allocated here, freed on return
    DevParts parts;
    parts.part(&d_rgb, nbytes).part(&d_img, n).part(&d_depth, nmap).part(&d_normal, 3 * nmap).part(&d_nb, std::max<uint64_t>(nnb, 1))
        .part(&d.claims, nmap).part(&d.flags, most_pix).part(&d_seeds, batch).part(&d.rec, 6 * batch).part(&d.color, batch)
        .part(&d.info, batch).part(&d.vis, batch * vis_stride).part(&d_slot, batch).part(&d_voff, batch + 1)
        .part(&d_out_xyz, 3 * batch).part(&d_out_normal, 3 * batch).part(&d_out_color, batch).part(&d_out_vis, batch * vis_stride);
    {
        const auto t0 = std::chrono::steady_clock::now();
        const hipError_t e = parts.carve(mem);
        if (e == hipErrorOutOfMemory) return api_fail(AMC_E_NOMEM, "%s: out of device memory", hipchk_who);
        HIPCHK(e);
        result->alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    // an early return must not leave copies in flight that read the tables or write the output's vectors
    struct Drain {
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{st};
    StreamTimer timer(st), kernels(st), copies(st);
    HIPCHK(timer.start());
    auto up = [&](void* dst, const void* s, size_t bytes) { return bytes ? hipMemcpyAsync(dst, s, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
    auto down = [&](void* dst, const void* s, size_t bytes) { return bytes ? hipMemcpyAsync(dst, s, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
    HIPCHK(copies.span_begin());
    HIPCHK(up(d_rgb, pb.rgb, nbytes));
    HIPCHK(up(d_img, img.data(), n * sizeof(ImgF)));
    HIPCHK(up(d_depth, pb.depth, nmap * 4));
    HIPCHK(up(d_normal, pb.normal, nmap * 12));
    HIPCHK(up(d_nb, pb.nb_images, nnb * 4));
    HIPCHK(hipMemsetAsync(d.claims, 0, nmap * 4, st));
    HIPCHK(copies.span_end());
    d.img = d_img;
    d.rgb = d_rgb;
    d.depth = d_depth;
    d.normal = d_normal;
    d.nb = d_nb;
    d.seeds = d_seeds;

    std::vector<uint8_t> flags(most_pix);
    std::vector<uint32_t> seeds, info(batch), slot, voff;
    for (size_t i = 0; i < n; ++i) {
        if (img[i].map_off == kNoMap) continue;
        const uint64_t hw = (uint64_t)img[i].w * (uint64_t)img[i].h;
        d.step = (uint32_t)i;
        HIPCHK(kernels.span_begin());
        hipLaunchKernelGGL(fusion_seed_kernel, dim3(blocks_for(hw)), dim3(kBlock), 0, st, d);
        HIPCHK(hipGetLastError());
        HIPCHK(kernels.span_end());
        result->num_launches += 1;
        HIPCHK(copies.span_begin());
        HIPCHK(down(flags.data(), d.flags, hw));
        HIPCHK(copies.span_end());
        HIPCHK(hipStreamSynchronize(st));
        seeds.clear();
        for (uint64_t k = 0; k < hw; ++k)
            if (flags[k]) seeds.push_back((uint32_t)k);
        result->num_seeds += seeds.size();
        for (uint64_t s0 = 0; s0 < seeds.size(); s0 += batch) {
            const uint32_t ns = (uint32_t)std::min<uint64_t>(batch, seeds.size() - s0);
            d.num_seeds = ns;
            HIPCHK(copies.span_begin());
            HIPCHK(up(d_seeds, seeds.data() + s0, (size_t)ns * 4));
            HIPCHK(copies.span_end());
            HIPCHK(kernels.span_begin());
            hipLaunchKernelGGL(fusion_cluster_kernel, dim3(ns), dim3(kWave), 0, st, d);
            HIPCHK(hipGetLastError());
            HIPCHK(kernels.span_end());
            result->num_launches += 1;
            result->num_batches += 1;
            HIPCHK(copies.span_begin());
            HIPCHK(down(info.data(), d.info, (size_t)ns * 4));
            HIPCHK(copies.span_end());
            HIPCHK(hipStreamSynchronize(st));
            slot.clear();
            voff.assign(1, 0u);
            for (uint32_t s = 0; s < ns; ++s) {
                const uint32_t w = info[s];
                if (w & kInfoTruncated) result->num_truncated += 1;
                if (!(w & kInfoValid)) continue;
                const uint32_t nv = (w >> kInfoVisShift) & 0x3ffu;
                slot.push_back(s);
                voff.push_back(voff.back() + nv);
                out.seed_image.push_back((uint32_t)i);
                out.seed_pixel.push_back(seeds[s0 + s]);
                out.num_fused.push_back(w & 0x3ffu);
                out.vis_off.push_back(out.vis_off.back() + nv);
            }
            const uint32_t np = (uint32_t)slot.size();
            if (!np) continue;
            const size_t p0 = out.color.size(), v0 = out.vis.size();
            out.xyz.resize(3 * (p0 + np));
            out.normal.resize(3 * (p0 + np));
            out.color.resize(p0 + np);
            out.vis.resize(v0 + voff.back());
            Gather g{np, vis_stride, d_slot, d_voff, d.rec, d.color, d.vis, d_out_xyz, d_out_normal, d_out_color, d_out_vis};
            HIPCHK(copies.span_begin());
            HIPCHK(up(d_slot, slot.data(), (size_t)np * 4));
            HIPCHK(up(d_voff, voff.data(), ((size_t)np + 1) * 4));
            HIPCHK(copies.span_end());
            HIPCHK(kernels.span_begin());
            hipLaunchKernelGGL(fusion_gather_kernel, dim3(blocks_for(np)), dim3(kBlock), 0, st, g);
            HIPCHK(hipGetLastError());
            HIPCHK(kernels.span_end());
            result->num_launches += 1;
            HIPCHK(copies.span_begin());
            HIPCHK(down(out.xyz.data() + 3 * p0, d_out_xyz, (size_t)np * 12));
            HIPCHK(down(out.normal.data() + 3 * p0, d_out_normal, (size_t)np * 12));
            HIPCHK(down(out.color.data() + p0, d_out_color, (size_t)np * 4));
            HIPCHK(down(out.vis.data() + v0, d_out_vis, (size_t)voff.back() * 4));
            HIPCHK(copies.span_end());
            HIPCHK(hipStreamSynchronize(st));
        }
    }
    HIPCHK(timer.stop(result->device_ms));
    HIPCHK(kernels.spans(result->kernel_ms));
    HIPCHK(copies.spans(result->copy_ms));
    return AMC_OK;
}

template <typename T>
bool copy_out(T*& dst, const T* src, size_t count) {
    dst = (T*)std::calloc(std::max<size_t>(count, 1), sizeof(T));
    if (!dst) return false;
    if (count) std::memcpy(dst, src, count * sizeof(T));
    return true;
}

int run(amc_ctx* ctx, const amc_fusion_opts* opts, const amc_fusion_problem* pb, amc_fusion_result* result) {
    const char* fn = "amc_fuse_depth_maps";
    const auto host_t0 = std::chrono::steady_clock::now();
    if (result) std::memset(result, 0, sizeof *result);
    if (!ctx || !pb || !result) return api_fail(AMC_E_INVALID, "%s: NULL argument", fn);
    amc_fusion_opts op;
    amc_fusion_opts_default(&op);
    if (opts) op = *opts;
    // (the test hook is read before anything can fail, once per call)
    const uint64_t batch_seeds = (uint64_t)env_int("AMC_FUSION_BATCH_SEEDS", kDefaultBatchSeeds, 1, 1ll << 24);
    const std::string bad = check_call(op, *pb);
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: %s", fn, bad.c_str());
    int rc = AMC_OK;
    try {
        Points out;
        if (pb->num_images) rc = run_device(ctx, *pb, op, batch_seeds, out, result);
        if (rc == AMC_OK) {
            const size_t np = out.seed_image.size();
            std::vector<uint8_t> rgb(3 * np);
            for (size_t p = 0; p < np; ++p)
                for (int k = 0; k < 3; ++k) rgb[3 * p + k] = (uint8_t)(out.color[p] >> (8 * k));
            result->num_points = np;
            const bool ok = copy_out(result->xyz, out.xyz.data(), 3 * np) && copy_out(result->normal, out.normal.data(), 3 * np) &&
                            copy_out(result->color, rgb.data(), 3 * np) && copy_out(result->seed_image, out.seed_image.data(), np) &&
                            copy_out(result->seed_pixel, out.seed_pixel.data(), np) && copy_out(result->num_fused, out.num_fused.data(), np) &&
                            copy_out(result->vis_offsets, out.vis_off.data(), np + 1) && copy_out(result->vis_images, out.vis.data(), out.vis.size());
            if (!ok) rc = api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
        }
    } catch (const std::bad_alloc&) {
        rc = api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    if (rc != AMC_OK) {
        free_arrays(result);
        const amc_fusion_result zero{};
        *result = zero;
        return rc;
    }
    result->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count() - result->device_ms;
    return AMC_OK;
}

}  // namespace

extern "C" {

void amc_fusion_opts_default(amc_fusion_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->min_num_pixels = 5;
    o->max_num_pixels = 10000;
    o->max_traversal_depth = 100;
    o->max_reproj_error = 2.0;
    o->max_depth_error = 0.01;
    o->max_normal_error = 10.0;
    for (int k = 0; k < 3; ++k) {
        o->bounding_box[k] = -(double)FLT_MAX;
        o->bounding_box[3 + k] = (double)FLT_MAX;
    }
}

int amc_fuse_depth_maps(amc_ctx* ctx, const amc_fusion_opts* opts, const amc_fusion_problem* problem, amc_fusion_result* result) {
    return run(ctx, opts, problem, result);
}

void amc_fusion_result_free(amc_fusion_result* r) {
    if (!r) return;
    free_arrays(r);
}

}  // extern "C"
