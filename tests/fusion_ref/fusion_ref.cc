// fusion_ref.cc — the sequential CPU reference of stereo fusion, written from DESIGN.md section 23: one seed after the
// other, an explicit queue popped from the back, a plain sort for the medians, the claims of a step applied when the step
// ends.  It shares pycolmap_amd/csrc/fusion_core.h (the float32 arithmetic) with the kernel and nothing else.
//
// Only the reference has the trace: for every child it looks at, the cluster, the member it came from, the child's image
// and pixel and why it was taken or dropped.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../pycolmap_amd/csrc/fusion_core.h"
#include "../../include/amc_fusion.h"

namespace {

enum Reason : int32_t {
    kTaken = 0,
    kNoMap = 1,         // the child image has no maps
    kEarlierImage = 2,  // the child image is not after the seed's
    kOutside = 3,       // the projection is behind the image, outside the map or not a number
    kClaimed = 4,       // an earlier step took the pixel
    kInCluster = 5,     // the pixel is a member already
    kNoDepth = 6,       // depth <= 0 or not a number
    kDepthError = 7,
    kNormalError = 8,
    kReprojError = 9,
    kCutShort = 10,     // it would have been taken, but the cluster is at the library's bound
};

struct Item {
    uint32_t image;
    int row, col, depth;
    int parent;  // the member that pushed it
};

struct Run {
    std::vector<float> xyz, normal;
    std::vector<uint8_t> color;
    std::vector<uint32_t> seed_image, seed_pixel, num_fused, vis;
    std::vector<uint64_t> vis_off{0};
    std::vector<int32_t> trace;  // 7 per line: cluster (the seed's number in the call), parent member, image, row, col, reason, members so far
    uint64_t num_seeds = 0, num_truncated = 0;
};

float median(std::vector<float> v) {
    std::sort(v.begin(), v.end(), [](float a, float b) { return fu::order_key(a) < fu::order_key(b); });
    const size_t m = v.size();
    return fu::median_of(v[(m - 1) / 2], v[m / 2], m % 2 == 1);
}

uint8_t median(std::vector<uint8_t> v) {
    std::sort(v.begin(), v.end());
    const size_t m = v.size();
    return (uint8_t)fu::median_of_u8(v[(m - 1) / 2], v[m / 2]);
}

void fuse(const amc_fusion_opts& op, const amc_fusion_problem& pb, bool want_trace, Run& out) {
    const size_t n = pb.num_images;
    double box[6];
    for (int k = 0; k < 6; ++k) box[k] = op.bounding_box[k];
    const fu::Params prm = fu::make_params(op.min_num_pixels, op.max_num_pixels, AMC_FUSION_MAX_CLUSTER, op.max_traversal_depth,
                                           op.max_reproj_error, op.max_depth_error, op.max_normal_error, box);
    std::vector<fu::Cam> cam(n);
    std::vector<std::vector<uint8_t>> claimed(n);
    for (size_t i = 0; i < n; ++i) {
        cam[i] = fu::make_cam(pb.K + 4 * i, pb.R + 9 * i, pb.t + 3 * i);
        if (pb.map_offsets[i] != AMC_FUSION_NO_MAP) claimed[i].assign((size_t)pb.widths[i] * (size_t)pb.heights[i], 0);
    }
    auto depth_at = [&](size_t i, size_t idx) { return pb.depth[pb.map_offsets[i] + idx]; };
    auto normal_at = [&](size_t i, size_t idx, float N[3]) {
        const size_t hw = (size_t)pb.widths[i] * (size_t)pb.heights[i];
        const float* nm = pb.normal + 3 * pb.map_offsets[i];
        fu::world_normal(cam[i], nm[idx], nm[hw + idx], nm[2 * hw + idx], N);
    };
    struct Member {
        uint32_t image, pixel;
        float X[3], N[3];
        uint8_t rgb[3];
    };
    for (size_t i = 0; i < n; ++i) {
        if (pb.map_offsets[i] == AMC_FUSION_NO_MAP) continue;
        const int w = pb.widths[i], h = pb.heights[i];
        std::vector<std::pair<uint32_t, uint32_t>> pending;  // this step's members: claimed when the step ends
        for (int row = 0; row < h; ++row) {
            for (int col = 0; col < w; ++col) {
                const size_t spix = (size_t)row * w + col;
                if (!(depth_at(i, spix) > 0.0f) || claimed[i][spix]) continue;
                const int32_t cluster = (int32_t)out.num_seeds++;
                const float su = (float)col + 0.5f, sv = (float)row + 0.5f;
                std::vector<Member> members;
                std::vector<Item> queue;
                auto push_children = [&](int parent, int depth) {
                    if (depth + 1 >= prm.max_traversal_depth) return;
                    const Member& m = members[parent];
                    for (uint64_t k = pb.nb_offsets[m.image]; k < pb.nb_offsets[m.image + 1]; ++k) {
                        const uint32_t b = pb.nb_images[k];
                        int r = -1, c = -1;
                        int32_t why = -1;
                        if (pb.map_offsets[b] == AMC_FUSION_NO_MAP) {
                            why = kNoMap;
                        } else if (b <= i) {
                            why = kEarlierImage;
                        } else {
                            float p[3];
                            fu::project(cam[b], m.X, p);
                            if (!fu::pixel_of(p, pb.widths[b], pb.heights[b], r, c)) why = kOutside;
                        }
                        if (why >= 0) {
                            if (want_trace) out.trace.insert(out.trace.end(), {cluster, parent, (int32_t)b, r, c, why, (int32_t)members.size()});
                            continue;
                        }
                        queue.push_back(Item{b, r, c, depth + 1, parent});
                    }
                };
                Member seed;
                seed.image = (uint32_t)i;
                seed.pixel = (uint32_t)spix;
                fu::lift(cam[i], su, sv, depth_at(i, spix), seed.X);
                normal_at(i, spix, seed.N);
                std::memcpy(seed.rgb, pb.rgb + pb.rgb_offsets[i] + 3 * spix, 3);
                members.push_back(seed);
                bool truncated = false;
                if (prm.limit > 1) push_children(0, 0);
                while (!queue.empty()) {
                    const Item it = queue.back();
                    queue.pop_back();
                    const uint32_t b = it.image;
                    const size_t idx = (size_t)it.row * pb.widths[b] + it.col;
                    int32_t why = kTaken;
                    Member m;
                    m.image = b;
                    m.pixel = (uint32_t)idx;
                    const float z = depth_at(b, idx);
                    if (claimed[b][idx]) {
                        why = kClaimed;
                    } else if (std::any_of(members.begin(), members.end(), [&](const Member& q) { return q.image == b && q.pixel == idx; })) {
                        why = kInCluster;
                    } else if (!(z > 0.0f)) {
                        why = kNoDepth;
                    } else {
                        float ps[3];
                        fu::project(cam[b], members[0].X, ps);
                        normal_at(b, idx, m.N);
                        fu::lift(cam[b], (float)it.col + 0.5f, (float)it.row + 0.5f, z, m.X);
                        if (!fu::depth_ok(prm, ps[2], z)) why = kDepthError;
                        else if (!fu::normal_ok(prm, members[0].N, m.N)) why = kNormalError;
                        else if (!fu::reproj_ok(prm, cam[i], m.X, su, sv)) why = kReprojError;
                        else if ((int)members.size() == prm.limit) why = kCutShort;
                    }
                    if (want_trace) out.trace.insert(out.trace.end(), {cluster, it.parent, (int32_t)b, it.row, it.col, why, (int32_t)members.size()});
                    if (why == kCutShort) {
                        truncated = true;
                        break;
                    }
                    if (why != kTaken) continue;
                    std::memcpy(m.rgb, pb.rgb + pb.rgb_offsets[b] + 3 * idx, 3);
                    members.push_back(m);
                    pending.emplace_back(b, (uint32_t)idx);
                    if ((int)members.size() == prm.limit && !prm.probe) break;
                    push_children((int)members.size() - 1, it.depth);
                }
                out.num_truncated += truncated ? 1 : 0;
                if ((int)members.size() < prm.min_num_pixels) continue;
                float X[3], N[3];
                uint8_t rgb[3];
                for (int k = 0; k < 3; ++k) {
                    std::vector<float> xs, ns;
                    std::vector<uint8_t> cs;
                    for (const Member& m : members) {
                        xs.push_back(m.X[k]);
                        ns.push_back(m.N[k]);
                        cs.push_back(m.rgb[k]);
                    }
                    X[k] = median(xs);
                    N[k] = median(ns);
                    rgb[k] = median(cs);
                }
                fu::normalise(N);
                if (!fu::in_box(prm, X)) continue;
                std::vector<uint32_t> seen;
                for (const Member& m : members) seen.push_back(m.image);
                std::sort(seen.begin(), seen.end());
                seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
                out.xyz.insert(out.xyz.end(), X, X + 3);
                out.normal.insert(out.normal.end(), N, N + 3);
                out.color.insert(out.color.end(), rgb, rgb + 3);
                out.seed_image.push_back((uint32_t)i);
                out.seed_pixel.push_back((uint32_t)spix);
                out.num_fused.push_back((uint32_t)members.size());
                out.vis.insert(out.vis.end(), seen.begin(), seen.end());
                out.vis_off.push_back(out.vis.size());
            }
        }
        for (const auto& bp : pending) claimed[bp.first][bp.second] = 1;
    }
}

}  // namespace

extern "C" {

void* furef_fuse(const amc_fusion_opts* op, const amc_fusion_problem* pb, int want_trace) {
    Run* r = new Run;
    fuse(*op, *pb, want_trace != 0, *r);
    return r;
}

// num_points, visibility entries, num_seeds, num_truncated, trace lines
void furef_counts(const void* h, uint64_t out[5]) {
    const Run& r = *static_cast<const Run*>(h);
    out[0] = r.seed_image.size();
    out[1] = r.vis.size();
    out[2] = r.num_seeds;
    out[3] = r.num_truncated;
    out[4] = r.trace.size() / 7;
}

void furef_copy(const void* h, float* xyz, float* normal, uint8_t* color, uint32_t* seed_image, uint32_t* seed_pixel, uint32_t* num_fused,
                uint64_t* vis_off, uint32_t* vis, int32_t* trace) {
    const Run& r = *static_cast<const Run*>(h);
    auto put = [](auto* dst, const auto& v) {
        if (!v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0]));
    };
    put(xyz, r.xyz);
    put(normal, r.normal);
    put(color, r.color);
    put(seed_image, r.seed_image);
    put(seed_pixel, r.seed_pixel);
    put(num_fused, r.num_fused);
    put(vis_off, r.vis_off);
    put(vis, r.vis);
    put(trace, r.trace);
}

void furef_free(void* h) { delete static_cast<Run*>(h); }

// The float32 quantities that the three tests compare, for a seed pixel and a child pixel: out = the relative depth
// error, the normals' cosine, the squared reprojection error, then the seed's point and the child's point (9 values).
void furef_measure(const amc_fusion_problem* pb, uint32_t si, int srow, int scol, uint32_t b, int row, int col, float* out) {
    const fu::Cam cs = fu::make_cam(pb->K + 4 * si, pb->R + 9 * si, pb->t + 3 * si), cb = fu::make_cam(pb->K + 4 * b, pb->R + 9 * b, pb->t + 3 * b);
    auto normal_at = [&](uint32_t i, const fu::Cam& cam, size_t idx, float N[3]) {
        const size_t hw = (size_t)pb->widths[i] * (size_t)pb->heights[i];
        const float* nm = pb->normal + 3 * pb->map_offsets[i];
        fu::world_normal(cam, nm[idx], nm[hw + idx], nm[2 * hw + idx], N);
    };
    const size_t sidx = (size_t)srow * pb->widths[si] + scol, idx = (size_t)row * pb->widths[b] + col;
    const float su = (float)scol + 0.5f, sv = (float)srow + 0.5f;
    float Xs[3], Ns[3], Xc[3], Nb[3], ps[3];
    fu::lift(cs, su, sv, pb->depth[pb->map_offsets[si] + sidx], Xs);
    normal_at(si, cs, sidx, Ns);
    const float z = pb->depth[pb->map_offsets[b] + idx];
    fu::project(cb, Xs, ps);
    normal_at(b, cb, idx, Nb);
    fu::lift(cb, (float)col + 0.5f, (float)row + 0.5f, z, Xc);
    out[0] = fu::depth_err(ps[2], z);
    out[1] = fu::normal_dot(Ns, Nb);
    out[2] = fu::reproj_sq(cs, Xc, su, sv);
    for (int k = 0; k < 3; ++k) {
        out[3 + k] = Xs[k];
        out[6 + k] = Xc[k];
    }
}

// the projection of a world point into image b: u, v, depth, and whether pixel_of finds a pixel (row, col)
int furef_project(const amc_fusion_problem* pb, uint32_t b, const float* X, float* uvz, int* rowcol) {
    const fu::Cam cb = fu::make_cam(pb->K + 4 * b, pb->R + 9 * b, pb->t + 3 * b);
    float p[3];
    fu::project(cb, X, p);
    uvz[0] = p[0] / p[2];
    uvz[1] = p[1] / p[2];
    uvz[2] = p[2];
    return fu::pixel_of(p, pb->widths[b], pb->heights[b], rowcol[0], rowcol[1]) ? 1 : 0;
}

}  // extern "C"
