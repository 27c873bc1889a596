// fusion_ref_fuzz.cc — a stand-alone program for tests/test_stereo_fusion_cpu.py (built with -fsanitize=address,undefined
// and run): the C++ of stereo fusion that runs on a host - pycolmap_amd/csrc/fusion_core.h, which the kernel shares, and the
// sequential reference tests/fusion_ref/fusion_ref.cc - on 300 seeded problems whose arrays live on the heap at their exact
// sizes: a few small images at poses near the identity, depth and normal maps salted with NaN, infinities, zeros and
// negative values, images without maps, neighbour lists with repeats, the image itself and earlier images, and options
// down to a traversal depth and a cluster of one.  Every result is checked for what DESIGN.md section 23 promises of any
// input: no NaN in a point, unit or zero normals, clusters within their bounds, ascending visibility lists without repeats,
// seeds in step and row-major order.  Prints "ok <problems>".
#include <cmath>
#include <cstdio>
#include <limits>
#include <memory>
#include <random>

#include "../fusion_ref/fusion_ref.cc"

namespace {

template <typename T>
std::unique_ptr<T[]> heap(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size()]);  // exactly v.size() elements: one past it is a report
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

int fail(const char* what, int problem) {
    std::printf("FAILED %s in problem %d\n", what, problem);
    return 1;
}

}  // namespace

int main() {
    std::mt19937 gen(7);
    auto uni = [&](double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(gen); };
    auto pick = [&](int n) { return (int)(gen() % (uint32_t)n); };
    const float bad[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                         -std::numeric_limits<float>::infinity(), 0.0f, -1.5f, 1e30f};
    const int problems = 300;
    for (int q = 0; q < problems; ++q) {
        const int n = 1 + pick(6);
        std::vector<uint8_t> rgb;
        std::vector<uint64_t> rgb_off, map_off, nb_off{0};
        std::vector<int32_t> w, h;
        std::vector<double> K, R, t;
        std::vector<float> depth, normal;
        std::vector<uint32_t> nb;
        for (int i = 0; i < n; ++i) {
            const int wi = 1 + pick(7), hi = 1 + pick(5), hw = wi * hi;
            w.push_back(wi);
            h.push_back(hi);
            rgb_off.push_back(rgb.size());
            for (int k = 0; k < 3 * hw; ++k) rgb.push_back((uint8_t)pick(256));
            const double f = uni(3.0, 9.0);
            K.insert(K.end(), {f, f * uni(0.9, 1.1), wi / 2.0, hi / 2.0});
            const double a = uni(-0.05, 0.05), c = std::cos(a), s = std::sin(a);  // a small turn about y
            R.insert(R.end(), {c, 0.0, s, 0.0, 1.0, 0.0, -s, 0.0, c});
            t.insert(t.end(), {uni(-0.2, 0.2), uni(-0.2, 0.2), uni(-0.1, 0.1)});
            if (pick(8) == 0) {
                map_off.push_back(AMC_FUSION_NO_MAP);
            } else {
                map_off.push_back(depth.size());
                // the normal maps are addressed at three times the depth maps' offsets
                std::vector<float> nm(3 * (size_t)hw);
                for (int k = 0; k < hw; ++k) {
                    depth.push_back(pick(12) == 0 ? bad[pick(6)] : (float)uni(1.9, 2.1));
                    nm[k] = pick(20) == 0 ? bad[pick(6)] : (float)uni(-0.1, 0.1);
                    nm[hw + k] = (float)uni(-0.1, 0.1);
                    nm[2 * hw + k] = -1.0f;
                }
                normal.insert(normal.end(), nm.begin(), nm.end());
            }
            const int count = pick(4) == 0 ? 0 : 1 + pick(8);
            for (int k = 0; k < count; ++k) nb.push_back((uint32_t)pick(n));
            nb_off.push_back(nb.size());
        }
        if (q % 50 == 0) t[0] = std::numeric_limits<double>::quiet_NaN();
        if (depth.empty()) depth.push_back(0.0f), normal.insert(normal.end(), 3, 0.0f);
        if (nb.empty()) nb.push_back(0);
        auto p_rgb = heap(rgb);
        auto p_rgb_off = heap(rgb_off);
        auto p_map_off = heap(map_off);
        auto p_nb_off = heap(nb_off);
        auto p_w = heap(w);
        auto p_h = heap(h);
        auto p_K = heap(K);
        auto p_R = heap(R);
        auto p_t = heap(t);
        auto p_depth = heap(depth);
        auto p_normal = heap(normal);
        auto p_nb = heap(nb);
        amc_fusion_problem pb{};
        pb.num_images = (size_t)n;
        pb.rgb = p_rgb.get();
        pb.rgb_offsets = p_rgb_off.get();
        pb.widths = p_w.get();
        pb.heights = p_h.get();
        pb.K = p_K.get();
        pb.R = p_R.get();
        pb.t = p_t.get();
        pb.depth = p_depth.get();
        pb.normal = p_normal.get();
        pb.map_offsets = p_map_off.get();
        pb.nb_offsets = p_nb_off.get();
        pb.nb_images = p_nb.get();
        amc_fusion_opts op{};
        op.min_num_pixels = pick(4);
        op.max_num_pixels = std::max(1, op.min_num_pixels) + (pick(3) == 0 ? 0 : pick(3) == 0 ? 10000 : pick(6));
        op.max_traversal_depth = 1 + pick(pick(2) ? 4 : 128);
        op.max_reproj_error = uni(0.0, 3.0);
        op.max_depth_error = uni(0.0, 0.2);
        op.max_normal_error = uni(0.0, 30.0);
        for (int k = 0; k < 3; ++k) {
            op.bounding_box[k] = pick(4) ? -3.4e38 : -0.2;
            op.bounding_box[3 + k] = pick(4) ? 3.4e38 : 2.05;
        }
        Run* run = static_cast<Run*>(furef_fuse(&op, &pb, 1));
        uint64_t cnt[5];
        furef_counts(run, cnt);
        const size_t np = cnt[0];
        const int limit = std::min(op.max_num_pixels, AMC_FUSION_MAX_CLUSTER);
        if (run->vis_off.size() != np + 1 || run->xyz.size() != 3 * np || run->color.size() != 3 * np) return fail("sizes", q);
        if (cnt[2] < np || cnt[3] > cnt[2]) return fail("counts", q);
        for (size_t p = 0; p < np; ++p) {
            const float* X = &run->xyz[3 * p];
            const float* N = &run->normal[3 * p];
            for (int k = 0; k < 3; ++k)
                if (!(X[k] >= (float)op.bounding_box[k] && X[k] <= (float)op.bounding_box[3 + k]) || N[k] != N[k]) return fail("a point outside the box or a NaN", q);
            const double len = std::sqrt((double)N[0] * N[0] + (double)N[1] * N[1] + (double)N[2] * N[2]);
            if (!(len == 0.0 || std::fabs(len - 1.0) < 1e-5)) return fail("the normal's length", q);
            const int m = (int)run->num_fused[p];
            if (m < std::max(1, op.min_num_pixels) || m > limit) return fail("the cluster's size", q);
            const uint64_t v0 = run->vis_off[p], v1 = run->vis_off[p + 1];
            if (v1 <= v0 || v1 - v0 > (uint64_t)m || run->vis[v0] != run->seed_image[p]) return fail("the visibility list", q);
            for (uint64_t v = v0 + 1; v < v1; ++v)
                if (run->vis[v] <= run->vis[v - 1] || run->vis[v] >= (uint32_t)n) return fail("the visibility order", q);
            if (p && (run->seed_image[p] < run->seed_image[p - 1] ||
                      (run->seed_image[p] == run->seed_image[p - 1] && run->seed_pixel[p] <= run->seed_pixel[p - 1])))
                return fail("the output order", q);
        }
        for (size_t k = 0; k + 6 < run->trace.size(); k += 7)
            if (run->trace[k + 5] < 0 || run->trace[k + 5] > kCutShort || run->trace[k + 6] < 1 || run->trace[k + 6] > limit) return fail("the trace", q);
        furef_free(run);
    }
    std::printf("ok %d\n", problems);
    return 0;
}
