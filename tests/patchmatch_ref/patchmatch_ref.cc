// patchmatch_ref.cc — the sequential CPU reference of PatchMatch stereo, written from DESIGN.md section 22: plain loops
// over problems, sweeps, lines, pixels, hypotheses and sources, one after the other, on the flat problem of
// include/amc_patchmatch.h.  The per-hypothesis arithmetic is pycolmap_amd/csrc/patchmatch_core.h, shared with the
// kernels the way tri_core.h and ba_core.h are; its float32 operations are compiled here with -ffp-contract=off
// -fno-fast-math.  Also the single pieces (a cost, a propagation, a forward-backward error, a draw) for the tests that
// compare them with a float64 restatement.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/amc_patchmatch.h"
#include "../../pycolmap_amd/csrc/patchmatch_core.h"

namespace {

pm::Params params_of(const amc_patch_match_opts& o) {
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
    return pm::make_params(c);
}

pm::View view_of(const amc_patch_match_problem& pb, uint32_t i) {
    pm::View v;
    v.px = pb.pixels + pb.pixel_offsets[i];
    v.w = pb.widths[i];
    v.h = pb.heights[i];
    v.k = pm::Cam{(float)pb.K[4 * i], (float)pb.K[4 * i + 1], (float)pb.K[4 * i + 2], (float)pb.K[4 * i + 3]};
    return v;
}
pm::Rel rel_of(const amc_patch_match_problem& pb, uint32_t r, uint32_t s) {
    return pm::make_rel(pb.R + 9 * (size_t)r, pb.t + 3 * (size_t)r, pb.R + 9 * (size_t)s, pb.t + 3 * (size_t)s);
}
const float* depth_map_of(const amc_patch_match_problem& pb, uint32_t i) {
    if (!pb.in_depth || !pb.in_map_offsets || pb.in_map_offsets[i] == AMC_PATCHMATCH_NO_MAP) return nullptr;
    return pb.in_depth + pb.in_map_offsets[i];
}

// one problem, everything in order; sel is the scratch of the selection probabilities ([source][h][w])
void run_problem(const pm::Params& P, const amc_patch_match_opts& o, const amc_patch_match_problem& pb, size_t p, float* depth, float* normal,
                 uint8_t* cnt, float* costs) {
    const uint32_t r = pb.ref_images[p];
    const int S = (int)(pb.src_offsets[p + 1] - pb.src_offsets[p]);
    const uint32_t* simg = pb.src_images + pb.src_offsets[p];
    const pm::View ref = view_of(pb, r);
    const int W = ref.w, Hh = ref.h;
    const size_t hw = (size_t)W * (size_t)Hh;
    float dmin = (float)pb.depth_ranges[2 * p], dmax = (float)pb.depth_ranges[2 * p + 1];
    if (dmax < dmin) dmax = dmin;
    std::vector<pm::View> sv(S);
    std::vector<pm::Rel> rel(S);
    std::vector<const float*> sdepth(S);
    for (int s = 0; s < S; ++s) {
        sv[s] = view_of(pb, simg[s]);
        rel[s] = rel_of(pb, r, simg[s]);
        sdepth[s] = depth_map_of(pb, simg[s]);
    }
    std::vector<float> sel((size_t)S * hw, 0.5f);
    // 22.4 the initial state
    const float* in_d = P.geom ? depth_map_of(pb, r) : nullptr;
    for (int row = 0; row < Hh; ++row)
        for (int col = 0; col < W; ++col) {
            const size_t idx = (size_t)row * W + col;
            float ray[3], d = 0.0f, n[3] = {0.0f, 0.0f, -1.0f};
            pm::pixel_ray(ref.k, row, col, ray);
            bool given = false;
            if (in_d) {
                const float* nm = pb.in_normal + 3 * pb.in_map_offsets[r];
                d = in_d[idx];
                n[0] = nm[idx];
                n[1] = nm[hw + idx];
                n[2] = nm[2 * hw + idx];
                given = d >= dmin && d <= dmax && pm::face_camera(ray, n);
            }
            if (!given) pm::random_hyp(pm::rng_at(P.seed, r, (uint32_t)row, (uint32_t)col, pm::kSweepInit), 0, ray, dmin, dmax, d, n);
            depth[idx] = d;
            normal[idx] = n[0];
            normal[hw + idx] = n[1];
            normal[2 * hw + idx] = n[2];
        }
    // 22.4 - 22.5 the sweeps
    std::vector<float> cost(pm::kNumHyps * S), geo(pm::kNumHyps * S, 0.0f), wsrc(S), fwd(S);
    for (int sweep = 0; sweep < 4 * o.num_iterations; ++sweep) {
        const int dir = sweep & 3, iter = sweep >> 2;
        const bool vertical = dir == 0 || dir == 2;
        const int lines = vertical ? W : Hh, len = vertical ? Hh : W;
        for (int line = 0; line < lines; ++line) {
            for (int s = 0; s < S; ++s) fwd[s] = 0.5f;
            int prow = 0, pcol = 0;
            float pdepth = 0.0f, pn[3] = {0.0f, 0.0f, -1.0f};
            for (int k = 0; k < len; ++k) {
                const int pos = (dir == 0 || dir == 1) ? k : len - 1 - k;
                const int row = vertical ? pos : line, col = vertical ? line : pos;
                const size_t idx = (size_t)row * W + col;
                const float d0 = depth[idx];
                const float n0[3] = {normal[idx], normal[hw + idx], normal[2 * hw + idx]};
                const pm::Rng g = pm::rng_at(P.seed, r, (uint32_t)row, (uint32_t)col, (uint32_t)sweep);
                pm::Hyps H;
                pm::make_hyps(ref.k, g, iter, dmin, dmax, row, col, d0, n0, k > 0, prow, pcol, pdepth, pn, H);
                const pm::DirectWindow win{&P, &ref, row, col};
                for (int h = 0; h < pm::kNumHyps; ++h)
                    for (int s = 0; s < S; ++s) {
                        cost[h * S + s] = pm::ncc_cost(P, ref.k, sv[s], rel[s], row, col, H.depth[h], H.n[h], win);
                        if (P.geom)
                            geo[h * S + s] = sdepth[s] ? pm::fb_error(ref.k, sv[s].k, sv[s].w, sv[s].h, sdepth[s], rel[s], row, col, H.depth[h], P.geom_max)
                                                       : P.geom_max;
                    }
                float ray[3];
                pm::pixel_ray(ref.k, row, col, ray);
                const float X[3] = {d0 * ray[0], d0 * ray[1], d0};
                for (int s = 0; s < S; ++s) wsrc[s] = pm::source_weight(P, cost[s], X, n0, rel[s].C, fwd[s], sel[(size_t)s * hw + idx]);
                const int best = pm::pick_hypothesis(P, S, wsrc.data(), cost.data(), geo.data(), g, pm::kDrawSamples);
                prow = row;
                pcol = col;
                pdepth = H.depth[best];
                for (int c = 0; c < 3; ++c) pn[c] = H.n[best][c];
                depth[idx] = pdepth;
                normal[idx] = pn[0];
                normal[hw + idx] = pn[1];
                normal[2 * hw + idx] = pn[2];
            }
        }
    }
    // 22.7 the final costs and the filter
    if (!o.filter && !costs) return;
    std::vector<float> fc((size_t)S * hw), fe(P.geom ? (size_t)S * hw : 0);
    for (int s = 0; s < S; ++s)
        for (int row = 0; row < Hh; ++row)
            for (int col = 0; col < W; ++col) {
                const size_t idx = (size_t)row * W + col;
                const float n[3] = {normal[idx], normal[hw + idx], normal[2 * hw + idx]};
                const pm::DirectWindow win{&P, &ref, row, col};
                fc[(size_t)s * hw + idx] = pm::ncc_cost(P, ref.k, sv[s], rel[s], row, col, depth[idx], n, win);
                if (P.geom)
                    fe[(size_t)s * hw + idx] =
                        sdepth[s] ? pm::fb_error(ref.k, sv[s].k, sv[s].w, sv[s].h, sdepth[s], rel[s], row, col, depth[idx], 3.0e38f) : 3.0e38f;
            }
    if (costs) std::memcpy(costs, fc.data(), fc.size() * 4);
    if (!o.filter) return;
    for (int row = 0; row < Hh; ++row)
        for (int col = 0; col < W; ++col) {
            const size_t idx = (size_t)row * W + col;
            float ray[3];
            pm::pixel_ray(ref.k, row, col, ray);
            const float X[3] = {depth[idx] * ray[0], depth[idx] * ray[1], depth[idx]};
            int count = 0;
            for (int s = 0; s < S; ++s) {
                const size_t at = (size_t)s * hw + idx;
                bool ok = sel[at] >= pm::kFilterMinSelProb && 1.0f - fc[at] >= P.filter_min_ncc && pm::cos_tri_angle(X, rel[s].C) <= P.cos_filter_tri;
                if (P.geom) ok = ok && fe[at] <= P.filter_geom_max;
                count += ok ? 1 : 0;
            }
            cnt[idx] = (uint8_t)(count > 255 ? 255 : count);
            if (count < P.filter_min_num) depth[idx] = normal[idx] = normal[hw + idx] = normal[2 * hw + idx] = 0.0f;
        }
}

}  // namespace

extern "C" {

// The whole pass.  The caller allocates the outputs at the offsets amc_patch_match reports: map_offsets / cost_offsets
// (num_problems + 1), depth, normal (3 x), cnt (zeroed), costs (or NULL).  Returns 0; the caller validates.
int pmref_patch_match(const amc_patch_match_opts* o, const amc_patch_match_problem* pb, const uint64_t* map_offsets, const uint64_t* cost_offsets,
                      float* depth, float* normal, uint8_t* cnt, float* costs) {
    const pm::Params P = params_of(*o);
    for (size_t p = 0; p < pb->num_problems; ++p)
        run_problem(P, *o, *pb, p, depth + map_offsets[p], normal + 3 * map_offsets[p], cnt + map_offsets[p], costs ? costs + cost_offsets[p] : nullptr);
    return 0;
}

// the cost of hypothesis (depth, n) at pixel (row, col) of problem p in its source s
float pmref_cost(const amc_patch_match_opts* o, const amc_patch_match_problem* pb, uint64_t p, uint32_t s, int row, int col, float depth, const float* n) {
    const pm::Params P = params_of(*o);
    const uint32_t r = pb->ref_images[p], si = pb->src_images[pb->src_offsets[p] + s];
    const pm::View ref = view_of(*pb, r), sv = view_of(*pb, si);
    const pm::DirectWindow win{&P, &ref, row, col};
    return pm::ncc_cost(P, ref.k, sv, rel_of(*pb, r, si), row, col, depth, n, win);
}

float pmref_propagate(const double* K, int prow, int pcol, float pdepth, const float* pn, int row, int col) {
    return pm::propagate_depth(pm::Cam{(float)K[0], (float)K[1], (float)K[2], (float)K[3]}, prow, pcol, pdepth, pn, row, col);
}

// the forward-backward error through source s's input depth map, unbounded (3e38 where there is none)
float pmref_fb_error(const amc_patch_match_problem* pb, uint64_t p, uint32_t s, int row, int col, float depth) {
    const uint32_t r = pb->ref_images[p], si = pb->src_images[pb->src_offsets[p] + s];
    const pm::View ref = view_of(*pb, r), sv = view_of(*pb, si);
    const float* sd = depth_map_of(*pb, si);
    return sd ? pm::fb_error(ref.k, sv.k, sv.w, sv.h, sd, rel_of(*pb, r, si), row, col, depth, 3.0e38f) : 3.0e38f;
}

float pmref_uniform(uint32_t seed, uint32_t image, uint32_t row, uint32_t col, uint32_t sweep, uint32_t draw) {
    return pm::rng_at(seed, image, row, col, sweep).u(draw);
}
float pmref_exp(float x) { return pm::exp_neg(x); }
float pmref_acos(float x) { return pm::acos_poly(x); }

}  // extern "C"
