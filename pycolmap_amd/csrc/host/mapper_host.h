// mapper_host.h — the host halves of IncrementalMapper::FindNextImages, RegisterNextImage and FindLocalBundle (DESIGN.md
// 20) on model_io's plain structs: the options and their check, the flat problems of include/amc_mapper.h, the ranking,
// the 2D-3D pairs and the rule for the estimation options, the way a registration goes into the model, and the selection
// of the local bundle from the pairs' percentile angles.  No Python and no HIP here: tests/shim/mapper_host_fuzz.cc runs
// it under ASan + UBSan.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../../../include/amc_mapper.h"
#include "correspondence_graph.h"
#include "model_io.h"
#include "triangulator_host.h"

namespace amchost {

enum class ImageSelectionMethod { MAX_VISIBLE_POINTS_NUM = 0, MAX_VISIBLE_POINTS_RATIO = 1, MIN_UNCERTAINTY = 2 };

// IncrementalMapper::Options with COLMAP 3.9.1's defaults: the fields the reference binding registers
struct MapperOptions {
    int init_min_num_inliers = 100;
    double init_max_error = 4.0;
    double init_max_forward_motion = 0.95;
    double init_min_tri_angle = 16.0;
    int init_max_reg_trials = 2;
    double abs_pose_max_error = 12.0;
    int abs_pose_min_num_inliers = 30;
    double abs_pose_min_inlier_ratio = 0.25;
    bool abs_pose_refine_focal_length = true;
    bool abs_pose_refine_extra_params = true;
    int local_ba_num_images = 6;
    double local_ba_min_tri_angle = 6.0;
    double min_focal_length_ratio = 0.1;
    double max_focal_length_ratio = 10.0;
    double max_extra_param = 1.0;
    double filter_max_reproj_error = 4.0;
    double filter_min_tri_angle = 1.5;
    int max_reg_trials = 3;
    bool fix_existing_images = false;
    int num_threads = -1;
    ImageSelectionMethod image_selection_method = ImageSelectionMethod::MIN_UNCERTAINTY;
    // IncrementalMapper::Options::Check: the first condition that fails, or the empty string
    std::string Check() const {
        if (!(init_min_num_inliers > 0)) return "init_min_num_inliers > 0";
        if (!(init_max_error > 0.0)) return "init_max_error > 0.0";
        if (!(init_max_forward_motion >= 0.0)) return "init_max_forward_motion >= 0.0";
        if (!(init_max_forward_motion <= 1.0)) return "init_max_forward_motion <= 1.0";
        if (!(init_min_tri_angle >= 0.0)) return "init_min_tri_angle >= 0.0";
        if (!(init_max_reg_trials >= 1)) return "init_max_reg_trials >= 1";
        if (!(abs_pose_max_error > 0.0)) return "abs_pose_max_error > 0.0";
        if (!(abs_pose_min_num_inliers > 0)) return "abs_pose_min_num_inliers > 0";
        if (!(abs_pose_min_inlier_ratio >= 0.0)) return "abs_pose_min_inlier_ratio >= 0.0";
        if (!(abs_pose_min_inlier_ratio <= 1.0)) return "abs_pose_min_inlier_ratio <= 1.0";
        if (!(local_ba_num_images >= 2)) return "local_ba_num_images >= 2";
        if (!(local_ba_min_tri_angle >= 0.0)) return "local_ba_min_tri_angle >= 0.0";
        if (!(min_focal_length_ratio >= 0.0)) return "min_focal_length_ratio >= 0.0";
        if (!(max_focal_length_ratio >= min_focal_length_ratio)) return "max_focal_length_ratio >= min_focal_length_ratio";
        if (!(max_extra_param >= 0.0)) return "max_extra_param >= 0.0";
        if (!(filter_max_reproj_error >= 0.0)) return "filter_max_reproj_error >= 0.0";
        if (!(filter_min_tri_angle >= 0.0)) return "filter_min_tri_angle >= 0.0";
        if (!(max_reg_trials >= 1)) return "max_reg_trials >= 1";
        return std::string();
    }
    // the three thresholds of Camera::HasBogusParams in the shape ModelIndex takes them
    TriangulatorOptions BogusThresholds() const {
        TriangulatorOptions t;
        t.min_focal_length_ratio = min_focal_length_ratio;
        t.max_focal_length_ratio = max_focal_length_ratio;
        t.max_extra_param = max_extra_param;
        return t;
    }
};

// an image that is not in the model yet (20.0): what add_candidate keeps of it
struct MapperCandidate {
    uint32_t image_id = 0, camera_id = 0;
    std::vector<double> xy;  // 2 per point2D
    size_t NumPoints2D() const { return xy.size() / 2; }
};
using MapperCandidates = std::map<uint32_t, MapperCandidate>;  // ascending image id
using MapperTrials = std::map<uint32_t, int>;

// ---- 20.1: FindNextImages ------------------------------------------------------------------------------------------------
// the flat problem of amc_image_visibility for every candidate, in ascending image id, and the arrays it points into
struct FlatVisibility {
    std::vector<uint64_t> image_point_offsets{0}, point2D_point3D, cand_point_offsets{0}, corr_offsets{0};
    std::vector<uint32_t> cand_width, cand_height, corr_image, corr_point2D, cand_ids;
    std::vector<double> cand_xy;
    amc_visibility_problem Problem() const {
        amc_visibility_problem pb{};
        pb.num_graph_images = image_point_offsets.size() - 1;
        pb.image_point_offsets = image_point_offsets.data();
        pb.point2D_point3D = point2D_point3D.data();
        pb.num_candidates = cand_ids.size();
        pb.cand_width = cand_width.data();
        pb.cand_height = cand_height.data();
        pb.cand_point_offsets = cand_point_offsets.data();
        pb.cand_xy = cand_xy.data();
        pb.corr_offsets = corr_offsets.data();
        pb.corr_image = corr_image.data();
        pb.corr_point2D = corr_point2D.data();
        return pb;
    }
};

// The table holds the images the candidates' correspondences lead to, in order of first use: a model image with its
// points2D's point3D ids, any other image with as many rows of "none" as the graph gives it points2D.  Throws
// std::invalid_argument for a candidate the graph does not hold, whose point2D count differs from the graph's or whose
// camera the model does not hold, and for a correspondence into a point2D a model image does not hold.
inline FlatVisibility PlanVisibility(const CorrespondenceGraph& graph, const SparseModel& m, const ModelIndex& ix, const MapperCandidates& cands) {
    FlatVisibility f;
    std::unordered_map<uint32_t, uint32_t> table_index;
    auto table_image = [&](uint32_t image_id) {
        const auto at = table_index.emplace(image_id, static_cast<uint32_t>(f.image_point_offsets.size() - 1));
        if (!at.second) return at.first->second;
        const auto mi = ix.image.find(image_id);
        if (mi != ix.image.end()) {
            for (const ModelPoint2D& p : m.images[mi->second].points2D) f.point2D_point3D.push_back(p.point3D_id);
        } else {
            f.point2D_point3D.resize(f.point2D_point3D.size() + graph.NumPoints2D(image_id), kInvalidPoint3DId);
        }
        f.image_point_offsets.push_back(f.point2D_point3D.size());
        return at.first->second;
    };
    for (const auto& kv : cands) {
        const MapperCandidate& c = kv.second;
        if (ix.image.count(c.image_id)) continue;  // registered by other means since it was added: not a candidate (R1)
        const auto cam = ix.camera.find(c.camera_id);
        if (cam == ix.camera.end()) throw std::invalid_argument("find_next_images: candidate " + std::to_string(c.image_id) + " names a camera the reconstruction does not hold");
        if (graph.NumPoints2D(c.image_id) != c.NumPoints2D())
            throw std::invalid_argument("find_next_images: candidate " + std::to_string(c.image_id) + " has " + std::to_string(c.NumPoints2D()) +
                                        " points2D, the graph gives it " + std::to_string(graph.NumPoints2D(c.image_id)));
        const ModelCamera& mc = m.cameras[cam->second];
        if (mc.width > UINT32_MAX || mc.height > UINT32_MAX) throw std::invalid_argument("find_next_images: a camera of 2^32 pixels or more across");
        f.cand_ids.push_back(c.image_id);
        f.cand_width.push_back(static_cast<uint32_t>(mc.width));
        f.cand_height.push_back(static_cast<uint32_t>(mc.height));
        for (size_t p = 0; p < c.NumPoints2D(); ++p) {
            for (const Correspondence& corr : graph.ExtractCorrespondences(c.image_id, static_cast<uint32_t>(p))) {
                const uint32_t g = table_image(corr.image_id);
                if (corr.point2D_idx >= f.image_point_offsets[g + 1] - f.image_point_offsets[g])
                    throw std::invalid_argument("find_next_images: the graph names point2D " + std::to_string(corr.point2D_idx) + " of image " +
                                                std::to_string(corr.image_id) + ", which the reconstruction does not hold");
                f.corr_image.push_back(g);
                f.corr_point2D.push_back(corr.point2D_idx);
            }
            f.corr_offsets.push_back(f.corr_image.size());
        }
        f.cand_xy.insert(f.cand_xy.end(), c.xy.begin(), c.xy.end());
        f.cand_point_offsets.push_back(f.cand_xy.size() / 2);
    }
    return f;
}

// 20.1: drop, rank as float, never-tried candidates first, each group by descending rank then ascending image id; a NaN
// rank (which Check() excludes) would come last.  The arrays have amc_visibility_result's shapes.  A candidate that
// filter_images removed from the model (`filtered`, 21.4) goes with the tried ones, as COLMAP's filtered_images_ does.
inline std::vector<uint32_t> RankNextImages(const FlatVisibility& f, const uint32_t* num_observations, const uint32_t* num_visible,
                                            const uint64_t* score, const MapperOptions& o, const MapperTrials& trials,
                                            const std::set<uint32_t>* filtered = nullptr) {
    std::vector<std::pair<uint32_t, float>> groups[2];
    for (size_t c = 0; c < f.cand_ids.size(); ++c) {
        if (static_cast<size_t>(num_visible[c]) < static_cast<size_t>(o.abs_pose_min_num_inliers)) continue;
        const auto t = trials.find(f.cand_ids[c]);
        const size_t tried = t == trials.end() ? 0 : static_cast<size_t>(t->second);
        if (tried >= static_cast<size_t>(o.max_reg_trials)) continue;
        float rank = 0.f;
        switch (o.image_selection_method) {
            case ImageSelectionMethod::MAX_VISIBLE_POINTS_NUM: rank = static_cast<float>(num_visible[c]); break;
            case ImageSelectionMethod::MAX_VISIBLE_POINTS_RATIO: rank = static_cast<float>(num_visible[c]) / static_cast<float>(num_observations[c]); break;
            case ImageSelectionMethod::MIN_UNCERTAINTY: rank = static_cast<float>(score[c]); break;
        }
        const bool was_filtered = filtered && filtered->count(f.cand_ids[c]);
        groups[tried == 0 && !was_filtered ? 0 : 1].emplace_back(f.cand_ids[c], rank);
    }
    std::vector<uint32_t> out;
    for (auto& g : groups) {
        std::sort(g.begin(), g.end(), [](const std::pair<uint32_t, float>& a, const std::pair<uint32_t, float>& b) {
            const bool an = a.second != a.second, bn = b.second != b.second;
            if (an != bn) return bn;  // NaN last
            if (!an && a.second != b.second) return a.second > b.second;
            return a.first < b.first;
        });
        for (const auto& e : g) out.push_back(e.first);
    }
    return out;
}

// ---- 20.2: RegisterNextImage ---------------------------------------------------------------------------------------------
struct RegistrationPairs {
    size_t num_visible = 0;             // the candidate's points2D with a correspondence that carries a point3D
    std::vector<uint32_t> point2D_idx;  // per pair
    std::vector<uint64_t> point3D_id;
    std::vector<double> points2D, points3D;  // 2 and 3 per pair
    size_t size() const { return point2D_idx.size(); }
};

// per point2D in order, per correspondence in the graph's order: into a model image, onto a point2D that carries a
// point3D this point2D has not paired with yet, through a camera that is not bogus (ix holds the mapper's thresholds)
inline RegistrationPairs CollectRegistrationPairs(const CorrespondenceGraph& graph, const SparseModel& m, const ModelIndex& ix, const MapperCandidate& c) {
    RegistrationPairs out;
    if (graph.NumPoints2D(c.image_id) != c.NumPoints2D())
        throw std::invalid_argument("register_next_image: candidate " + std::to_string(c.image_id) + " has " + std::to_string(c.NumPoints2D()) +
                                    " points2D, the graph gives it " + std::to_string(graph.NumPoints2D(c.image_id)));
    std::unordered_set<uint64_t> paired;
    for (size_t p = 0; p < c.NumPoints2D(); ++p) {
        paired.clear();
        bool visible = false;
        for (const Correspondence& corr : graph.ExtractCorrespondences(c.image_id, static_cast<uint32_t>(p))) {
            const auto mi = ix.image.find(corr.image_id);
            if (mi == ix.image.end()) continue;
            const ModelImage& other = m.images[mi->second];
            if (corr.point2D_idx >= other.points2D.size())
                throw std::invalid_argument("register_next_image: the graph names point2D " + std::to_string(corr.point2D_idx) + " of image " +
                                            std::to_string(corr.image_id) + ", which the reconstruction does not hold");
            const uint64_t pid = other.points2D[corr.point2D_idx].point3D_id;
            if (pid == kInvalidPoint3DId) continue;
            visible = true;
            if (paired.count(pid)) continue;
            if (ix.image_bogus[mi->second]) continue;
            const double* X = m.points3D[ix.point.at(pid)].xyz;
            paired.insert(pid);
            out.point2D_idx.push_back(static_cast<uint32_t>(p));
            out.point3D_id.push_back(pid);
            out.points2D.push_back(c.xy[2 * p]);
            out.points2D.push_back(c.xy[2 * p + 1]);
            out.points3D.insert(out.points3D.end(), X, X + 3);
        }
        out.num_visible += visible ? 1 : 0;
    }
    return out;
}

// COLMAP's rule for the estimation and refinement options (20.2)
struct RegistrationRule {
    bool camera_in_use = false;     // num_reg_images_per_camera > 0: a model image has this camera
    bool camera_bogus = false;
    bool estimate_focal_length = false;
    bool refine_focal_length = false;   // what COLMAP would have set; the refinement here never refines intrinsics (J5)
    bool refine_extra_params = false;
};
inline RegistrationRule PlanRegistration(const SparseModel& m, const ModelCamera& camera, bool has_prior_focal_length, const MapperOptions& o) {
    RegistrationRule r;
    for (const ModelImage& im : m.images) r.camera_in_use = r.camera_in_use || im.camera_id == camera.camera_id;
    r.camera_bogus = CameraHasBogusParams(camera, o.min_focal_length_ratio, o.max_focal_length_ratio, o.max_extra_param);
    if (r.camera_in_use && !r.camera_bogus) {
        r.estimate_focal_length = r.refine_focal_length = r.refine_extra_params = false;
    } else {
        r.estimate_focal_length = !has_prior_focal_length;
        r.refine_focal_length = r.refine_extra_params = true;
    }
    if (!o.abs_pose_refine_focal_length) r.estimate_focal_length = r.refine_focal_length = false;
    if (!o.abs_pose_refine_extra_params) r.refine_extra_params = false;
    return r;
}

// A successful registration into the model: the image with its pose (qvec x y z w) behind the others, the camera's focal
// lengths times focal_factor when the focal length was estimated, and every inlier pair whose point2D has no point yet
// onto its point3D, in pair order.  Returns the number of attached observations.  Throws std::invalid_argument when the
// mask does not fit.
inline size_t ApplyRegistration(const MapperCandidate& c, const RegistrationPairs& pairs, const uint8_t* inlier_mask, const double* qvec_xyzw,
                                const double* tvec, bool scale_focal, double focal_factor, SparseModel* m, ModelIndex* ix, std::set<uint64_t>* modified) {
    if (ix->image.count(c.image_id)) throw std::invalid_argument("register_next_image: image " + std::to_string(c.image_id) + " is in the reconstruction");
    ModelImage im;
    im.image_id = c.image_id;
    im.camera_id = c.camera_id;
    im.qvec[0] = qvec_xyzw[3];
    for (int k = 0; k < 3; ++k) im.qvec[1 + k] = qvec_xyzw[k];
    for (int k = 0; k < 3; ++k) im.tvec[k] = tvec[k];
    im.points2D.resize(c.NumPoints2D());
    for (size_t p = 0; p < c.NumPoints2D(); ++p) {
        im.points2D[p].x = c.xy[2 * p];
        im.points2D[p].y = c.xy[2 * p + 1];
    }
    size_t attached = 0;
    for (size_t i = 0; i < pairs.size(); ++i) {
        if (!inlier_mask[i]) continue;
        ModelPoint2D& p2 = im.points2D.at(pairs.point2D_idx[i]);
        if (p2.point3D_id != kInvalidPoint3DId) continue;
        const auto pt = ix->point.find(pairs.point3D_id[i]);
        if (pt == ix->point.end()) throw std::invalid_argument("register_next_image: a pair names a point3D the reconstruction does not hold");
        p2.point3D_id = pairs.point3D_id[i];
        m->points3D[pt->second].track.emplace_back(c.image_id, pairs.point2D_idx[i]);
        modified->insert(pairs.point3D_id[i]);
        attached += 1;
    }
    if (scale_focal) {
        ModelCamera& cam = m->cameras[ix->camera.at(c.camera_id)];
        const int nf = (cam.model == 0 || cam.model == 2 || cam.model == 3 || cam.model == 8 || cam.model == 9) ? 1 : 2;
        for (int k = 0; k < nf; ++k) cam.params[k] *= focal_factor;
    }
    ix->image[c.image_id] = m->images.size();
    ix->image_bogus.push_back(0);
    m->images.push_back(std::move(im));
    return attached;
}

// ---- 20.3: FindLocalBundle -----------------------------------------------------------------------------------------------
constexpr double kMapperDegToRad = 0.0174532925199432954743716805978692718781530857086181640625;

struct FlatBundle {
    std::vector<std::pair<uint32_t, size_t>> overlapping;  // (image id, shared observations), sorted
    size_t num_eff_images = 0;
    size_t num_points3D = 0;         // the image's points2D that carry a point
    bool all_taken = false;          // as many overlapping images as wanted: the list is the answer, no angles needed
    // the flat problem of amc_shared_point_angles: one pair per overlapping image that reaches the smallest overlap
    // threshold, in the sorted order (they are a prefix of `overlapping`)
    std::vector<double> qvec, tvec, point_xyz;
    std::vector<uint32_t> pair_images, shared_points;
    std::vector<uint64_t> pair_offsets{0};
    size_t NumPairs() const { return pair_offsets.size() - 1; }
    amc_pair_angle_problem Problem() const {
        amc_pair_angle_problem pb{};
        pb.num_images = tvec.size() / 3;
        pb.qvec = qvec.data();
        pb.tvec = tvec.data();
        pb.num_points = point_xyz.size() / 3;
        pb.point_xyz = point_xyz.data();
        pb.num_pairs = NumPairs();
        pb.pair_images = pair_images.data();
        pb.pair_offsets = pair_offsets.data();
        pb.shared_points = shared_points.data();
        return pb;
    }
};

// the eight (angle divisor, share of the image's points) rows of the selection
constexpr double kBundleAngleDivisor[8] = {1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0};
constexpr double kBundleShare[8] = {0.6, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.1};

inline FlatBundle PlanLocalBundle(const SparseModel& m, const ModelIndex& ix, const MapperOptions& o, uint32_t image_id,
                                  uint64_t max_pair_points = AMC_MAPPER_MAX_PAIR_POINTS) {
    const auto self = ix.image.find(image_id);
    if (self == ix.image.end()) throw std::invalid_argument("find_local_bundle: the reconstruction has no image " + std::to_string(image_id));
    const ModelImage& image = m.images[self->second];
    FlatBundle f;
    std::map<uint32_t, size_t> shared;
    std::unordered_map<uint64_t, uint32_t> point_index;  // the image's points, by first appearance
    for (const ModelPoint2D& p2 : image.points2D) {
        if (p2.point3D_id == kInvalidPoint3DId) continue;
        f.num_points3D += 1;
        const ModelPoint3D& pt = m.points3D[ix.point.at(p2.point3D_id)];
        if (point_index.emplace(p2.point3D_id, static_cast<uint32_t>(f.point_xyz.size() / 3)).second) f.point_xyz.insert(f.point_xyz.end(), pt.xyz, pt.xyz + 3);
        for (const auto& e : pt.track)
            if (e.first != image_id) shared[e.first] += 1;
    }
    f.overlapping.assign(shared.begin(), shared.end());  // ascending id; the stable sort keeps that among equal counts
    std::stable_sort(f.overlapping.begin(), f.overlapping.end(),
                     [](const std::pair<uint32_t, size_t>& a, const std::pair<uint32_t, size_t>& b) { return a.second > b.second; });
    const size_t num_images = static_cast<size_t>(o.local_ba_num_images - 1);
    f.num_eff_images = std::min(num_images, f.overlapping.size());
    f.all_taken = f.overlapping.size() == f.num_eff_images;
    if (f.all_taken) return f;
    // the image itself is pose 0
    auto add_pose = [&](const ModelImage& im) {
        for (int k = 0; k < 3; ++k) f.qvec.push_back(im.qvec[1 + k]);  // w x y z -> x y z w
        f.qvec.push_back(im.qvec[0]);
        for (int k = 0; k < 3; ++k) f.tvec.push_back(im.tvec[k]);
    };
    add_pose(image);
    const double least = kBundleShare[7] * static_cast<double>(f.num_points3D);
    for (const auto& ov : f.overlapping) {
        if (static_cast<double>(ov.second) < least) break;
        const auto oi = ix.image.find(ov.first);
        if (oi == ix.image.end()) throw std::invalid_argument("find_local_bundle: a track names image " + std::to_string(ov.first) + ", which the reconstruction does not hold");
        const ModelImage& other = m.images[oi->second];
        for (const ModelPoint2D& p2 : other.points2D) {
            if (p2.point3D_id == kInvalidPoint3DId) continue;
            const auto at = point_index.find(p2.point3D_id);
            if (at != point_index.end()) f.shared_points.push_back(at->second);
        }
        const uint64_t n = f.shared_points.size() - f.pair_offsets.back();
        if (n == 0) throw std::invalid_argument("find_local_bundle: image " + std::to_string(ov.first) + " is in a track of image " + std::to_string(image_id) +
                                                " but none of its points2D carries a shared point");
        if (n > max_pair_points)
            throw std::invalid_argument("find_local_bundle: images " + std::to_string(image_id) + " and " + std::to_string(ov.first) + " share " + std::to_string(n) +
                                        " points, more than " + std::to_string(max_pair_points) + " (AMC_MAPPER_MAX_PAIR_POINTS, DESIGN.md 20.5)");
        f.pair_images.push_back(0);
        f.pair_images.push_back(static_cast<uint32_t>(f.tvec.size() / 3));
        add_pose(other);
        f.pair_offsets.push_back(f.shared_points.size());
    }
    return f;
}

// COLMAP's loop over the eight thresholds and the fill-up, on the angles of the pairs (amc_pair_angle_result's shape)
inline std::vector<uint32_t> SelectLocalBundle(const FlatBundle& f, const MapperOptions& o, const double* angle) {
    std::vector<uint32_t> out;
    if (f.all_taken) {
        for (const auto& ov : f.overlapping) out.push_back(ov.first);
        return out;
    }
    const double min_tri_angle_rad = kMapperDegToRad * o.local_ba_min_tri_angle;
    std::vector<char> used(f.overlapping.size(), 0);
    for (int row = 0; row < 8 && out.size() < f.num_eff_images; ++row) {
        const double min_angle = min_tri_angle_rad / kBundleAngleDivisor[row];
        const double min_shared = kBundleShare[row] * static_cast<double>(f.num_points3D);
        for (size_t i = 0; i < f.overlapping.size(); ++i) {
            if (static_cast<double>(f.overlapping[i].second) < min_shared) break;
            if (used[i]) continue;
            if (i >= f.NumPairs()) throw std::invalid_argument("find_local_bundle: no angle for overlapping image " + std::to_string(f.overlapping[i].first));
            if (angle[i] >= min_angle) {  // NaN is not
                out.push_back(f.overlapping[i].first);
                used[i] = 1;
                if (out.size() >= f.num_eff_images) break;
            }
        }
    }
    for (size_t i = 0; i < f.overlapping.size() && out.size() < f.num_eff_images; ++i) {
        if (used[i]) continue;
        out.push_back(f.overlapping[i].first);
        used[i] = 1;
    }
    return out;
}

}  // namespace amchost
