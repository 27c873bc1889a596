// triangulator_host.h — the host half of IncrementalTriangulator::TriangulateImage on
// model_io's plain structs: the options and their check, Camera::HasBogusParams, Find for a run of points2D with
// pairwise disjoint observation sets, the flat problem of include/amc_triobs.h, and the way its result goes back into
// the model.  No Python and no HIP here: tests/shim/triangulator_host_fuzz.cc runs it under ASan + UBSan.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../../include/amc_triobs.h"
#include "correspondence_graph.h"
#include "model_io.h"

namespace amchost {

// IncrementalTriangulator::Options with COLMAP's defaults
struct TriangulatorOptions {
    int max_transitivity = 1;
    double create_max_angle_error = 2.0;
    double continue_max_angle_error = 2.0;
    double merge_max_reproj_error = 4.0;
    double complete_max_reproj_error = 4.0;
    int complete_max_transitivity = 5;
    double re_max_angle_error = 5.0;
    double re_min_ratio = 0.2;
    int re_max_trials = 1;
    double min_angle = 1.5;
    bool ignore_two_view_tracks = true;
    double min_focal_length_ratio = 0.1;
    double max_focal_length_ratio = 10.0;
    double max_extra_param = 1.0;
    // IncrementalTriangulator::Options::Check: the first condition that fails, or the empty string
    std::string Check() const {
        if (!(max_transitivity >= 0)) return "max_transitivity >= 0";
        if (!(create_max_angle_error > 0)) return "create_max_angle_error > 0";
        if (!(continue_max_angle_error > 0)) return "continue_max_angle_error > 0";
        if (!(merge_max_reproj_error > 0)) return "merge_max_reproj_error > 0";
        if (!(complete_max_reproj_error > 0)) return "complete_max_reproj_error > 0";
        if (!(complete_max_transitivity >= 0)) return "complete_max_transitivity >= 0";
        if (!(re_max_angle_error > 0)) return "re_max_angle_error > 0";
        if (!(re_min_ratio >= 0)) return "re_min_ratio >= 0";
        if (!(re_min_ratio <= 1)) return "re_min_ratio <= 1";
        if (!(re_max_trials >= 0)) return "re_max_trials >= 0";
        if (!(min_angle > 0)) return "min_angle > 0";
        return std::string();
    }
};

// Camera::HasBogusParams: a principal point outside the image, a focal length ratio outside the bounds or an extra
// parameter above the bound
inline bool CameraHasBogusParams(const ModelCamera& c, double min_focal_length_ratio, double max_focal_length_ratio,
                                 double max_extra_param) {
    const int n = ModelNumParams(c.model);
    if (n < 0 || c.params.size() != static_cast<size_t>(n)) return true;
    const int nf = (c.model == 0 || c.model == 2 || c.model == 3 || c.model == 8 || c.model == 9) ? 1 : 2;
    const double cx = c.params[nf], cy = c.params[nf + 1];
    if (cx < 0 || cx > static_cast<double>(c.width) || cy < 0 || cy > static_cast<double>(c.height)) return true;
    const double max_size = static_cast<double>(std::max(c.width, c.height));
    for (int i = 0; i < nf; ++i) {
        const double ratio = c.params[i] / max_size;
        if (ratio < min_focal_length_ratio || ratio > max_focal_length_ratio) return true;
    }
    for (int i = nf + 2; i < n; ++i)
        if (std::abs(c.params[i]) > max_extra_param) return true;
    return false;
}

// where a checked model's ids are, and which of its cameras are bogus under the options
struct ModelIndex {
    std::unordered_map<uint32_t, size_t> camera, image;
    std::unordered_map<uint64_t, size_t> point;
    std::vector<uint8_t> image_bogus;  // by image index: its camera is bogus
    uint64_t next_point3D_id = 1;      // Reconstruction.add_point3D's rule: one above the largest id, at least 1
    ModelIndex(const SparseModel& m, const TriangulatorOptions& o) {
        for (size_t i = 0; i < m.cameras.size(); ++i) camera[m.cameras[i].camera_id] = i;
        for (size_t i = 0; i < m.images.size(); ++i) {
            image[m.images[i].image_id] = i;
            const auto c = camera.find(m.images[i].camera_id);
            if (c == camera.end()) throw std::invalid_argument("image " + std::to_string(m.images[i].image_id) + " names a camera the model does not hold");
            image_bogus.push_back(CameraHasBogusParams(m.cameras[c->second], o.min_focal_length_ratio, o.max_focal_length_ratio, o.max_extra_param));
        }
        for (size_t i = 0; i < m.points3D.size(); ++i) {
            point[m.points3D[i].point3D_id] = i;
            next_point3D_id = std::max(next_point3D_id, m.points3D[i].point3D_id + 1);
        }
    }
};

// the flat problem of amc_triangulate_observations for one run, and the arrays it points into
struct FlatTriobs {
    std::vector<int32_t> camera_models;
    std::vector<double> camera_params, qvec, tvec, cand_xy, cand_xyz;
    std::vector<uint32_t> image_cameras, cand_image;
    std::vector<uint64_t> item_offsets{0};
    std::vector<uint8_t> cand_has_point, no_create_two_view;
    // what the write-back needs: every candidate's observation and point id, every item's point2D
    std::vector<Correspondence> cand_obs;
    std::vector<uint64_t> cand_point3D;
    uint32_t image_id = 0;
    std::vector<uint32_t> item_point2D;
    size_t NumItems() const { return item_offsets.size() - 1; }
    amc_triobs_problem Problem() const {
        amc_triobs_problem pb{};
        pb.num_cameras = camera_models.size();
        pb.camera_models = camera_models.data();
        pb.camera_params = camera_params.data();
        pb.num_images = image_cameras.size();
        pb.image_cameras = image_cameras.data();
        pb.qvec = qvec.data();
        pb.tvec = tvec.data();
        pb.num_items = NumItems();
        pb.item_offsets = item_offsets.data();
        pb.cand_image = cand_image.data();
        pb.cand_xy = cand_xy.data();
        pb.cand_has_point = cand_has_point.data();
        pb.cand_xyz = cand_xyz.data();
        pb.no_create_two_view = no_create_two_view.data();
        return pb;
    }
};

// The cameras and images of a checked model in its order (15.2 / 16.4), without items.
inline FlatTriobs FlattenModelForTriobs(const SparseModel& m, const ModelIndex& ix) {
    FlatTriobs f;
    for (const ModelCamera& c : m.cameras) {
        f.camera_models.push_back(c.model);
        for (size_t k = 0; k < 12; ++k) f.camera_params.push_back(k < c.params.size() ? c.params[k] : 0.0);
    }
    for (const ModelImage& im : m.images) {
        f.image_cameras.push_back(static_cast<uint32_t>(ix.camera.at(im.camera_id)));
        for (int k = 0; k < 3; ++k) f.qvec.push_back(im.qvec[1 + k]);  // w x y z -> x y z w
        f.qvec.push_back(im.qvec[0]);
        for (int k = 0; k < 3; ++k) f.tvec.push_back(im.tvec[k]);
    }
    return f;
}

// 17.4: Find for the points2D begin, begin + 1, .. of the image while their observation sets (the found
// correspondences and the reference observation) stay pairwise disjoint; a point2D without found correspondences is
// passed over.  Appends the run's items to `f` (whose items are cleared first) and returns the first point2D index that
// is not part of the run.  Throws std::invalid_argument for an image the model or the graph does not hold.
inline size_t PlanTriangulationRun(const CorrespondenceGraph& graph, const SparseModel& m, const ModelIndex& ix,
                                   const TriangulatorOptions& o, uint32_t image_id, size_t begin, FlatTriobs* f) {
    f->item_offsets.assign(1, 0);
    f->cand_image.clear();
    f->cand_xy.clear();
    f->cand_xyz.clear();
    f->cand_has_point.clear();
    f->no_create_two_view.clear();
    f->cand_obs.clear();
    f->cand_point3D.clear();
    f->item_point2D.clear();
    f->image_id = image_id;
    const auto self = ix.image.find(image_id);
    if (self == ix.image.end()) throw std::invalid_argument("triangulate_image: the reconstruction has no image " + std::to_string(image_id));
    const ModelImage& image = m.images[self->second];
    std::set<std::pair<uint32_t, uint32_t>> used;
    std::vector<Correspondence> found, kept;
    size_t p = begin;
    for (; p < image.points2D.size(); ++p) {
        graph.ExtractTransitiveCorrespondences(image_id, static_cast<uint32_t>(p), static_cast<size_t>(o.max_transitivity), &found);
        kept.clear();
        for (const Correspondence& c : found) {
            const auto it = ix.image.find(c.image_id);
            if (it == ix.image.end() || ix.image_bogus[it->second]) continue;
            if (c.point2D_idx >= m.images[it->second].points2D.size())
                throw std::invalid_argument("triangulate_image: the graph names point2D " + std::to_string(c.point2D_idx) + " of image " +
                                            std::to_string(c.image_id) + ", which the reconstruction does not hold");
            kept.push_back(c);
        }
        if (kept.empty()) continue;
        kept.emplace_back(image_id, static_cast<uint32_t>(p));
        bool overlap = false;
        for (const Correspondence& c : kept) overlap = overlap || used.count({c.image_id, c.point2D_idx}) != 0;
        if (overlap) break;  // the run ends in front of this point2D
        bool first_without = true, two_view = false;
        for (size_t k = 0; k < kept.size(); ++k) {
            const Correspondence& c = kept[k];
            used.insert({c.image_id, c.point2D_idx});
            const size_t ii = ix.image.at(c.image_id);
            const ModelPoint2D& p2 = m.images[ii].points2D[c.point2D_idx];
            const bool has = p2.point3D_id != kInvalidPoint3DId;
            if (!has && first_without && k + 1 < kept.size()) {
                first_without = false;
                two_view = o.ignore_two_view_tracks && graph.IsTwoViewObservation(c.image_id, c.point2D_idx);
            }
            f->cand_image.push_back(static_cast<uint32_t>(ii));
            f->cand_xy.push_back(p2.x);
            f->cand_xy.push_back(p2.y);
            f->cand_has_point.push_back(has ? 1 : 0);
            const double* X = has ? m.points3D[ix.point.at(p2.point3D_id)].xyz : nullptr;
            for (int d = 0; d < 3; ++d) f->cand_xyz.push_back(X ? X[d] : 0.0);
            f->cand_obs.push_back(c);
            f->cand_point3D.push_back(p2.point3D_id);
        }
        f->no_create_two_view.push_back(two_view ? 1 : 0);
        f->item_offsets.push_back(f->cand_image.size());
        f->item_point2D.push_back(static_cast<uint32_t>(p));
    }
    return p;
}

struct TriobsApplied {
    size_t num_tris = 0;  // TriangulateImage's return: continued observations plus the created tracks' lengths
    size_t num_created = 0, num_continued = 0;
};

// A run's result (arrays of the flat problem's sizes) into the model it was planned on, item by item and within an
// item in round order; the new ids go into `ix` and `modified`.  Throws std::invalid_argument when the result does not
// fit the problem.
inline TriobsApplied ApplyTriobsResult(const FlatTriobs& f, const int32_t* continued, const uint32_t* cand_round,
                                       const uint64_t* round_offsets, const double* round_xyz, SparseModel* m, ModelIndex* ix,
                                       std::set<uint64_t>* modified) {
    TriobsApplied out;
    const size_t image_index = ix->image.at(f.image_id);
    for (size_t i = 0; i < f.NumItems(); ++i) {
        const uint64_t c0 = f.item_offsets[i], n = f.item_offsets[i + 1] - c0;
        const uint32_t p = f.item_point2D[i];
        if (continued[i] >= 0) {
            if (static_cast<uint64_t>(continued[i]) + 1 >= n || !f.cand_has_point[c0 + continued[i]])
                throw std::invalid_argument("triangulate_image: the result continues item " + std::to_string(i) + " to a candidate without a point");
            const uint64_t pid = f.cand_point3D[c0 + continued[i]];
            ModelPoint2D& p2 = m->images[image_index].points2D[p];
            if (p2.point3D_id != kInvalidPoint3DId) throw std::invalid_argument("triangulate_image: the result continues a point2D that has a point");
            m->points3D[ix->point.at(pid)].track.emplace_back(f.image_id, p);
            p2.point3D_id = pid;
            modified->insert(pid);
            out.num_tris += 1;
            out.num_continued += 1;
        }
        const uint64_t nrounds = round_offsets[i + 1] - round_offsets[i];
        for (uint64_t r = 1; r <= nrounds; ++r) {
            ModelPoint3D pt;
            pt.point3D_id = ix->next_point3D_id;
            for (int d = 0; d < 3; ++d) pt.xyz[d] = round_xyz[3 * (round_offsets[i] + r - 1) + d];
            pt.error = -1.0;
            for (uint64_t k = 0; k < n; ++k) {
                if (cand_round[c0 + k] != r) continue;
                const Correspondence& c = f.cand_obs[c0 + k];
                ModelPoint2D& p2 = m->images[ix->image.at(c.image_id)].points2D[c.point2D_idx];
                if (p2.point3D_id != kInvalidPoint3DId) throw std::invalid_argument("triangulate_image: the result gives a second point to an observation");
                p2.point3D_id = pt.point3D_id;
                pt.track.emplace_back(c.image_id, c.point2D_idx);
            }
            if (pt.track.size() < 2) throw std::invalid_argument("triangulate_image: the result creates a track of fewer than two observations");
            out.num_tris += pt.track.size();
            out.num_created += 1;
            ix->point[pt.point3D_id] = m->points3D.size();
            ix->next_point3D_id += 1;
            modified->insert(pt.point3D_id);
            m->points3D.push_back(std::move(pt));
        }
    }
    return out;
}

}  // namespace amchost
