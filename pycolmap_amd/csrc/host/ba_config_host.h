// ba_config_host.h — COLMAP 3.9.1's BundleAdjustmentConfig and the set-up of BundleAdjuster::Solve on model_io's
// structs: which images, cameras, points and observations of a model take part in an adjustment of a
// part of it, what is constant, the flat problem of include/amc_ba.h with its point mask, and the write-back.  No Python
// and no HIP here (the binding in bind_bundle.cc calls amc_bundle_adjust_masked between Flatten and WriteBack):
// tests/shim/ba_config_host_fuzz.cc runs it under ASan + UBSan.  A failed COLMAP CHECK is a std::invalid_argument in the
// THROW_CHECK format (COLMAP aborts).
#pragma once

#include <cstdint>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "ba_host.h"
#include "model_io.h"
#include "reconstruction.h"

namespace amchost {

class BundleAdjustmentConfig {
  public:
    size_t NumImages() const { return image_ids_.size(); }
    size_t NumPoints() const { return variable_point3D_ids_.size() + constant_point3D_ids_.size(); }
    size_t NumConstantCamIntrinsics() const { return constant_intrinsics_.size(); }
    size_t NumConstantCamPoses() const { return constant_cam_poses_.size(); }
    size_t NumConstantCamPositions() const { return constant_cam_positions_.size(); }
    size_t NumVariablePoints() const { return variable_point3D_ids_.size(); }
    size_t NumConstantPoints() const { return constant_point3D_ids_.size(); }

    // twice the observations of the config's images plus those of the listed points in images outside the config
    // (COLMAP counts every point2D with a point; the single-element tracks of R3 are not taken off).  Throws
    // std::invalid_argument for an id the model does not hold.
    size_t NumResiduals(const SparseModel& m) const {
        size_t n = 0;
        std::set<uint32_t> found;
        for (const ModelImage& im : m.images) {
            if (!HasImage(im.image_id)) continue;
            found.insert(im.image_id);
            for (const ModelPoint2D& p : im.points2D) n += p.point3D_id != kInvalidPoint3DId;
        }
        if (found.size() != image_ids_.size()) Fail(__LINE__, "reconstruction.exists_image(image_id)");
        size_t points = 0;
        for (const ModelPoint3D& p : m.points3D) {
            if (!HasPoint(p.point3D_id)) continue;
            ++points;
            for (const auto& el : p.track) n += !HasImage(el.first);
        }
        if (points != NumPoints()) Fail(__LINE__, "reconstruction.exists_point3D(point3D_id)");
        return 2 * n;
    }

    void AddImage(uint32_t image_id) { image_ids_.insert(image_id); }
    bool HasImage(uint32_t image_id) const { return image_ids_.count(image_id) != 0; }
    void RemoveImage(uint32_t image_id) { image_ids_.erase(image_id); }

    void SetConstantCamIntrinsics(uint32_t camera_id) { constant_intrinsics_.insert(camera_id); }
    void SetVariableCamIntrinsics(uint32_t camera_id) { constant_intrinsics_.erase(camera_id); }
    bool IsConstantCamIntrinsics(uint32_t camera_id) const { return constant_intrinsics_.count(camera_id) != 0; }

    void SetConstantCamPose(uint32_t image_id) {
        if (!HasImage(image_id)) Fail(__LINE__, "HasImage(image_id)");
        if (HasConstantCamPositions(image_id)) Fail(__LINE__, "!HasConstantCamPositions(image_id)");
        constant_cam_poses_.insert(image_id);
    }
    void SetVariableCamPose(uint32_t image_id) { constant_cam_poses_.erase(image_id); }
    bool HasConstantCamPose(uint32_t image_id) const { return constant_cam_poses_.count(image_id) != 0; }

    void SetConstantCamPositions(uint32_t image_id, const std::vector<int>& idxs) {
        if (idxs.empty()) Fail(__LINE__, "idxs.size() > 0");
        if (idxs.size() > 3) Fail(__LINE__, "idxs.size() <= 3");
        if (!HasImage(image_id)) Fail(__LINE__, "HasImage(image_id)");
        if (HasConstantCamPose(image_id)) Fail(__LINE__, "!HasConstantCamPose(image_id)");
        for (size_t a = 0; a < idxs.size(); ++a) {
            if (idxs[a] < 0 || idxs[a] > 2) Fail(__LINE__, "idx >= 0 && idx < 3");
            for (size_t b = 0; b < a; ++b)
                if (idxs[a] == idxs[b]) Fail(__LINE__, "!VectorContainsDuplicateValues(idxs)");
        }
        constant_cam_positions_[image_id] = idxs;
    }
    void RemoveConstantCamPositions(uint32_t image_id) { constant_cam_positions_.erase(image_id); }
    bool HasConstantCamPositions(uint32_t image_id) const { return constant_cam_positions_.count(image_id) != 0; }
    const std::vector<int>& ConstantCamPositions(uint32_t image_id) const {
        const auto it = constant_cam_positions_.find(image_id);
        if (it == constant_cam_positions_.end()) Fail(__LINE__, "HasConstantCamPositions(image_id)");
        return it->second;
    }

    void AddVariablePoint(uint64_t point3D_id) {
        if (HasConstantPoint(point3D_id)) Fail(__LINE__, "!HasConstantPoint(point3D_id)");
        variable_point3D_ids_.insert(point3D_id);
    }
    void AddConstantPoint(uint64_t point3D_id) {
        if (HasVariablePoint(point3D_id)) Fail(__LINE__, "!HasVariablePoint(point3D_id)");
        constant_point3D_ids_.insert(point3D_id);
    }
    bool HasPoint(uint64_t point3D_id) const { return HasVariablePoint(point3D_id) || HasConstantPoint(point3D_id); }
    bool HasVariablePoint(uint64_t point3D_id) const { return variable_point3D_ids_.count(point3D_id) != 0; }
    bool HasConstantPoint(uint64_t point3D_id) const { return constant_point3D_ids_.count(point3D_id) != 0; }
    void RemoveVariablePoint(uint64_t point3D_id) { variable_point3D_ids_.erase(point3D_id); }
    void RemoveConstantPoint(uint64_t point3D_id) { constant_point3D_ids_.erase(point3D_id); }

    // ascending ids (COLMAP's sets are unordered)
    const std::set<uint32_t>& Images() const { return image_ids_; }
    const std::set<uint32_t>& ConstantIntrinsics() const { return constant_intrinsics_; }
    const std::set<uint32_t>& ConstantCamPoses() const { return constant_cam_poses_; }
    const std::map<uint32_t, std::vector<int>>& AllConstantCamPositions() const { return constant_cam_positions_; }
    const std::set<uint64_t>& VariablePoints() const { return variable_point3D_ids_; }
    const std::set<uint64_t>& ConstantPoints() const { return constant_point3D_ids_; }

  private:
    [[noreturn]] static void Fail(int line, const std::string& expr) {
        throw std::invalid_argument("[ba_config_host.h:" + std::to_string(line) + "] Check Failed: " + expr);
    }
    std::set<uint32_t> image_ids_, constant_intrinsics_, constant_cam_poses_;
    std::map<uint32_t, std::vector<int>> constant_cam_positions_;
    std::set<uint64_t> variable_point3D_ids_, constant_point3D_ids_;
};

// the flat problem of a config, the point mask of amc_bundle_adjust_masked, and where each entry came from
struct FlatBaConfig {
    FlatBa flat;
    std::vector<uint8_t> point_const;   // per flat point
    std::vector<uint32_t> camera_at, image_at;  // per flat camera / image: its index in the model
    std::vector<size_t> point_at;               // per flat point: its index in the model
    size_t skipped_points = 0;                  // single-element tracks left out (R3)
    size_t num_constant_points = 0;
};

// BundleAdjuster::SetUp on a checked model (throws std::invalid_argument otherwise, and for a config
// id the model does not hold).  The flat images are the config's images that have an observation, in the model's order,
// then the images outside the config that a listed point pulls in, in the order they are met; the flat cameras and points
// follow the model's order; the observations are the config images' points2D image by image, then the outside elements
// of the listed points (variable first, then constant, each list in the model's order) in track order.  The config is
// not modified (COLMAP writes the pulled-in cameras into it as constant).
inline FlatBaConfig FlattenForBundleAdjuster(const SparseModel& m, const BundleAdjustmentConfig& cfg, const BaRefineFlags& f) {
    const std::string bad = CheckModel(m);
    if (!bad.empty()) throw std::invalid_argument("BundleAdjuster: " + bad);
    auto missing = [](const char* what, uint64_t id) {
        return std::invalid_argument(std::string("BundleAdjuster: the reconstruction has no ") + what + " " + std::to_string(id));
    };
    std::unordered_map<uint32_t, uint32_t> cam_of, img_of;
    std::unordered_map<uint64_t, size_t> pt_of;
    for (size_t c = 0; c < m.cameras.size(); ++c) cam_of[m.cameras[c].camera_id] = static_cast<uint32_t>(c);
    for (size_t i = 0; i < m.images.size(); ++i) img_of[m.images[i].image_id] = static_cast<uint32_t>(i);
    for (size_t j = 0; j < m.points3D.size(); ++j) pt_of[m.points3D[j].point3D_id] = j;
    for (uint32_t id : cfg.Images())
        if (!img_of.count(id)) throw missing("image", id);
    for (uint64_t id : cfg.VariablePoints())
        if (!pt_of.count(id)) throw missing("point3D", id);
    for (uint64_t id : cfg.ConstantPoints())
        if (!pt_of.count(id)) throw missing("point3D", id);

    // who takes part: (model image, model point, pixel) per residual pair; residual counts per point
    struct Obs {
        uint32_t image;
        size_t point;
        double x, y;
    };
    std::vector<Obs> obs;
    std::vector<uint32_t> images_in;                    // model indices in flat order
    std::vector<uint8_t> image_used(m.images.size(), 0), camera_used(m.cameras.size(), 0), camera_pulled(m.cameras.size(), 0);
    std::vector<size_t> nres(m.points3D.size(), 0);
    std::vector<uint8_t> skipped(m.points3D.size(), 0);
    // 1. the config's images
    for (size_t i = 0; i < m.images.size(); ++i) {
        const ModelImage& im = m.images[i];
        if (!cfg.HasImage(im.image_id)) continue;
        size_t n = 0;
        for (const ModelPoint2D& p2 : im.points2D) {
            if (p2.point3D_id == kInvalidPoint3DId) continue;
            const size_t j = pt_of.at(p2.point3D_id);
            if (m.points3D[j].track.size() < 2) {  // R3
                skipped[j] = 1;
                continue;
            }
            obs.push_back({static_cast<uint32_t>(i), j, p2.x, p2.y});
            ++nres[j];
            ++n;
        }
        if (n) {
            image_used[i] = 1;
            images_in.push_back(static_cast<uint32_t>(i));
            camera_used[cam_of.at(im.camera_id)] = 1;
        }
    }
    // 2. the listed points: their elements in images outside the config, through constant poses
    auto add_point = [&](size_t j) {
        const ModelPoint3D& p = m.points3D[j];
        if (p.track.size() < 2) {
            skipped[j] = 1;
            return;
        }
        if (nres[j] == p.track.size()) return;
        for (const auto& el : p.track) {
            if (cfg.HasImage(el.first)) continue;
            const uint32_t i = img_of.at(el.first);
            const ModelPoint2D& p2 = m.images[i].points2D.at(el.second);
            obs.push_back({i, j, p2.x, p2.y});
            ++nres[j];
            if (!image_used[i]) {
                image_used[i] = 1;
                images_in.push_back(i);
            }
            const uint32_t c = cam_of.at(m.images[i].camera_id);
            if (!camera_used[c]) {
                camera_used[c] = 1;
                camera_pulled[c] = 1;  // COLMAP: config_.SetConstantCamIntrinsics(camera_id)
            }
        }
    };
    for (size_t j = 0; j < m.points3D.size(); ++j)
        if (cfg.HasVariablePoint(m.points3D[j].point3D_id)) add_point(j);
    for (size_t j = 0; j < m.points3D.size(); ++j)
        if (cfg.HasConstantPoint(m.points3D[j].point3D_id)) add_point(j);

    FlatBaConfig out;
    FlatBa& o = out.flat;
    // 3. the cameras
    std::vector<uint32_t> flat_cam(m.cameras.size(), 0), flat_img(m.images.size(), 0);
    const bool constant_camera = !f.refine_focal_length && !f.refine_principal_point && !f.refine_extra_params;
    for (size_t c = 0; c < m.cameras.size(); ++c) {
        if (!camera_used[c]) continue;
        const ModelCamera& cam = m.cameras[c];
        flat_cam[c] = static_cast<uint32_t>(o.camera_models.size());
        out.camera_at.push_back(static_cast<uint32_t>(c));
        o.camera_models.push_back(cam.model);
        const bool all_const = constant_camera || camera_pulled[c] || cfg.IsConstantCamIntrinsics(cam.camera_id);
        const int nf = ModelNumFocal(cam.model), np = static_cast<int>(cam.params.size());
        for (int k = 0; k < 12; ++k) {
            o.camera_params.push_back(k < np ? cam.params[k] : 0.0);
            const bool refine = k >= np || all_const ? false : k < nf ? f.refine_focal_length : k < nf + 2 ? f.refine_principal_point : f.refine_extra_params;
            o.camera_const.push_back(refine ? 0 : 1);
        }
    }
    for (uint32_t i : images_in) {
        const ModelImage& im = m.images[i];
        flat_img[i] = static_cast<uint32_t>(o.image_cameras.size());
        out.image_at.push_back(i);
        o.image_cameras.push_back(flat_cam[cam_of.at(im.camera_id)]);
        o.qvec.insert(o.qvec.end(), {im.qvec[1], im.qvec[2], im.qvec[3], im.qvec[0]});  // x y z w
        o.tvec.insert(o.tvec.end(), im.tvec, im.tvec + 3);
        uint8_t pc[6] = {0, 0, 0, 0, 0, 0};
        if (!cfg.HasImage(im.image_id) || !f.refine_extrinsics || cfg.HasConstantCamPose(im.image_id)) {
            for (int k = 0; k < 6; ++k) pc[k] = 1;
        } else if (cfg.HasConstantCamPositions(im.image_id)) {
            for (int k : cfg.ConstantCamPositions(im.image_id)) pc[3 + k] = 1;
        }
        o.pose_const.insert(o.pose_const.end(), pc, pc + 6);
    }
    // 4. the points
    std::vector<uint32_t> flat_pt(m.points3D.size(), 0);
    for (size_t j = 0; j < m.points3D.size(); ++j) {
        out.skipped_points += skipped[j];
        if (!nres[j]) continue;
        const ModelPoint3D& p = m.points3D[j];
        flat_pt[j] = static_cast<uint32_t>(out.point_at.size());
        out.point_at.push_back(j);
        o.xyz.insert(o.xyz.end(), p.xyz, p.xyz + 3);
        const bool constant = p.track.size() > nres[j] || cfg.HasConstantPoint(p.point3D_id);
        out.point_const.push_back(constant ? 1 : 0);
        out.num_constant_points += constant;
    }
    for (const Obs& ob : obs) {
        o.obs_image.push_back(flat_img[ob.image]);
        o.obs_point.push_back(flat_pt[ob.point]);
        o.obs_xy.push_back(ob.x);
        o.obs_xy.push_back(ob.y);
    }
    return out;
}

// the refined arrays back into the model the problem was flattened from: only what was in the problem is written
inline void WriteBackBundleAdjuster(const FlatBaConfig& fc, SparseModel* m) {
    const FlatBa& o = fc.flat;
    auto changed = []() { return std::invalid_argument("BundleAdjuster: the model changed between flattening and write-back"); };
    if (fc.camera_at.size() != o.camera_models.size() || fc.image_at.size() != o.image_cameras.size() ||
        3 * fc.point_at.size() != o.xyz.size() || o.camera_params.size() != 12 * o.camera_models.size() ||
        o.qvec.size() != 4 * o.image_cameras.size() || o.tvec.size() != 3 * o.image_cameras.size())
        throw changed();
    for (size_t c = 0; c < fc.camera_at.size(); ++c) {
        if (fc.camera_at[c] >= m->cameras.size()) throw changed();
        ModelCamera& cam = m->cameras[fc.camera_at[c]];
        for (size_t k = 0; k < cam.params.size() && k < 12; ++k) cam.params[k] = o.camera_params[12 * c + k];
    }
    for (size_t i = 0; i < fc.image_at.size(); ++i) {
        if (fc.image_at[i] >= m->images.size()) throw changed();
        ModelImage& im = m->images[fc.image_at[i]];
        im.qvec[0] = o.qvec[4 * i + 3];
        for (int k = 0; k < 3; ++k) im.qvec[1 + k] = o.qvec[4 * i + k];
        for (int k = 0; k < 3; ++k) im.tvec[k] = o.tvec[3 * i + k];
    }
    for (size_t j = 0; j < fc.point_at.size(); ++j) {
        if (fc.point_at[j] >= m->points3D.size()) throw changed();
        for (int k = 0; k < 3; ++k) m->points3D[fc.point_at[j]].xyz[k] = o.xyz[3 * j + k];
    }
}

}  // namespace amchost
