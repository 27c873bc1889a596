// ba_host.h — bundle_adjustment's controller on model_io's structs: which parameters are constant, the
// flat problem of include/amc_ba.h, and the write-back.  No Python and no HIP here (the binding in bind_bundle.cc calls
// amc_bundle_adjust between Flatten and WriteBack): tests/shim/ba_host_fuzz.cc runs it under ASan + UBSan.
#pragma once

#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/amc_ba.h"
#include "model_io.h"
#include "reconstruction.h"

namespace amchost {

struct BaRefineFlags {
    bool refine_focal_length = true, refine_principal_point = false, refine_extra_params = true, refine_extrinsics = true;
};

// the flat problem and the arrays it points into
struct FlatBa {
    std::vector<int32_t> camera_models;
    std::vector<double> camera_params, qvec, tvec, xyz, obs_xy;
    std::vector<uint8_t> camera_const, pose_const;
    std::vector<uint32_t> image_cameras, obs_image, obs_point;
    amc_ba_problem Problem() {
        amc_ba_problem p{};
        p.num_cameras = camera_models.size();
        p.camera_models = camera_models.data();
        p.camera_params = camera_params.data();
        p.camera_const = camera_const.data();
        p.num_images = image_cameras.size();
        p.image_cameras = image_cameras.data();
        p.qvec = qvec.data();
        p.tvec = tvec.data();
        p.pose_const = pose_const.data();
        p.num_points = xyz.size() / 3;
        p.xyz = xyz.data();
        p.num_observations = obs_image.size();
        p.obs_image = obs_image.data();
        p.obs_point = obs_point.data();
        p.obs_xy = obs_xy.data();
        return p;
    }
};

// one focal length (params[0]) or two; the principal point follows; the rest are the extra parameters
inline int ModelNumFocal(int model) { return (model == 0 || model == 2 || model == 3 || model == 8 || model == 9) ? 1 : 2; }

// Flattens a checked model (CheckModel(m) is empty; throws std::invalid_argument otherwise).  Cameras, images and points
// keep the model's order; the observations are the tracks' elements, point by point.  Constant: the first image's
// pose, the second image's x translation, every pose without refine_extrinsics; a camera parameter unless its group's
// flag is set.  A point whose track has fewer than two elements is left out with its observations (it cannot be
// refined); `skipped_points` counts them.
inline FlatBa FlattenForBundleAdjustment(const SparseModel& m, const BaRefineFlags& f, size_t* skipped_points) {
    const std::string bad = CheckModel(m);
    if (!bad.empty()) throw std::invalid_argument("bundle_adjustment: " + bad);
    FlatBa o;
    std::unordered_map<uint32_t, uint32_t> cam_index, img_index;
    for (const ModelCamera& c : m.cameras) {
        cam_index[c.camera_id] = static_cast<uint32_t>(o.camera_models.size());
        o.camera_models.push_back(c.model);
        const int nf = ModelNumFocal(c.model), np = static_cast<int>(c.params.size());
        for (int k = 0; k < 12; ++k) {
            o.camera_params.push_back(k < np ? c.params[k] : 0.0);
            const bool refine = k >= np ? false : k < nf ? f.refine_focal_length : k < nf + 2 ? f.refine_principal_point : f.refine_extra_params;
            o.camera_const.push_back(refine ? 0 : 1);
        }
    }
    for (const ModelImage& im : m.images) {
        const uint32_t i = static_cast<uint32_t>(o.image_cameras.size());
        img_index[im.image_id] = i;
        o.image_cameras.push_back(cam_index.at(im.camera_id));
        o.qvec.insert(o.qvec.end(), {im.qvec[1], im.qvec[2], im.qvec[3], im.qvec[0]});  // x y z w
        o.tvec.insert(o.tvec.end(), im.tvec, im.tvec + 3);
        for (int k = 0; k < 6; ++k) o.pose_const.push_back(!f.refine_extrinsics || i == 0 || (i == 1 && k == 3) ? 1 : 0);
    }
    size_t skipped = 0;
    for (const ModelPoint3D& p : m.points3D) {
        if (p.track.size() < 2) {
            ++skipped;
            continue;
        }
        const uint32_t j = static_cast<uint32_t>(o.xyz.size() / 3);
        o.xyz.insert(o.xyz.end(), p.xyz, p.xyz + 3);
        for (const auto& el : p.track) {
            const uint32_t i = img_index.at(el.first);
            const ModelPoint2D& p2 = m.images[i].points2D.at(el.second);
            o.obs_image.push_back(i);
            o.obs_point.push_back(j);
            o.obs_xy.push_back(p2.x);
            o.obs_xy.push_back(p2.y);
        }
    }
    if (skipped_points) *skipped_points = skipped;
    return o;
}

// the refined arrays back into the model the problem was flattened from
inline void WriteBackBundleAdjustment(const FlatBa& o, SparseModel* m) {
    if (o.camera_models.size() != m->cameras.size() || o.image_cameras.size() != m->images.size())
        throw std::invalid_argument("bundle_adjustment: the model changed between flattening and write-back");
    for (size_t c = 0; c < m->cameras.size(); ++c)
        for (size_t k = 0; k < m->cameras[c].params.size() && k < 12; ++k) m->cameras[c].params[k] = o.camera_params[12 * c + k];
    for (size_t i = 0; i < m->images.size(); ++i) {
        ModelImage& im = m->images[i];
        im.qvec[0] = o.qvec[4 * i + 3];
        for (int k = 0; k < 3; ++k) im.qvec[1 + k] = o.qvec[4 * i + k];
        for (int k = 0; k < 3; ++k) im.tvec[k] = o.tvec[3 * i + k];
    }
    size_t j = 0;
    for (ModelPoint3D& p : m->points3D) {
        if (p.track.size() < 2) continue;
        if (3 * j + 3 > o.xyz.size()) throw std::invalid_argument("bundle_adjustment: the model changed between flattening and write-back");
        for (int k = 0; k < 3; ++k) p.xyz[k] = o.xyz[3 * j + k];
        ++j;
    }
}

}  // namespace amchost
