// initial_pair_host.h — the host halves of IncrementalMapper::RegisterInitialImagePair, AdjustGlobalBundle (with
// Reconstruction::Normalize) and FilterImages on model_io's plain structs: the verdict on the initial
// two-view geometry, the flat problem of include/amc_initpair.h for one pair and the way its result goes into the model,
// the configuration of the global adjustment, the normalisation, and the removal of images.  No Python and no HIP here:
// tests/shim/initial_pair_host_fuzz.cc runs it under ASan + UBSan.
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/amc_initpair.h"
#include "ba_config_host.h"
#include "correspondence_graph.h"
#include "mapper_host.h"
#include "model_io.h"
#include "triangulator_host.h"

namespace amchost {

// ---- 21.1: RegisterInitialImagePair ----------------------------------------------------------------------------------------
// EstimateInitialTwoViewGeometry's verdict on the geometry after the pose step (NaN fails every comparison)
inline bool InitialPairAccepted(bool pose_ok, size_t num_inliers, double tz, double tri_angle, const MapperOptions& o) {
    return pose_ok && num_inliers >= static_cast<size_t>(o.init_min_num_inliers) && std::abs(tz) < o.init_max_forward_motion &&
           tri_angle > kMapperDegToRad * o.init_min_tri_angle;
}

// the flat problem of amc_triangulate_pairs for one pair, and the arrays it points into
struct FlatInitialPair {
    std::vector<int32_t> camera_models;
    std::vector<double> camera_params, qvec, tvec, corr_xy1, corr_xy2;
    std::vector<uint32_t> image_cameras, pair_images, corrs;  // corrs: 2 per correspondence, the graph's point2D indices
    std::vector<uint64_t> pair_offsets{0};
    size_t NumCorrs() const { return corrs.size() / 2; }
    amc_pair_tri_problem Problem() const {
        amc_pair_tri_problem pb{};
        pb.num_cameras = camera_models.size();
        pb.camera_models = camera_models.data();
        pb.camera_params = camera_params.data();
        pb.num_images = image_cameras.size();
        pb.image_cameras = image_cameras.data();
        pb.qvec = qvec.data();
        pb.tvec = tvec.data();
        pb.num_pairs = pair_offsets.size() - 1;
        pb.pair_images = pair_images.data();
        pb.pair_offsets = pair_offsets.data();
        pb.corr_xy1 = corr_xy1.data();
        pb.corr_xy2 = corr_xy2.data();
        return pb;
    }
};

// Image 1 at the identity, image 2 at cam2_from_cam1 (qvec x y z w), every correspondence the graph holds between them in
// the graph's order.  `matches` is FindCorrespondencesBetweenImages' result (2 per correspondence).  Throws
// std::invalid_argument for a camera of an unknown model or a correspondence onto a point2D a candidate does not hold.
inline FlatInitialPair PlanInitialPair(const ModelCamera& cam1, const ModelCamera& cam2, const MapperCandidate& c1, const MapperCandidate& c2,
                                       const std::vector<uint32_t>& matches, const double* q2_xyzw, const double* t2) {
    FlatInitialPair f;
    for (const ModelCamera* c : {&cam1, &cam2}) {
        const int n = ModelNumParams(c->model);
        if (n < 0 || c->params.size() != static_cast<size_t>(n) || n > 12)
            throw std::invalid_argument("register_initial_image_pair: camera " + std::to_string(c->camera_id) + " has an unknown model or the wrong number of parameters");
        f.camera_models.push_back(c->model);
        f.camera_params.insert(f.camera_params.end(), c->params.begin(), c->params.end());
        f.camera_params.resize(12 * f.camera_models.size(), 0.0);
    }
    f.image_cameras = {0, 1};
    f.qvec = {0, 0, 0, 1, q2_xyzw[0], q2_xyzw[1], q2_xyzw[2], q2_xyzw[3]};
    f.tvec = {0, 0, 0, t2[0], t2[1], t2[2]};
    f.pair_images = {0, 1};
    for (size_t k = 0; k + 1 < matches.size(); k += 2) {
        const uint32_t a = matches[k], b = matches[k + 1];
        if (a >= c1.NumPoints2D() || b >= c2.NumPoints2D())
            throw std::invalid_argument("register_initial_image_pair: the graph names point2D " + std::to_string(a >= c1.NumPoints2D() ? a : b) +
                                        " of image " + std::to_string(a >= c1.NumPoints2D() ? c1.image_id : c2.image_id) + ", which the candidate does not hold");
        f.corrs.push_back(a);
        f.corrs.push_back(b);
        f.corr_xy1.push_back(c1.xy[2 * a]);
        f.corr_xy1.push_back(c1.xy[2 * a + 1]);
        f.corr_xy2.push_back(c2.xy[2 * b]);
        f.corr_xy2.push_back(c2.xy[2 * b + 1]);
    }
    f.pair_offsets.push_back(f.NumCorrs());
    return f;
}

// A successful initial pair into the model: both images behind the others with the poses of `f`, then one point3D with a
// two-element track per accepted correspondence, in correspondence order, ids counting up from ix's next id.  A
// correspondence onto a point2D that an earlier one gave a point is skipped (the graph holds every observation pair
// once, so this does not happen with a CorrespondenceGraph's output).  Returns the number of points created.
inline size_t ApplyInitialPair(const MapperCandidate& c1, const MapperCandidate& c2, const FlatInitialPair& f, const uint8_t* accepted, const double* xyz,
                               SparseModel* m, ModelIndex* ix) {
    if (ix->image.count(c1.image_id) || ix->image.count(c2.image_id) || c1.image_id == c2.image_id)
        throw std::invalid_argument("register_initial_image_pair: an image of the pair is in the reconstruction, or both are one image");
    const MapperCandidate* cands[2] = {&c1, &c2};
    for (int s = 0; s < 2; ++s) {
        const MapperCandidate& c = *cands[s];
        ModelImage im;
        im.image_id = c.image_id;
        im.camera_id = c.camera_id;
        im.qvec[0] = f.qvec[4 * s + 3];
        for (int k = 0; k < 3; ++k) im.qvec[1 + k] = f.qvec[4 * s + k];
        for (int k = 0; k < 3; ++k) im.tvec[k] = f.tvec[3 * s + k];
        im.points2D.resize(c.NumPoints2D());
        for (size_t p = 0; p < c.NumPoints2D(); ++p) {
            im.points2D[p].x = c.xy[2 * p];
            im.points2D[p].y = c.xy[2 * p + 1];
        }
        ix->image[c.image_id] = m->images.size();
        ix->image_bogus.push_back(0);
        m->images.push_back(std::move(im));
    }
    ModelImage& im1 = m->images[m->images.size() - 2];
    ModelImage& im2 = m->images[m->images.size() - 1];
    size_t created = 0;
    for (size_t k = 0; k < f.NumCorrs(); ++k) {
        if (!accepted[k]) continue;
        ModelPoint2D& p1 = im1.points2D.at(f.corrs[2 * k]);
        ModelPoint2D& p2 = im2.points2D.at(f.corrs[2 * k + 1]);
        if (p1.point3D_id != kInvalidPoint3DId || p2.point3D_id != kInvalidPoint3DId) continue;
        ModelPoint3D pt;
        pt.point3D_id = ix->next_point3D_id++;
        for (int i = 0; i < 3; ++i) pt.xyz[i] = xyz[3 * k + i];
        pt.error = -1.0;
        pt.track.emplace_back(c1.image_id, f.corrs[2 * k]);
        pt.track.emplace_back(c2.image_id, f.corrs[2 * k + 1]);
        p1.point3D_id = p2.point3D_id = pt.point3D_id;
        ix->point[pt.point3D_id] = m->points3D.size();
        m->points3D.push_back(std::move(pt));
        created += 1;
    }
    return created;
}

// ---- 21.3: AdjustGlobalBundle ----------------------------------------------------------------------------------------------
// every registered image; with fix_existing_images the images of `existing` keep their poses; the first registered image
// keeps its pose and the second its x position unless its pose is constant already (the seven degrees of the gauge)
inline BundleAdjustmentConfig GlobalBundleConfig(const std::vector<uint32_t>& reg_image_ids, const std::set<uint32_t>& existing, bool fix_existing_images) {
    if (reg_image_ids.size() < 2) throw std::invalid_argument("adjust_global_bundle: at least two registered images are needed");
    BundleAdjustmentConfig c;
    for (uint32_t id : reg_image_ids) c.AddImage(id);
    if (fix_existing_images)
        for (uint32_t id : reg_image_ids)
            if (existing.count(id)) c.SetConstantCamPose(id);
    if (!c.HasConstantCamPose(reg_image_ids[0])) c.SetConstantCamPose(reg_image_ids[0]);
    if (!c.HasConstantCamPose(reg_image_ids[1])) c.SetConstantCamPositions(reg_image_ids[1], {0});
    return c;
}

// rotation matrix of a quaternion w x y z, row-major, with 11.1's arithmetic
inline void RotationMatrix(const double* q_wxyz, double* R) {
    const double w = q_wxyz[0], x = q_wxyz[1], y = q_wxyz[2], z = q_wxyz[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double M[9] = {1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)};
    std::copy(M, M + 9, R);
}

struct NormalizeResult {
    bool applied = false;  // false: fewer than two images, nothing changed
    double scale = 1.0;
    double centroid[3] = {0, 0, 0};
};

// Reconstruction::Normalize(extent, p0, p1, use_images = true) over the images of reg_image_ids (21.3): the projection
// centres as floats, sorted per axis; the box between the elements of rank trunc(p0 (n - 1)) and trunc(p1 (n - 1)) (the
// whole range up to three images), the centroid the mean of the elements between them; scale = extent / |box diagonal|,
// 1 when the diagonal is below DBL_EPSILON; every pose t' = scale (t + R centroid), every point X' = scale X - scale
// centroid.  Rotations keep their bits.  Ids of reg_image_ids the model does not hold throw std::invalid_argument.
inline NormalizeResult NormalizeModel(SparseModel* m, const std::vector<uint32_t>& reg_image_ids, double extent = 10.0, double p0 = 0.1, double p1 = 0.9) {
    NormalizeResult out;
    if (!(extent > 0.0) || !(p0 >= 0.0 && p0 <= 1.0) || !(p1 >= 0.0 && p1 <= 1.0) || !(p0 <= p1)) throw std::invalid_argument("normalize: extent > 0 and 0 <= p0 <= p1 <= 1");
    if (reg_image_ids.size() < 2) return out;
    std::unordered_map<uint32_t, size_t> at;
    for (size_t i = 0; i < m->images.size(); ++i) at[m->images[i].image_id] = i;
    std::vector<float> coords[3];
    for (uint32_t id : reg_image_ids) {
        const auto it = at.find(id);
        if (it == at.end()) throw std::invalid_argument("normalize: the reconstruction has no image " + std::to_string(id));
        const ModelImage& im = m->images[it->second];
        double R[9];
        RotationMatrix(im.qvec, R);
        for (int c = 0; c < 3; ++c) coords[c].push_back(static_cast<float>(-(R[c] * im.tvec[0] + R[3 + c] * im.tvec[1] + R[6 + c] * im.tvec[2])));
    }
    const size_t n = coords[0].size();
    // (NaN centres: the order of std::sort on them is unspecified, as it is in COLMAP; they sort last here)
    for (auto& v : coords) std::sort(v.begin(), v.end(), [](float a, float b) { return b != b ? a == a : a < b; });
    const size_t P0 = n > 3 ? static_cast<size_t>(p0 * static_cast<double>(n - 1)) : 0;
    const size_t P1 = n > 3 ? static_cast<size_t>(p1 * static_cast<double>(n - 1)) : n - 1;
    double lo[3], hi[3], mean[3];
    for (int c = 0; c < 3; ++c) {
        lo[c] = coords[c][P0];
        hi[c] = coords[c][P1];
        mean[c] = 0.0;
        for (size_t i = P0; i <= P1; ++i) mean[c] += static_cast<double>(coords[c][i]);
        mean[c] /= static_cast<double>(P1 - P0 + 1);
    }
    const double d0 = hi[0] - lo[0], d1 = hi[1] - lo[1], d2 = hi[2] - lo[2];
    const double old_extent = std::sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    const double scale = old_extent < DBL_EPSILON ? 1.0 : extent / old_extent;  // (a NaN extent scales by NaN, as in COLMAP)
    out.applied = true;
    out.scale = scale;
    for (int c = 0; c < 3; ++c) out.centroid[c] = mean[c];
    for (ModelImage& im : m->images) {
        double R[9];
        RotationMatrix(im.qvec, R);
        for (int r = 0; r < 3; ++r) im.tvec[r] = (im.tvec[r] + (R[3 * r] * mean[0] + R[3 * r + 1] * mean[1] + R[3 * r + 2] * mean[2])) * scale;
    }
    for (ModelPoint3D& p : m->points3D)
        for (int c = 0; c < 3; ++c) p.xyz[c] = scale * p.xyz[c] + -(scale * mean[c]);
    return out;
}

// ---- 21.4: FilterImages ----------------------------------------------------------------------------------------------------
constexpr size_t kFilterImagesMinNumImages = 20;

// the registered images FilterImages removes, in reg_image_ids' order: those without a point3D and those whose camera is
// bogus under the options; nothing below kFilterImagesMinNumImages registered images
inline std::vector<uint32_t> PlanFilterImages(const SparseModel& m, const std::vector<uint32_t>& reg_image_ids, const MapperOptions& o) {
    std::vector<uint32_t> out;
    if (reg_image_ids.size() < kFilterImagesMinNumImages) return out;
    const ModelIndex ix(m, o.BogusThresholds());
    for (uint32_t id : reg_image_ids) {
        const auto it = ix.image.find(id);
        if (it == ix.image.end()) throw std::invalid_argument("filter_images: the reconstruction has no image " + std::to_string(id));
        const ModelImage& im = m.images[it->second];
        bool any = false;
        for (const ModelPoint2D& p : im.points2D) any = any || p.point3D_id != kInvalidPoint3DId;
        if (!any || ix.image_bogus[it->second]) out.push_back(id);
    }
    return out;
}

// Reconstruction::DeRegisterImage under R1: every observation of the image is deleted (a point whose track has two
// elements or fewer goes entirely, as DeleteObservation has it), then the image leaves the model
inline void DeRegisterImage(SparseModel* m, uint32_t image_id) {
    size_t at = m->images.size();
    for (size_t i = 0; i < m->images.size(); ++i)
        if (m->images[i].image_id == image_id) at = i;
    if (at == m->images.size()) throw std::invalid_argument("filter_images: the reconstruction has no image " + std::to_string(image_id));
    std::unordered_map<uint32_t, size_t> imgs;
    for (size_t i = 0; i < m->images.size(); ++i) imgs[m->images[i].image_id] = i;
    std::vector<ModelPoint3D> kept;
    kept.reserve(m->points3D.size());
    for (ModelPoint3D& p : m->points3D) {
        bool seen = false;
        for (const auto& e : p.track) seen = seen || e.first == image_id;
        if (!seen) {
            kept.push_back(std::move(p));
            continue;
        }
        // the image's points2D in index order, as DeRegisterImage walks them; a point goes with the first deletion that
        // finds its track at two elements or fewer
        bool gone = false;
        while (!gone) {
            size_t k = p.track.size();
            for (size_t j = 0; j < p.track.size(); ++j)
                if (p.track[j].first == image_id && (k == p.track.size() || p.track[j].second < p.track[k].second)) k = j;
            if (k == p.track.size()) break;
            if (p.track.size() <= 2) {
                for (const auto& e : p.track) {
                    const auto ii = imgs.find(e.first);
                    if (ii != imgs.end() && e.second < m->images[ii->second].points2D.size()) m->images[ii->second].points2D[e.second].point3D_id = kInvalidPoint3DId;
                }
                gone = true;
            } else {
                if (p.track[k].second < m->images[at].points2D.size()) m->images[at].points2D[p.track[k].second].point3D_id = kInvalidPoint3DId;
                p.track.erase(p.track.begin() + static_cast<std::ptrdiff_t>(k));
            }
        }
        if (!gone) kept.push_back(std::move(p));
    }
    m->points3D.swap(kept);
    m->images.erase(m->images.begin() + static_cast<std::ptrdiff_t>(at));
}

}  // namespace amchost
