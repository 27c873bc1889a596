// reconstruction.cc — see reconstruction.h
#include "reconstruction.h"

#include <algorithm>
#include <cfloat>
#include <unordered_map>

namespace amchost {

std::string CheckModel(const SparseModel& m) {
    std::unordered_map<uint32_t, size_t> cams, imgs;
    std::unordered_map<uint64_t, size_t> pts;
    for (size_t i = 0; i < m.cameras.size(); ++i) {
        const ModelCamera& c = m.cameras[i];
        if (!cams.emplace(c.camera_id, i).second) return "camera id " + std::to_string(c.camera_id) + " appears twice";
        const int np = ModelNumParams(c.model);
        if (np < 0) return "camera " + std::to_string(c.camera_id) + " has an unknown model";
        if (c.params.size() != static_cast<size_t>(np))
            return "camera " + std::to_string(c.camera_id) + " has " + std::to_string(c.params.size()) + " parameters, its model " + std::to_string(np);
    }
    for (size_t i = 0; i < m.images.size(); ++i) {
        const ModelImage& im = m.images[i];
        if (!imgs.emplace(im.image_id, i).second) return "image id " + std::to_string(im.image_id) + " appears twice";
        if (!cams.count(im.camera_id))
            return "image " + std::to_string(im.image_id) + " names camera " + std::to_string(im.camera_id) + ", which does not exist";
    }
    for (size_t i = 0; i < m.points3D.size(); ++i)
        if (m.points3D[i].point3D_id == kInvalidPoint3DId || !pts.emplace(m.points3D[i].point3D_id, i).second)
            return "point3D id " + std::to_string(m.points3D[i].point3D_id) + " is invalid or appears twice";
    std::vector<size_t> track_refs(m.points3D.size(), 0);
    for (const ModelImage& im : m.images)
        for (const ModelPoint2D& p : im.points2D) {
            if (p.point3D_id == kInvalidPoint3DId) continue;
            const auto it = pts.find(p.point3D_id);
            if (it == pts.end())
                return "image " + std::to_string(im.image_id) + " observes point3D " + std::to_string(p.point3D_id) + ", which does not exist";
            ++track_refs[it->second];
        }
    for (size_t j = 0; j < m.points3D.size(); ++j) {
        const ModelPoint3D& p = m.points3D[j];
        for (const auto& el : p.track) {
            const auto it = imgs.find(el.first);
            if (it == imgs.end())
                return "point3D " + std::to_string(p.point3D_id) + " has a track element in image " + std::to_string(el.first) + ", which does not exist";
            const ModelImage& im = m.images[it->second];
            if (el.second >= im.points2D.size() || im.points2D[el.second].point3D_id != p.point3D_id)
                return "point3D " + std::to_string(p.point3D_id) + " has a track element (" + std::to_string(el.first) + ", " +
                       std::to_string(el.second) + ") that the image's points2D do not name back";
        }
        if (track_refs[j] != p.track.size())
            return "point3D " + std::to_string(p.point3D_id) + " is observed by " + std::to_string(track_refs[j]) +
                   " points2D, its track has " + std::to_string(p.track.size()) + " elements";
    }
    return std::string();
}

size_t ComputeNumObservations(const SparseModel& m) {
    size_t n = 0;
    for (const ModelImage& im : m.images)
        for (const ModelPoint2D& p : im.points2D) n += p.point3D_id != kInvalidPoint3DId;
    return n;
}

double ComputeMeanTrackLength(const SparseModel& m) {
    return m.points3D.empty() ? 0.0 : static_cast<double>(ComputeNumObservations(m)) / static_cast<double>(m.points3D.size());
}

double PointDepth(const ModelImage& im, const double* X) {
    const double w = im.qvec[0], x = im.qvec[1], y = im.qvec[2], z = im.qvec[3];
    // third row of Eigen's toRotationMatrix
    const double r20 = 2.0 * x * z - 2.0 * y * w, r21 = 2.0 * y * z + 2.0 * x * w, r22 = 1.0 - (2.0 * x * x + 2.0 * y * y);
    return r20 * X[0] + r21 * X[1] + r22 * X[2] + im.tvec[2];
}

size_t FilterObservationsWithNegativeDepth(SparseModel* m) {
    std::unordered_map<uint32_t, size_t> imgs;
    for (size_t i = 0; i < m->images.size(); ++i) imgs[m->images[i].image_id] = i;
    size_t removed = 0;
    std::vector<ModelPoint3D> kept;
    kept.reserve(m->points3D.size());
    for (ModelPoint3D& p : m->points3D) {
        bool deleted = false;
        for (size_t k = 0; k < p.track.size() && !deleted;) {
            ModelImage& im = m->images[imgs.at(p.track[k].first)];
            if (PointDepth(im, p.xyz) < DBL_EPSILON) {
                ++removed;
                if (p.track.size() <= 2) {  // DeleteObservation: the point goes with it
                    for (const auto& el : p.track) m->images[imgs.at(el.first)].points2D[el.second].point3D_id = kInvalidPoint3DId;
                    deleted = true;
                } else {
                    im.points2D[p.track[k].second].point3D_id = kInvalidPoint3DId;
                    p.track.erase(p.track.begin() + static_cast<std::ptrdiff_t>(k));
                }
            } else {
                ++k;
            }
        }
        if (!deleted) kept.push_back(std::move(p));
    }
    m->points3D.swap(kept);
    return removed;
}

}  // namespace amchost
