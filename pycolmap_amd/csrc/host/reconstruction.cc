// reconstruction.cc — see reconstruction.h
#include "reconstruction.h"

#include <algorithm>
#include <cfloat>
#include <stdexcept>
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

namespace {

using ImageIndex = std::unordered_map<uint32_t, size_t>;

ImageIndex IndexImages(const SparseModel& m) {
    ImageIndex imgs;
    for (size_t i = 0; i < m.images.size(); ++i) imgs[m.images[i].image_id] = i;
    return imgs;
}

void ClearTrack(SparseModel* m, const ImageIndex& imgs, const ModelPoint3D& p) {
    for (const auto& el : p.track) m->images[imgs.at(el.first)].points2D[el.second].point3D_id = kInvalidPoint3DId;
}

// DeleteObservation's rule on element k of p's track: true = the whole point goes (its points2D are cleared, the caller
// drops it); false = that element left the track and its point2D lost the point
bool DeleteTrackElement(SparseModel* m, const ImageIndex& imgs, ModelPoint3D* p, size_t k) {
    if (p->track.size() <= 2) {
        ClearTrack(m, imgs, *p);
        return true;
    }
    m->images[imgs.at(p->track[k].first)].points2D[p->track[k].second].point3D_id = kInvalidPoint3DId;
    p->track.erase(p->track.begin() + static_cast<std::ptrdiff_t>(k));
    return false;
}

}  // namespace

size_t FilterObservationsWithNegativeDepth(SparseModel* m) {
    const ImageIndex imgs = IndexImages(*m);
    size_t removed = 0;
    std::vector<ModelPoint3D> kept;
    kept.reserve(m->points3D.size());
    for (ModelPoint3D& p : m->points3D) {
        bool deleted = false;
        for (size_t k = 0; k < p.track.size() && !deleted;) {
            const ModelImage& im = m->images[imgs.at(p.track[k].first)];
            if (PointDepth(im, p.xyz) < DBL_EPSILON) {
                ++removed;
                deleted = DeleteTrackElement(m, imgs, &p, k);
            } else {
                ++k;
            }
        }
        if (!deleted) kept.push_back(std::move(p));
    }
    m->points3D.swap(kept);
    return removed;
}

void DeletePoint3D(SparseModel* m, uint64_t point3D_id) {
    const auto it = std::find_if(m->points3D.begin(), m->points3D.end(), [&](const ModelPoint3D& p) { return p.point3D_id == point3D_id; });
    if (it == m->points3D.end()) throw std::invalid_argument("delete_point3D: point3D " + std::to_string(point3D_id) + " does not exist");
    ClearTrack(m, IndexImages(*m), *it);
    m->points3D.erase(it);
}

void DeleteObservation(SparseModel* m, uint32_t image_id, uint32_t point2D_idx) {
    const ImageIndex imgs = IndexImages(*m);
    const auto ii = imgs.find(image_id);
    if (ii == imgs.end()) throw std::invalid_argument("delete_observation: image " + std::to_string(image_id) + " does not exist");
    const ModelImage& im = m->images[ii->second];
    if (point2D_idx >= im.points2D.size())
        throw std::invalid_argument("delete_observation: image " + std::to_string(image_id) + " has no point2D " + std::to_string(point2D_idx));
    const uint64_t id = im.points2D[point2D_idx].point3D_id;
    if (id == kInvalidPoint3DId)
        throw std::invalid_argument("delete_observation: point2D " + std::to_string(point2D_idx) + " of image " + std::to_string(image_id) + " has no point3D");
    const auto it = std::find_if(m->points3D.begin(), m->points3D.end(), [&](const ModelPoint3D& p) { return p.point3D_id == id; });
    if (it == m->points3D.end()) throw std::invalid_argument("delete_observation: point3D " + std::to_string(id) + " does not exist");
    const auto el = std::find(it->track.begin(), it->track.end(), std::make_pair(image_id, point2D_idx));
    if (el == it->track.end()) throw std::invalid_argument("delete_observation: the point's track does not hold the observation");
    if (DeleteTrackElement(m, imgs, &*it, static_cast<size_t>(el - it->track.begin()))) m->points3D.erase(it);
}

double ComputeMeanReprojectionError(const SparseModel& m) {
    if (m.points3D.empty()) return 0.0;
    std::vector<std::pair<uint64_t, double>> byid;
    byid.reserve(m.points3D.size());
    for (const ModelPoint3D& p : m.points3D) byid.emplace_back(p.point3D_id, p.error);
    std::sort(byid.begin(), byid.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    double sum = 0.0;
    for (const auto& e : byid) sum += e.second;
    return sum / static_cast<double>(byid.size());
}

double ComputeMeanObservationsPerRegImage(const SparseModel& m) {
    return m.images.empty() ? 0.0 : static_cast<double>(ComputeNumObservations(m)) / static_cast<double>(m.images.size());
}

amc_filter_problem FlatFilter::Problem() const {
    amc_filter_problem p{};
    p.num_cameras = camera_models.size();
    p.camera_models = camera_models.data();
    p.camera_params = camera_params.data();
    p.num_images = image_cameras.size();
    p.image_cameras = image_cameras.data();
    p.qvec = qvec.data();
    p.tvec = tvec.data();
    p.num_points = point_ids.size();
    p.xyz = xyz.data();
    p.track_offsets = track_offsets.data();
    p.obs_image = obs_image.data();
    p.obs_xy = obs_xy.data();
    p.selected = selected.empty() ? nullptr : selected.data();
    return p;
}

FlatFilter FlattenForFilter(const SparseModel& m, const std::vector<uint64_t>* ids) {
    const std::string bad = CheckModel(m);
    if (!bad.empty()) throw std::invalid_argument("filter_points3D: " + bad);
    FlatFilter o;
    std::unordered_map<uint32_t, uint32_t> cam_index, img_index;
    for (const ModelCamera& c : m.cameras) {
        cam_index[c.camera_id] = static_cast<uint32_t>(o.camera_models.size());
        o.camera_models.push_back(c.model);
        for (size_t k = 0; k < 12; ++k) o.camera_params.push_back(k < c.params.size() ? c.params[k] : 0.0);
    }
    for (const ModelImage& im : m.images) {
        img_index[im.image_id] = static_cast<uint32_t>(o.image_cameras.size());
        o.image_cameras.push_back(cam_index.at(im.camera_id));
        o.qvec.insert(o.qvec.end(), {im.qvec[1], im.qvec[2], im.qvec[3], im.qvec[0]});  // x y z w
        o.tvec.insert(o.tvec.end(), im.tvec, im.tvec + 3);
    }
    std::unordered_map<uint64_t, size_t> wanted;
    if (ids)
        for (uint64_t id : *ids) wanted.emplace(id, 0);
    for (const ModelPoint3D& p : m.points3D) {
        o.point_ids.push_back(p.point3D_id);
        o.xyz.insert(o.xyz.end(), p.xyz, p.xyz + 3);
        for (const auto& el : p.track) {
            const uint32_t i = img_index.at(el.first);
            const ModelPoint2D& p2 = m.images[i].points2D.at(el.second);
            o.obs_image.push_back(i);
            o.obs_xy.push_back(p2.x);
            o.obs_xy.push_back(p2.y);
        }
        o.track_offsets.push_back(o.obs_image.size());
        if (ids) o.selected.push_back(wanted.count(p.point3D_id) ? 1 : 0);
    }
    return o;
}

std::vector<uint64_t> Point3DIdsInImages(const SparseModel& m, const std::vector<uint32_t>& image_ids) {
    const ImageIndex imgs = IndexImages(m);
    std::vector<uint64_t> ids;
    for (uint32_t image_id : image_ids) {
        const auto it = imgs.find(image_id);
        if (it == imgs.end()) throw std::invalid_argument("filter_points3D_in_images: image " + std::to_string(image_id) + " does not exist");
        for (const ModelPoint2D& p : m.images[it->second].points2D)
            if (p.point3D_id != kInvalidPoint3DId) ids.push_back(p.point3D_id);
    }
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    return ids;
}

namespace {

// the model still has the flat problem's points and track lengths
void CheckSameShape(const FlatFilter& f, const SparseModel& m, const char* who) {
    bool same = f.point_ids.size() == m.points3D.size() && f.track_offsets.size() == f.point_ids.size() + 1;
    for (size_t j = 0; same && j < m.points3D.size(); ++j)
        same = m.points3D[j].point3D_id == f.point_ids[j] && f.track_offsets[j + 1] >= f.track_offsets[j] &&
               f.track_offsets[j + 1] - f.track_offsets[j] == m.points3D[j].track.size();
    if (!same) throw std::invalid_argument(std::string(who) + ": the model changed between flattening and write-back");
}

}  // namespace

size_t ApplyFilterResult(const FlatFilter& f, const uint8_t* verdict, const uint8_t* deleted, const double* error, SparseModel* m) {
    CheckSameShape(f, *m, "filter_points3D");
    if (CheckModel(*m) != std::string()) throw std::invalid_argument("filter_points3D: the model changed between flattening and write-back");
    for (size_t j = 0; j < m->points3D.size(); ++j)
        if (verdict[j] > AMC_FILTER_ANGLE) throw std::invalid_argument("filter_points3D: unknown verdict " + std::to_string(verdict[j]));
    const ImageIndex imgs = IndexImages(*m);
    size_t count = 0;
    std::vector<ModelPoint3D> kept;
    kept.reserve(m->points3D.size());
    for (size_t j = 0; j < m->points3D.size(); ++j) {
        ModelPoint3D& p = m->points3D[j];
        const uint64_t o0 = f.track_offsets[j];
        const size_t L = p.track.size();
        if (verdict[j] == AMC_FILTER_NOT_SELECTED) {
            kept.push_back(std::move(p));
            continue;
        }
        if (verdict[j] == AMC_FILTER_SHORT_TRACK || verdict[j] == AMC_FILTER_REPROJECTION) {
            count += L;
            ClearTrack(m, imgs, p);
            continue;
        }
        size_t marked = 0;
        for (size_t k = 0; k < L; ++k) marked += deleted[o0 + k] != 0;
        count += marked;
        if (verdict[j] == AMC_FILTER_ANGLE) {
            ++count;
            ClearTrack(m, imgs, p);
            continue;
        }
        std::vector<std::pair<uint32_t, uint32_t>> track;
        track.reserve(L - marked);
        for (size_t k = 0; k < L; ++k) {
            if (deleted[o0 + k])
                m->images[imgs.at(p.track[k].first)].points2D[p.track[k].second].point3D_id = kInvalidPoint3DId;
            else
                track.push_back(p.track[k]);
        }
        p.track.swap(track);
        p.error = error[j];
        kept.push_back(std::move(p));
    }
    m->points3D.swap(kept);
    return count;
}

void ApplyPointErrors(const FlatFilter& f, const double* error, SparseModel* m) {
    CheckSameShape(f, *m, "update_point3D_errors");
    for (size_t j = 0; j < m->points3D.size(); ++j) m->points3D[j].error = error[j];
}

}  // namespace amchost
