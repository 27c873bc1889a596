// track_ops_host.h — the host half of IncrementalTriangulator::CompleteTracks and MergeTracks on
// model_io's plain structs.  Completion: the superset closure of every listed point, the flat problem of
// include/amc_tracks.h, and the sequential walk that reads the library's pass bytes instead of computing errors.
// Merging: the connected components of the listed points laid out as the flat merge problem, and the library's merge
// logs applied root by root in ascending id order.  Adding an observation to a track and merging two points are done
// here, on the SparseModel; Reconstruction does not expose them.  No Python and no HIP here:
// tests/shim/track_ops_host_fuzz.cc runs it under ASan + UBSan.
#pragma once

#include <algorithm>
#include <cstdint>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../../include/amc_tracks.h"
#include "correspondence_graph.h"
#include "model_io.h"
#include "triangulator_host.h"

namespace amchost {

// the flat problem of amc_complete_tracks for one call, and the arrays it points into
struct FlatComplete {
    std::vector<int32_t> camera_models;
    std::vector<double> camera_params, qvec, tvec, item_xyz, cand_xy;
    std::vector<uint32_t> image_cameras, cand_image;
    std::vector<uint64_t> item_offsets{0};
    // what the walk needs: every item's point id, and where an observation is among its item's candidates
    std::vector<uint64_t> item_point3D;
    std::vector<std::unordered_map<uint64_t, uint64_t>> item_index;  // (image id << 32 | point2D) -> candidate
    size_t NumItems() const { return item_offsets.size() - 1; }
    size_t NumCandidates() const { return cand_image.size(); }
    amc_complete_problem Problem() const {
        amc_complete_problem pb{};
        pb.num_cameras = camera_models.size();
        pb.camera_models = camera_models.data();
        pb.camera_params = camera_params.data();
        pb.num_images = image_cameras.size();
        pb.image_cameras = image_cameras.data();
        pb.qvec = qvec.data();
        pb.tvec = tvec.data();
        pb.num_items = NumItems();
        pb.item_xyz = item_xyz.data();
        pb.item_offsets = item_offsets.data();
        pb.cand_image = cand_image.data();
        pb.cand_xy = cand_xy.data();
        return pb;
    }
};

inline uint64_t ObservationKey(uint32_t image_id, uint32_t point2D_idx) {
    return (static_cast<uint64_t>(image_id) << 32) | point2D_idx;
}

// 18.1's three tests that do not need the error: the observation's image index when the walk may test it, -1 when the
// walk passes it over.  Throws std::invalid_argument for a point2D the reconstruction does not hold.
inline long CompletionCandidateImage(const SparseModel& m, const ModelIndex& ix, const Correspondence& c, const char* who) {
    const auto it = ix.image.find(c.image_id);
    if (it == ix.image.end()) return -1;
    if (c.point2D_idx >= m.images[it->second].points2D.size())
        throw std::invalid_argument(std::string(who) + ": the graph names point2D " + std::to_string(c.point2D_idx) + " of image " +
                                    std::to_string(c.image_id) + ", which the reconstruction does not hold");
    if (m.images[it->second].points2D[c.point2D_idx].point3D_id != kInvalidPoint3DId) return -1;
    if (ix.image_bogus[it->second]) return -1;
    return static_cast<long>(it->second);
}

// 18.3: per listed point (ascending ids, as std::set gives them) that exists and has a track, the breadth-first walk of
// complete_max_transitivity levels from its track through the observations 18.1 could test on the model as it stands,
// ignoring the error test; unique observations in the order the walk meets them.  Points whose walk finds nothing are
// not items.  Throws std::invalid_argument for an image the graph does not hold.
inline FlatComplete PlanCompletion(const CorrespondenceGraph& graph, const SparseModel& m, const ModelIndex& ix,
                                   const TriangulatorOptions& o, const std::set<uint64_t>& point3D_ids) {
    const FlatTriobs cams = FlattenModelForTriobs(m, ix);
    FlatComplete f;
    f.camera_models = cams.camera_models;
    f.camera_params = cams.camera_params;
    f.image_cameras = cams.image_cameras;
    f.qvec = cams.qvec;
    f.tvec = cams.tvec;
    std::vector<Correspondence> queue, next;
    for (const uint64_t pid : point3D_ids) {
        const auto at = ix.point.find(pid);
        if (at == ix.point.end()) continue;
        const ModelPoint3D& P = m.points3D[at->second];
        queue.clear();
        for (const auto& e : P.track) queue.emplace_back(e.first, e.second);
        std::unordered_map<uint64_t, uint64_t> index;
        const size_t first = f.cand_image.size();
        for (int t = 0; t < o.complete_max_transitivity && !queue.empty(); ++t) {
            next.clear();
            for (const Correspondence& ref : queue)
                for (const Correspondence& c : graph.ExtractCorrespondences(ref.image_id, ref.point2D_idx)) {
                    const long image = CompletionCandidateImage(m, ix, c, "complete_tracks");
                    if (image < 0) continue;
                    if (!index.emplace(ObservationKey(c.image_id, c.point2D_idx), f.cand_image.size()).second) continue;
                    const ModelPoint2D& p2 = m.images[image].points2D[c.point2D_idx];
                    f.cand_image.push_back(static_cast<uint32_t>(image));
                    f.cand_xy.push_back(p2.x);
                    f.cand_xy.push_back(p2.y);
                    next.push_back(c);
                }
            queue.swap(next);
        }
        if (f.cand_image.size() == first) continue;
        for (int d = 0; d < 3; ++d) f.item_xyz.push_back(P.xyz[d]);
        f.item_offsets.push_back(f.cand_image.size());
        f.item_point3D.push_back(pid);
        f.item_index.push_back(std::move(index));
    }
    return f;
}

struct CompletionApplied {
    size_t num_completed = 0;  // CompleteTracks' return: the observations added
    size_t num_visited = 0;    // the candidates the walks read a pass byte for
};

// 18.1, literally, for the plan's items in their (ascending id) order on the model the plan was made on: the walk reads
// cand_pass (NumCandidates() bytes) where COLMAP computes an error, and sees the observations earlier items took.
// Throws std::logic_error when a walk reaches an observation outside its item's closure (18.3 proves it cannot).
inline CompletionApplied ApplyCompletion(const FlatComplete& f, const uint8_t* cand_pass, const CorrespondenceGraph& graph,
                                         const TriangulatorOptions& o, SparseModel* m, const ModelIndex& ix,
                                         std::set<uint64_t>* modified) {
    CompletionApplied out;
    std::vector<Correspondence> queue, next;
    for (size_t i = 0; i < f.NumItems(); ++i) {
        const uint64_t pid = f.item_point3D[i];
        ModelPoint3D& P = m->points3D[ix.point.at(pid)];
        queue.clear();
        for (const auto& e : P.track) queue.emplace_back(e.first, e.second);
        for (int t = 0; t < o.complete_max_transitivity && !queue.empty(); ++t) {
            next.clear();
            for (const Correspondence& ref : queue)
                for (const Correspondence& c : graph.ExtractCorrespondences(ref.image_id, ref.point2D_idx)) {
                    const long image = CompletionCandidateImage(*m, ix, c, "complete_tracks");
                    if (image < 0) continue;
                    const auto k = f.item_index[i].find(ObservationKey(c.image_id, c.point2D_idx));
                    if (k == f.item_index[i].end() || k->second < f.item_offsets[i] || k->second >= f.item_offsets[i + 1])
                        throw std::logic_error("complete_tracks: the walk of point " + std::to_string(pid) + " left its closure at image " +
                                               std::to_string(c.image_id) + ", point2D " + std::to_string(c.point2D_idx));
                    out.num_visited += 1;
                    if (!cand_pass[k->second]) continue;
                    P.track.emplace_back(c.image_id, c.point2D_idx);
                    m->images[image].points2D[c.point2D_idx].point3D_id = pid;
                    modified->insert(pid);
                    out.num_completed += 1;
                    if (t < o.complete_max_transitivity - 1) next.push_back(c);
                }
            queue.swap(next);
        }
    }
    return out;
}

// the flat problem of amc_merge_tracks for one call, and the arrays it points into
struct FlatMerge {
    std::vector<int32_t> camera_models;
    std::vector<double> camera_params, qvec, tvec, point_xyz, obs_xy;
    std::vector<uint32_t> image_cameras, roots, obs_image, corr_obs;
    std::vector<uint64_t> comp_point_offsets{0}, comp_root_offsets{0}, point_obs_offsets{0}, obs_corr_offsets{0};
    std::vector<uint64_t> point3D_ids;  // of the problem's points
    size_t largest_component = 0;       // in observations
    size_t NumComponents() const { return comp_point_offsets.size() - 1; }
    amc_merge_problem Problem() const {
        amc_merge_problem pb{};
        pb.num_cameras = camera_models.size();
        pb.camera_models = camera_models.data();
        pb.camera_params = camera_params.data();
        pb.num_images = image_cameras.size();
        pb.image_cameras = image_cameras.data();
        pb.qvec = qvec.data();
        pb.tvec = tvec.data();
        pb.num_components = NumComponents();
        pb.comp_point_offsets = comp_point_offsets.data();
        pb.comp_root_offsets = comp_root_offsets.data();
        pb.roots = roots.data();
        pb.point_xyz = point_xyz.data();
        pb.point_obs_offsets = point_obs_offsets.data();
        pb.obs_image = obs_image.data();
        pb.obs_xy = obs_xy.data();
        pb.obs_corr_offsets = obs_corr_offsets.data();
        pb.corr_obs = corr_obs.data();
        return pb;
    }
};

// the point a correspondence carries, or kInvalidPoint3DId (an image outside the reconstruction, a point2D without a
// point).  Throws std::invalid_argument for a point2D the reconstruction does not hold.
inline uint64_t CorrespondencePoint3D(const SparseModel& m, const ModelIndex& ix, const Correspondence& c, const char* who) {
    const auto it = ix.image.find(c.image_id);
    if (it == ix.image.end()) return kInvalidPoint3DId;
    if (c.point2D_idx >= m.images[it->second].points2D.size())
        throw std::invalid_argument(std::string(who) + ": the graph names point2D " + std::to_string(c.point2D_idx) + " of image " +
                                    std::to_string(c.image_id) + ", which the reconstruction does not hold");
    return m.images[it->second].points2D[c.point2D_idx].point3D_id;
}

// 18.4: the connected components (two points are adjacent when an observation of one has a direct correspondence that
// carries the other) that the listed points lie in, each with its points in ascending id order, their tracks in track
// order, every observation's point-carrying correspondences in the graph's list order and its roots, the listed points,
// in ascending id order.  Components of one point are left out; the others are sorted by observation count, largest
// first (11.5), ties in the order of their smallest listed id.  Throws std::invalid_argument for an image the graph does
// not hold and for a component of more than AMC_MERGE_MAX_COMPONENT_OBS observations.
inline FlatMerge PlanMerge(const CorrespondenceGraph& graph, const SparseModel& m, const ModelIndex& ix,
                           const std::set<uint64_t>& point3D_ids) {
    const FlatTriobs cams = FlattenModelForTriobs(m, ix);
    FlatMerge f;
    f.camera_models = cams.camera_models;
    f.camera_params = cams.camera_params;
    f.image_cameras = cams.image_cameras;
    f.qvec = cams.qvec;
    f.tvec = cams.tvec;
    struct Component {
        std::vector<uint64_t> points;  // ascending ids
        size_t num_obs = 0;
    };
    std::vector<Component> comps;
    std::set<uint64_t> seen;
    for (const uint64_t seed : point3D_ids) {
        if (!ix.point.count(seed) || seen.count(seed)) continue;
        Component comp;
        std::vector<uint64_t> stack{seed};
        seen.insert(seed);
        while (!stack.empty()) {
            const uint64_t pid = stack.back();
            stack.pop_back();
            comp.points.push_back(pid);
            const ModelPoint3D& P = m.points3D[ix.point.at(pid)];
            comp.num_obs += P.track.size();
            for (const auto& e : P.track)
                for (const Correspondence& c : graph.ExtractCorrespondences(e.first, e.second)) {
                    const uint64_t q = CorrespondencePoint3D(m, ix, c, "merge_tracks");
                    if (q != kInvalidPoint3DId && seen.insert(q).second) stack.push_back(q);
                }
        }
        if (comp.points.size() < 2) continue;
        if (comp.num_obs > AMC_MERGE_MAX_COMPONENT_OBS)
            throw std::invalid_argument("merge_tracks: point3D " + std::to_string(seed) + " lies in a connected component of " +
                                        std::to_string(comp.num_obs) + " observations, more than " +
                                        std::to_string(AMC_MERGE_MAX_COMPONENT_OBS) + " (DESIGN.md 18.4 H4)");
        std::sort(comp.points.begin(), comp.points.end());
        comps.push_back(std::move(comp));
    }
    std::stable_sort(comps.begin(), comps.end(), [](const Component& a, const Component& b) { return a.num_obs > b.num_obs; });
    std::unordered_map<uint64_t, uint32_t> obs_index;
    for (const Component& comp : comps) {
        f.largest_component = std::max(f.largest_component, comp.num_obs);
        obs_index.clear();
        for (const uint64_t pid : comp.points) {
            const ModelPoint3D& P = m.points3D[ix.point.at(pid)];
            if (point3D_ids.count(pid)) f.roots.push_back(static_cast<uint32_t>(f.point3D_ids.size()));
            f.point3D_ids.push_back(pid);
            for (int d = 0; d < 3; ++d) f.point_xyz.push_back(P.xyz[d]);
            for (const auto& e : P.track) {
                const size_t image = ix.image.at(e.first);
                const ModelPoint2D& p2 = m.images[image].points2D[e.second];
                obs_index[ObservationKey(e.first, e.second)] = static_cast<uint32_t>(f.obs_image.size());
                f.obs_image.push_back(static_cast<uint32_t>(image));
                f.obs_xy.push_back(p2.x);
                f.obs_xy.push_back(p2.y);
            }
            f.point_obs_offsets.push_back(f.obs_image.size());
        }
        for (const uint64_t pid : comp.points)
            for (const auto& e : m.points3D[ix.point.at(pid)].track) {
                for (const Correspondence& c : graph.ExtractCorrespondences(e.first, e.second))
                    if (CorrespondencePoint3D(m, ix, c, "merge_tracks") != kInvalidPoint3DId)
                        f.corr_obs.push_back(obs_index.at(ObservationKey(c.image_id, c.point2D_idx)));
                f.obs_corr_offsets.push_back(f.corr_obs.size());
            }
        f.comp_point_offsets.push_back(f.point3D_ids.size());
        f.comp_root_offsets.push_back(f.roots.size());
    }
    return f;
}

struct MergeApplied {
    size_t num_merged = 0;  // MergeTracks' return: the sum of the roots' return values
    size_t num_merges = 0;
};

// The library's logs (arrays of amc_merge_result's shapes) into the model the plan was made on, root by root in global
// ascending id order (18.4): a merge's new point takes the id one above the largest id present (18.2 H3), the position
// the log gives, `current`'s track and then the other's, the weighted colour and the error -1; its points2D take the
// id; the modified set loses the two ids and gains the new one.  Throws std::invalid_argument when a log does not fit
// the problem.
inline MergeApplied ApplyMergeResult(const FlatMerge& f, const uint32_t* root_return, const uint64_t* root_merge_offsets,
                                     const uint32_t* merge_current, const uint32_t* merge_other, const double* merge_xyz,
                                     SparseModel* m, std::set<uint64_t>* modified) {
    MergeApplied out;
    const size_t nc = f.NumComponents();
    // a component's slots: its points, then the points its merges made so far (0 = not there, or merged away)
    std::vector<std::vector<uint64_t>> slot_id(nc);
    std::map<uint64_t, std::pair<size_t, size_t>> by_root;  // root id -> (component, root)
    for (size_t c = 0; c < nc; ++c) {
        for (uint64_t p = f.comp_point_offsets[c]; p < f.comp_point_offsets[c + 1]; ++p) slot_id[c].push_back(f.point3D_ids[p]);
        for (uint64_t r = f.comp_root_offsets[c]; r < f.comp_root_offsets[c + 1]; ++r) by_root[f.point3D_ids[f.roots[r]]] = {c, r};
    }
    // the model's points while they come and go: survivors keep their place, new points follow in the order they are made
    std::vector<ModelPoint3D>& pts = m->points3D;
    std::map<uint64_t, size_t> present;  // id -> place in pts
    std::vector<uint8_t> gone(pts.size(), 0);
    for (size_t i = 0; i < pts.size(); ++i) present[pts[i].point3D_id] = i;
    std::unordered_map<uint32_t, size_t> image_at;
    for (size_t i = 0; i < m->images.size(); ++i) image_at[m->images[i].image_id] = i;
    bool bad = false;
    for (const auto& root : by_root) {
        const size_t c = root.second.first, r = root.second.second;
        out.num_merged += root_return[r];
        for (uint64_t j = root_merge_offsets[r]; j < root_merge_offsets[r + 1]; ++j) {
            const uint32_t a = merge_current[j], b = merge_other[j];
            if (a >= slot_id[c].size() || b >= slot_id[c].size() || a == b || !present.count(slot_id[c][a]) || !present.count(slot_id[c][b])) {
                bad = true;
                break;
            }
            const size_t ia = present.at(slot_id[c][a]), ib = present.at(slot_id[c][b]);
            ModelPoint3D M;
            M.point3D_id = present.rbegin()->first + 1;
            for (int d = 0; d < 3; ++d) M.xyz[d] = merge_xyz[3 * j + d];
            const double n1 = static_cast<double>(pts[ia].track.size()), n2 = static_cast<double>(pts[ib].track.size());
            for (int d = 0; d < 3; ++d) M.rgb[d] = static_cast<uint8_t>((n1 * pts[ia].rgb[d] + n2 * pts[ib].rgb[d]) / (n1 + n2));
            M.error = -1.0;
            M.track = pts[ia].track;
            M.track.insert(M.track.end(), pts[ib].track.begin(), pts[ib].track.end());
            for (const auto& e : M.track) m->images[image_at.at(e.first)].points2D[e.second].point3D_id = M.point3D_id;
            modified->erase(pts[ia].point3D_id);
            modified->erase(pts[ib].point3D_id);
            modified->insert(M.point3D_id);
            present.erase(pts[ia].point3D_id);
            present.erase(pts[ib].point3D_id);
            gone[ia] = gone[ib] = 1;
            slot_id[c].push_back(M.point3D_id);
            present[M.point3D_id] = pts.size();
            gone.push_back(0);
            pts.push_back(std::move(M));
            out.num_merges += 1;
        }
        if (bad) break;
    }
    size_t kept = 0;
    for (size_t i = 0; i < pts.size(); ++i)
        if (!gone[i]) {
            if (kept != i) pts[kept] = std::move(pts[i]);
            ++kept;
        }
    pts.resize(kept);
    if (bad) throw std::invalid_argument("merge_tracks: the result's merge log does not fit the problem");
    return out;
}

}  // namespace amchost
