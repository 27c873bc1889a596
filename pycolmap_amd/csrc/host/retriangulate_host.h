// retriangulate_host.h — the host half of IncrementalTriangulator::Retriangulate on model_io's plain
// structs: which image pairs are statically eligible, their greedy colouring into rounds of image-disjoint pairs, the
// flat problem of include/amc_retri.h, and the replay of the library's result in the sequential order (round, pair id,
// correspondence) on the model.  No Python and no HIP here: tests/shim/retriangulate_host_fuzz.cc runs it under
// ASan + UBSan.
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

#include "../../../include/amc_retri.h"
#include "correspondence_graph.h"
#include "model_io.h"
#include "track_ops_host.h"
#include "triangulator_host.h"

namespace amchost {

// the triangulator's per-pair trial counters, by (smaller image id << 32 | larger image id)
using RetriTrials = std::map<uint64_t, int>;

// 19.3: pairs (first image, second image) in the order they are given; every pair takes the lowest-numbered round in
// which neither of its images is taken yet.  Returns the round of every pair.
inline std::vector<uint32_t> ColourRetriRounds(const std::vector<std::pair<uint32_t, uint32_t>>& pairs) {
    std::unordered_map<uint32_t, std::vector<uint8_t>> taken;  // per image: the rounds that hold it
    std::vector<uint32_t> round(pairs.size(), 0);
    for (size_t i = 0; i < pairs.size(); ++i) {
        std::vector<uint8_t>& a = taken[pairs[i].first];
        std::vector<uint8_t>& b = taken[pairs[i].second];  // (a stays valid: unordered_map keeps references)
        uint32_t r = 0;
        while ((r < a.size() && a[r]) || (r < b.size() && b[r])) ++r;
        if (a.size() <= r) a.resize(r + 1, 0);
        if (b.size() <= r) b.resize(r + 1, 0);
        a[r] = b[r] = 1;
        round[i] = r;
    }
    return round;
}

// the flat problem of amc_retriangulate_pairs for one call, and the arrays it points into
struct FlatRetri {
    std::vector<int32_t> camera_models, obs_point;
    std::vector<double> camera_params, qvec, tvec, obs_xy, point_xyz;
    std::vector<uint32_t> image_cameras, obs_image, pair_images, corr_obs;
    std::vector<uint64_t> pair_offsets{0}, round_offsets{0};
    std::vector<uint8_t> corr_two_view;
    // what the replay needs: every observation's and point's identity, every pair's image ids
    std::vector<Correspondence> obs_id;
    std::vector<uint64_t> point3D_ids;
    std::vector<std::pair<uint32_t, uint32_t>> pair_ids;
    // the pairs with a bogus camera that pass the ratio test with trials left (19.2): they only spend a trial
    std::vector<uint64_t> bogus_spent;
    size_t NumPairs() const { return pair_ids.size(); }
    size_t NumCorrs() const { return corr_two_view.size(); }
    size_t NumRounds() const { return round_offsets.size() - 1; }
    amc_retri_problem Problem() const {
        amc_retri_problem pb{};
        pb.num_cameras = camera_models.size();
        pb.camera_models = camera_models.data();
        pb.camera_params = camera_params.data();
        pb.num_images = image_cameras.size();
        pb.image_cameras = image_cameras.data();
        pb.qvec = qvec.data();
        pb.tvec = tvec.data();
        pb.num_obs = obs_image.size();
        pb.obs_image = obs_image.data();
        pb.obs_xy = obs_xy.data();
        pb.obs_point = obs_point.data();
        pb.num_points = point3D_ids.size();
        pb.point_xyz = point_xyz.data();
        pb.num_pairs = NumPairs();
        pb.pair_images = pair_images.data();
        pb.pair_offsets = pair_offsets.data();
        pb.corr_obs = corr_obs.data();
        pb.corr_two_view = corr_two_view.data();
        pb.num_rounds = NumRounds();
        pb.round_offsets = round_offsets.data();
        return pb;
    }
};

inline uint64_t RetriPairKey(uint32_t id1, uint32_t id2) { return (static_cast<uint64_t>(id1) << 32) | id2; }

// 19.2's num_tri_corrs of a pair on the model as it stands
inline size_t NumTriangulatedCorrespondences(const SparseModel& m, const ModelIndex& ix, uint32_t id1, uint32_t id2,
                                             const std::vector<uint32_t>& corrs) {
    const ModelImage& a = m.images[ix.image.at(id1)];
    const ModelImage& b = m.images[ix.image.at(id2)];
    size_t n = 0;
    for (size_t k = 0; k + 1 < corrs.size(); k += 2) {
        if (corrs[k] >= a.points2D.size() || corrs[k + 1] >= b.points2D.size())
            throw std::invalid_argument("retriangulate: the graph names a point2D of image " + std::to_string(id1) + " or " +
                                        std::to_string(id2) + " which the reconstruction does not hold");
        const uint64_t p = a.points2D[corrs[k]].point3D_id;
        n += p != kInvalidPoint3DId && p == b.points2D[corrs[k + 1]].point3D_id;
    }
    return n;
}

// 19.2 - 19.4: the statically eligible pairs of the graph (a count above 0, both images in the model, trials left,
// no bogus camera) in ascending pair id, coloured into rounds and laid out by round with the observations and points
// they touch.  Throws std::invalid_argument for a point2D the reconstruction does not hold and for a call of more than
// max_corrs correspondences (the library's bound; tests pass a smaller one).
inline FlatRetri PlanRetriangulation(const CorrespondenceGraph& graph, const SparseModel& m, const ModelIndex& ix,
                                     const TriangulatorOptions& o, const RetriTrials& trials,
                                     uint64_t max_corrs = AMC_RETRI_MAX_CORRS) {
    const FlatTriobs cams = FlattenModelForTriobs(m, ix);
    FlatRetri f;
    f.camera_models = cams.camera_models;
    f.camera_params = cams.camera_params;
    f.image_cameras = cams.image_cameras;
    f.qvec = cams.qvec;
    f.tvec = cams.tvec;
    std::vector<std::pair<uint32_t, uint32_t>> eligible;
    uint64_t total = 0;
    for (const auto& pc : graph.ImagePairs()) {
        const uint32_t id1 = static_cast<uint32_t>(pc.first >> 32), id2 = static_cast<uint32_t>(pc.first);
        if (pc.second == 0) continue;
        const auto i1 = ix.image.find(id1), i2 = ix.image.find(id2);
        if (i1 == ix.image.end() || i2 == ix.image.end()) continue;
        const auto t = trials.find(pc.first);
        if (t != trials.end() && t->second >= o.re_max_trials) continue;
        if (o.re_max_trials <= 0) continue;
        if (ix.image_bogus[i1->second] || ix.image_bogus[i2->second]) {
            // the ratio on the model as the call found it; the trial is spent and nothing else happens
            const std::vector<uint32_t> corrs = graph.FindCorrespondencesBetweenImages(id1, id2);
            const double tri_ratio = static_cast<double>(NumTriangulatedCorrespondences(m, ix, id1, id2, corrs)) / static_cast<double>(pc.second);
            if (!(tri_ratio >= o.re_min_ratio)) f.bogus_spent.push_back(pc.first);
            continue;
        }
        eligible.emplace_back(id1, id2);
        total += pc.second;
    }
    if (total > max_corrs)
        throw std::invalid_argument("retriangulate: the eligible image pairs hold " + std::to_string(total) + " correspondences, more than " +
                                    std::to_string(max_corrs) + " (AMC_RETRI_MAX_CORRS, DESIGN.md 19.4)");
    const std::vector<uint32_t> round = ColourRetriRounds(eligible);
    uint32_t nrounds = 0;
    for (const uint32_t r : round) nrounds = std::max(nrounds, r + 1);
    std::vector<std::vector<size_t>> by_round(nrounds);
    for (size_t i = 0; i < eligible.size(); ++i) by_round[round[i]].push_back(i);  // ascending pair id within a round
    std::unordered_map<uint64_t, uint32_t> obs_index;
    std::unordered_map<uint64_t, int32_t> point_index;
    auto observation = [&](uint32_t image_id, size_t image, uint32_t idx) {
        const auto at = obs_index.emplace(ObservationKey(image_id, idx), static_cast<uint32_t>(f.obs_image.size()));
        if (!at.second) return at.first->second;
        if (idx >= m.images[image].points2D.size())
            throw std::invalid_argument("retriangulate: the graph names point2D " + std::to_string(idx) + " of image " + std::to_string(image_id) +
                                        ", which the reconstruction does not hold");
        const ModelPoint2D& p2 = m.images[image].points2D[idx];
        int32_t point = -1;
        if (p2.point3D_id != kInvalidPoint3DId) {
            const auto pt = point_index.emplace(p2.point3D_id, static_cast<int32_t>(f.point3D_ids.size()));
            if (pt.second) {
                const double* X = m.points3D[ix.point.at(p2.point3D_id)].xyz;
                f.point_xyz.insert(f.point_xyz.end(), X, X + 3);
                f.point3D_ids.push_back(p2.point3D_id);
            }
            point = pt.first->second;
        }
        f.obs_image.push_back(static_cast<uint32_t>(image));
        f.obs_xy.push_back(p2.x);
        f.obs_xy.push_back(p2.y);
        f.obs_point.push_back(point);
        f.obs_id.emplace_back(image_id, idx);
        return at.first->second;
    };
    for (uint32_t r = 0; r < nrounds; ++r) {
        for (const size_t i : by_round[r]) {
            const uint32_t id1 = eligible[i].first, id2 = eligible[i].second;
            const size_t i1 = ix.image.at(id1), i2 = ix.image.at(id2);
            const std::vector<uint32_t> corrs = graph.FindCorrespondencesBetweenImages(id1, id2);
            for (size_t k = 0; k + 1 < corrs.size(); k += 2) {
                f.corr_obs.push_back(observation(id1, i1, corrs[k]));
                f.corr_obs.push_back(observation(id2, i2, corrs[k + 1]));
                f.corr_two_view.push_back(o.ignore_two_view_tracks && graph.IsTwoViewObservation(id1, corrs[k]) ? 1 : 0);
            }
            f.pair_images.push_back(static_cast<uint32_t>(i1));
            f.pair_images.push_back(static_cast<uint32_t>(i2));
            f.pair_offsets.push_back(f.corr_two_view.size());
            f.pair_ids.emplace_back(id1, id2);
        }
        f.round_offsets.push_back(f.pair_ids.size());
    }
    return f;
}

struct RetriApplied {
    size_t num_tris = 0;  // Retriangulate's return: continued observations plus two per created point
    size_t num_created = 0, num_continued = 0, num_pairs_run = 0;
};

// The library's result (arrays of amc_retri_result's shapes) into the model the plan was made on, in the sequential
// order: round, pair id, correspondence.  A pair that ran spends a trial; a continued observation joins the point the
// other observation carries by then; a created point takes the next id (17.2's rule).  Throws std::invalid_argument
// when the result does not fit the problem; the caller then drops the model, the modified set and the counters.
inline RetriApplied ApplyRetriResult(const FlatRetri& f, const uint8_t* pair_ran, const uint8_t* corr_action, const uint64_t* created_offsets,
                                     const double* created_xyz, SparseModel* m, ModelIndex* ix, std::set<uint64_t>* modified,
                                     RetriTrials* trials) {
    RetriApplied out;
    for (const uint64_t key : f.bogus_spent) (*trials)[key] += 1;
    auto point2D = [&](uint32_t obs) -> ModelPoint2D& {
        const Correspondence& c = f.obs_id[obs];
        return m->images[ix->image.at(c.image_id)].points2D[c.point2D_idx];
    };
    for (size_t p = 0; p < f.NumPairs(); ++p) {
        if (!pair_ran[p]) continue;
        out.num_pairs_run += 1;
        (*trials)[RetriPairKey(f.pair_ids[p].first, f.pair_ids[p].second)] += 1;
        uint64_t made = created_offsets[p];
        for (uint64_t k = f.pair_offsets[p]; k < f.pair_offsets[p + 1]; ++k) {
            const uint8_t action = corr_action[k];
            if (action == AMC_RETRI_NONE) continue;
            const uint32_t o1 = f.corr_obs[2 * k], o2 = f.corr_obs[2 * k + 1];
            if (action == AMC_RETRI_CONTINUE_1TO2 || action == AMC_RETRI_CONTINUE_2TO1) {
                const uint32_t from = action == AMC_RETRI_CONTINUE_1TO2 ? o1 : o2, to = action == AMC_RETRI_CONTINUE_1TO2 ? o2 : o1;
                const uint64_t pid = point2D(from).point3D_id;
                if (pid == kInvalidPoint3DId || point2D(to).point3D_id != kInvalidPoint3DId)
                    throw std::invalid_argument("retriangulate: the result continues correspondence " + std::to_string(k) + " without a point or onto one");
                m->points3D[ix->point.at(pid)].track.emplace_back(f.obs_id[to].image_id, f.obs_id[to].point2D_idx);
                point2D(to).point3D_id = pid;
                modified->insert(pid);
                out.num_tris += 1;
                out.num_continued += 1;
            } else if (action == AMC_RETRI_CREATED) {
                if (point2D(o1).point3D_id != kInvalidPoint3DId || point2D(o2).point3D_id != kInvalidPoint3DId || made >= created_offsets[p + 1])
                    throw std::invalid_argument("retriangulate: the result creates a point on correspondence " + std::to_string(k) + ", which has one or has no position");
                ModelPoint3D pt;
                pt.point3D_id = ix->next_point3D_id;
                for (int d = 0; d < 3; ++d) pt.xyz[d] = created_xyz[3 * made + d];
                made += 1;
                pt.error = -1.0;
                pt.track.emplace_back(f.obs_id[o1].image_id, f.obs_id[o1].point2D_idx);
                pt.track.emplace_back(f.obs_id[o2].image_id, f.obs_id[o2].point2D_idx);
                point2D(o1).point3D_id = pt.point3D_id;
                point2D(o2).point3D_id = pt.point3D_id;
                ix->point[pt.point3D_id] = m->points3D.size();
                ix->next_point3D_id += 1;
                modified->insert(pt.point3D_id);
                m->points3D.push_back(std::move(pt));
                out.num_tris += 2;
                out.num_created += 1;
            } else {
                throw std::invalid_argument("retriangulate: the result has the unknown action " + std::to_string(action));
            }
        }
        if (made != created_offsets[p + 1]) throw std::invalid_argument("retriangulate: the result's created positions do not fit pair " + std::to_string(p));
    }
    return out;
}

}  // namespace amchost
