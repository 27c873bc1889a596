// correspondence_graph.h — COLMAP 3.9.1's CorrespondenceGraph as DESIGN.md 17.1 restates it: per image and point2D the
// list of (image, point2D) it was matched to, at most one per other image.  No Python and no HIP here:
// tests/shim/triangulator_host_fuzz.cc runs it under ASan + UBSan.  A query for an image the graph does not hold throws
// std::invalid_argument in the THROW_CHECK format (COLMAP aborts).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace amchost {

struct Correspondence {
    uint32_t image_id = 0xFFFFFFFFu;
    uint32_t point2D_idx = 0xFFFFFFFFu;
    Correspondence() = default;
    Correspondence(uint32_t image, uint32_t idx) : image_id(image), point2D_idx(idx) {}
};

class CorrespondenceGraph {
  public:
    size_t NumImages() const { return images_.size(); }
    size_t NumImagePairs() const { return pairs_.size(); }
    bool ExistsImage(uint32_t image_id) const { return images_.count(image_id) != 0; }

    void AddImage(uint32_t image_id, size_t num_points2D) {
        if (ExistsImage(image_id)) Fail(__LINE__, "!ExistsImage(image_id)", image_id);
        images_[image_id].corrs.resize(num_points2D);
    }

    // `matches`: n pairs (point2D of image 1, point2D of image 2).  Returns the warnings to log: one for a self pair,
    // one with the number of matches dropped for an index out of range, one with the number of duplicates (COLMAP logs
    // every dropped match).
    std::vector<std::string> AddCorrespondences(uint32_t image_id1, uint32_t image_id2, const uint32_t* matches, size_t n) {
        std::vector<std::string> warnings;
        if (image_id1 == image_id2) {
            warnings.push_back("Cannot use self-matches for image_id=" + std::to_string(image_id1));
            return warnings;
        }
        Image& im1 = At(image_id1, __LINE__);
        Image& im2 = At(image_id2, __LINE__);
        im1.num_correspondences += n;
        im2.num_correspondences += n;
        size_t& pair = pairs_[PairKey(image_id1, image_id2)];
        pair += n;
        size_t out_of_range = 0, duplicates = 0;
        for (size_t i = 0; i < n; ++i) {
            const uint32_t a = matches[2 * i], b = matches[2 * i + 1];
            bool keep = a < im1.corrs.size() && b < im2.corrs.size();
            if (!keep) {
                out_of_range += 1;
            } else if (HasInto(im1.corrs[a], image_id2) || HasInto(im2.corrs[b], image_id1)) {
                keep = false;
                duplicates += 1;
            }
            if (keep) {
                im1.corrs[a].emplace_back(image_id2, b);
                im2.corrs[b].emplace_back(image_id1, a);
            } else {
                im1.num_correspondences -= 1;
                im2.num_correspondences -= 1;
                pair -= 1;
            }
        }
        const std::string between = " between images " + std::to_string(image_id1) + " and " + std::to_string(image_id2);
        if (out_of_range) warnings.push_back(std::to_string(out_of_range) + " correspondences with a point2D index out of range" + between);
        if (duplicates) warnings.push_back(std::to_string(duplicates) + " duplicate correspondences" + between);
        return warnings;
    }

    // counts every image's observations and erases the images without any
    void Finalize() {
        for (auto it = images_.begin(); it != images_.end();) {
            it->second.num_observations = 0;
            for (auto& c : it->second.corrs) {
                if (!c.empty()) it->second.num_observations += 1;
                c.shrink_to_fit();
            }
            if (it->second.num_observations == 0)
                it = images_.erase(it);
            else
                ++it;
        }
    }

    size_t NumObservationsForImage(uint32_t image_id) const { return At(image_id, __LINE__).num_observations; }
    size_t NumCorrespondencesForImage(uint32_t image_id) const { return At(image_id, __LINE__).num_correspondences; }
    size_t NumCorrespondencesBetweenImages(uint32_t image_id1, uint32_t image_id2) const {
        const auto it = pairs_.find(PairKey(image_id1, image_id2));
        return it == pairs_.end() ? 0 : it->second;
    }
    size_t NumPoints2D(uint32_t image_id) const { return At(image_id, __LINE__).corrs.size(); }
    // every image pair the graph holds as (smaller id << 32 | larger id, correspondence count), ascending
    std::vector<std::pair<uint64_t, size_t>> ImagePairs() const {
        std::vector<std::pair<uint64_t, size_t>> out(pairs_.begin(), pairs_.end());
        std::sort(out.begin(), out.end());
        return out;
    }

    const std::vector<Correspondence>& ExtractCorrespondences(uint32_t image_id, uint32_t point2D_idx) const {
        return Corrs(image_id, point2D_idx, __LINE__);
    }
    bool HasCorrespondences(uint32_t image_id, uint32_t point2D_idx) const {
        return !Corrs(image_id, point2D_idx, __LINE__).empty();
    }
    bool IsTwoViewObservation(uint32_t image_id, uint32_t point2D_idx) const {
        const std::vector<Correspondence>& c = Corrs(image_id, point2D_idx, __LINE__);
        if (c.size() != 1) return false;
        return Corrs(c[0].image_id, c[0].point2D_idx, __LINE__).size() == 1;
    }

    // 17.1: transitivity 1 is the direct list; otherwise a breadth-first walk by levels from the observation itself
    void ExtractTransitiveCorrespondences(uint32_t image_id, uint32_t point2D_idx, size_t transitivity,
                                          std::vector<Correspondence>* found) const {
        if (transitivity == 1) {
            *found = Corrs(image_id, point2D_idx, __LINE__);
            return;
        }
        found->clear();
        if (!HasCorrespondences(image_id, point2D_idx)) return;
        found->emplace_back(image_id, point2D_idx);
        std::map<uint32_t, std::set<uint32_t>> seen;
        seen[image_id].insert(point2D_idx);
        size_t begin = 0, end = 1;
        for (size_t t = 0; t < transitivity; ++t) {
            for (size_t i = begin; i < end; ++i) {
                const Correspondence ref = (*found)[i];
                for (const Correspondence& c : Corrs(ref.image_id, ref.point2D_idx, __LINE__))
                    if (seen[c.image_id].insert(c.point2D_idx).second) found->push_back(c);
            }
            begin = end;
            end = found->size();
            if (begin == end) break;
        }
        // the seed leaves: the last element takes its place
        found->front() = found->back();
        found->pop_back();
    }

    // n x 2 (point2D of image 1, point2D of image 2), by image 1's point2D index
    std::vector<uint32_t> FindCorrespondencesBetweenImages(uint32_t image_id1, uint32_t image_id2) const {
        std::vector<uint32_t> out;
        if (NumCorrespondencesBetweenImages(image_id1, image_id2) == 0) return out;
        const Image& im1 = At(image_id1, __LINE__);
        for (size_t a = 0; a < im1.corrs.size(); ++a)
            for (const Correspondence& c : im1.corrs[a])
                if (c.image_id == image_id2) {
                    out.push_back(static_cast<uint32_t>(a));
                    out.push_back(c.point2D_idx);
                }
        return out;
    }

  private:
    struct Image {
        size_t num_observations = 0, num_correspondences = 0;
        std::vector<std::vector<Correspondence>> corrs;
    };
    static uint64_t PairKey(uint32_t a, uint32_t b) {
        return a < b ? (static_cast<uint64_t>(a) << 32) | b : (static_cast<uint64_t>(b) << 32) | a;
    }
    static bool HasInto(const std::vector<Correspondence>& v, uint32_t image_id) {
        for (const Correspondence& c : v)
            if (c.image_id == image_id) return true;
        return false;
    }
    [[noreturn]] static void Fail(int line, const std::string& expr, uint32_t image_id) {
        throw std::invalid_argument("[correspondence_graph.h:" + std::to_string(line) + "] Check Failed: " + expr +
                                    " (image_id=" + std::to_string(image_id) + ")");
    }
    const Image& At(uint32_t image_id, int line) const {
        const auto it = images_.find(image_id);
        if (it == images_.end()) Fail(line, "ExistsImage(image_id)", image_id);
        return it->second;
    }
    Image& At(uint32_t image_id, int line) { return const_cast<Image&>(static_cast<const CorrespondenceGraph*>(this)->At(image_id, line)); }
    const std::vector<Correspondence>& Corrs(uint32_t image_id, uint32_t point2D_idx, int line) const {
        const Image& im = At(image_id, line);
        if (point2D_idx >= im.corrs.size())
            throw std::invalid_argument("[correspondence_graph.h:" + std::to_string(line) + "] Check Failed: point2D_idx < num_points2D (" +
                                        std::to_string(point2D_idx) + " vs. " + std::to_string(im.corrs.size()) + ")");
        return im.corrs[point2D_idx];
    }

    std::unordered_map<uint32_t, Image> images_;
    std::unordered_map<uint64_t, size_t> pairs_;
};

}  // namespace amchost
