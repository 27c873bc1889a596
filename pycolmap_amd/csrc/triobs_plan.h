// triobs_plan.h — the host half of the observation triangulator: the checks of amc_triobs_opts and
// amc_triobs_problem, a batch's item order and round capacities, the lift of the candidates whose camera model needs
// libm, and the trial table.  No HIP here.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/amc_triobs.h"
#include "camera_math.h"

namespace amc {
namespace triobs {

// DegToRad's factor, as COLMAP writes it
constexpr double kDegToRad = 0.0174532925199432954743716805978692718781530857086181640625;
// Create's EstimateTriangulation settings (17.3)
constexpr double kConfidence = 0.9999, kMinInlierRatio = 0.02, kDynMultiplier = 3.0;
constexpr int64_t kMaxNumTrials = 10000;
constexpr uint64_t kAllTrialsUpTo = 15;  // min_num_trials = n (n - 1) / 2 for n <= 15 observations, else 0
constexpr int kMinSamples = 2;

// empty string = valid
inline std::string check_options(const amc_triobs_opts& o) {
    if (!(o.create_max_angle_error > 0.0)) return "create_max_angle_error > 0";
    if (!(o.continue_max_angle_error >= 0.0)) return "continue_max_angle_error >= 0";
    if (!(o.min_angle >= 0.0)) return "min_angle >= 0";
    return std::string();
}

// What is wrong with the problem, or the empty string.  Nothing is read through an offset or an index before it has
// been checked.
inline std::string check_problem(const amc_triobs_problem& pb) {
    const size_t ncam = pb.num_cameras, nimg = pb.num_images, nit = pb.num_items;
    if (!pb.item_offsets || (ncam && (!pb.camera_models || !pb.camera_params)) ||
        (nimg && (!pb.image_cameras || !pb.qvec || !pb.tvec)))
        return "NULL array";
    if (ncam > 0x7fffffffu / 16 || nimg > 0x7fffffffu / 16) return "too many cameras or images for 32-bit indices";
    if (pb.item_offsets[0] != 0) return "item_offsets does not start at 0";
    for (size_t i = 0; i < nit; ++i) {
        if (pb.item_offsets[i + 1] <= pb.item_offsets[i])
            return "item " + std::to_string(i) + " has no candidate (the reference observation is one)";
        if (pb.item_offsets[i + 1] - pb.item_offsets[i] > AMC_TRIOBS_MAX_ITEM_CANDIDATES)
            return "item " + std::to_string(i) + " has more than " + std::to_string(AMC_TRIOBS_MAX_ITEM_CANDIDATES) + " candidates";
    }
    const uint64_t ncand = pb.item_offsets[nit];
    if (ncand && (!pb.cand_image || !pb.cand_xy || !pb.cand_has_point || !pb.cand_xyz)) return "NULL array";
    for (size_t c = 0; c < ncam; ++c)
        if (pb.camera_models[c] < 0 || pb.camera_models[c] >= cam::kNumModels)
            return "camera " + std::to_string(c) + " has model " + std::to_string(pb.camera_models[c]);
    for (size_t i = 0; i < nimg; ++i)
        if (pb.image_cameras[i] >= ncam)
            return "image " + std::to_string(i) + " has camera index " + std::to_string(pb.image_cameras[i]);
    for (uint64_t k = 0; k < ncand; ++k)
        if (pb.cand_image[k] >= nimg)
            return "candidate " + std::to_string(k) + " has image index " + std::to_string(pb.cand_image[k]);
    return std::string();
}

// the most tracks an item of n candidates can create: every round takes at least two observations
inline uint32_t round_capacity(uint64_t n) { return static_cast<uint32_t>(n / 2); }

// A batch's items first .. last, appended to the call's plan: the batch-local item indices, longest item first (a
// counting sort; lengths above 64 share the first bin, in item order: DESIGN.md 11.5), and the batch-local offsets of
// the items' round slots (last - first + 1 of them).
inline void plan_batch(const uint64_t* item_offsets, size_t first, size_t last, std::vector<uint32_t>* order,
                       std::vector<uint32_t>* round_slots) {
    constexpr int kBins = 66;
    size_t cnt[kBins + 1] = {};
    auto bin_of = [&](size_t i) {
        const uint64_t n = item_offsets[i + 1] - item_offsets[i];
        return n > 64 ? 0 : static_cast<int>(65 - n);
    };
    for (size_t i = first; i < last; ++i) cnt[bin_of(i) + 1] += 1;
    for (int b = 0; b < kBins; ++b) cnt[b + 1] += cnt[b];
    const size_t at = order->size();
    order->resize(at + (last - first));
    for (size_t i = first; i < last; ++i) (*order)[at + cnt[bin_of(i)]++] = static_cast<uint32_t>(i - first);
    uint32_t slot = 0;
    round_slots->push_back(0);
    for (size_t i = first; i < last; ++i) {
        slot += round_capacity(item_offsets[i + 1] - item_offsets[i]);
        round_slots->push_back(slot);
    }
}

// Camera::CamFromImg with the host's libm for the candidates whose model needs it (camera_math.h has the why); the
// device lifts the others.  Returns whether there was any; nxy (2 per candidate) is written for those only.
inline bool lift_libm_candidates(const amc_triobs_problem& pb, std::vector<double>* nxy) {
    bool any = false;
    for (size_t c = 0; c < pb.num_cameras && !any; ++c) any = cam::needs_libm(pb.camera_models[c]);
    if (!any) return false;
    const uint64_t ncand = pb.item_offsets[pb.num_items];
    nxy->assign(2 * ncand, 0.0);
    any = false;
    for (uint64_t k = 0; k < ncand; ++k) {
        const uint32_t c = pb.image_cameras[pb.cand_image[k]];
        if (!cam::needs_libm(pb.camera_models[c])) continue;
        cam::cam_from_img(pb.camera_models[c], pb.camera_params + cam::kMaxParams * c, pb.cand_xy[2 * k], pb.cand_xy[2 * k + 1],
                          (*nxy)[2 * k], (*nxy)[2 * k + 1]);
        any = true;
    }
    return any;
}

}  // namespace triobs
}  // namespace amc
