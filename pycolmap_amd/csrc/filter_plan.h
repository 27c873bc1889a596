// filter_plan.h — the host half of the point filter: the checks of amc_filter_opts and
// amc_filter_problem, a batch's two classes of points, and the reference's count from the verdicts.  No HIP here.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/amc_filter.h"

namespace amc {
namespace filt {

constexpr int kPlanNumModels = 11;  // COLMAP's camera model ids 0 .. 10

// empty string = valid
inline std::string check_options(const amc_filter_opts& o) {
    if (!(o.max_reproj_error >= 0.0)) return "max_reproj_error >= 0";
    if (!(o.min_tri_angle >= 0.0)) return "min_tri_angle >= 0";
    return std::string();
}

// What is wrong with the problem, or the empty string.  Nothing is read through an offset or an index before it has
// been checked.
inline std::string check_problem(const amc_filter_problem& pb) {
    const size_t ncam = pb.num_cameras, nimg = pb.num_images, npts = pb.num_points;
    if (!pb.track_offsets || (ncam && (!pb.camera_models || !pb.camera_params)) ||
        (nimg && (!pb.image_cameras || !pb.qvec || !pb.tvec)) || (npts && !pb.xyz))
        return "NULL array";
    if (ncam > 0x7fffffffu / 16 || nimg > 0x7fffffffu / 16) return "too many cameras or images for 32-bit indices";
    if (pb.track_offsets[0] != 0) return "track_offsets does not start at 0";
    for (size_t j = 0; j < npts; ++j)
        if (pb.track_offsets[j + 1] < pb.track_offsets[j])
            return "track_offsets decreases at point " + std::to_string(j);
    const uint64_t nobs = pb.track_offsets[npts];
    if (nobs && (!pb.obs_image || !pb.obs_xy)) return "NULL array";
    for (size_t j = 0; j < npts; ++j)
        if (pb.track_offsets[j + 1] - pb.track_offsets[j] > 0x7fffffffu / 32)
            return "point " + std::to_string(j) + " has too long a track for 32-bit offsets";
    for (size_t c = 0; c < ncam; ++c)
        if (pb.camera_models[c] < 0 || pb.camera_models[c] >= kPlanNumModels)
            return "camera " + std::to_string(c) + " has model " + std::to_string(pb.camera_models[c]);
    for (size_t i = 0; i < nimg; ++i)
        if (pb.image_cameras[i] >= ncam)
            return "image " + std::to_string(i) + " has camera index " + std::to_string(pb.image_cameras[i]);
    for (uint64_t o = 0; o < nobs; ++o)
        if (pb.obs_image[o] >= nimg)
            return "observation " + std::to_string(o) + " has image index " + std::to_string(pb.obs_image[o]);
    return std::string();
}

// A batch's points first .. last, appended to the call's plan: the batch-local offsets (last - first + 1 of them), the
// observations' batch-local point indices, and the wave class (selected points whose track has at least wave_min
// elements), ascending.  Every other point is the lane kernel's.
inline void plan_batch(const amc_filter_problem& pb, size_t first, size_t last, uint32_t wave_min,
                       std::vector<uint32_t>* offsets, std::vector<uint32_t>* obs_point, std::vector<uint32_t>* wave_points) {
    const uint64_t base = pb.track_offsets[first];
    for (size_t j = first; j <= last; ++j) offsets->push_back(static_cast<uint32_t>(pb.track_offsets[j] - base));
    for (size_t j = first; j < last; ++j) {
        const uint64_t n = pb.track_offsets[j + 1] - pb.track_offsets[j];
        obs_point->insert(obs_point->end(), static_cast<size_t>(n), static_cast<uint32_t>(j - first));
        if (n >= wave_min && (!pb.selected || pb.selected[j])) wave_points->push_back(static_cast<uint32_t>(j - first));
    }
}

// 16.3's count: a point that goes in stage one counts its whole track, a point that stays counts its marked elements,
// and a point that goes in stage two counts one more
inline uint64_t count_filtered(const uint64_t* track_offsets, size_t npts, const uint8_t* verdict, const uint8_t* deleted) {
    uint64_t n = 0;
    for (size_t j = 0; j < npts; ++j) {
        const uint64_t o0 = track_offsets[j], o1 = track_offsets[j + 1];
        if (verdict[j] == AMC_FILTER_SHORT_TRACK || verdict[j] == AMC_FILTER_REPROJECTION) {
            n += o1 - o0;
        } else if (verdict[j] == AMC_FILTER_KEPT || verdict[j] == AMC_FILTER_ANGLE) {
            for (uint64_t o = o0; o < o1; ++o) n += deleted[o] != 0;
            n += verdict[j] == AMC_FILTER_ANGLE;
        }
    }
    return n;
}

}  // namespace filt
}  // namespace amc
