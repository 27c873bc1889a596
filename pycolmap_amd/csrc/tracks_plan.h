// tracks_plan.h — the host half of the device calls of track completion and track merging: the
// checks of the options and the problems, every candidate's item, and a merge batch's own 32-bit offsets and indices.
// No HIP here.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/amc_tracks.h"

namespace amc {
namespace trk {

constexpr int kPlanNumModels = 11;  // COLMAP's camera model ids 0 .. 10

// empty string = valid
inline std::string check_options(const amc_complete_opts& o) {
    if (!(o.complete_max_reproj_error >= 0.0)) return "complete_max_reproj_error >= 0";
    return std::string();
}

// What is wrong with the problem, or the empty string.  Nothing is read through an offset or an index before it has
// been checked.
inline std::string check_problem(const amc_complete_problem& pb) {
    const size_t ncam = pb.num_cameras, nimg = pb.num_images, nit = pb.num_items;
    if (!pb.item_offsets || (ncam && (!pb.camera_models || !pb.camera_params)) ||
        (nimg && (!pb.image_cameras || !pb.qvec || !pb.tvec)) || (nit && !pb.item_xyz))
        return "NULL array";
    if (ncam > 0x7fffffffu / 16 || nimg > 0x7fffffffu / 16) return "too many cameras or images for 32-bit indices";
    if (nit > 0x7fffffffu / 4) return "too many items for 32-bit indices";
    if (pb.item_offsets[0] != 0) return "item_offsets does not start at 0";
    for (size_t i = 0; i < nit; ++i)
        if (pb.item_offsets[i + 1] < pb.item_offsets[i]) return "item_offsets decreases at item " + std::to_string(i);
    const uint64_t ncand = pb.item_offsets[nit];
    if (ncand && (!pb.cand_image || !pb.cand_xy)) return "NULL array";
    for (size_t c = 0; c < ncam; ++c)
        if (pb.camera_models[c] < 0 || pb.camera_models[c] >= kPlanNumModels)
            return "camera " + std::to_string(c) + " has model " + std::to_string(pb.camera_models[c]);
    for (size_t i = 0; i < nimg; ++i)
        if (pb.image_cameras[i] >= ncam)
            return "image " + std::to_string(i) + " has camera index " + std::to_string(pb.image_cameras[i]);
    for (uint64_t k = 0; k < ncand; ++k)
        if (pb.cand_image[k] >= nimg)
            return "candidate " + std::to_string(k) + " has image index " + std::to_string(pb.cand_image[k]);
    return std::string();
}

// the item of every candidate of a checked problem
inline std::vector<uint32_t> candidate_items(const amc_complete_problem& pb) {
    std::vector<uint32_t> item;
    item.reserve(static_cast<size_t>(pb.item_offsets[pb.num_items]));
    for (size_t i = 0; i < pb.num_items; ++i)
        item.insert(item.end(), static_cast<size_t>(pb.item_offsets[i + 1] - pb.item_offsets[i]), static_cast<uint32_t>(i));
    return item;
}

inline std::string check_merge_options(const amc_merge_opts& o) {
    if (!(o.merge_max_reproj_error >= 0.0)) return "merge_max_reproj_error >= 0";
    return std::string();
}

// What is wrong with the merge problem, or the empty string.  Nothing is read through an offset or an index before it
// has been checked; a problem that passes keeps every index the kernel follows inside its own component.
inline std::string check_merge_problem(const amc_merge_problem& pb) {
    const size_t ncam = pb.num_cameras, nimg = pb.num_images, nc = pb.num_components;
    if (!pb.comp_point_offsets || !pb.comp_root_offsets || !pb.point_obs_offsets || !pb.obs_corr_offsets ||
        (ncam && (!pb.camera_models || !pb.camera_params)) || (nimg && (!pb.image_cameras || !pb.qvec || !pb.tvec)))
        return "NULL array";
    if (ncam > 0x7fffffffu / 16 || nimg > 0x7fffffffu / 16) return "too many cameras or images for 32-bit indices";
    if (nc > 0x7fffffffu / 4) return "too many components for 32-bit indices";
    if (pb.comp_point_offsets[0] != 0 || pb.comp_root_offsets[0] != 0 || pb.point_obs_offsets[0] != 0 || pb.obs_corr_offsets[0] != 0)
        return "offsets do not start at 0";
    for (size_t c = 0; c < nc; ++c) {
        if (pb.comp_point_offsets[c + 1] <= pb.comp_point_offsets[c]) return "component " + std::to_string(c) + " has no point";
        if (pb.comp_root_offsets[c + 1] < pb.comp_root_offsets[c]) return "comp_root_offsets decreases at component " + std::to_string(c);
        if (pb.comp_point_offsets[c + 1] - pb.comp_point_offsets[c] > AMC_MERGE_MAX_COMPONENT_OBS)
            return "component " + std::to_string(c) + " has more than " + std::to_string(AMC_MERGE_MAX_COMPONENT_OBS) + " observations";
    }
    const uint64_t npts = pb.comp_point_offsets[nc], nroots = pb.comp_root_offsets[nc];
    if (npts > 0x7fffffffu / 4 || nroots > 0x7fffffffu / 4) return "too many points or roots for 32-bit indices";
    if ((npts && !pb.point_xyz) || (nroots && !pb.roots)) return "NULL array";
    for (uint64_t p = 0; p < npts; ++p)
        if (pb.point_obs_offsets[p + 1] <= pb.point_obs_offsets[p]) return "point " + std::to_string(p) + " has no observation";
    const uint64_t nobs = pb.point_obs_offsets[npts];
    if (nobs > 0x7fffffffu / 4) return "too many observations for 32-bit indices";
    if (nobs && (!pb.obs_image || !pb.obs_xy)) return "NULL array";
    for (uint64_t o = 0; o < nobs; ++o)
        if (pb.obs_corr_offsets[o + 1] < pb.obs_corr_offsets[o]) return "obs_corr_offsets decreases at observation " + std::to_string(o);
    const uint64_t ncorr = pb.obs_corr_offsets[nobs];
    if (ncorr > 0x7fffffffu) return "too many correspondences for 32-bit indices";
    if (ncorr && !pb.corr_obs) return "NULL array";
    for (size_t c = 0; c < ncam; ++c)
        if (pb.camera_models[c] < 0 || pb.camera_models[c] >= kPlanNumModels)
            return "camera " + std::to_string(c) + " has model " + std::to_string(pb.camera_models[c]);
    for (size_t i = 0; i < nimg; ++i)
        if (pb.image_cameras[i] >= ncam)
            return "image " + std::to_string(i) + " has camera index " + std::to_string(pb.image_cameras[i]);
    for (uint64_t o = 0; o < nobs; ++o)
        if (pb.obs_image[o] >= nimg)
            return "observation " + std::to_string(o) + " has image index " + std::to_string(pb.obs_image[o]);
    for (size_t c = 0; c < nc; ++c) {
        const uint64_t p0 = pb.comp_point_offsets[c], p1 = pb.comp_point_offsets[c + 1];
        const uint64_t o0 = pb.point_obs_offsets[p0], o1 = pb.point_obs_offsets[p1];
        if (o1 - o0 > AMC_MERGE_MAX_COMPONENT_OBS)
            return "component " + std::to_string(c) + " has " + std::to_string(o1 - o0) + " observations, more than " +
                   std::to_string(AMC_MERGE_MAX_COMPONENT_OBS);
        for (uint64_t r = pb.comp_root_offsets[c]; r < pb.comp_root_offsets[c + 1]; ++r)
            if (pb.roots[r] < p0 || pb.roots[r] >= p1) return "root " + std::to_string(r) + " is outside its component";
        for (uint64_t k = pb.obs_corr_offsets[o0]; k < pb.obs_corr_offsets[o1]; ++k)
            if (pb.corr_obs[k] < o0 || pb.corr_obs[k] >= o1) return "correspondence " + std::to_string(k) + " is outside its component";
    }
    return std::string();
}

// the observations' offsets of a checked merge problem's components (num_components + 1): what the split goes by
inline std::vector<uint64_t> component_obs_offsets(const amc_merge_problem& pb) {
    std::vector<uint64_t> off(pb.num_components + 1);
    for (size_t c = 0; c <= pb.num_components; ++c) off[c] = pb.point_obs_offsets[pb.comp_point_offsets[c]];
    return off;
}

// A batch's components first .. last with offsets and indices that count from the batch's own first point, root,
// observation and correspondence.
struct MergeBatchPlan {
    std::vector<uint32_t> comp_point, comp_root, roots, point_obs, obs_corr, corr_obs;
};
inline MergeBatchPlan plan_merge_batch(const amc_merge_problem& pb, size_t first, size_t last) {
    MergeBatchPlan b;
    const uint64_t p0 = pb.comp_point_offsets[first], p1 = pb.comp_point_offsets[last];
    const uint64_t r0 = pb.comp_root_offsets[first], r1 = pb.comp_root_offsets[last];
    const uint64_t o0 = pb.point_obs_offsets[p0], o1 = pb.point_obs_offsets[p1];
    const uint64_t k0 = pb.obs_corr_offsets[o0], k1 = pb.obs_corr_offsets[o1];
    for (size_t c = first; c <= last; ++c) {
        b.comp_point.push_back(static_cast<uint32_t>(pb.comp_point_offsets[c] - p0));
        b.comp_root.push_back(static_cast<uint32_t>(pb.comp_root_offsets[c] - r0));
    }
    for (uint64_t r = r0; r < r1; ++r) b.roots.push_back(static_cast<uint32_t>(pb.roots[r] - p0));
    for (uint64_t p = p0; p <= p1; ++p) b.point_obs.push_back(static_cast<uint32_t>(pb.point_obs_offsets[p] - o0));
    for (uint64_t o = o0; o <= o1; ++o) b.obs_corr.push_back(static_cast<uint32_t>(pb.obs_corr_offsets[o] - k0));
    for (uint64_t k = k0; k < k1; ++k) b.corr_obs.push_back(static_cast<uint32_t>(pb.corr_obs[k] - o0));
    return b;
}

}  // namespace trk
}  // namespace amc
