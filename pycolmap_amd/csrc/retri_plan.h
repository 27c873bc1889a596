// retri_plan.h — the host half of the pair retriangulator: the checks of amc_retri_opts and
// amc_retri_problem, the launches of a call (the rounds in order, a round cut on pair boundaries) and the lift of the
// observations whose camera model needs libm.  No HIP here.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/amc_retri.h"
#include "camera_math.h"

namespace amc {
namespace retri {

// A launch's correspondences: a lane each, 2^20 of them are 4096 workgroups, sixteen per compute unit, and a lane's
// work is bounded (one angular error, or one 4 x 4 Jacobi and four residuals), so no launch holds the stream for long.
constexpr uint64_t kMaxLaunchCorrs = (uint64_t)1 << 20;

// empty string = valid
inline std::string check_options(const amc_retri_opts& o) {
    if (!(o.create_max_angle_error > 0.0)) return "create_max_angle_error > 0";
    if (!(o.re_max_angle_error >= 0.0)) return "re_max_angle_error >= 0";
    if (!(o.min_angle >= 0.0)) return "min_angle >= 0";
    if (!(o.re_min_ratio >= 0.0)) return "re_min_ratio >= 0";
    return std::string();
}

// What is wrong with the problem, or the empty string.  Nothing is read through an offset or an index before it has
// been checked.
inline std::string check_problem(const amc_retri_problem& pb) {
    const size_t ncam = pb.num_cameras, nimg = pb.num_images, nobs = pb.num_obs, npt = pb.num_points, np = pb.num_pairs,
                 nr = pb.num_rounds;
    if (!pb.pair_offsets || !pb.round_offsets || (ncam && (!pb.camera_models || !pb.camera_params)) ||
        (nimg && (!pb.image_cameras || !pb.qvec || !pb.tvec)) || (nobs && (!pb.obs_image || !pb.obs_xy || !pb.obs_point)) ||
        (npt && !pb.point_xyz) || (np && !pb.pair_images))
        return "NULL array";
    if (ncam > 0x7fffffffu / 16 || nimg > 0x7fffffffu / 16 || nobs > 0x7fffffffu || np > 0x7fffffffu || npt > 0x7fffffffu)
        return "too many cameras, images, observations, points or pairs for 32-bit indices";
    if (pb.pair_offsets[0] != 0) return "pair_offsets does not start at 0";
    for (size_t p = 0; p < np; ++p)
        if (pb.pair_offsets[p + 1] < pb.pair_offsets[p]) return "pair_offsets decreases at pair " + std::to_string(p);
    const uint64_t nc = pb.pair_offsets[np];
    if (nc > AMC_RETRI_MAX_CORRS)
        return std::to_string(nc) + " correspondences, more than " + std::to_string(AMC_RETRI_MAX_CORRS) + " (AMC_RETRI_MAX_CORRS)";
    if (nc + npt > 0x7fffffffu) return "too many points and correspondences for 32-bit point slots";
    if (nc && !pb.corr_obs) return "NULL array";
    // what bounds the working set by the correspondences: a correspondence uses two observations, an observation one point
    if (nobs > 2 * nc) return std::to_string(nobs) + " observations, more than two per correspondence (" + std::to_string(nc) + " correspondences)";
    if (npt > 2 * nc) return std::to_string(npt) + " points, more than two per correspondence (" + std::to_string(nc) + " correspondences)";
    if (pb.round_offsets[0] != 0) return "round_offsets does not start at 0";
    for (size_t r = 0; r < nr; ++r)
        if (pb.round_offsets[r + 1] < pb.round_offsets[r]) return "round_offsets decreases at round " + std::to_string(r);
    if (pb.round_offsets[nr] != np) return "round_offsets ends at " + std::to_string(pb.round_offsets[nr]) + ", " + std::to_string(np) + " pairs";
    for (size_t c = 0; c < ncam; ++c)
        if (pb.camera_models[c] < 0 || pb.camera_models[c] >= cam::kNumModels)
            return "camera " + std::to_string(c) + " has model " + std::to_string(pb.camera_models[c]);
    for (size_t i = 0; i < nimg; ++i)
        if (pb.image_cameras[i] >= ncam)
            return "image " + std::to_string(i) + " has camera index " + std::to_string(pb.image_cameras[i]);
    for (size_t o = 0; o < nobs; ++o) {
        if (pb.obs_image[o] >= nimg) return "observation " + std::to_string(o) + " has image index " + std::to_string(pb.obs_image[o]);
        if (pb.obs_point[o] < -1 || (pb.obs_point[o] >= 0 && static_cast<size_t>(pb.obs_point[o]) >= npt))
            return "observation " + std::to_string(o) + " has point index " + std::to_string(pb.obs_point[o]);
    }
    // a round's pairs share no image: the image's stamp is the last round that used it
    std::vector<uint64_t> image_round(nimg, 0), obs_pair(nobs, 0);
    for (size_t r = 0; r < nr; ++r)
        for (uint64_t p = pb.round_offsets[r]; p < pb.round_offsets[r + 1]; ++p) {
            const uint32_t a = pb.pair_images[2 * p], b = pb.pair_images[2 * p + 1];
            if (a >= nimg || b >= nimg || a == b)
                return "pair " + std::to_string(p) + " has the images " + std::to_string(a) + " and " + std::to_string(b);
            if (image_round[a] == r + 1 || image_round[b] == r + 1)
                return "round " + std::to_string(r) + " has two pairs with image " + std::to_string(image_round[a] == r + 1 ? a : b);
            image_round[a] = image_round[b] = r + 1;
            for (uint64_t k = pb.pair_offsets[p]; k < pb.pair_offsets[p + 1]; ++k)
                for (int s = 0; s < 2; ++s) {
                    const uint32_t o = pb.corr_obs[2 * k + s];
                    if (o >= nobs) return "correspondence " + std::to_string(k) + " has observation index " + std::to_string(o);
                    if (pb.obs_image[o] != pb.pair_images[2 * p + s])
                        return "correspondence " + std::to_string(k) + " has an observation of image " + std::to_string(pb.obs_image[o]) +
                               ", not of its pair's image " + std::to_string(pb.pair_images[2 * p + s]);
                    if (obs_pair[o] == p + 1) return "pair " + std::to_string(p) + " lists observation " + std::to_string(o) + " twice";
                    obs_pair[o] = p + 1;
                }
        }
    return std::string();
}

// one ratio kernel and one correspondence kernel: the pairs first .. last of one round
struct Launch {
    uint64_t first, last;
};

// The call's launches: the rounds in order, a round's pairs in order, cut greedily so that a launch holds at most
// max_corrs correspondences; a larger pair is a launch of its own.  A round without pairs has no launch.
inline std::vector<Launch> plan_launches(const amc_retri_problem& pb, uint64_t max_corrs) {
    std::vector<Launch> out;
    for (size_t r = 0; r < pb.num_rounds; ++r)
        for (uint64_t i = pb.round_offsets[r]; i < pb.round_offsets[r + 1];) {
            uint64_t j = i + 1;
            while (j < pb.round_offsets[r + 1] && pb.pair_offsets[j + 1] - pb.pair_offsets[i] <= max_corrs) ++j;
            out.push_back(Launch{i, j});
            i = j;
        }
    return out;
}

// Camera::CamFromImg with the host's libm for the observations whose model needs it (camera_math.h has the why); the
// device lifts the others.  Returns whether there was any; nxy (2 per observation) is written for those only.
inline bool lift_libm_observations(const amc_retri_problem& pb, std::vector<double>* nxy) {
    bool any = false;
    for (size_t c = 0; c < pb.num_cameras && !any; ++c) any = cam::needs_libm(pb.camera_models[c]);
    if (!any) return false;
    nxy->assign(2 * pb.num_obs, 0.0);
    any = false;
    for (size_t o = 0; o < pb.num_obs; ++o) {
        const uint32_t c = pb.image_cameras[pb.obs_image[o]];
        if (!cam::needs_libm(pb.camera_models[c])) continue;
        cam::cam_from_img(pb.camera_models[c], pb.camera_params + cam::kMaxParams * c, pb.obs_xy[2 * o], pb.obs_xy[2 * o + 1],
                          (*nxy)[2 * o], (*nxy)[2 * o + 1]);
        any = true;
    }
    return any;
}

}  // namespace retri
}  // namespace amc
