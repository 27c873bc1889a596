// ba_plan.h — the host half of bundle adjustment: the checks of amc_ba_opts and amc_ba_problem, the
// variable columns, the observations in image order, the points' observation lists and the cameras' image lists.  No HIP
// here: tests/shim/ba_plan_fuzz.cc runs it under ASan + UBSan.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "camera_math.h"
#include "../../include/amc_ba.h"

namespace amc {
namespace ba {

struct Plan {
    uint64_t num_variable = 0;   // tangent columns of the system
    uint32_t kc = 0;             // the largest parameter count among the cameras
    bool camvar = false;         // is any camera parameter variable
    std::vector<uint8_t> cvar, ivar;            // 12 per camera, 6 per image: 1 = variable
    std::vector<uint8_t> pvar;                  // 1 per point: 1 = variable (0: a constant point, 15.12)
    std::vector<uint32_t> ioff, poff, coff;     // CSR offsets by image, by point, by camera
    std::vector<uint32_t> oimg, opt;            // image and point of each observation, in image order
    std::vector<double> oxy;                    // its pixel
    std::vector<uint32_t> pobs;                 // by point: indices into the image order, ascending
    std::vector<uint32_t> cimg;                 // by camera: image indices, ascending
    std::vector<double> cparams;                // 12 per camera: the model's parameters, then zeros
};

inline bool all_finite(const double* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!(p[i] - p[i] == 0.0)) return false;
    return true;
}

// empty string = valid
inline std::string check_options(const amc_ba_opts& o) {
    if (o.loss_function_type < 0 || o.loss_function_type > 2) return "loss_function_type in 0 .. 2";
    if (!(o.loss_function_scale > 0.0)) return "loss_function_scale > 0";
    if (o.max_num_iterations < 0) return "max_num_iterations >= 0";
    if (o.max_linear_solver_iterations < 1) return "max_linear_solver_iterations >= 1";
    if (o.max_num_consecutive_invalid_steps < 1) return "max_num_consecutive_invalid_steps >= 1";
    if (!(o.function_tolerance >= 0.0)) return "function_tolerance >= 0";
    if (!(o.gradient_tolerance >= 0.0)) return "gradient_tolerance >= 0";
    if (!(o.parameter_tolerance >= 0.0)) return "parameter_tolerance >= 0";
    return std::string();
}

// Checks the problem and fills the plan; returns what is wrong with the problem, or the empty string.  Nothing is read
// through an index before that index has been checked.  point_const: num_points bytes, non-zero = the point is constant
// (15.12), or NULL for no constant point.
inline std::string make_plan(const amc_ba_problem& pb, const uint8_t* point_const, Plan* plan) {
    constexpr int kP = cam::kMaxParams;
    const size_t ncam = pb.num_cameras, nimg = pb.num_images, npts = pb.num_points, nobs = pb.num_observations;
    if ((ncam && (!pb.camera_models || !pb.camera_params || !pb.camera_const)) ||
        (nimg && (!pb.image_cameras || !pb.qvec || !pb.tvec || !pb.pose_const)) || (npts && !pb.xyz) ||
        (nobs && (!pb.obs_image || !pb.obs_point || !pb.obs_xy)))
        return "NULL array";
    if (ncam > 0x3fffffffu / 16 || nimg > 0x3fffffffu / 16 || npts > 0x3fffffffu / 4 || nobs > 0x7fffffffu / 24)
        return "the problem is too large for 32-bit offsets";
    for (size_t c = 0; c < ncam; ++c)
        if (pb.camera_models[c] < 0 || pb.camera_models[c] >= cam::kNumModels)
            return "camera " + std::to_string(c) + " has model " + std::to_string(pb.camera_models[c]);
    for (size_t i = 0; i < nimg; ++i)
        if (pb.image_cameras[i] >= ncam)
            return "image " + std::to_string(i) + " has camera index " + std::to_string(pb.image_cameras[i]);
    std::vector<uint32_t> pcount(npts, 0), icount(nimg, 0);
    for (size_t o = 0; o < nobs; ++o) {
        if (pb.obs_image[o] >= nimg || pb.obs_point[o] >= npts)
            return "observation " + std::to_string(o) + " has an index out of range";
        ++pcount[pb.obs_point[o]];
        ++icount[pb.obs_image[o]];
    }
    for (size_t j = 0; j < npts; ++j) {
        const bool constant = point_const && point_const[j];
        if (constant ? pcount[j] < 1 : pcount[j] < 2)
            return "point " + std::to_string(j) + " has " + std::to_string(pcount[j]) + " observations (at least " +
                   (constant ? "one for a constant point)" : "two)");
    }
    bool fin = all_finite(pb.qvec, 4 * nimg) && all_finite(pb.tvec, 3 * nimg) && all_finite(pb.xyz, 3 * npts) &&
               all_finite(pb.obs_xy, 2 * nobs);
    for (size_t c = 0; c < ncam && fin; ++c) fin = all_finite(pb.camera_params + kP * c, cam::num_params(pb.camera_models[c]));
    if (!fin) return "an input value is not finite";

    Plan& p = *plan;
    p = Plan();
    p.cvar.assign(kP * ncam, 0);
    p.ivar.assign(6 * nimg, 0);
    p.cparams.assign(kP * ncam, 0.0);
    p.pvar.assign(npts, 1);
    for (size_t j = 0; j < npts; ++j) {
        if (point_const && point_const[j])
            p.pvar[j] = 0;
        else
            p.num_variable += 3;
    }
    for (size_t c = 0; c < ncam; ++c) {
        const int np = cam::num_params(pb.camera_models[c]);
        p.kc = std::max<uint32_t>(p.kc, (uint32_t)np);
        for (int k = 0; k < np; ++k) {
            p.cparams[kP * c + k] = pb.camera_params[kP * c + k];
            if (!pb.camera_const[kP * c + k]) {
                p.cvar[kP * c + k] = 1;
                p.camvar = true;
                ++p.num_variable;
            }
        }
    }
    for (size_t k = 0; k < 6 * nimg; ++k)
        if (!pb.pose_const[k]) {
            p.ivar[k] = 1;
            ++p.num_variable;
        }
    p.ioff.assign(nimg + 1, 0);
    p.poff.assign(npts + 1, 0);
    p.coff.assign(ncam + 1, 0);
    for (size_t i = 0; i < nimg; ++i) p.ioff[i + 1] = p.ioff[i] + icount[i];
    for (size_t j = 0; j < npts; ++j) p.poff[j + 1] = p.poff[j] + pcount[j];
    p.oimg.resize(nobs);
    p.opt.resize(nobs);
    p.oxy.resize(2 * nobs);
    p.pobs.resize(nobs);
    p.cimg.resize(nimg);
    std::vector<uint32_t> at(p.ioff.begin(), p.ioff.end() - 1);
    for (size_t o = 0; o < nobs; ++o) {  // by image, the input order within an image
        const uint32_t k = at[pb.obs_image[o]]++;
        p.oimg[k] = pb.obs_image[o];
        p.opt[k] = pb.obs_point[o];
        p.oxy[2 * k] = pb.obs_xy[2 * o];
        p.oxy[2 * k + 1] = pb.obs_xy[2 * o + 1];
    }
    std::vector<uint32_t> pat(p.poff.begin(), p.poff.end() - 1);
    for (size_t k = 0; k < nobs; ++k) p.pobs[pat[p.opt[k]]++] = (uint32_t)k;  // by point, image order within
    for (size_t i = 0; i < nimg; ++i) ++p.coff[pb.image_cameras[i] + 1];
    for (size_t c = 0; c < ncam; ++c) p.coff[c + 1] += p.coff[c];
    std::vector<uint32_t> cat(p.coff.begin(), p.coff.end() - 1);
    for (size_t i = 0; i < nimg; ++i) p.cimg[cat[pb.image_cameras[i]]++] = (uint32_t)i;
    return std::string();
}
inline std::string make_plan(const amc_ba_problem& pb, Plan* plan) { return make_plan(pb, nullptr, plan); }

}  // namespace ba
}  // namespace amc
