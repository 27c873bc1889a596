// rigpose_host.h — rig_absolute_pose_estimation (pycolmap/estimators/generalized_absolute_pose.h of the reference
// binding) over the C ABI of include/amc_rigpose.h: one query, run through amc_estimate_rig_absolute_poses on the
// estimators' shared context, GIL released.
#pragma once

#include <algorithm>
#include <array>
#include <string>
#include <vector>

#include "../../../include/amc_rigpose.h"
#include "abspose_host.h"

namespace amchost {

// THROW_CHECK_GE / THROW_CHECK_LT on the camera indices: ValueError "[file:line] Check Failed: a op b (x vs. y)"
#define CheckIndexBound(ok, a, b, what) CheckIndexBoundAt(__FILE__, __LINE__, (ok), (a), (b), (what))
inline void CheckIndexBoundAt(const char* file, int line, bool ok, long long a, long long b, const char* what) {
    if (!ok)
        throw py::value_error(CheckMessage(file, line, std::string(what) + " (" + std::to_string(a) + " vs. " +
                                                             std::to_string(b) + ")"));
}

// PyEstimateAndRefineGeneralizedAbsolutePose
inline py::object EstimateAndRefineGeneralizedAbsolutePose(const py::object& points2D, const py::object& points3D,
                                                           const py::object& camera_idxs,
                                                           const std::vector<PyRigid3d>& cams_from_rig,
                                                           std::vector<PyCamera>& cameras, const RANSACOptions& eo,
                                                           const AbsolutePoseRefinementOptions& ro,
                                                           bool return_covariance) {
    const amc_abspose_refine_opts r = ToRefineOpts(ro);
    const std::vector<double> p2 = PointRows(points2D, 2, "points2D"), p3 = PointRows(points3D, 3, "points3D");
    const auto ia = py::array_t<long long, py::array::c_style | py::array::forcecast>::ensure(camera_idxs);
    if (!ia || ia.ndim() > 1) throw py::value_error("camera_idxs must be convertible to a list of integers");
    const size_t n = p2.size() / 2, ncam = cameras.size();
    CheckSameSize(n, p3.size() / 3, "points2D.size() == points3D.size()");
    CheckSameSize(n, static_cast<size_t>(ia.size()), "points2D.size() == camera_idxs.size()");
    CheckSameSize(cams_from_rig.size(), ncam, "cams_from_rig.size() == cameras.size()");
    if (n == 0) return py::none();  // the reference dereferences the end of an empty range
    const long long lo = *std::min_element(ia.data(), ia.data() + n), hi = *std::max_element(ia.data(), ia.data() + n);
    CheckIndexBound(lo >= 0, lo, 0, "*std::min_element(camera_idxs.begin(), camera_idxs.end()) >= 0");
    CheckIndexBound(hi < static_cast<long long>(ncam), hi, static_cast<long long>(ncam),
                    "*std::max_element(camera_idxs.begin(), camera_idxs.end()) < cameras.size()");
    amc_ransac_opts o;
    o.max_error = eo.max_error;
    o.min_inlier_ratio = eo.min_inlier_ratio;
    o.confidence = eo.confidence;
    o.dyn_num_trials_multiplier = eo.dyn_num_trials_multiplier;
    o.min_num_trials = static_cast<int64_t>(eo.min_num_trials);
    o.max_num_trials = static_cast<int64_t>(eo.max_num_trials);
    std::vector<int32_t> models(ncam), idx(n);
    std::vector<double> prm(12 * ncam), rigs(7 * ncam);
    for (size_t c = 0; c < ncam; ++c) {
        models[c] = cameras[c].model;
        const std::array<double, 12> p = CameraParams12(cameras[c]);
        std::copy(p.begin(), p.end(), prm.begin() + 12 * c);
        for (int i = 0; i < 4; ++i) rigs[7 * c + i] = cams_from_rig[c].rotation.xyzw[i];
        for (int i = 0; i < 3; ++i) rigs[7 * c + 4 + i] = cams_from_rig[c].translation[i];
    }
    for (size_t k = 0; k < n; ++k) idx[k] = static_cast<int32_t>(ia.data()[k]);
    const uint64_t off[2] = {0, n}, coff[2] = {0, ncam};
    amc_rigpose_result res{};
    {
        py::gil_scoped_release release;
        EstimatorCtx& E = TheEstimatorCtx();
        std::lock_guard<std::mutex> lock(E.mu);
        EstCheck(amc_estimate_rig_absolute_poses(E.Get(), off, 1, coff, models.data(), prm.data(), rigs.data(),
                                                 idx.data(), p2.data(), p3.data(), &o, &r, return_covariance ? 1 : 0,
                                                 &res),
                 "amc_estimate_rig_absolute_poses");
    }
    if (!res.success[0]) {
        amc_rigpose_result_free(&res);
        return py::none();
    }
    py::array_t<bool> inl(static_cast<py::ssize_t>(n));
    for (size_t i = 0; i < n; ++i) inl.mutable_data()[i] = res.inlier_mask[i] != 0;
    PyRigid3d g;
    for (int i = 0; i < 4; ++i) g.rotation.xyzw[i] = res.qvec[i];
    for (int i = 0; i < 3; ++i) g.translation[i] = res.tvec[i];
    py::dict d;
    d["rig_from_world"] = g;
    d["num_inliers"] = static_cast<size_t>(res.num_inliers[0]);
    d["inliers"] = inl;
    if (return_covariance) {
        py::array_t<double> cov({6, 6});
        for (int i = 0; i < 36; ++i) cov.mutable_data()[i] = res.covariance[i];
        d["covariance"] = cov;
    }
    amc_rigpose_result_free(&res);
    return d;
}

}  // namespace amchost
