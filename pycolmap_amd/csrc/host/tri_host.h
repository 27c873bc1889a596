// tri_host.h — estimate_triangulation (/root/reference/pycolmap/estimators/triangulation.h) over the C ABI of
// include/amc_tri.h: one track, run through amc_triangulate_tracks on the estimators' shared context, GIL released.
#pragma once

#include <array>
#include <vector>

#include "../../../include/amc_tri.h"
#include "controller.h"
#include "estimators.h"
#include "py_types.h"

namespace amchost {

// TriangulationEstimator::PointData: pixel and normalized image coordinates (only the latter enters the angular
// residual)
struct TriPointData {
    std::array<double, 2> point{{0, 0}};
    std::array<double, 2> point_normalized{{0, 0}};
};

// EstimateTriangulationOptions as the binding exposes it (residual_type stays ANGULAR_ERROR)
struct EstimateTriangulationOptions {
    double min_tri_angle = 0.0;
    RANSACOptions ransac;
};

// cam_from_world [R | t] of each image, as Rigid3d::ToMatrix builds it
inline std::array<double, 12> TriPoseMatrix(const PyRigid3d& cam_from_world) {
    const std::array<double, 9> R = cam_from_world.rotation.Matrix();
    std::array<double, 12> P;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) P[4 * r + c] = R[3 * r + c];
        P[4 * r + 3] = cam_from_world.translation[r];
    }
    return P;
}

// PyEstimateTriangulation after its size checks: None on failure, else {"xyz": (3,), "inliers": (n,) bool}
inline py::object EstimateTriangulationTrack(const std::vector<TriPointData>& point_data,
                                             const std::vector<std::array<double, 12>>& poses,
                                             const EstimateTriangulationOptions& options) {
    const size_t n = point_data.size();
    if (n < 2)  // CHECK_GE(point_data.size(), 2) of EstimateTriangulation
        throw py::value_error(CheckMessage(__FILE__, __LINE__, "point_data.size() >= 2 (" + std::to_string(n) + " vs. 2)"));
    amc_tri_opts o;
    amc_tri_opts_default(&o);
    o.min_tri_angle = options.min_tri_angle;
    o.max_error = options.ransac.max_error;
    o.min_inlier_ratio = options.ransac.min_inlier_ratio;
    o.confidence = options.ransac.confidence;
    o.dyn_num_trials_multiplier = options.ransac.dyn_num_trials_multiplier;
    o.min_num_trials = static_cast<int64_t>(options.ransac.min_num_trials);
    o.max_num_trials = static_cast<int64_t>(options.ransac.max_num_trials);
    std::vector<double> P(12 * n), xy(2 * n);
    std::vector<uint32_t> pose(n);
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 12; ++k) P[12 * i + k] = poses[i][k];
        xy[2 * i] = point_data[i].point_normalized[0];
        xy[2 * i + 1] = point_data[i].point_normalized[1];
        pose[i] = static_cast<uint32_t>(i);
    }
    const uint64_t off[2] = {0, n};
    amc_tri_result r{};
    {
        py::gil_scoped_release release;
        EstimatorCtx& E = TheEstimatorCtx();
        std::lock_guard<std::mutex> lock(E.mu);
        EstCheck(amc_triangulate_tracks(E.Get(), P.data(), n, off, 1, pose.data(), xy.data(), &o, &r),
                 "amc_triangulate_tracks");
    }
    if (!r.success[0]) {
        amc_tri_result_free(&r);
        return py::none();
    }
    py::array_t<double> xyz(3);
    py::array_t<bool> inl(static_cast<py::ssize_t>(n));
    for (int k = 0; k < 3; ++k) xyz.mutable_data()[k] = r.xyz[k];
    for (size_t i = 0; i < n; ++i) inl.mutable_data()[i] = r.inlier_mask[i] != 0;
    amc_tri_result_free(&r);
    return py::dict(py::arg("xyz") = xyz, py::arg("inliers") = inl);
}

}  // namespace amchost
