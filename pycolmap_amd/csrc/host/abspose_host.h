// abspose_host.h — absolute_pose_estimation / pose_refinement (pycolmap/estimators/absolute_pose.h of the reference
// binding) over the C ABI of include/amc_abspose.h: one query, run through amc_estimate_absolute_poses /
// amc_refine_absolute_poses on the estimators' shared context, GIL released.
#pragma once

#include <array>
#include <string>
#include <vector>

#include "../../../include/amc_abspose.h"
#include "controller.h"
#include "estimators.h"
#include "py_types.h"

namespace amchost {

// AbsolutePoseEstimationOptions as the binding builds it (ransac: pycolmap's RANSACOptions() with max_error = 12)
struct AbsolutePoseEstimationOptions {
    bool estimate_focal_length = false;
    int num_focal_length_samples = 30;
    double min_focal_length_ratio = 0.1;
    double max_focal_length_ratio = 10.0;
    RANSACOptions ransac;
};
// AbsolutePoseRefinementOptions; refine_focal_length / refine_extra_params must stay false, print_summary has no
// effect
struct AbsolutePoseRefinementOptions {
    double gradient_tolerance = 1.0;
    int max_num_iterations = 100;
    double loss_function_scale = 1.0;
    bool refine_focal_length = false;
    bool refine_extra_params = false;
    bool print_summary = false;
};

inline amc_abspose_refine_opts ToRefineOpts(const AbsolutePoseRefinementOptions& r) {
    if (r.refine_focal_length)
        throw py::value_error("refine_focal_length=True is not supported (DESIGN.md 12, deviation A11)");
    if (r.refine_extra_params)
        throw py::value_error("refine_extra_params=True is not supported (DESIGN.md 12, deviation A11)");
    amc_abspose_refine_opts o;
    amc_abspose_refine_opts_default(&o);
    o.gradient_tolerance = r.gradient_tolerance;
    o.max_num_iterations = r.max_num_iterations;
    o.loss_function_scale = r.loss_function_scale;
    o.refine_focal_length = r.refine_focal_length ? 1 : 0;
    o.refine_extra_params = r.refine_extra_params ? 1 : 0;
    o.print_summary = r.print_summary ? 1 : 0;
    return o;
}

// N x `cols` float64 rows from an array or a list of vectors (an empty input is 0 rows)
inline std::vector<double> PointRows(const py::object& obj, int cols, const char* name) {
    const auto a = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(obj);
    if (!a) throw py::value_error(std::string(name) + " must be convertible to an N x " + std::to_string(cols) + " array");
    if (a.size() == 0) return {};
    if (a.ndim() != 2 || a.shape(1) != cols)
        throw py::value_error(std::string(name) + " must be an N x " + std::to_string(cols) + " array");
    return std::vector<double>(a.data(), a.data() + a.size());
}

inline std::array<double, 12> CameraParams12(const PyCamera& c) {
    c.CheckParams();
    std::array<double, 12> p{};
    for (size_t i = 0; i < c.params.size() && i < 12; ++i) p[i] = c.params[i];
    return p;
}

inline PyRigid3d PoseOf(const amc_abspose_result& r) {
    PyRigid3d g;
    for (int i = 0; i < 4; ++i) g.rotation.xyzw[i] = r.qvec[i];
    for (int i = 0; i < 3; ++i) g.translation[i] = r.tvec[i];
    return g;
}

// PyEstimateAndRefineAbsolutePose
inline py::object EstimateAndRefineAbsolutePose(const py::object& points2D, const py::object& points3D, PyCamera& camera,
                                                const AbsolutePoseEstimationOptions& eo,
                                                const AbsolutePoseRefinementOptions& ro, bool return_covariance) {
    const amc_abspose_refine_opts r = ToRefineOpts(ro);
    const std::vector<double> p2 = PointRows(points2D, 2, "points2D"), p3 = PointRows(points3D, 3, "points3D");
    const size_t n = p2.size() / 2;
    CheckSameSize(n, p3.size() / 3, "points2D.size() == points3D.size()");
    amc_abspose_opts o;
    amc_abspose_opts_default(&o);
    o.estimate_focal_length = eo.estimate_focal_length ? 1 : 0;
    o.num_focal_length_samples = eo.num_focal_length_samples;
    o.min_focal_length_ratio = eo.min_focal_length_ratio;
    o.max_focal_length_ratio = eo.max_focal_length_ratio;
    o.max_error = eo.ransac.max_error;
    o.min_inlier_ratio = eo.ransac.min_inlier_ratio;
    o.confidence = eo.ransac.confidence;
    o.dyn_num_trials_multiplier = eo.ransac.dyn_num_trials_multiplier;
    o.min_num_trials = static_cast<int64_t>(eo.ransac.min_num_trials);
    o.max_num_trials = static_cast<int64_t>(eo.ransac.max_num_trials);
    const std::array<double, 12> prm = CameraParams12(camera);
    const int32_t model = camera.model;
    const uint64_t off[2] = {0, n};
    amc_abspose_result res{};
    {
        py::gil_scoped_release release;
        EstimatorCtx& E = TheEstimatorCtx();
        std::lock_guard<std::mutex> lock(E.mu);
        EstCheck(amc_estimate_absolute_poses(E.Get(), off, 1, &model, prm.data(), p2.data(), p3.data(), &o, &r,
                                             return_covariance ? 1 : 0, &res),
                 "amc_estimate_absolute_poses");
    }
    // EstimateAbsolutePose scales the caller's camera before the refinement, whatever the refinement then says
    if (eo.estimate_focal_length && res.num_inliers[0] > 0)
        for (int i = 0; i < camera.Info().num_focal; ++i) camera.params[i] *= res.focal_factor[0];
    if (!res.success[0]) {
        amc_abspose_result_free(&res);
        return py::none();
    }
    py::array_t<bool> inl(static_cast<py::ssize_t>(n));
    for (size_t i = 0; i < n; ++i) inl.mutable_data()[i] = res.inlier_mask[i] != 0;
    py::dict d;
    d["cam_from_world"] = PoseOf(res);
    d["num_inliers"] = static_cast<size_t>(res.num_inliers[0]);
    d["inliers"] = inl;
    if (return_covariance) {
        py::array_t<double> cov({6, 6});
        for (int i = 0; i < 36; ++i) cov.mutable_data()[i] = res.covariance[i];
        d["covariance"] = cov;
    }
    amc_abspose_result_free(&res);
    return d;
}

// PyRefineAbsolutePose
inline py::object RefineAbsolutePose(const PyRigid3d& init, const py::object& points2D, const py::object& points3D,
                                     const py::object& inlier_mask, const PyCamera& camera,
                                     const AbsolutePoseRefinementOptions& ro) {
    const amc_abspose_refine_opts r = ToRefineOpts(ro);
    const std::vector<double> p2 = PointRows(points2D, 2, "points2D"), p3 = PointRows(points3D, 3, "points3D");
    const size_t n = p2.size() / 2;
    const auto m = py::array_t<bool, py::array::c_style | py::array::forcecast>::ensure(inlier_mask);
    if (!m) throw py::value_error("inlier_mask must be convertible to a boolean array");
    CheckSameSize(n, p3.size() / 3, "points2D.size() == points3D.size()");
    CheckSameSize(static_cast<size_t>(m.size()), n, "inlier_mask.size() == points2D.size()");
    std::vector<uint8_t> mask(n);
    for (size_t i = 0; i < n; ++i) mask[i] = m.data()[i] ? 1 : 0;
    const std::array<double, 12> prm = CameraParams12(camera);
    const int32_t model = camera.model;
    const uint64_t off[2] = {0, n};
    amc_abspose_result res{};
    {
        py::gil_scoped_release release;
        EstimatorCtx& E = TheEstimatorCtx();
        std::lock_guard<std::mutex> lock(E.mu);
        EstCheck(amc_refine_absolute_poses(E.Get(), off, 1, &model, prm.data(), p2.data(), p3.data(),
                                           init.rotation.xyzw.data(), init.translation.data(), mask.data(), &r, 0,
                                           &res),
                 "amc_refine_absolute_poses");
    }
    if (!res.success[0]) {
        amc_abspose_result_free(&res);
        return py::none();
    }
    py::dict d;
    d["cam_from_world"] = PoseOf(res);
    amc_abspose_result_free(&res);
    return d;
}

}  // namespace amchost
