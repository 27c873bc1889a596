// bind_bundle.cc — LossFunctionType, CeresSolverOptions, BundleAdjustmentOptions, bundle_adjustment
// (/root/reference/pycolmap/pipeline/sfm.h:95-103, 259-362; ba_host.h), BundleAdjustmentConfig and
// BundleAdjuster (COLMAP 3.9.1's classes under the names later pycolmap releases bind; ba_config_host.h).
#include <map>

#include "ba_host.h"
#include "py_scene.h"
#include "reconstruction.h"

namespace amchost {

amc_ba_opts ToAmcBaOpts(const BundleAdjustmentOptions& o) {
    amc_ba_opts opts;
    amc_ba_opts_default(&opts);
    opts.loss_function_type = static_cast<int32_t>(o.loss_function_type);
    opts.loss_function_scale = o.loss_function_scale;
    opts.max_num_iterations = o.solver_options.max_num_iterations;
    opts.max_linear_solver_iterations = o.solver_options.max_linear_solver_iterations;
    opts.max_num_consecutive_invalid_steps = o.solver_options.max_num_consecutive_invalid_steps;
    opts.function_tolerance = o.solver_options.function_tolerance;
    opts.gradient_tolerance = o.solver_options.gradient_tolerance;
    opts.parameter_tolerance = o.solver_options.parameter_tolerance;
    return opts;
}

namespace {

const char* TerminationName(int termination) {
    static const char* const kTermination[] = {"FUNCTION_TOLERANCE", "PARAMETER_TOLERANCE", "GRADIENT_TOLERANCE", "MAX_ITERATIONS",
                                               "MIN_RADIUS", "INVALID_STEPS", "NOTHING_TO_REFINE"};
    return kTermination[termination >= 0 && termination < 7 ? termination : 5];
}
BaRefineFlags RefineFlags(const BundleAdjustmentOptions& o) {
    return BaRefineFlags{o.refine_focal_length, o.refine_principal_point, o.refine_extra_params, o.refine_extrinsics};
}
// what the solver left in the result, in the statistics' order
void SolverStats(const amc_ba_result& res, py::dict& st) {
    st["initial_cost"] = res.initial_cost;
    st["final_cost"] = res.final_cost;
    st["num_successful_steps"] = res.num_successful_steps;
    st["num_unsuccessful_steps"] = res.num_unsuccessful_steps;
    st["num_pcg_iterations"] = res.num_pcg_iterations;
    st["termination"] = TerminationName(res.termination);
    st["device_ms"] = res.device_ms;
    st["kernel_ms"] = res.kernel_ms;
}
py::dict FlatBaDict(const FlatBa& f) {
    py::dict d;
    d["camera_models"] = NpArray(f.camera_models, 1);
    d["camera_params"] = NpArray(f.camera_params, 12);
    d["camera_const"] = NpArray(f.camera_const, 12);
    d["image_cameras"] = NpArray(f.image_cameras, 1);
    d["qvec"] = NpArray(f.qvec, 4);
    d["tvec"] = NpArray(f.tvec, 3);
    d["pose_const"] = NpArray(f.pose_const, 6);
    d["xyz"] = NpArray(f.xyz, 3);
    d["obs_image"] = NpArray(f.obs_image, 1);
    d["obs_point"] = NpArray(f.obs_point, 1);
    d["obs_xy"] = NpArray(f.obs_xy, 2);
    return d;
}

// the flat problem bundle_adjustment hands to amc_bundle_adjust, after the controller's filter (a test hook: the GPU
// tests run Context.bundle_adjust on it)
py::dict flat_problem(const PyReconstruction& r, const BundleAdjustmentOptions& o) {
    SparseModel model = checked_model(r);
    FilterObservationsWithNegativeDepth(&model);
    size_t skipped = 0;
    return FlatBaDict(FlattenForBundleAdjustment(model, RefineFlags(o), &skipped));
}

void bundle_adjustment(PyReconstruction& r, const BundleAdjustmentOptions& o) {
    const auto t0 = std::chrono::steady_clock::now();
    if (r.images.size() < 2) {
        const auto f = PythonCallFrame();
        Logging::Write(Logging::ERROR, f.first, f.second, "Need at least two views.");
        return;
    }
    SparseModel model = checked_model(r);
    const size_t filtered = FilterObservationsWithNegativeDepth(&model);
    size_t skipped = 0;
    FlatBa flat = FlattenForBundleAdjustment(model, RefineFlags(o), &skipped);
    const amc_ba_opts opts = ToAmcBaOpts(o);
    amc_ba_problem pb = flat.Problem();
    amc_ba_result res{};
    {   // not CallLibrary: a failure here is a RuntimeError, as for the single-call estimators
        py::gil_scoped_release release;
        EstimatorCtx& E = TheEstimatorCtx();
        std::lock_guard<std::mutex> lock(E.mu);
        EstCheck(amc_bundle_adjust(E.Get(), &pb, &opts, &res), "amc_bundle_adjust");
    }
    WriteBackBundleAdjustment(flat, &model);
    update_from_model(r, model);
    py::dict st;
    st["call"] = "bundle_adjustment";
    st["num_images"] = res.num_images;
    st["num_points"] = res.num_points;
    st["num_observations"] = res.num_observations;
    st["num_variable_parameters"] = res.num_variable_parameters;
    st["num_filtered_observations"] = filtered;
    st["num_skipped_points"] = skipped;
    SolverStats(res, st);
    st["host_ms"] = HostMs(t0, res.device_ms);
    SetLastStats(st);
}

FlatBaConfig adjuster_flat(const PyBundleAdjuster& a, const PyReconstruction& r, SparseModel* model) {
    *model = checked_model(r);
    return FlattenForBundleAdjuster(*model, a.config, RefineFlags(a.options));
}
py::dict adjuster_dict(const FlatBaConfig& fc) {
    py::dict d = FlatBaDict(fc.flat);
    d["point_const"] = NpArray(fc.point_const, 1);
    d["camera_at"] = NpArray(fc.camera_at, 1);
    d["image_at"] = NpArray(fc.image_at, 1);
    d["point_at"] = NpArray(fc.point_at, 1);
    d["num_skipped_points"] = fc.skipped_points;
    return d;
}

}  // namespace

// Solve: one amc_bundle_adjust_masked call on the config's part of the checked model.  Nothing of r
// changes unless the call succeeds.  Without a device the call raises pycolmap_amd._capi.AmcError.
// solver: None, or a callable that stands in for the library (a test hook: the CPU tests pass the reference): it takes
// the flat problem as a dict of arrays with the options and returns camera_params, qvec, tvec, xyz and the statistics.
bool adjuster_solve(PyBundleAdjuster& a, PyReconstruction& r, const py::object& solver) {
    const auto t0 = std::chrono::steady_clock::now();
    SparseModel model;
    FlatBaConfig fc = adjuster_flat(a, r, &model);
    FlatBa& flat = fc.flat;
    if (flat.obs_image.empty()) return false;  // COLMAP: "No residuals" — nothing to solve
    const amc_ba_opts opts = ToAmcBaOpts(a.options);
    py::dict st;
    st["call"] = "BundleAdjuster.solve";
    st["num_images"] = flat.image_cameras.size();
    st["num_points"] = fc.point_at.size();
    st["num_observations"] = flat.obs_image.size();
    st["num_filtered_observations"] = 0;
    st["num_skipped_points"] = fc.skipped_points;
    st["num_constant_points"] = fc.num_constant_points;
    if (!solver.is_none()) {
        py::dict d = adjuster_dict(fc);
        py::dict od;
        od["loss_function_type"] = opts.loss_function_type;
        od["loss_function_scale"] = opts.loss_function_scale;
        od["max_num_iterations"] = opts.max_num_iterations;
        od["max_linear_solver_iterations"] = opts.max_linear_solver_iterations;
        od["max_num_consecutive_invalid_steps"] = opts.max_num_consecutive_invalid_steps;
        od["function_tolerance"] = opts.function_tolerance;
        od["gradient_tolerance"] = opts.gradient_tolerance;
        od["parameter_tolerance"] = opts.parameter_tolerance;
        d["options"] = od;
        const py::dict out = solver(d);
        const auto cp = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(out["camera_params"]);
        const auto q = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(out["qvec"]);
        const auto t = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(out["tvec"]);
        const auto X = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(out["xyz"]);
        if (!cp || !q || !t || !X || static_cast<size_t>(cp.size()) != flat.camera_params.size() || static_cast<size_t>(q.size()) != flat.qvec.size() ||
            static_cast<size_t>(t.size()) != flat.tvec.size() || static_cast<size_t>(X.size()) != flat.xyz.size())
            throw py::value_error("BundleAdjuster.solve: the solver's result does not have the problem's shape");
        std::copy(cp.data(), cp.data() + cp.size(), flat.camera_params.begin());
        std::copy(q.data(), q.data() + q.size(), flat.qvec.begin());
        std::copy(t.data(), t.data() + t.size(), flat.tvec.begin());
        std::copy(X.data(), X.data() + X.size(), flat.xyz.begin());
        for (const char* k : {"num_variable_parameters", "initial_cost", "final_cost", "num_successful_steps", "num_unsuccessful_steps",
                              "num_pcg_iterations", "termination"})
            st[k] = out[k];
        st["device_ms"] = 0.0;
        st["kernel_ms"] = 0.0;
    } else {
        amc_ba_problem pb = flat.Problem();
        amc_ba_result res{};
        CallLibrary([&](amc_ctx* ctx) { return amc_bundle_adjust_masked(ctx, &pb, fc.point_const.data(), &opts, &res); }, "amc_bundle_adjust_masked");
        st["num_variable_parameters"] = res.num_variable_parameters;
        SolverStats(res, st);
    }
    WriteBackBundleAdjuster(fc, &model);
    update_from_model(r, model);
    st["host_ms"] = HostMs(t0, st["device_ms"].cast<double>());
    a.summary = st;
    SetLastStats(st);
    return true;
}

void BindBundle(py::module_& m) {
    py::enum_<LossFunctionType> PyLoss(m, "LossFunctionType");
    PyLoss.value("TRIVIAL", LossFunctionType::TRIVIAL).value("SOFT_L1", LossFunctionType::SOFT_L1).value("CAUCHY", LossFunctionType::CAUCHY);
    PyLoss.def(py::init([](const std::string& s) {
        if (s == "TRIVIAL") return LossFunctionType::TRIVIAL;
        if (s == "SOFT_L1") return LossFunctionType::SOFT_L1;
        if (s == "CAUCHY") return LossFunctionType::CAUCHY;
        throw py::value_error("Invalid string value " + s + " for enum LossFunctionType");
    }));
    py::implicitly_convertible<std::string, LossFunctionType>();
    py::class_<CeresSolverOptions> PyCeres(m, "CeresSolverOptions");
    PyCeres.def(py::init<>())
        .def_readwrite("function_tolerance", &CeresSolverOptions::function_tolerance)
        .def_readwrite("gradient_tolerance", &CeresSolverOptions::gradient_tolerance)
        .def_readwrite("parameter_tolerance", &CeresSolverOptions::parameter_tolerance)
        .def_readwrite("max_num_iterations", &CeresSolverOptions::max_num_iterations)
        .def_readwrite("max_linear_solver_iterations", &CeresSolverOptions::max_linear_solver_iterations)
        .def_readwrite("max_num_consecutive_invalid_steps", &CeresSolverOptions::max_num_consecutive_invalid_steps)
        .def_readwrite("max_consecutive_nonmonotonic_steps", &CeresSolverOptions::max_consecutive_nonmonotonic_steps,
                       "Accepted, no effect (DESIGN.md 15.9, B9).")
        .def_readwrite("minimizer_progress_to_stdout", &CeresSolverOptions::minimizer_progress_to_stdout, "Accepted, no effect.")
        .def_readwrite("num_threads", &CeresSolverOptions::num_threads, "Accepted, no effect: the solver runs on the GPU.");
    MakeDataclass(PyCeres, {"function_tolerance", "gradient_tolerance", "parameter_tolerance", "max_num_iterations",
                            "max_linear_solver_iterations", "max_num_consecutive_invalid_steps",
                            "max_consecutive_nonmonotonic_steps", "minimizer_progress_to_stdout", "num_threads"});
    py::class_<BundleAdjustmentOptions> PyBaOpts(m, "BundleAdjustmentOptions");
    PyBaOpts.def(py::init<>())
        .def_readwrite("loss_function_type", &BundleAdjustmentOptions::loss_function_type, "Loss function types: Trivial (non-robust) and Cauchy (robust) loss.")
        .def_readwrite("loss_function_scale", &BundleAdjustmentOptions::loss_function_scale, "Scaling factor determines residual at which robustification takes place.")
        .def_readwrite("refine_focal_length", &BundleAdjustmentOptions::refine_focal_length, "Whether to refine the focal length parameter group.")
        .def_readwrite("refine_principal_point", &BundleAdjustmentOptions::refine_principal_point, "Whether to refine the principal point parameter group.")
        .def_readwrite("refine_extra_params", &BundleAdjustmentOptions::refine_extra_params, "Whether to refine the extra parameter group.")
        .def_readwrite("refine_extrinsics", &BundleAdjustmentOptions::refine_extrinsics, "Whether to refine the extrinsic parameter group.")
        .def_readwrite("print_summary", &BundleAdjustmentOptions::print_summary, "Accepted, prints nothing.")
        .def_readwrite("min_num_residuals_for_multi_threading", &BundleAdjustmentOptions::min_num_residuals_for_multi_threading, "Accepted, no effect.")
        .def_readwrite("solver_options", &BundleAdjustmentOptions::solver_options, "Ceres-Solver options.");
    MakeDataclass(PyBaOpts, {"loss_function_type", "loss_function_scale", "refine_focal_length", "refine_principal_point",
                             "refine_extra_params", "refine_extrinsics", "print_summary",
                             "min_num_residuals_for_multi_threading", "solver_options"});
    m.def("_bundle_adjustment_problem", &flat_problem, "reconstruction"_a, "options"_a = BundleAdjustmentOptions(),
          "The flat problem bundle_adjustment solves (test hook).");
    m.def("bundle_adjustment", &bundle_adjustment, "reconstruction"_a, "options"_a = BundleAdjustmentOptions(),
          "Jointly refine every pose, point and camera of the reconstruction on the GPU, in place (DESIGN.md section 15).");

    py::class_<BundleAdjustmentConfig>(m, "BundleAdjustmentConfig")
        .def(py::init<>())
        .def("num_images", &BundleAdjustmentConfig::NumImages)
        .def("num_points", &BundleAdjustmentConfig::NumPoints)
        .def("num_constant_cam_intrinsics", &BundleAdjustmentConfig::NumConstantCamIntrinsics)
        .def("num_constant_cam_poses", &BundleAdjustmentConfig::NumConstantCamPoses)
        .def("num_constant_cam_positions", &BundleAdjustmentConfig::NumConstantCamPositions)
        .def("num_variable_points", &BundleAdjustmentConfig::NumVariablePoints)
        .def("num_constant_points", &BundleAdjustmentConfig::NumConstantPoints)
        .def("num_residuals", [](const BundleAdjustmentConfig& c, const PyReconstruction& r) { return c.NumResiduals(checked_model(r)); },
             "reconstruction"_a)
        .def("add_image", &BundleAdjustmentConfig::AddImage, "image_id"_a)
        .def("has_image", &BundleAdjustmentConfig::HasImage, "image_id"_a)
        .def("remove_image", &BundleAdjustmentConfig::RemoveImage, "image_id"_a)
        .def("set_constant_cam_intrinsics", &BundleAdjustmentConfig::SetConstantCamIntrinsics, "camera_id"_a)
        .def("set_variable_cam_intrinsics", &BundleAdjustmentConfig::SetVariableCamIntrinsics, "camera_id"_a)
        .def("is_constant_cam_intrinsics", &BundleAdjustmentConfig::IsConstantCamIntrinsics, "camera_id"_a)
        .def("set_constant_cam_pose", &BundleAdjustmentConfig::SetConstantCamPose, "image_id"_a)
        .def("set_variable_cam_pose", &BundleAdjustmentConfig::SetVariableCamPose, "image_id"_a)
        .def("has_constant_cam_pose", &BundleAdjustmentConfig::HasConstantCamPose, "image_id"_a)
        .def("set_constant_cam_positions", &BundleAdjustmentConfig::SetConstantCamPositions, "image_id"_a, "idxs"_a)
        .def("remove_constant_cam_positions", &BundleAdjustmentConfig::RemoveConstantCamPositions, "image_id"_a)
        .def("has_constant_cam_positions", &BundleAdjustmentConfig::HasConstantCamPositions, "image_id"_a)
        .def("constant_cam_positions", [](const BundleAdjustmentConfig& c, uint32_t image_id) { return c.ConstantCamPositions(image_id); }, "image_id"_a)
        .def("add_variable_point", &BundleAdjustmentConfig::AddVariablePoint, "point3D_id"_a)
        .def("add_constant_point", &BundleAdjustmentConfig::AddConstantPoint, "point3D_id"_a)
        .def("has_point", &BundleAdjustmentConfig::HasPoint, "point3D_id"_a)
        .def("has_variable_point", &BundleAdjustmentConfig::HasVariablePoint, "point3D_id"_a)
        .def("has_constant_point", &BundleAdjustmentConfig::HasConstantPoint, "point3D_id"_a)
        .def("remove_variable_point", &BundleAdjustmentConfig::RemoveVariablePoint, "point3D_id"_a)
        .def("remove_constant_point", &BundleAdjustmentConfig::RemoveConstantPoint, "point3D_id"_a)
        .def_property_readonly("image_ids", [](const BundleAdjustmentConfig& c) { return c.Images(); })
        .def_property_readonly("variable_point3D_ids", [](const BundleAdjustmentConfig& c) { return c.VariablePoints(); })
        .def_property_readonly("constant_point3D_ids", [](const BundleAdjustmentConfig& c) { return c.ConstantPoints(); })
        .def("__copy__", [](const BundleAdjustmentConfig& c) { return BundleAdjustmentConfig(c); })
        .def("__deepcopy__", [](const BundleAdjustmentConfig& c, const py::dict&) { return BundleAdjustmentConfig(c); })
        .def(py::pickle(
            [](const BundleAdjustmentConfig& c) {
                return py::make_tuple(c.Images(), c.ConstantIntrinsics(), c.ConstantCamPoses(), c.AllConstantCamPositions(), c.VariablePoints(),
                                      c.ConstantPoints());
            },
            [](const py::tuple& t) {
                if (t.size() != 6) throw py::value_error("BundleAdjustmentConfig: invalid pickled state");
                BundleAdjustmentConfig c;
                for (uint32_t id : t[0].cast<std::set<uint32_t>>()) c.AddImage(id);
                for (uint32_t id : t[1].cast<std::set<uint32_t>>()) c.SetConstantCamIntrinsics(id);
                for (uint32_t id : t[2].cast<std::set<uint32_t>>()) c.SetConstantCamPose(id);
                for (const auto& kv : t[3].cast<std::map<uint32_t, std::vector<int>>>()) c.SetConstantCamPositions(kv.first, kv.second);
                for (uint64_t id : t[4].cast<std::set<uint64_t>>()) c.AddVariablePoint(id);
                for (uint64_t id : t[5].cast<std::set<uint64_t>>()) c.AddConstantPoint(id);
                return c;
            }))
        .def("__repr__", [](const BundleAdjustmentConfig& c) {
            return "BundleAdjustmentConfig(num_images=" + std::to_string(c.NumImages()) + ", num_constant_cam_intrinsics=" +
                   std::to_string(c.NumConstantCamIntrinsics()) + ", num_constant_cam_poses=" + std::to_string(c.NumConstantCamPoses()) +
                   ", num_constant_cam_positions=" + std::to_string(c.NumConstantCamPositions()) + ", num_variable_points=" +
                   std::to_string(c.NumVariablePoints()) + ", num_constant_points=" + std::to_string(c.NumConstantPoints()) + ")";
        });
    py::class_<PyBundleAdjuster>(m, "BundleAdjuster")
        .def(py::init([](const BundleAdjustmentOptions& options, const BundleAdjustmentConfig& config) {
                 return PyBundleAdjuster{options, config, py::dict()};
             }), "options"_a, "config"_a)
        .def("solve", [](PyBundleAdjuster& a, PyReconstruction& r) { return adjuster_solve(a, r, py::none()); }, "reconstruction"_a,
             "Refine the config's part of the reconstruction on the GPU, in place (DESIGN.md 15.12).  False when the\n"
             "config gives no residual.")
        .def("_solve_with", &adjuster_solve, "reconstruction"_a, "solver"_a, "solve with a callable in the library's place (test hook).")
        .def("_problem", [](const PyBundleAdjuster& a, const PyReconstruction& r) {
                 SparseModel model;
                 return adjuster_dict(adjuster_flat(a, r, &model));
             }, "reconstruction"_a, "The flat problem solve hands to amc_bundle_adjust_masked (test hook).")
        .def_property_readonly("options", [](const PyBundleAdjuster& a) { return a.options; })
        .def_property_readonly("config", [](const PyBundleAdjuster& a) { return a.config; })
        .def_property_readonly("summary", [](const PyBundleAdjuster& a) { return a.summary; });
}

}  // namespace amchost
