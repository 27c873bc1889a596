// py_scene.h — the Python-facing scene types the binding files share, and the bridge between a Reconstruction's dicts
// and model_io's SparseModel.  The bridge functions are defined once, in bind_reconstruction.cc (the model) and
// bind_bundle.cc (the adjuster); the types and the row converters are inline.
#pragma once
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <array>
#include <cmath>
#include <cstdint>
#include <set>
#include <string>
#include <vector>

#include "ba_config_host.h"
#include "binding_support.h"
#include "database.h"
#include "estimators.h"
#include "model_io.h"
#include "py_types.h"
#include "retriangulate_host.h"

namespace amchost {

// Image: the database-facing part of /root/reference/pycolmap/scene/image.h:74-130 (identifiers, name, pose and pose
// prior, the keypoints it was constructed with); the reconstruction bookkeeping (points3D, observations) belongs
// to COLMAP's mapper and is not part of this library
struct PyPoint2D {
    std::array<double, 2> xy{{0.0, 0.0}};
    uint64_t point3D_id = kInvalidPoint3DId;
};
struct PyImage {
    uint32_t image_id = 0xFFFFFFFFu, camera_id = 0xFFFFFFFFu;  // kInvalidImageId / kInvalidCameraId
    std::string name;
    PyRigid3d cam_from_world, cam_from_world_prior;
    std::vector<std::array<double, 2>> keypoints;
    std::vector<PyPoint2D> points2D;  // the reconstruction's view of the image (Reconstruction, bundle_adjustment)
    PyImage() {
        const double nan = std::nan("");  // Image(): the prior is "unknown"
        cam_from_world_prior.rotation.xyzw = {{nan, nan, nan, nan}};
        cam_from_world_prior.translation = {{nan, nan, nan}};
    }
};
inline PyImage image_from_row(const ImageRow& r) {
    PyImage im;
    im.image_id = r.image_id;
    im.camera_id = r.camera_id;
    im.name = r.name;
    im.cam_from_world_prior.rotation.xyzw = {{r.prior_q[1], r.prior_q[2], r.prior_q[3], r.prior_q[0]}};
    im.cam_from_world_prior.translation = r.prior_t;
    return im;
}
inline ImageRow row_from_image(const PyImage& im) {
    ImageRow r;
    r.image_id = im.image_id;
    r.camera_id = im.camera_id;
    r.name = im.name;
    const auto& q = im.cam_from_world_prior.rotation.xyzw;
    r.prior_q = {{q[3], q[0], q[1], q[2]}};
    r.prior_t = im.cam_from_world_prior.translation;
    return r;
}
inline PyCamera camera_from_row(const CameraRow& r) {
    PyCamera c;
    c.camera_id = r.camera_id;
    c.model = r.model_id;
    c.width = r.width;
    c.height = r.height;
    c.params = r.params;
    c.has_prior_focal_length = r.has_prior_focal_length;
    return c;
}
inline CameraRow row_from_camera(const PyCamera& c) {
    c.CheckParams();
    CameraRow r;
    r.camera_id = c.camera_id;
    r.model_id = c.model;
    r.width = c.width;
    r.height = c.height;
    r.params = c.params;
    r.has_prior_focal_length = c.has_prior_focal_length;
    return r;
}

// ---- Reconstruction (/root/reference/pycolmap/scene/reconstruction.h): the minimal subset.  The three
// maps are Python dicts of Camera / Image / Point3D objects in file order, so they have reference semantics; every
// operation converts them to model_io's structs and writes the outcome back into the same objects. ----
struct PyTrackElement {
    uint32_t image_id = 0xFFFFFFFFu, point2D_idx = 0xFFFFFFFFu;
};
struct PyTrack {
    std::vector<PyTrackElement> elements;
};
struct PyPoint3D {
    std::array<double, 3> xyz{{0.0, 0.0, 0.0}};
    std::array<uint8_t, 3> color{{0, 0, 0}};
    double error = -1.0;
    PyTrack track;
};
struct PyReconstruction {
    py::dict cameras, images, points3D;
};
// keeps the caller's graph and reconstruction alive and works on that reconstruction in place
struct PyTriangulator {
    py::object graph, reconstruction;
    std::set<uint64_t> modified;
    RetriTrials re_trials;  // retriangulate's per-pair trial counters
};

enum class LossFunctionType { TRIVIAL = 0, SOFT_L1 = 1, CAUCHY = 2 };
struct CeresSolverOptions {
    double function_tolerance = 0.0, gradient_tolerance = 0.0, parameter_tolerance = 0.0;  // COLMAP's BundleAdjustmentOptions
    int max_num_iterations = 100, max_linear_solver_iterations = 200, max_num_consecutive_invalid_steps = 10,
        max_consecutive_nonmonotonic_steps = 10;
    bool minimizer_progress_to_stdout = false;
    int num_threads = -1;
};
struct BundleAdjustmentOptions {
    LossFunctionType loss_function_type = LossFunctionType::TRIVIAL;
    double loss_function_scale = 1.0;
    bool refine_focal_length = true, refine_principal_point = false, refine_extra_params = true, refine_extrinsics = true,
         print_summary = true;
    int min_num_residuals_for_multi_threading = 50000;
    CeresSolverOptions solver_options;
};
struct PyBundleAdjuster {
    BundleAdjustmentOptions options;
    BundleAdjustmentConfig config;
    py::dict summary;
};

// ---- the model bridge (bind_reconstruction.cc) ----
// the dicts as a plain model; a key that is not its object's id is a ValueError
SparseModel to_model(const PyReconstruction& r);
// a model read from files as fresh objects
void from_model(PyReconstruction& r, const SparseModel& m);
// the outcome of an operation on to_model(r) back into r's own objects: camera parameters, poses, the points2D's
// point ids, the points' positions and tracks; points the operation deleted leave the dict
void update_from_model(PyReconstruction& r, const SparseModel& m);
// to_model, refused with a ValueError when CheckModel finds the model inconsistent
SparseModel checked_model(const PyReconstruction& r);
// update_from_model plus the points' errors (the point filter and update_point3D_errors write them; bundle_adjustment
// does not)
void update_with_errors(PyReconstruction& r, const SparseModel& m);
// the outcome of triangulate_image back into r: the created points as new objects first, then update_with_errors
void update_with_new_points(PyReconstruction& r, const SparseModel& m);

// ---- the adjuster (bind_bundle.cc) ----
amc_ba_opts ToAmcBaOpts(const BundleAdjustmentOptions& o);
// BundleAdjuster.solve; solver: None, or a callable that stands in for the library
bool adjuster_solve(PyBundleAdjuster& a, PyReconstruction& r, const py::object& solver);

void BindReconstruction(py::module_& m);
void BindBundle(py::module_& m);
void BindTriangulator(py::module_& m);
void BindMapper(py::module_& m);
void BindDatabase(py::module_& m);

}  // namespace amchost
