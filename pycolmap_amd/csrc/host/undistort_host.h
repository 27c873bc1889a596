// undistort_host.h — the host side of undistort_images (/root/reference/pycolmap/pipeline/images.h:96-148, 203-261)
// over the C ABI of include/amc_undistort.h: UndistortCameraOptions and CopyType, undistort_camera / undistort_image
// (the names later pycolmap releases use), the per-image plan of a workspace and the undistorted sparse model.  The
// pipeline itself (decode, batches, encode, the workspace's files) is pycolmap_amd/_undistortion.py.
#pragma once

#include <functional>
#include <string>
#include <vector>

#include "../../../include/amc_undistort.h"
#include "estimators.h"
#include "model_io.h"
#include "py_types.h"

namespace amchost {

// UndistortCameraOptions (images.h:203-240)
struct UndistortCameraOptions {
    double blank_pixels = 0.0;
    double min_scale = 0.2;
    double max_scale = 2.0;
    int max_image_size = -1;
    double roi_min_x = 0.0;
    double roi_min_y = 0.0;
    double roi_max_x = 1.0;
    double roi_max_y = 1.0;
};
// CopyType (images.h:248-254)
enum class CopyType { COPY = 0, HARD_LINK = 1, SOFT_LINK = 2 };

// UndistortCameraOptions::Check as THROW_CHECK errors
#define AMC_UNDISTORT_CHECK(cond)                                                       \
    do {                                                                                \
        if (!(cond)) throw py::value_error(CheckMessage(__FILE__, __LINE__, #cond));   \
    } while (0)
inline amc_undistort_opts CheckedUndistortOpts(const UndistortCameraOptions& options) {
    const double blank_pixels = options.blank_pixels, min_scale = options.min_scale, max_scale = options.max_scale;
    const int max_image_size = options.max_image_size;
    const double roi_min_x = options.roi_min_x, roi_min_y = options.roi_min_y, roi_max_x = options.roi_max_x,
                 roi_max_y = options.roi_max_y;
    AMC_UNDISTORT_CHECK(blank_pixels >= 0);
    AMC_UNDISTORT_CHECK(blank_pixels <= 1);
    AMC_UNDISTORT_CHECK(min_scale > 0);
    AMC_UNDISTORT_CHECK(min_scale <= max_scale);
    AMC_UNDISTORT_CHECK(max_image_size != 0);
    AMC_UNDISTORT_CHECK(roi_min_x >= 0);
    AMC_UNDISTORT_CHECK(roi_min_y >= 0);
    AMC_UNDISTORT_CHECK(roi_max_x <= 1);
    AMC_UNDISTORT_CHECK(roi_max_y <= 1);
    AMC_UNDISTORT_CHECK(roi_min_x < roi_max_x);
    AMC_UNDISTORT_CHECK(roi_min_y < roi_max_y);
    amc_undistort_opts o;
    amc_undistort_opts_default(&o);
    o.blank_pixels = blank_pixels;
    o.min_scale = min_scale;
    o.max_scale = max_scale;
    o.max_image_size = max_image_size;
    o.roi_min_x = roi_min_x;
    o.roi_min_y = roi_min_y;
    o.roi_max_x = roi_max_x;
    o.roi_max_y = roi_max_y;
    return o;
}

inline amc_undistort_cam ToAmcCam(int model, uint64_t width, uint64_t height, const std::vector<double>& params) {
    amc_undistort_cam c{};
    c.model = model;
    c.width = width;
    c.height = height;
    for (size_t i = 0; i < params.size() && i < 12; ++i) c.params[i] = params[i];
    return c;
}
inline amc_undistort_cam ToAmcCam(const PyCamera& c) {
    c.CheckParams();
    return ToAmcCam(c.model, c.width, c.height, c.params);
}
inline PyCamera FromAmcCam(const amc_undistort_cam& c, uint32_t camera_id, bool has_prior) {
    PyCamera out;
    out.camera_id = camera_id;
    out.model = c.model;
    out.width = c.width;
    out.height = c.height;
    out.params.assign(c.params, c.params + ModelNumParams(c.model));
    out.has_prior_focal_length = has_prior;
    return out;
}

// UndistortCamera
inline PyCamera UndistortCameraPy(const UndistortCameraOptions& options, const PyCamera& camera) {
    const amc_undistort_opts o = CheckedUndistortOpts(options);
    const amc_undistort_cam in = ToAmcCam(camera);
    amc_undistort_cam out;
    EstCheck(amc_undistort_camera(&o, &in, &out), "amc_undistort_camera");
    return FromAmcCam(out, camera.camera_id, camera.has_prior_focal_length);
}

// UndistortImage on an H x W or H x W x 3 uint8 array: (undistorted array, undistorted camera)
inline py::tuple UndistortImagePy(const UndistortCameraOptions& options, const py::array& image, const PyCamera& camera) {
    if (!py::isinstance<py::array_t<uint8_t>>(image) || (image.ndim() != 2 && image.ndim() != 3) ||
        (image.ndim() == 3 && image.shape(2) != 3 && image.shape(2) != 1) || image.size() == 0)
        throw py::value_error("undistort_image: image must be a non-empty H x W or H x W x 3 uint8 array");
    const auto img = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>::ensure(image);
    const uint64_t h = static_cast<uint64_t>(img.shape(0)), w = static_cast<uint64_t>(img.shape(1));
    if (w != camera.width || h != camera.height)
        throw py::value_error("undistort_image: the image is " + std::to_string(w) + " x " + std::to_string(h) +
                              ", the camera " + std::to_string(camera.width) + " x " + std::to_string(camera.height));
    const int ch = img.ndim() == 3 ? static_cast<int>(img.shape(2)) : 1;
    const PyCamera undistorted = UndistortCameraPy(options, camera);
    std::vector<py::ssize_t> shape = {static_cast<py::ssize_t>(undistorted.height), static_cast<py::ssize_t>(undistorted.width)};
    if (img.ndim() == 3) shape.push_back(ch);
    py::array_t<uint8_t> out(shape);
    amc_undistort_image job{};
    job.src = img.data();
    job.src_stride = w * static_cast<uint64_t>(ch);
    job.channels = ch;
    job.src_camera = ToAmcCam(camera);
    job.dst_camera = ToAmcCam(undistorted);
    job.dst = out.mutable_data();
    amc_undistort_result res;
    {
        py::gil_scoped_release release;
        EstimatorCtx& E = TheEstimatorCtx();
        std::lock_guard<std::mutex> lock(E.mu);
        EstCheck(amc_undistort_images(E.Get(), 1, &job, &res), "amc_undistort_images");
    }
    return py::make_tuple(out, undistorted);
}

// Camera::IsUndistorted: a (SIMPLE_)PINHOLE model, or every extra parameter zero
inline bool IsUndistorted(const ModelCamera& c) {
    if (c.model == 0 || c.model == 1) return true;
    const int first = (c.model == 2 || c.model == 3 || c.model == 8 || c.model == 9) ? 3 : 4;
    for (size_t i = first; i < c.params.size(); ++i)
        if (c.params[i] != 0.0) return false;
    return true;
}

struct UndistortPlanItem {
    uint32_t image_id = 0;
    std::string name;
    ModelCamera camera;
    amc_undistort_cam undistorted{};
    bool copy = false;  // the image is copied or linked, not warped
};

inline amc_undistort_cam UndistortModelCamera(const amc_undistort_opts& o, const ModelCamera& c) {
    const amc_undistort_cam in = ToAmcCam(c.model, c.width, c.height, c.params);
    amc_undistort_cam out;
    EstCheck(amc_undistort_camera(&o, &in, &out), "amc_undistort_camera");
    return out;
}

// the images a workspace holds, in the list's order (an empty list: every image, in the model's order); a listed
// name the model does not hold is reported through `warn` and skipped
inline std::vector<UndistortPlanItem> UndistortPlan(const SparseModel& model, const std::vector<std::string>& image_list,
                                                    const UndistortCameraOptions& options,
                                                    const std::function<void(const std::string&)>& warn) {
    const amc_undistort_opts o = CheckedUndistortOpts(options);
    std::vector<const ModelImage*> chosen;
    if (image_list.empty()) {
        for (const ModelImage& im : model.images) chosen.push_back(&im);
    } else {
        for (const std::string& name : image_list) {
            const ModelImage* found = nullptr;
            for (const ModelImage& im : model.images)
                if (im.name == name) found = &im;
            if (!found) {
                warn("Cannot find image " + name);
                continue;
            }
            chosen.push_back(found);
        }
    }
    std::vector<UndistortPlanItem> plan;
    for (const ModelImage* im : chosen) {
        UndistortPlanItem it;
        it.image_id = im->image_id;
        it.name = im->name;
        it.camera = *model.FindCamera(im->camera_id);
        it.undistorted = UndistortModelCamera(o, it.camera);
        it.copy = IsUndistorted(it.camera) && it.undistorted.width == it.camera.width && it.undistorted.height == it.camera.height;
        plan.push_back(std::move(it));
    }
    return plan;
}

// UndistortReconstruction: every camera becomes its undistort_camera, every point2D moves with it; poses, ids, tracks
// and points3D stay.  A (SIMPLE_)PINHOLE camera that keeps its focal lengths and principal point keeps its points2D
// as they are (the map is the identity there).
inline SparseModel UndistortModel(const SparseModel& model, const UndistortCameraOptions& options) {
    const amc_undistort_opts o = CheckedUndistortOpts(options);
    SparseModel out = model;
    std::vector<amc_undistort_cam> und(model.cameras.size());
    for (size_t i = 0; i < model.cameras.size(); ++i) {
        und[i] = UndistortModelCamera(o, model.cameras[i]);
        ModelCamera& c = out.cameras[i];
        c.model = und[i].model;
        c.width = und[i].width;
        c.height = und[i].height;
        c.params.assign(und[i].params, und[i].params + 4);
    }
    for (ModelImage& im : out.images) {
        size_t ci = 0;
        while (model.cameras[ci].camera_id != im.camera_id) ++ci;
        const ModelCamera& src = model.cameras[ci];
        const amc_undistort_cam& u = und[ci];
        const int nf = (src.model == 0 || src.model == 2 || src.model == 3 || src.model == 8 || src.model == 9) ? 1 : 2;
        if ((src.model == 0 || src.model == 1) && u.params[0] == src.params[0] && u.params[1] == src.params[nf - 1] &&
            u.params[2] == src.params[nf] && u.params[3] == src.params[nf + 1])
            continue;
        if (im.points2D.empty()) continue;
        std::vector<double> xy(2 * im.points2D.size());
        for (size_t k = 0; k < im.points2D.size(); ++k) {
            xy[2 * k] = im.points2D[k].x;
            xy[2 * k + 1] = im.points2D[k].y;
        }
        const amc_undistort_cam in = ToAmcCam(src.model, src.width, src.height, src.params);
        EstCheck(amc_undistort_points(&in, &u, im.points2D.size(), xy.data(), xy.data()), "amc_undistort_points");
        for (size_t k = 0; k < im.points2D.size(); ++k) {
            im.points2D[k].x = xy[2 * k];
            im.points2D[k].y = xy[2 * k + 1];
        }
    }
    return out;
}

}  // namespace amchost
