// bind_reconstruction.cc — Point2D, Image, TrackElement, Track, Point3D and Reconstruction with its point filter, and the
// bridge between a Reconstruction's dicts and model_io's SparseModel that the other binding files use (py_scene.h).
#include <sstream>
#include <unordered_set>

#include "py_scene.h"
#include "reconstruction.h"

namespace amchost {

SparseModel to_model(const PyReconstruction& r) {
    SparseModel m;
    for (auto item : r.cameras) {
        const PyCamera& c = item.second.cast<const PyCamera&>();
        if (item.first.cast<uint32_t>() != c.camera_id) throw py::value_error("Reconstruction.cameras: a key differs from its camera's camera_id");
        ModelCamera mc;
        mc.camera_id = c.camera_id;
        mc.model = c.model;
        mc.width = c.width;
        mc.height = c.height;
        mc.params = c.params;
        m.cameras.push_back(std::move(mc));
    }
    for (auto item : r.images) {
        const PyImage& im = item.second.cast<const PyImage&>();
        if (item.first.cast<uint32_t>() != im.image_id) throw py::value_error("Reconstruction.images: a key differs from its image's image_id");
        ModelImage mi;
        mi.image_id = im.image_id;
        mi.camera_id = im.camera_id;
        mi.name = im.name;
        const auto& q = im.cam_from_world.rotation.xyzw;
        mi.qvec[0] = q[3];
        for (int k = 0; k < 3; ++k) mi.qvec[1 + k] = q[k];
        for (int k = 0; k < 3; ++k) mi.tvec[k] = im.cam_from_world.translation[k];
        for (const PyPoint2D& p : im.points2D) {
            ModelPoint2D mp;
            mp.x = p.xy[0];
            mp.y = p.xy[1];
            mp.point3D_id = p.point3D_id;
            mi.points2D.push_back(mp);
        }
        m.images.push_back(std::move(mi));
    }
    for (auto item : r.points3D) {
        const PyPoint3D& p = item.second.cast<const PyPoint3D&>();
        ModelPoint3D mp;
        mp.point3D_id = item.first.cast<uint64_t>();
        for (int k = 0; k < 3; ++k) mp.xyz[k] = p.xyz[k];
        for (int k = 0; k < 3; ++k) mp.rgb[k] = p.color[k];
        mp.error = p.error;
        for (const PyTrackElement& e : p.track.elements) mp.track.emplace_back(e.image_id, e.point2D_idx);
        m.points3D.push_back(std::move(mp));
    }
    return m;
}

void from_model(PyReconstruction& r, const SparseModel& m) {
    r.cameras = py::dict();
    r.images = py::dict();
    r.points3D = py::dict();
    for (const ModelCamera& mc : m.cameras) {
        PyCamera c;
        c.camera_id = mc.camera_id;
        c.model = mc.model;
        c.width = mc.width;
        c.height = mc.height;
        c.params = mc.params;
        r.cameras[py::int_(mc.camera_id)] = py::cast(c);
    }
    for (const ModelImage& mi : m.images) {
        PyImage im;
        im.image_id = mi.image_id;
        im.camera_id = mi.camera_id;
        im.name = mi.name;
        im.cam_from_world.rotation.xyzw = {{mi.qvec[1], mi.qvec[2], mi.qvec[3], mi.qvec[0]}};
        im.cam_from_world.translation = {{mi.tvec[0], mi.tvec[1], mi.tvec[2]}};
        for (const ModelPoint2D& mp : mi.points2D) {
            PyPoint2D p;
            p.xy = {{mp.x, mp.y}};
            p.point3D_id = mp.point3D_id;
            im.points2D.push_back(p);
        }
        r.images[py::int_(mi.image_id)] = py::cast(im);
    }
    for (const ModelPoint3D& mp : m.points3D) {
        PyPoint3D p;
        p.xyz = {{mp.xyz[0], mp.xyz[1], mp.xyz[2]}};
        p.color = {{mp.rgb[0], mp.rgb[1], mp.rgb[2]}};
        p.error = mp.error;
        for (const auto& e : mp.track) p.track.elements.push_back({e.first, e.second});
        r.points3D[py::int_(mp.point3D_id)] = py::cast(p);
    }
}

void update_from_model(PyReconstruction& r, const SparseModel& m) {
    for (const ModelCamera& mc : m.cameras) r.cameras[py::int_(mc.camera_id)].cast<PyCamera&>().params = mc.params;
    for (const ModelImage& mi : m.images) {
        PyImage& im = r.images[py::int_(mi.image_id)].cast<PyImage&>();
        im.cam_from_world.rotation.xyzw = {{mi.qvec[1], mi.qvec[2], mi.qvec[3], mi.qvec[0]}};
        im.cam_from_world.translation = {{mi.tvec[0], mi.tvec[1], mi.tvec[2]}};
        for (size_t k = 0; k < mi.points2D.size() && k < im.points2D.size(); ++k) im.points2D[k].point3D_id = mi.points2D[k].point3D_id;
    }
    py::dict kept;
    for (const ModelPoint3D& mp : m.points3D) {
        py::object obj = r.points3D[py::int_(mp.point3D_id)];
        PyPoint3D& p = obj.cast<PyPoint3D&>();
        p.xyz = {{mp.xyz[0], mp.xyz[1], mp.xyz[2]}};
        p.track.elements.clear();
        for (const auto& e : mp.track) p.track.elements.push_back({e.first, e.second});
        kept[py::int_(mp.point3D_id)] = obj;
    }
    r.points3D.attr("clear")();
    r.points3D.attr("update")(kept);  // the same dict object: references to rec.points3D stay valid
}

SparseModel checked_model(const PyReconstruction& r) {
    SparseModel m = to_model(r);
    const std::string bad = CheckModel(m);
    if (!bad.empty()) throw py::value_error("Reconstruction: " + bad);
    return m;
}

void update_with_errors(PyReconstruction& r, const SparseModel& m) {
    update_from_model(r, m);
    for (const ModelPoint3D& mp : m.points3D) r.points3D[py::int_(mp.point3D_id)].cast<PyPoint3D&>().error = mp.error;
}

void update_with_new_points(PyReconstruction& r, const SparseModel& m) {
    for (const ModelPoint3D& mp : m.points3D) {
        if (r.points3D.contains(py::int_(mp.point3D_id))) continue;
        PyPoint3D p;
        p.color = {{mp.rgb[0], mp.rgb[1], mp.rgb[2]}};
        r.points3D[py::int_(mp.point3D_id)] = py::cast(p);
    }
    update_with_errors(r, m);
}

namespace {

// One amc_filter_points3d call on the checked model: ids == nullptr filters every point.  Nothing
// of r changes unless the call succeeds.  Without a device the call raises pycolmap_amd._capi.AmcError.
size_t filter_model(PyReconstruction& r, const std::vector<uint64_t>* ids, const std::vector<uint32_t>* image_ids, double max_reproj_error,
                    double min_tri_angle, bool errors_only) {
    const auto t0 = std::chrono::steady_clock::now();
    SparseModel model = checked_model(r);
    std::vector<uint64_t> in_images;
    if (image_ids) {
        in_images = Point3DIdsInImages(model, *image_ids);
        ids = &in_images;
    }
    const FlatFilter flat = FlattenForFilter(model, ids);
    amc_filter_opts opts;
    amc_filter_opts_default(&opts);
    opts.max_reproj_error = max_reproj_error;
    opts.min_tri_angle = min_tri_angle;
    opts.errors_only = errors_only ? 1 : 0;
    const amc_filter_problem pb = flat.Problem();
    ResultGuard<amc_filter_result, amc_filter_result_free> res;
    CallLibrary([&](amc_ctx* ctx) { return amc_filter_points3d(ctx, &pb, &opts, res.get()); }, "amc_filter_points3d");
    size_t count = 0;
    if (errors_only)
        ApplyPointErrors(flat, res->point_error, &model);
    else
        count = ApplyFilterResult(flat, res->point_verdict, res->obs_deleted, res->point_error, &model);
    py::dict st;
    st["call"] = errors_only ? "update_point3D_errors" : "filter_points3D";
    st["num_points"] = res->num_points;
    st["num_observations"] = res->num_observations;
    st["num_filtered"] = res->num_filtered;
    st["num_batches"] = res->num_batches;
    if (!errors_only && res->num_filtered != count)
        throw std::runtime_error("filter_points3D: the library counted " + std::to_string(res->num_filtered) + ", the write-back " + std::to_string(count));
    update_with_errors(r, model);
    FinishStats(st, t0, res->device_ms, res->kernel_ms, res->copy_ms);
    return count;
}

std::string summary(const PyReconstruction& r) {
    const SparseModel m = checked_model(r);
    const size_t nobs = ComputeNumObservations(m);
    std::ostringstream ss;
    ss << "Reconstruction:\n\tnum_reg_images = " << m.images.size() << "\n\tnum_cameras = " << m.cameras.size()
       << "\n\tnum_points3D = " << m.points3D.size() << "\n\tnum_observations = " << nobs
       << "\n\tmean_track_length = " << ComputeMeanTrackLength(m) << "\n\tmean_observations_per_image = "
       << (m.images.empty() ? 0.0 : static_cast<double>(nobs) / static_cast<double>(m.images.size()));
    return ss.str();
}

void read_into(PyReconstruction& r, const std::string& path, int how) {
    const SparseModel m = how == 0 ? ReadSparseModel(path) : how == 1 ? ReadSparseModelBin(path) : ReadSparseModelTxt(path);
    const std::string bad = CheckModel(m);
    if (!bad.empty()) throw py::value_error(path + ": " + bad);
    from_model(r, m);
}

PyReconstruction deep_copy(const PyReconstruction& r) {
    const py::object deepcopy = py::module_::import("copy").attr("deepcopy");
    PyReconstruction c;
    c.cameras = deepcopy(r.cameras);
    c.images = deepcopy(r.images);
    c.points3D = deepcopy(r.points3D);
    return c;
}

}  // namespace

void BindReconstruction(py::module_& m) {
    py::class_<PyPoint2D>(m, "Point2D")
        .def(py::init<>())
        .def(py::init([](const std::array<double, 2>& xy, uint64_t point3D_id) {
                 PyPoint2D p;
                 p.xy = xy;
                 p.point3D_id = point3D_id;
                 return p;
             }),
             "xy"_a, "point3D_id"_a = kInvalidPoint3DId)
        .def_readwrite("xy", &PyPoint2D::xy)
        .def_readwrite("point3D_id", &PyPoint2D::point3D_id)
        .def("has_point3D", [](const PyPoint2D& p) { return p.point3D_id != kInvalidPoint3DId; })
        .def("__copy__", [](const PyPoint2D& p) { return PyPoint2D(p); })
        .def("__deepcopy__", [](const PyPoint2D& p, const py::dict&) { return PyPoint2D(p); })
        .def("__repr__", [](const PyPoint2D& p) {
            std::ostringstream ss;
            ss << "Point2D(xy=[" << p.xy[0] << ", " << p.xy[1] << "], point3D_id="
               << (p.point3D_id != kInvalidPoint3DId ? std::to_string(p.point3D_id) : "Invalid") << ")";
            return ss.str();
        });
    py::class_<PyImage>(m, "Image")
        .def(py::init<>())
        .def(py::init([](const std::string& name, const std::vector<std::array<double, 2>>& keypoints,
                         const PyRigid3d& cam_from_world, uint32_t camera_id, uint32_t id) {
                 PyImage im;
                 im.name = name;
                 im.keypoints = keypoints;
                 im.cam_from_world = cam_from_world;
                 im.camera_id = camera_id;
                 im.image_id = id;
                 return im;
             }),
             "name"_a = "", "keypoints"_a = std::vector<std::array<double, 2>>(), "cam_from_world"_a = PyRigid3d(),
             "camera_id"_a = 0xFFFFFFFFu, "id"_a = 0xFFFFFFFFu)
        .def_readwrite("image_id", &PyImage::image_id, "Unique identifier of image.")
        .def_property(
            "camera_id", [](const PyImage& im) { return im.camera_id; },
            [](PyImage& im, uint32_t id) {
                if (id == 0xFFFFFFFFu) throw py::value_error(CheckMessage(__FILE__, __LINE__, "camera_id != kInvalidCameraId"));
                im.camera_id = id;
            },
            "Unique identifier of the camera.")
        .def_readwrite("name", &PyImage::name, "Name of the image.")
        .def_readwrite("cam_from_world", &PyImage::cam_from_world,
                       "The pose of the image, defined as the transformation from world to camera space.")
        .def_readwrite("cam_from_world_prior", &PyImage::cam_from_world_prior,
                       "The pose prior of the image, e.g. extracted from EXIF tags.")
        .def("has_camera", [](const PyImage& im) { return im.camera_id != 0xFFFFFFFFu; },
             "Check whether identifier of camera has been set.")
        .def("num_points2D", [](const PyImage& im) { return im.keypoints.size(); },
             "Get the number of image points (keypoints).")
        .def_readwrite("points2D", &PyImage::points2D,
                       "The image's points with their 3D point ids (a copy of the list; assign to change it).")
        .def("num_points3D", [](const PyImage& im) {
            size_t n = 0;
            for (const PyPoint2D& p : im.points2D) n += p.point3D_id != kInvalidPoint3DId;
            return n;
        }, "Get the number of triangulated points2D.")
        .def("__copy__", [](const PyImage& im) { return PyImage(im); })
        .def("__deepcopy__", [](const PyImage& im, const py::dict&) { return PyImage(im); })
        .def("__repr__", [](const PyImage& im) {
            std::ostringstream ss;
            ss << "Image(image_id=" << (im.image_id != 0xFFFFFFFFu ? std::to_string(im.image_id) : "Invalid")
               << ", camera_id=" << (im.camera_id != 0xFFFFFFFFu ? std::to_string(im.camera_id) : "Invalid") << ", name=\""
               << im.name << "\", triangulated=";
            size_t tri = 0;
            for (const PyPoint2D& p : im.points2D) tri += p.point3D_id != kInvalidPoint3DId;
            ss << tri << "/" << (tri ? im.points2D.size() : im.keypoints.size()) << ")";
            return ss.str();
        });

    py::class_<PyTrackElement>(m, "TrackElement")
        .def(py::init<>())
        .def(py::init([](uint32_t image_id, uint32_t point2D_idx) { return PyTrackElement{image_id, point2D_idx}; }),
             "image_id"_a, "point2D_idx"_a)
        .def_readwrite("image_id", &PyTrackElement::image_id)
        .def_readwrite("point2D_idx", &PyTrackElement::point2D_idx)
        .def("__copy__", [](const PyTrackElement& e) { return PyTrackElement(e); })
        .def("__deepcopy__", [](const PyTrackElement& e, const py::dict&) { return PyTrackElement(e); })
        .def("__repr__", [](const PyTrackElement& e) {
            return "TrackElement(image_id=" + std::to_string(e.image_id) + ", point2D_idx=" + std::to_string(e.point2D_idx) + ")";
        });
    py::class_<PyTrack>(m, "Track")
        .def(py::init<>())
        .def(py::init([](const std::vector<PyTrackElement>& elements) { return PyTrack{elements}; }), "elements"_a)
        .def_readwrite("elements", &PyTrack::elements)
        .def("length", [](const PyTrack& t) { return t.elements.size(); })
        .def("add_element", [](PyTrack& t, uint32_t image_id, uint32_t point2D_idx) { t.elements.push_back({image_id, point2D_idx}); },
             "image_id"_a, "point2D_idx"_a)
        .def("__copy__", [](const PyTrack& t) { return PyTrack(t); })
        .def("__deepcopy__", [](const PyTrack& t, const py::dict&) { return PyTrack(t); })
        .def("__repr__", [](const PyTrack& t) { return "Track(length=" + std::to_string(t.elements.size()) + ")"; });
    py::class_<PyPoint3D>(m, "Point3D")
        .def(py::init<>())
        .def_readwrite("xyz", &PyPoint3D::xyz)
        .def_readwrite("color", &PyPoint3D::color)
        .def_readwrite("error", &PyPoint3D::error)
        .def_readwrite("track", &PyPoint3D::track)
        .def("__copy__", [](const PyPoint3D& p) { return PyPoint3D(p); })
        .def("__deepcopy__", [](const PyPoint3D& p, const py::dict&) { return PyPoint3D(p); })
        .def("__repr__", [](const PyPoint3D& p) {
            std::ostringstream ss;
            ss << "Point3D(xyz=[" << p.xyz[0] << ", " << p.xyz[1] << ", " << p.xyz[2] << "], track=Track(length="
               << p.track.elements.size() << "))";
            return ss.str();
        });

    py::class_<PyReconstruction>(m, "Reconstruction")
        .def(py::init<>())
        .def(py::init([](const std::string& path) {
                 PyReconstruction r;
                 read_into(r, path, 0);
                 return r;
             }),
             "path"_a)
        .def("read", [](PyReconstruction& r, const std::string& path) { read_into(r, path, 0); }, "path"_a,
             "Read the model from `path`: the three .bin files when all exist, else the three .txt files.")
        .def("read_binary", [](PyReconstruction& r, const std::string& path) { read_into(r, path, 1); }, "path"_a)
        .def("read_text", [](PyReconstruction& r, const std::string& path) { read_into(r, path, 2); }, "path"_a)
        .def("write", [](const PyReconstruction& r, const std::string& path) { WriteSparseModelBin(path, checked_model(r)); },
             "path"_a, "Write cameras.bin, images.bin and points3D.bin into the existing directory `path`, in the maps' order.")
        .def("write_binary", [](const PyReconstruction& r, const std::string& path) { WriteSparseModelBin(path, checked_model(r)); },
             "path"_a)
        .def("num_cameras", [](const PyReconstruction& r) { return r.cameras.size(); })
        .def("num_images", [](const PyReconstruction& r) { return r.images.size(); })
        .def("num_reg_images", [](const PyReconstruction& r) { return r.images.size(); },
             "Every image of this minimal Reconstruction is registered.")
        .def("num_points3D", [](const PyReconstruction& r) { return r.points3D.size(); })
        .def("reg_image_ids", [](const PyReconstruction& r) { return py::list(r.images.attr("keys")()); })
        .def_property_readonly("cameras", [](const PyReconstruction& r) { return r.cameras; })
        .def_property_readonly("images", [](const PyReconstruction& r) { return r.images; })
        .def_property_readonly("points3D", [](const PyReconstruction& r) { return r.points3D; })
        .def("add_camera", [](PyReconstruction& r, const py::object& camera) {
                 const PyCamera& c = camera.cast<const PyCamera&>();
                 c.CheckParams();
                 if (r.cameras.contains(py::int_(c.camera_id))) throw py::value_error("add_camera: camera_id " + std::to_string(c.camera_id) + " exists");
                 r.cameras[py::int_(c.camera_id)] = camera;
             }, "camera"_a)
        .def("add_image", [](PyReconstruction& r, const py::object& image) {
                 const PyImage& im = image.cast<const PyImage&>();
                 if (im.image_id == 0xFFFFFFFFu) throw py::value_error("add_image: the image has no image_id");
                 if (r.images.contains(py::int_(im.image_id))) throw py::value_error("add_image: image_id " + std::to_string(im.image_id) + " exists");
                 r.images[py::int_(im.image_id)] = image;
             }, "image"_a)
        .def("add_point3D", [](PyReconstruction& r, const std::array<double, 3>& xyz, const PyTrack& track,
                               const std::array<uint8_t, 3>& color) {
                 uint64_t id = 1;
                 for (auto item : r.points3D) id = std::max<uint64_t>(id, item.first.cast<uint64_t>() + 1);
                 for (const PyTrackElement& e : track.elements) {  // every element first, then the change
                     if (!r.images.contains(py::int_(e.image_id))) throw py::value_error("add_point3D: image " + std::to_string(e.image_id) + " does not exist");
                     const PyImage& im = r.images[py::int_(e.image_id)].cast<const PyImage&>();
                     if (e.point2D_idx >= im.points2D.size()) throw py::value_error("add_point3D: image " + std::to_string(e.image_id) + " has no point2D " + std::to_string(e.point2D_idx));
                     if (im.points2D[e.point2D_idx].point3D_id != kInvalidPoint3DId) throw py::value_error("add_point3D: point2D " + std::to_string(e.point2D_idx) + " of image " + std::to_string(e.image_id) + " already has a point3D");
                 }
                 for (const PyTrackElement& e : track.elements) r.images[py::int_(e.image_id)].cast<PyImage&>().points2D[e.point2D_idx].point3D_id = id;
                 PyPoint3D p;
                 p.xyz = xyz;
                 p.color = color;
                 p.track = track;
                 r.points3D[py::int_(id)] = py::cast(p);
                 return id;
             }, "xyz"_a, "track"_a, "color"_a = std::array<uint8_t, 3>{{0, 0, 0}})
        .def("compute_num_observations", [](const PyReconstruction& r) { return ComputeNumObservations(checked_model(r)); })
        .def("compute_mean_track_length", [](const PyReconstruction& r) { return ComputeMeanTrackLength(checked_model(r)); })
        .def("filter_observations_with_negative_depth", [](PyReconstruction& r) {
                 SparseModel m = checked_model(r);
                 const size_t n = FilterObservationsWithNegativeDepth(&m);
                 update_from_model(r, m);
                 return n;
             })
        .def("point3D_ids", [](const PyReconstruction& r) {
                 py::set ids;
                 for (auto item : r.points3D) ids.add(item.first);
                 return ids;
             })
        .def("exists_camera", [](const PyReconstruction& r, uint32_t camera_id) { return r.cameras.contains(py::int_(camera_id)); }, "camera_id"_a)
        .def("exists_image", [](const PyReconstruction& r, uint32_t image_id) { return r.images.contains(py::int_(image_id)); }, "image_id"_a)
        .def("exists_point3D", [](const PyReconstruction& r, uint64_t point3D_id) { return r.points3D.contains(py::int_(point3D_id)); }, "point3D_id"_a)
        .def("delete_point3D", [](PyReconstruction& r, uint64_t point3D_id) {
                 SparseModel m = checked_model(r);
                 DeletePoint3D(&m, point3D_id);
                 update_with_errors(r, m);
             }, "point3D_id"_a, "Delete a 3D point, and all its references in the observed images.")
        .def("delete_observation", [](PyReconstruction& r, uint32_t image_id, uint32_t point2D_idx) {
                 SparseModel m = checked_model(r);
                 DeleteObservation(&m, image_id, point2D_idx);
                 update_with_errors(r, m);
             }, "image_id"_a, "point2D_idx"_a,
             "Delete one observation from an image and the corresponding 3D point.\n"
             "Note that this deletes the entire 3D point, if the track has two elements\n"
             "prior to calling this method.")
        .def("filter_points3D", [](PyReconstruction& r, double max_reproj_error, double min_tri_angle, const std::unordered_set<uint64_t>& point3D_ids) {
                 const std::vector<uint64_t> ids(point3D_ids.begin(), point3D_ids.end());
                 return filter_model(r, &ids, nullptr, max_reproj_error, min_tri_angle, false);
             }, "max_reproj_error"_a, "min_tri_angle"_a, "point3D_ids"_a,
             "Filter 3D points with large reprojection error, negative depth, or\n"
             "insufficient triangulation angle.\n\n"
             "@param max_reproj_error    The maximum reprojection error.\n"
             "@param min_tri_angle       The minimum triangulation angle.\n"
             "@param point3D_ids         The points to be filtered.\n\n"
             "@return                    The number of filtered observations.")
        .def("filter_points3D_in_images", [](PyReconstruction& r, double max_reproj_error, double min_tri_angle, const std::unordered_set<uint32_t>& image_ids) {
                 const std::vector<uint32_t> ids(image_ids.begin(), image_ids.end());
                 return filter_model(r, nullptr, &ids, max_reproj_error, min_tri_angle, false);
             }, "max_reproj_error"_a, "min_tri_angle"_a, "image_ids"_a,
             "Filter 3D points with large reprojection error, negative depth, or\n"
             "insufficient triangulation angle.\n\n"
             "@param max_reproj_error    The maximum reprojection error.\n"
             "@param min_tri_angle       The minimum triangulation angle.\n"
             "@param image_ids           The the image ids in which the points3D are filtered.\n\n"
             "@return                    The number of filtered observations.")
        .def("filter_all_points3D", [](PyReconstruction& r, double max_reproj_error, double min_tri_angle) {
                 return filter_model(r, nullptr, nullptr, max_reproj_error, min_tri_angle, false);
             }, "max_reproj_error"_a, "min_tri_angle"_a,
             "Filter 3D points with large reprojection error, negative depth, or\n"
             "insufficient triangulation angle.\n\n"
             "@param max_reproj_error    The maximum reprojection error.\n"
             "@param min_tri_angle       The minimum triangulation angle.\n\n"
             "@return                    The number of filtered observations.")
        .def("update_point3D_errors", [](PyReconstruction& r) { filter_model(r, nullptr, nullptr, 0.0, 0.0, true); },
             "Set every 3D point's error to the mean reprojection error over its track, on the GPU (DESIGN.md section 16).")
        .def("update_point_3d_errors", [](PyReconstruction& r) { filter_model(r, nullptr, nullptr, 0.0, 0.0, true); },
             "Later pycolmap's spelling of update_point3D_errors.")
        .def("compute_mean_observations_per_reg_image", [](const PyReconstruction& r) { return ComputeMeanObservationsPerRegImage(checked_model(r)); })
        .def("compute_mean_reprojection_error", [](const PyReconstruction& r) { return ComputeMeanReprojectionError(checked_model(r)); })
        .def("summary", &summary)
        .def("__repr__", [](const PyReconstruction& r) {
            const SparseModel m = checked_model(r);
            return "Reconstruction(num_reg_images=" + std::to_string(m.images.size()) + ", num_cameras=" + std::to_string(m.cameras.size()) +
                   ", num_points3D=" + std::to_string(m.points3D.size()) + ", num_observations=" + std::to_string(ComputeNumObservations(m)) + ")";
        })
        .def("__copy__", &deep_copy)
        .def("__deepcopy__", [](const PyReconstruction& r, const py::dict&) { return deep_copy(r); });
}

}  // namespace amchost
