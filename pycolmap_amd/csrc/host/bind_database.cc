// bind_database.cc — Database and DatabaseTransaction (/root/reference/pycolmap/scene/database.h:9-46; database.h).
#include <memory>

#include "database.h"
#include "py_scene.h"

namespace amchost {
namespace {

// DatabaseTransaction (/root/reference/pycolmap/scene/database.h:44-45): BEGIN on construction, END when the
// object goes away - COLMAP's scope guard as Python sees it; also usable as a context manager, where an exception
// rolls back (an extension)
struct PyDbTransaction {
    Database* db;
    bool open = true;
    explicit PyDbTransaction(Database* d) : db(d) { db->BeginTransaction(); }
    PyDbTransaction(const PyDbTransaction&) = delete;
    void End(bool commit) {
        if (!open) return;
        open = false;
        if (commit) db->EndTransaction(); else db->RollbackTransaction();
    }
    ~PyDbTransaction() {
        try {
            End(true);
        } catch (...) {
        }
    }
};

}  // namespace

void BindDatabase(py::module_& m) {
    py::class_<Database>(m, "Database")
        .def(py::init([](const py::object& path) {
                 // Database::Open: creates the file and COLMAP's tables when they are missing
                 return std::make_unique<Database>(PathToString(path));
             }),
             "path"_a)
        .def("open", [](Database& db, const py::object& path) { db.Open(PathToString(path)); }, "path"_a)
        .def("close", &Database::Close)
        .def("num_keypoints_for_image", &Database::NumKeypointsForImage, "image_id"_a)
        .def("num_descriptors_for_image", &Database::NumDescriptorsForImage, "image_id"_a)
        .def("exists_camera", &Database::ExistsCamera, "camera_id"_a)
        .def("exists_image", &Database::ExistsImage, "image_id"_a)
        .def("read_camera", [](const Database& db, camera_t id) { return camera_from_row(db.ReadCamera(id)); },
             "camera_id"_a)
        .def("read_all_cameras",
             [](const Database& db) {
                 std::vector<PyCamera> out;
                 for (const CameraRow& r : db.ReadAllCameras()) out.push_back(camera_from_row(r));
                 return out;
             })
        .def("read_image", [](const Database& db, image_t id) { return image_from_row(db.ReadImage(id)); },
             "image_id"_a)
        .def("read_image_with_name",
             [](const Database& db, const std::string& name) { return image_from_row(db.ReadImageWithName(name)); },
             "name"_a)
        .def("read_all_images",
             [](const Database& db) {
                 std::vector<PyImage> out;
                 for (const ImageRow& r : db.ReadAllImages()) out.push_back(image_from_row(r));
                 return out;
             })
        .def("write_camera",
             [](Database& db, const PyCamera& c, bool use_camera_id) {
                 return db.WriteCamera(row_from_camera(c), use_camera_id);
             },
             "camera"_a, "use_camera_id"_a = false, "Returns the camera_id of the new row.")
        .def("write_image",
             [](Database& db, const PyImage& im, bool use_image_id) {
                 return db.WriteImage(row_from_image(im), use_image_id);
             },
             "image"_a, "use_image_id"_a = false, "Returns the image_id of the new row.")
        .def_property_readonly("num_cameras", &Database::NumCameras)
        .def_property_readonly("num_images", &Database::NumImages)
        .def_property_readonly("num_keypoints", &Database::NumKeypoints)
        .def_property_readonly("num_descriptors", &Database::NumDescriptors)
        .def_property_readonly("num_matches", &Database::NumMatches)
        .def_property_readonly("num_inlier_matches", &Database::NumInlierMatches)
        .def_property_readonly("num_matched_image_pairs", &Database::NumMatchedImagePairs)
        .def_property_readonly("num_verified_image_pairs", &Database::NumVerifiedImagePairs)
        .def_static("image_pair_to_pair_id", &Database::ImagePairToPairId, "image_id1"_a, "image_id2"_a)
        .def_static("pair_id_to_image_pair",
                    [](image_pair_t pid) {
                        image_t a, b;
                        Database::PairIdToImagePair(pid, &a, &b);
                        return std::make_pair(a, b);
                    },
                    "pair_id"_a)
        .def("exists_matches", &Database::ExistsMatches, "image_id1"_a, "image_id2"_a)
        .def("exists_inlier_matches", &Database::ExistsInlierMatches, "image_id1"_a, "image_id2"_a)
        .def("read_matches",
             [](const Database& db, image_t a, image_t b) { return MatchesArray(db.ReadMatches(a, b)); },
             "image_id1"_a, "image_id2"_a)
        // keypoints / descriptors / matches accessors: the reference leaves them unbound
        // (/root/reference/pycolmap/scene/database.h:35-41); names follow COLMAP's Database methods
        .def("set_bulk_write_mode", &Database::SetBulkWriteMode, "on"_a,
             "Rollback journal instead of WAL while appending many blobs; returns the journal mode in effect. "
             "WAL (COLMAP's mode) is restored when switched off or on close.")
        .def("exists_keypoints", &Database::ExistsKeypoints, "image_id"_a)
        .def("exists_descriptors", &Database::ExistsDescriptors, "image_id"_a)
        .def("read_keypoints",
             [](const Database& db, image_t id) {
                 uint32_t rows = 0, cols = 0;
                 const std::vector<float> v = db.ReadKeypoints(id, &rows, &cols);
                 py::array_t<float> a({static_cast<py::ssize_t>(rows), static_cast<py::ssize_t>(cols)});
                 if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(float));
                 return a;
             },
             "image_id"_a, "rows x cols float32 (cols = 2, 4 or 6: x, y[, scale, orientation | a11, a12, a21, a22])")
        .def("read_descriptors",
             [](const Database& db, image_t id) {
                 uint32_t rows = 0;
                 const std::vector<uint8_t> v = db.ReadDescriptors(id, &rows);
                 py::array_t<uint8_t> a({static_cast<py::ssize_t>(rows), static_cast<py::ssize_t>(128)});
                 if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size());
                 return a;
             },
             "image_id"_a, "rows x 128 uint8")
        .def("write_keypoints",
             [](Database& db, image_t id, const py::array_t<float, py::array::c_style | py::array::forcecast>& kp) {
                 if (kp.ndim() != 2 || (kp.shape(1) != 2 && kp.shape(1) != 4 && kp.shape(1) != 6))
                     throw py::value_error("keypoints must be an N x 2, N x 4 or N x 6 float32 array");
                 db.WriteKeypoints(id, kp.data(), static_cast<uint32_t>(kp.shape(0)), static_cast<uint32_t>(kp.shape(1)));
             },
             "image_id"_a, "keypoints"_a)
        .def("write_descriptors",
             [](Database& db, image_t id, const py::array_t<uint8_t, py::array::c_style>& d) {
                 if (d.ndim() != 2 || d.shape(1) != 128)
                     throw py::value_error("descriptors must be an N x 128 uint8 array");
                 db.WriteDescriptors(id, d.data(), static_cast<uint32_t>(d.shape(0)));
             },
             "image_id"_a, "descriptors"_a)
        .def("write_matches",
             [](Database& db, image_t a, image_t b,
                const py::array_t<uint32_t, py::array::c_style | py::array::forcecast>& m) {
                 if (m.size() != 0 && (m.ndim() != 2 || m.shape(1) != 2))
                     throw py::value_error("matches must be an M x 2 unsigned integer array");
                 db.WriteMatches(a, b, std::vector<uint32_t>(m.data(), m.data() + m.size()));
             },
             "image_id1"_a, "image_id2"_a, "matches"_a)
        .def("delete_matches", &Database::DeleteMatches, "image_id1"_a, "image_id2"_a)
        .def("delete_inlier_matches", &Database::DeleteInlierMatches, "image_id1"_a, "image_id2"_a)
        .def("read_two_view_geometry",
             [](const Database& db, image_t a, image_t b) {
                 const TwoViewGeometryRow r = db.ReadTwoViewGeometry(a, b);
                 PyTwoViewGeometry g;
                 g.config = r.config;
                 g.E = r.E;
                 g.F = r.F;
                 g.H = r.H;
                 g.inlier_matches = r.inlier_matches;
                 g.cam2_from_cam1.rotation.xyzw = {{r.qvec[1], r.qvec[2], r.qvec[3], r.qvec[0]}};
                 g.cam2_from_cam1.translation = r.tvec;
                 return g;
             },
             "image_id1"_a, "image_id2"_a);

    py::class_<PyDbTransaction>(m, "DatabaseTransaction")
        .def(py::init<Database*>(), "database"_a, py::keep_alive<1, 2>())
        .def("__enter__", [](PyDbTransaction& t) -> PyDbTransaction& { return t; }, py::return_value_policy::reference)
        .def("__exit__", [](PyDbTransaction& t, const py::object& type, const py::object&, const py::object&) {
            t.End(type.is_none());
            return false;
        });
}

}  // namespace amchost
