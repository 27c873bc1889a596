// module.cc — the entry of the Python-visible host layer: a C++/pybind11 extension with pycolmap's API
// surface, implemented over libamc.so (C ABI) + SQLite.  This file registers the module, logging, the option classes of
// matching, the value types, the single-call estimators and the pipeline entry points; the scene classes are bound in
// bind_reconstruction.cc, bind_bundle.cc, bind_triangulator.cc, bind_mapper.cc and bind_database.cc (py_scene.h), and
// what all of them share is binding_support.h.
//
// Mirrors (names, argument meaning, error behaviour):
//   match_exhaustive / match_sequential / match_spatial / verify_matches    /root/reference/pycolmap/pipeline/match_features.h:22-68, 219-260
//   SiftMatchingOptions / ExhaustiveMatchingOptions / SequentialMatchingOptions      ...:71-152
//   TwoViewGeometryOptions / TwoViewGeometryConfiguration / TwoViewGeometry
//                                                           /root/reference/pycolmap/estimators/two_view_geometry.h:41-93
//   RANSACOptions (Python-side defaults)                    /root/reference/pycolmap/optim/bindings.h:10-25
//   interruptible blocking wait                             /root/reference/pycolmap/helpers.h:306-347
//   Camera, *_matrix_estimation, estimate_two_view_geometry, squared_sampson_error -> estimators.h
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cctype>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <ctime>
#include <exception>
#include <fstream>
#include <functional>
#include <iostream>
#include <mutex>
#include <sstream>
#include <thread>

#include "abspose_host.h"
#include "binding_support.h"
#include "controller.h"
#include "estimators.h"
#include "py_scene.h"
#include "py_types.h"
#include "rigpose_host.h"
#include "sift_host.h"
#include "tri_host.h"
#include "undistort_host.h"

namespace py = pybind11;
using namespace pybind11::literals;
using namespace amchost;

namespace {

// ---- interruptible blocking run (PyWait analogue) ------------------------------------------------
void RunInterruptible(MatchController& ctrl, const std::function<void()>& work) {
    std::exception_ptr err;
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
    std::thread th([&] {
        try {
            work();
        } catch (...) {
            err = std::current_exception();
        }
        {
            std::lock_guard<std::mutex> lock(mu);
            done = true;
        }
        cv.notify_one();
    });
    bool interrupted = false;
    {
        py::gil_scoped_release release;
        for (;;) {
            {   // woken when the work is done; every 50 ms to look for a pending signal
                std::unique_lock<std::mutex> lock(mu);
                if (cv.wait_for(lock, std::chrono::milliseconds(50), [&] { return done; })) break;
            }
            py::gil_scoped_acquire acquire;
            if (PyErr_CheckSignals() != 0) {  // Ctrl-C: stop cooperatively between blocks
                interrupted = true;
                ctrl.RequestStop();
                break;
            }
        }
        th.join();
    }
    if (interrupted) throw py::error_already_set();
    if (err) {
        try {
            std::rethrow_exception(err);
        } catch (const AmcFailure& e) {
            if (e.code == AMC_E_INVALID) throw py::value_error(e.what());
            throw std::runtime_error(e.what());
        } catch (const std::invalid_argument& e) {
            throw py::value_error(e.what());
        }
    }
}

py::dict StatsDict(const MatchStats& s) {
    return py::dict("pairs_matched"_a = s.pairs_matched, "pairs_verified"_a = s.pairs_verified,
                    "pairs_skipped"_a = s.pairs_skipped, "match_device_ms"_a = s.match_device_ms,
                    "verify_device_ms"_a = s.verify_device_ms, "db_ms"_a = s.db_ms,
                    "match_call_ms"_a = s.match_call_ms, "verify_call_ms"_a = s.verify_call_ms,
                    "match_total_ms"_a = s.match_total_ms, "setup_ms"_a = s.setup_ms, "write_ms"_a = s.write_ms,
                    "num_distances"_a = s.num_distances, "pairs_guided"_a = s.pairs_guided,
                    "guided_device_ms"_a = s.guided_device_ms, "loop_queries"_a = s.loop_queries,
                    "loop_pairs_scored"_a = s.loop_pairs_scored, "loop_device_ms"_a = s.loop_device_ms,
                    "fused_call_timeline_ms"_a = py::dict("verify_setup"_a = s.fused_setup_ms, "match_call"_a = s.fused_match_ms,
                                                        "close_and_launch"_a = s.fused_launch_ms,
                                                        "verify_wait_pack_download"_a = s.fused_verify_wait_ms,
                                                        "batch_handover_hidden"_a = s.fused_handover_hidden_ms));
}

}  // namespace

// SiftMatchingOptions.gpu_index (/root/reference/pycolmap/pipeline/match_features.h:76-81; COLMAP:
// "Index of the GPU used for feature matching. For multi-GPU matching, you should separate multiple GPU indices
// by comma, e.g., '0,1,2,3'", "-1" = every device): the list of devices the controller opens a context on.
// An index may repeat.  Anything that is not a list of device numbers raises instead of being ignored.
static std::vector<int> ParseGpuIndex(const std::string& gpu_index) {
    std::vector<int> out;
    std::string tok;
    auto flush = [&] {
        size_t a = 0, b = tok.size();
        while (a < b && std::isspace(static_cast<unsigned char>(tok[a]))) ++a;
        while (b > a && std::isspace(static_cast<unsigned char>(tok[b - 1]))) --b;
        const std::string t = tok.substr(a, b - a);
        tok.clear();
        if (t.empty()) throw py::value_error("gpu_index: empty entry in '" + gpu_index + "'");
        size_t pos = 0;
        int v = 0;
        try {
            v = std::stoi(t, &pos);
        } catch (const std::exception&) {
            pos = 0;
        }
        if (pos != t.size()) throw py::value_error("gpu_index: '" + t + "' is not a device number (in '" + gpu_index + "')");
        out.push_back(v);
    };
    for (char ch : gpu_index) {
        if (ch == ',') flush();
        else tok.push_back(ch);
    }
    flush();
    if (out.size() == 1 && out[0] == -1) {  // all devices
        const int n = amc_device_count();
        if (n <= 0) throw std::runtime_error(std::string("gpu_index -1: no MI355X device visible: ") + (n < 0 ? amc_last_error() : ""));
        out.clear();
        for (int i = 0; i < n; ++i) out.push_back(i);
        return out;
    }
    for (int v : out)
        if (v < 0) throw py::value_error("gpu_index: negative device number in '" + gpu_index + "' (-1 alone means all devices)");
    return out;
}

// ---- pycolmap.logging (binding_support.h declares the sink; /root/reference/pycolmap/main.cc:39-89): glog's line
// format, severity filtering by minloglevel / stderrthreshold, optional files.  fatal raises (glog aborts the process).
void amchost::Logging::Write(Level lv, const std::string& where, int line, const std::string& msg) {
    if (static_cast<int>(lv) < minloglevel) return;
    const auto now = std::chrono::system_clock::now();
    const std::time_t t = std::chrono::system_clock::to_time_t(now);
    const long us = static_cast<long>(std::chrono::duration_cast<std::chrono::microseconds>(now.time_since_epoch()).count() % 1000000);
    std::tm tmv;
    localtime_r(&t, &tmv);
    char head[64];
    std::snprintf(head, sizeof head, "%c%04d%02d%02d %02d:%02d:%02d.%06ld", "IWEF"[lv], tmv.tm_year + 1900, tmv.tm_mon + 1,
                  tmv.tm_mday, tmv.tm_hour, tmv.tm_min, tmv.tm_sec, us);
    std::ostringstream ln;
    ln << head << " " << std::this_thread::get_id() << " " << where << ":" << line << "] " << msg << "\n";
    std::lock_guard<std::mutex> lock(mu);
    if (logtostderr || alsologtostderr || static_cast<int>(lv) >= stderrthreshold) std::cerr << ln.str() << std::flush;
    if (!logtostderr)
        for (int k = 0; k <= static_cast<int>(lv); ++k) {  // glog: a message goes to its severity's file and all lower ones
            std::string path = destination[k];
            if (path.empty() && !log_dir.empty()) path = log_dir + "/pycolmap_amd." + "IWEF"[k] + ".log";
            if (path.empty()) continue;
            std::ofstream f(path, std::ios::app);
            f << ln.str();
        }
}
int Logging::minloglevel = 0;
int Logging::stderrthreshold = 2;
std::string Logging::log_dir;
bool Logging::logtostderr = false;
bool Logging::alsologtostderr = true;   // the reference sets FLAGS_alsologtostderr = true at import
std::string Logging::destination[4];
std::mutex Logging::mu;

std::pair<std::string, int> amchost::PythonCallFrame() {
    const py::object frame = py::module_::import("sys").attr("_getframe")(0);
    const std::string file = py::str(frame.attr("f_code").attr("co_filename"));
    const std::string function = py::str(frame.attr("f_code").attr("co_name"));
    return {file + ":" + function, py::int_(frame.attr("f_lineno"))};
}

static void BindLogging(py::module_& m) {
    py::class_<Logging> PyLogging(m, "logging");
    PyLogging.def_readwrite_static("minloglevel", &Logging::minloglevel)
        .def_readwrite_static("stderrthreshold", &Logging::stderrthreshold)
        .def_readwrite_static("log_dir", &Logging::log_dir)
        .def_readwrite_static("logtostderr", &Logging::logtostderr)
        .def_readwrite_static("alsologtostderr", &Logging::alsologtostderr)
        .def_static("set_log_destination",
                    [](Logging::Level severity, const std::string& path) { Logging::destination[severity] = path; })
        .def_static("info", [](const std::string& msg) { auto f = PythonCallFrame(); Logging::Write(Logging::INFO, f.first, f.second, msg); })
        .def_static("warning", [](const std::string& msg) { auto f = PythonCallFrame(); Logging::Write(Logging::WARNING, f.first, f.second, msg); })
        .def_static("error", [](const std::string& msg) { auto f = PythonCallFrame(); Logging::Write(Logging::ERROR, f.first, f.second, msg); })
        .def_static("fatal", [](const std::string& msg) {
            auto f = PythonCallFrame();
            Logging::Write(Logging::FATAL, f.first, f.second, msg);
            throw std::runtime_error("pycolmap.logging.fatal: " + msg);
        });
    py::enum_<Logging::Level>(PyLogging, "Level")
        .value("INFO", Logging::INFO)
        .value("WARNING", Logging::WARNING)
        .value("ERROR", Logging::ERROR)
        .value("FATAL", Logging::FATAL)
        .export_values();
}

PYBIND11_MODULE(_pycolmap, m) {
    m.doc() = "MI355X-native match + verify path behind the pycolmap API (pycolmap_amd)";
    m.attr("has_cuda") = true;  // drop-in: "an accelerator is available" (it is an MI355X)
    m.attr("has_hip") = true;
    m.attr("COLMAP_version") = "3.9.1-semantics";
    m.attr("COLMAP_build") = "pycolmap_amd (libamc.so, gfx950)";
    BindLogging(m);

    py::enum_<Device> PyDevice(m, "Device");
    PyDevice.value("auto", Device::AUTO).value("cpu", Device::CPU).value("cuda", Device::CUDA);
    PyDevice.def(py::init([](const std::string& s) {
        if (s == "auto") return Device::AUTO;
        if (s == "cpu") return Device::CPU;
        if (s == "cuda" || s == "hip") return Device::CUDA;
        throw py::value_error("Invalid string value " + s + " for enum Device");
    }));
    py::implicitly_convertible<std::string, Device>();

    // ---- RANSACOptions: Python-side defaults differ from the C++ struct's -------------------
    py::class_<RANSACOptions> PyRANSAC(m, "RANSACOptions");
    PyRANSAC.def(py::init([]() {
        RANSACOptions o;  // /root/reference/pycolmap/optim/bindings.h:10-18
        o.max_error = 4.0;
        o.min_inlier_ratio = 0.01;
        o.confidence = 0.9999;
        o.min_num_trials = 1000;
        o.max_num_trials = 100000;
        return o;
    }));
    PyRANSAC.def_readwrite("max_error", &RANSACOptions::max_error)
        .def_readwrite("min_inlier_ratio", &RANSACOptions::min_inlier_ratio)
        .def_readwrite("confidence", &RANSACOptions::confidence)
        .def_readwrite("dyn_num_trials_multiplier", &RANSACOptions::dyn_num_trials_multiplier)
        .def_readwrite("min_num_trials", &RANSACOptions::min_num_trials)
        .def_readwrite("max_num_trials", &RANSACOptions::max_num_trials);
    MakeDataclass(PyRANSAC, {"max_error", "min_inlier_ratio", "confidence", "dyn_num_trials_multiplier",
                             "min_num_trials", "max_num_trials"});

    py::class_<SiftMatchingOptions> PySift(m, "SiftMatchingOptions");
    PySift.def(py::init<>())
        .def_readwrite("num_threads", &SiftMatchingOptions::num_threads)
        .def_readwrite("gpu_index", &SiftMatchingOptions::gpu_index,
                       "Index of the GPU used for feature matching. For multi-GPU matching, you should "
                       "separate multiple GPU indices by comma, e.g., \"0,1,2,3\".")
        .def_readwrite("max_ratio", &SiftMatchingOptions::max_ratio,
                       "Maximum distance ratio between first and second best match.")
        .def_readwrite("max_distance", &SiftMatchingOptions::max_distance, "Maximum distance to best match.")
        .def_readwrite("cross_check", &SiftMatchingOptions::cross_check,
                       "Whether to enable cross checking in matching.")
        .def_readwrite("max_num_matches", &SiftMatchingOptions::max_num_matches, "Maximum number of matches.")
        .def_readwrite("guided_matching", &SiftMatchingOptions::guided_matching,
                       "Whether to perform guided matching, if geometric verification succeeds.");
    MakeDataclass(PySift, {"num_threads", "gpu_index", "max_ratio", "max_distance", "cross_check",
                           "max_num_matches", "guided_matching"});

    // ---- SIFT extraction (/root/reference/pycolmap/pipeline/extract_features.h:71-138, feature/sift.h) ---------------
    using SEOpts = SiftExtractionOptions;
    py::enum_<SEOpts::Normalization> PyNorm(m, "Normalization");
    PyNorm.value("L1_ROOT", SEOpts::Normalization::L1_ROOT,
                  "L1-normalizes each descriptor followed by element-wise square rooting.")
        .value("L2", SEOpts::Normalization::L2, "Each vector is L2-normalized.");
    PyNorm.def(py::init([](const std::string& s) {
        if (s == "L1_ROOT") return SEOpts::Normalization::L1_ROOT;
        if (s == "L2") return SEOpts::Normalization::L2;
        throw py::value_error("Invalid string value " + s + " for enum Normalization");
    }));
    py::implicitly_convertible<std::string, SEOpts::Normalization>();
    py::class_<SEOpts> PySEOpts(m, "SiftExtractionOptions");
    PySEOpts.def(py::init<>())
        .def_readwrite("num_threads", &SEOpts::num_threads)
        .def_readwrite("gpu_index", &SEOpts::gpu_index, "Index of the GPU used for feature extraction.")
        .def_readwrite("max_image_size", &SEOpts::max_image_size,
                       "Maximum image size, otherwise image will be down-scaled.")
        .def_readwrite("max_num_features", &SEOpts::max_num_features,
                       "Maximum number of features to detect, keeping larger-scale features.")
        .def_readwrite("first_octave", &SEOpts::first_octave,
                       "First octave in the pyramid, i.e. -1 upsamples the image by one level.")
        .def_readwrite("num_octaves", &SEOpts::num_octaves)
        .def_readwrite("octave_resolution", &SEOpts::octave_resolution, "Number of levels per octave.")
        .def_readwrite("peak_threshold", &SEOpts::peak_threshold, "Peak threshold for detection.")
        .def_readwrite("edge_threshold", &SEOpts::edge_threshold, "Edge threshold for detection.")
        .def_readwrite("estimate_affine_shape", &SEOpts::estimate_affine_shape,
                       "Estimate affine shape of SIFT features (not supported: raises ValueError).")
        .def_readwrite("max_num_orientations", &SEOpts::max_num_orientations,
                       "Maximum number of orientations per keypoint if not estimate_affine_shape.")
        .def_readwrite("upright", &SEOpts::upright, "Fix the orientation to 0 for upright features")
        .def_readwrite("darkness_adaptivity", &SEOpts::darkness_adaptivity, "Not supported: raises ValueError.")
        .def_readwrite("domain_size_pooling", &SEOpts::domain_size_pooling, "Not supported: raises ValueError.")
        .def_readwrite("dsp_min_scale", &SEOpts::dsp_min_scale)
        .def_readwrite("dsp_max_scale", &SEOpts::dsp_max_scale)
        .def_readwrite("dsp_num_scales", &SEOpts::dsp_num_scales)
        .def_readwrite("normalization", &SEOpts::normalization, "L1_ROOT or L2 descriptor normalization");
    MakeDataclass(PySEOpts, {"num_threads", "gpu_index", "max_image_size", "max_num_features", "first_octave",
                             "num_octaves", "octave_resolution", "peak_threshold", "edge_threshold",
                             "estimate_affine_shape", "max_num_orientations", "upright", "darkness_adaptivity",
                             "domain_size_pooling", "dsp_min_scale", "dsp_max_scale", "dsp_num_scales",
                             "normalization"});
    {
        py::dict sift_defaults;  // "for backwards consistency" (/root/reference/pycolmap/feature/sift.h:98-102)
        sift_defaults["peak_threshold"] = 0.01;
        sift_defaults["first_octave"] = 0;
        sift_defaults["max_image_size"] = 7000;
        py::class_<SiftExtractor>(m, "Sift")
            .def(py::init([](SEOpts options, Device device) {
                     RequireAccelerator(device);
                     return std::make_unique<SiftExtractor>(std::move(options));
                 }),
                 "options"_a = sift_defaults, "device"_a = Device::AUTO)
            .def("extract", &SiftExtractor::Extract, "image"_a.noconvert())
            .def("extract", &SiftExtractor::ExtractFloat, "image"_a.noconvert())
            .def_property_readonly("options", &SiftExtractor::Options)
            .def_property_readonly("device", [](const SiftExtractor&) { return Device::CUDA; })
            .def_property_readonly("last_device_ms", &SiftExtractor::LastDeviceMs,
                                   "Device time of the last extract call, ms (pycolmap_amd extension).");
    }

    py::enum_<CameraMode> PyCameraMode(m, "CameraMode");
    PyCameraMode.value("AUTO", CameraMode::AUTO)
        .value("SINGLE", CameraMode::SINGLE)
        .value("PER_FOLDER", CameraMode::PER_FOLDER)
        .value("PER_IMAGE", CameraMode::PER_IMAGE);
    PyCameraMode.def(py::init([](const std::string& s) {
        if (s == "AUTO") return CameraMode::AUTO;
        if (s == "SINGLE") return CameraMode::SINGLE;
        if (s == "PER_FOLDER") return CameraMode::PER_FOLDER;
        if (s == "PER_IMAGE") return CameraMode::PER_IMAGE;
        throw py::value_error("Invalid string value " + s + " for enum CameraMode");
    }));
    py::implicitly_convertible<std::string, CameraMode>();
    py::class_<ImageReaderOptions> PyIROpts(m, "ImageReaderOptions");
    PyIROpts.def(py::init<>())
        .def_readwrite("camera_model", &ImageReaderOptions::camera_model, "Name of the camera model.")
        .def_readwrite("mask_path", &ImageReaderOptions::mask_path, "Image masks (not supported: raises ValueError).")
        .def_readwrite("existing_camera_id", &ImageReaderOptions::existing_camera_id,
                       "Use an existing camera for all images (not supported: raises ValueError).")
        .def_readwrite("camera_params", &ImageReaderOptions::camera_params,
                       "Manual specification of camera parameters (comma-separated).")
        .def_readwrite("default_focal_length_factor", &ImageReaderOptions::default_focal_length_factor,
                       "The focal length is set to `default_focal_length_factor * max(width, height)` (EXIF is not read).")
        .def_readwrite("camera_mask_path", &ImageReaderOptions::camera_mask_path,
                       "A mask for all images (not supported: raises ValueError).");
    MakeDataclass(PyIROpts, {"camera_model", "mask_path", "existing_camera_id", "camera_params",
                             "default_focal_length_factor", "camera_mask_path"});

    py::class_<ExhaustiveMatchingOptions> PyExh(m, "ExhaustiveMatchingOptions");
    PyExh.def(py::init<>()).def_readwrite("block_size", &ExhaustiveMatchingOptions::block_size);
    MakeDataclass(PyExh, {"block_size"});

    py::class_<SequentialMatchingOptions> PySeq(m, "SequentialMatchingOptions");
    PySeq.def(py::init<>())
        .def_readwrite("overlap", &SequentialMatchingOptions::overlap, "Number of overlapping image pairs.")
        .def_readwrite("quadratic_overlap", &SequentialMatchingOptions::quadratic_overlap,
                       "Whether to match images against their quadratic neighbors.")
        .def_readwrite("loop_detection", &SequentialMatchingOptions::loop_detection)
        .def_readwrite("loop_detection_num_images", &SequentialMatchingOptions::loop_detection_num_images)
        .def_readwrite("loop_detection_num_nearest_neighbors",
                       &SequentialMatchingOptions::loop_detection_num_nearest_neighbors)
        .def_readwrite("loop_detection_num_checks", &SequentialMatchingOptions::loop_detection_num_checks)
        .def_readwrite("loop_detection_num_images_after_verification",
                       &SequentialMatchingOptions::loop_detection_num_images_after_verification)
        .def_readwrite("loop_detection_max_num_features",
                       &SequentialMatchingOptions::loop_detection_max_num_features)
        .def_readwrite("vocab_tree_path", &SequentialMatchingOptions::vocab_tree_path);
    MakeDataclass(PySeq, {"overlap", "quadratic_overlap", "loop_detection", "loop_detection_num_images",
                          "loop_detection_num_nearest_neighbors", "loop_detection_num_checks",
                          "loop_detection_num_images_after_verification", "loop_detection_max_num_features",
                          "vocab_tree_path"});

    // match_vocabtree is outside this library's scope, but its option class exists so that a
    // script written for the reference constructs it without error and fails at the call, with the reason
    // (/root/reference/pycolmap/pipeline/match_features.h:177-214; defaults of COLMAP 3.9.1)
    struct VocabTreeMatchingOptions {
        int num_images = 100, num_nearest_neighbors = 5, num_checks = 256, num_images_after_verification = 0;
        int max_num_features = -1;
        std::string vocab_tree_path, match_list_path;
    };
    py::class_<SpatialMatchingOptions> PySp(m, "SpatialMatchingOptions");
    PySp.def(py::init<>())
        .def_readwrite("is_gps", &SpatialMatchingOptions::is_gps,
                       "Whether the location priors in the database are GPS coordinates in the form of longitude and "
                       "latitude coordinates in degrees.")
        .def_readwrite("ignore_z", &SpatialMatchingOptions::ignore_z,
                       "Whether to ignore the Z-component of the location prior.")
        .def_readwrite("max_num_neighbors", &SpatialMatchingOptions::max_num_neighbors,
                       "The maximum number of nearest neighbors to match.")
        .def_readwrite("max_distance", &SpatialMatchingOptions::max_distance,
                       "The maximum distance between the query and nearest neighbor [meters].");
    MakeDataclass(PySp, {"is_gps", "ignore_z", "max_num_neighbors", "max_distance"});
    py::class_<VocabTreeMatchingOptions> PyVt(m, "VocabTreeMatchingOptions");
    PyVt.def(py::init<>())
        .def_readwrite("num_images", &VocabTreeMatchingOptions::num_images)
        .def_readwrite("num_nearest_neighbors", &VocabTreeMatchingOptions::num_nearest_neighbors)
        .def_readwrite("num_checks", &VocabTreeMatchingOptions::num_checks)
        .def_readwrite("num_images_after_verification", &VocabTreeMatchingOptions::num_images_after_verification)
        .def_readwrite("max_num_features", &VocabTreeMatchingOptions::max_num_features)
        .def_readwrite("vocab_tree_path", &VocabTreeMatchingOptions::vocab_tree_path)
        .def_readwrite("match_list_path", &VocabTreeMatchingOptions::match_list_path);
    MakeDataclass(PyVt, {"num_images", "num_nearest_neighbors", "num_checks", "num_images_after_verification",
                         "max_num_features", "vocab_tree_path", "match_list_path"});

    py::class_<TwoViewGeometryOptions> PyTvgO(m, "TwoViewGeometryOptions");
    PyTvgO.def(py::init<>())  // C++ defaults, incl. the C++ RANSAC defaults
        .def_readwrite("min_num_inliers", &TwoViewGeometryOptions::min_num_inliers)
        .def_readwrite("min_E_F_inlier_ratio", &TwoViewGeometryOptions::min_E_F_inlier_ratio)
        .def_readwrite("max_H_inlier_ratio", &TwoViewGeometryOptions::max_H_inlier_ratio)
        .def_readwrite("watermark_min_inlier_ratio", &TwoViewGeometryOptions::watermark_min_inlier_ratio)
        .def_readwrite("watermark_border_size", &TwoViewGeometryOptions::watermark_border_size)
        .def_readwrite("detect_watermark", &TwoViewGeometryOptions::detect_watermark)
        .def_readwrite("multiple_ignore_watermark", &TwoViewGeometryOptions::multiple_ignore_watermark)
        .def_readwrite("force_H_use", &TwoViewGeometryOptions::force_H_use)
        .def_readwrite("compute_relative_pose", &TwoViewGeometryOptions::compute_relative_pose)
        .def_readwrite("multiple_models", &TwoViewGeometryOptions::multiple_models)
        .def_readwrite("ransac", &TwoViewGeometryOptions::ransac_options);
    MakeDataclass(PyTvgO, {"min_num_inliers", "min_E_F_inlier_ratio", "max_H_inlier_ratio",
                           "watermark_min_inlier_ratio", "watermark_border_size", "detect_watermark",
                           "multiple_ignore_watermark", "force_H_use", "compute_relative_pose",
                           "multiple_models", "ransac"});

    // Rotation3d / Rigid3d: value types of cam2_from_cam1 (/root/reference/pycolmap/geometry/bindings.h:24-104)
    py::class_<PyRotation3d>(m, "Rotation3d")
        .def(py::init<>())
        .def(py::init([](const std::array<double, 4>& xyzw) {
                 PyRotation3d r;
                 r.xyzw = xyzw;
                 return r;
             }),
             "xyzw"_a, "Quaternion in [x,y,z,w] format.")
        .def(py::init([](const py::array_t<double, py::array::c_style | py::array::forcecast>& a) {
                 // a 3 x 3 rotation matrix or an axis-angle 3-vector (the reference's two other constructors)
                 if (a.ndim() == 2 && a.shape(0) == 3 && a.shape(1) == 3) {
                     std::array<double, 9> m;
                     std::memcpy(m.data(), a.data(), sizeof(double) * 9);
                     return PyRotation3d::FromMatrix(m);
                 }
                 if (a.ndim() == 1 && a.shape(0) == 3) return PyRotation3d::FromAxisAngle({{a.at(0), a.at(1), a.at(2)}});
                 if (a.ndim() == 1 && a.shape(0) == 4) {
                     PyRotation3d r;
                     r.xyzw = {{a.at(0), a.at(1), a.at(2), a.at(3)}};
                     return r;
                 }
                 throw py::value_error("Rotation3d: expected a quaternion [x,y,z,w], a 3 x 3 rotation matrix or an axis-angle 3-vector");
             }),
             "rotmat_or_axis_angle"_a, "3x3 rotation matrix, or axis-angle 3D vector.")
        .def("__mul__", [](const PyRotation3d& a, const PyRotation3d& b) { return a.Mul(b); }, py::is_operator())
        .def("__mul__",
             [](const PyRotation3d& r, const py::array_t<double, py::array::c_style | py::array::forcecast>& v) -> py::array_t<double> {
                 if (v.ndim() == 1 && v.shape(0) == 3) {
                     const std::array<double, 3> o = r.Rotate({{v.at(0), v.at(1), v.at(2)}});
                     py::array_t<double> out(3);
                     std::memcpy(out.mutable_data(), o.data(), sizeof(double) * 3);
                     return out;
                 }
                 if (v.ndim() == 2 && v.shape(1) == 3) {  // points * R^T
                     const std::array<double, 9> R = r.Matrix();
                     py::array_t<double> out({v.shape(0), static_cast<py::ssize_t>(3)});
                     for (py::ssize_t i = 0; i < v.shape(0); ++i)
                         for (int j = 0; j < 3; ++j)
                             out.mutable_at(i, j) = v.at(i, 0) * R[3 * j] + v.at(i, 1) * R[3 * j + 1] + v.at(i, 2) * R[3 * j + 2];
                     return out;
                 }
                 throw py::value_error("Rotation3d * x: x must be a Rotation3d, a 3-vector or an N x 3 array");
             },
             py::is_operator())
        .def("normalize",
             [](PyRotation3d& r) {
                 const double n = std::sqrt(r.SquaredNorm());
                 for (double& c : r.xyzw) c /= n;
             })
        .def("angle", &PyRotation3d::Angle)
        .def("angle_to", &PyRotation3d::AngleTo, "other"_a)
        .def("inverse", &PyRotation3d::Inverse)
        .def_property(
            "quat",
            [](const PyRotation3d& r) {
                py::array_t<double> a(4);
                std::memcpy(a.mutable_data(), r.xyzw.data(), sizeof(double) * 4);
                return a;
            },
            [](PyRotation3d& r, const std::array<double, 4>& q) { r.xyzw = q; }, "Quaternion in [x,y,z,w] format.")
        .def("matrix", [](const PyRotation3d& r) { return Mat3(r.Matrix()); })
        .def("norm",
             [](const PyRotation3d& r) {
                 return std::sqrt(r.xyzw[0] * r.xyzw[0] + r.xyzw[1] * r.xyzw[1] + r.xyzw[2] * r.xyzw[2] +
                                  r.xyzw[3] * r.xyzw[3]);
             })
        .def("__repr__", [](const PyRotation3d& r) {
            std::ostringstream ss;
            ss << "Rotation3d(quat_xyzw=[" << r.xyzw[0] << ", " << r.xyzw[1] << ", " << r.xyzw[2] << ", " << r.xyzw[3]
               << "])";
            return ss.str();
        });
    py::class_<PyRigid3d>(m, "Rigid3d")
        .def(py::init<>())
        .def(py::init([](const PyRotation3d& r, const std::array<double, 3>& t) {
            PyRigid3d x;
            x.rotation = r;
            x.translation = t;
            return x;
        }))
        .def(py::init([](const py::array_t<double, py::array::c_style | py::array::forcecast>& a) {
                 if (a.ndim() != 2 || a.shape(0) != 3 || a.shape(1) != 4) throw py::value_error("Rigid3d: expected a 3 x 4 matrix [R | t]");
                 std::array<double, 9> m;
                 PyRigid3d x;
                 for (int i = 0; i < 3; ++i) {
                     for (int j = 0; j < 3; ++j) m[3 * i + j] = a.at(i, j);
                     x.translation[i] = a.at(i, 3);
                 }
                 x.rotation = PyRotation3d::FromMatrix(m);
                 return x;
             }),
             "matrix"_a)
        .def("__mul__", [](const PyRigid3d& a, const PyRigid3d& b) { return a.Mul(b); }, py::is_operator())
        .def("__mul__",
             [](const PyRigid3d& r, const py::array_t<double, py::array::c_style | py::array::forcecast>& v) -> py::array_t<double> {
                 if (v.ndim() == 1 && v.shape(0) == 3) {
                     const std::array<double, 3> o = r.Apply({{v.at(0), v.at(1), v.at(2)}});
                     py::array_t<double> out(3);
                     std::memcpy(out.mutable_data(), o.data(), sizeof(double) * 3);
                     return out;
                 }
                 if (v.ndim() == 2 && v.shape(1) == 3) {  // points * R^T, + t to every row
                     const std::array<double, 9> R = r.rotation.Matrix();
                     py::array_t<double> out({v.shape(0), static_cast<py::ssize_t>(3)});
                     for (py::ssize_t i = 0; i < v.shape(0); ++i)
                         for (int j = 0; j < 3; ++j)
                             out.mutable_at(i, j) =
                                 (v.at(i, 0) * R[3 * j] + v.at(i, 1) * R[3 * j + 1] + v.at(i, 2) * R[3 * j + 2]) + r.translation[j];
                     return out;
                 }
                 throw py::value_error("Rigid3d * x: x must be a Rigid3d, a 3-vector or an N x 3 array");
             },
             py::is_operator())
        .def("inverse", &PyRigid3d::Inverse)
        .def("essential_matrix",
             [](const PyRigid3d& r) {  // EssentialMatrixFromPose: [t / |t|]_x R
                 const double n = std::sqrt(r.translation[0] * r.translation[0] + r.translation[1] * r.translation[1] +
                                            r.translation[2] * r.translation[2]);
                 std::array<double, 3> t = r.translation;
                 if (n > 0.0)
                     for (double& c : t) c /= n;
                 const std::array<double, 9> R = r.rotation.Matrix();
                 const double X[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
                 std::array<double, 9> E{};
                 for (int i = 0; i < 3; ++i)
                     for (int j = 0; j < 3; ++j) E[3 * i + j] = X[3 * i] * R[j] + X[3 * i + 1] * R[3 + j] + X[3 * i + 2] * R[6 + j];
                 return Mat3(E);
             })
        .def_static(
            "interpolate",
            [](const PyRigid3d& a, const PyRigid3d& b, double t) {  // InterpolateCameraPoses: slerp + linear translation
                PyRigid3d r;
                r.rotation = a.rotation.Slerp(t, b.rotation);
                for (int i = 0; i < 3; ++i) r.translation[i] = a.translation[i] + (b.translation[i] - a.translation[i]) * t;
                return r;
            },
            "cam_from_world1"_a, "cam_from_world2"_a, "t"_a)
        .def_readwrite("rotation", &PyRigid3d::rotation)
        .def_property(
            "translation",
            [](const PyRigid3d& r) {
                py::array_t<double> a(3);
                std::memcpy(a.mutable_data(), r.translation.data(), sizeof(double) * 3);
                return a;
            },
            [](PyRigid3d& r, const std::array<double, 3>& t) { r.translation = t; })
        .def("matrix",
             [](const PyRigid3d& r) {  // Rigid3d::ToMatrix: [R | t], 3 x 4
                 const std::array<double, 9> R = r.rotation.Matrix();
                 py::array_t<double> a({3, 4});
                 double* d = a.mutable_data();
                 for (int i = 0; i < 3; ++i) {
                     for (int j = 0; j < 3; ++j) d[4 * i + j] = R[3 * i + j];
                     d[4 * i + 3] = r.translation[i];
                 }
                 return a;
             })
        .def("__repr__", [](const PyRigid3d& r) {
            std::ostringstream ss;
            ss << "Rigid3d(quat_xyzw=[" << r.rotation.xyzw[0] << ", " << r.rotation.xyzw[1] << ", " << r.rotation.xyzw[2]
               << ", " << r.rotation.xyzw[3] << "], t=[" << r.translation[0] << ", " << r.translation[1] << ", "
               << r.translation[2] << "])";
            return ss.str();
        });

    py::class_<PyTwoViewGeometry> PyTvg(m, "TwoViewGeometry");
    py::object cfg_enum = py::module_::import("enum").attr("IntEnum")(
        "TwoViewGeometryConfiguration",
        py::dict("UNDEFINED"_a = 0, "DEGENERATE"_a = 1, "CALIBRATED"_a = 2, "UNCALIBRATED"_a = 3, "PLANAR"_a = 4,
                 "PANORAMIC"_a = 5, "PLANAR_OR_PANORAMIC"_a = 6, "WATERMARK"_a = 7, "MULTIPLE"_a = 8));
    m.attr("TwoViewGeometryConfiguration") = cfg_enum;
    PyTvg.def(py::init<>())
        .def_property_readonly("config", [cfg_enum](const PyTwoViewGeometry& s) { return cfg_enum(s.config); })
        .def_property_readonly("E", [](const PyTwoViewGeometry& s) { return Mat3(s.E); })
        .def_property_readonly("F", [](const PyTwoViewGeometry& s) { return Mat3(s.F); })
        .def_property_readonly("H", [](const PyTwoViewGeometry& s) { return Mat3(s.H); })
        .def_readonly("cam2_from_cam1", &PyTwoViewGeometry::cam2_from_cam1)
        .def_property_readonly("inlier_matches",
                               [](const PyTwoViewGeometry& s) { return MatchesArray(s.inlier_matches); })
        .def_readonly("tri_angle", &PyTwoViewGeometry::tri_angle)
        .def("invert",
             [](PyTwoViewGeometry& g) {  // TwoViewGeometry::Invert: the geometry as seen from image 2
                 TwoViewGeometryRow r;
                 r.config = g.config;
                 r.E = g.E;
                 r.F = g.F;
                 r.H = g.H;
                 r.inlier_matches = std::move(g.inlier_matches);
                 r.qvec = {{g.cam2_from_cam1.rotation.xyzw[3], g.cam2_from_cam1.rotation.xyzw[0],
                            g.cam2_from_cam1.rotation.xyzw[1], g.cam2_from_cam1.rotation.xyzw[2]}};
                 r.tvec = g.cam2_from_cam1.translation;
                 r.Invert();
                 g.E = r.E;
                 g.F = r.F;
                 g.H = r.H;
                 g.inlier_matches = std::move(r.inlier_matches);
                 g.cam2_from_cam1.rotation.xyzw = {{r.qvec[1], r.qvec[2], r.qvec[3], r.qvec[0]}};
                 g.cam2_from_cam1.translation = r.tvec;
             })
        .def("todict",
             [cfg_enum](const PyTwoViewGeometry& s) {
                 return py::dict("config"_a = cfg_enum(s.config), "E"_a = Mat3(s.E), "F"_a = Mat3(s.F), "H"_a = Mat3(s.H),
                                 "cam2_from_cam1"_a = s.cam2_from_cam1, "inlier_matches"_a = MatchesArray(s.inlier_matches),
                                 "tri_angle"_a = s.tri_angle);
             })
        .def("__copy__", [](const PyTwoViewGeometry& s) { return PyTwoViewGeometry(s); })
        .def("__deepcopy__", [](const PyTwoViewGeometry& s, const py::dict&) { return PyTwoViewGeometry(s); });

    // ---- Camera (estimators.h), then the scene classes in the order their signatures and default arguments need:
    // Point2D ... Reconstruction, the bundle adjustment, the triangulator and track operations, the mapper ----
    BindCamera(m);
    BindReconstruction(m);
    BindBundle(m);
    BindTriangulator(m);
    BindMapper(m);

    // ---- estimate_triangulation (/root/reference/pycolmap/estimators/triangulation.h; tri_host.h) ----------------------
    py::class_<TriPointData>(m, "PointData")
        .def(py::init([](const std::array<double, 2>& point, const std::array<double, 2>& point_normalized) {
                 return TriPointData{point, point_normalized};
             }),
             "point"_a, "point_normalized"_a)
        .def_readwrite("point", &TriPointData::point, "Pixel coordinates of the observation.")
        .def_readwrite("point_normalized", &TriPointData::point_normalized,
                       "Normalized image coordinates (Camera.cam_from_img of the pixel).")
        .def("__repr__", [](const TriPointData& d) {
            std::ostringstream ss;
            ss.precision(17);
            ss << "PointData(point=[" << d.point[0] << ", " << d.point[1] << "], point_normalized=["
               << d.point_normalized[0] << ", " << d.point_normalized[1] << "])";
            return ss.str();
        });
    const py::object py_ransac_cls = m.attr("RANSACOptions");
    py::class_<EstimateTriangulationOptions> PyTriOpts(m, "EstimateTriangulationOptions");
    PyTriOpts
        .def(py::init([py_ransac_cls]() {
            EstimateTriangulationOptions o;  // the RANSACOptions of pycolmap's Python-side defaults
            o.ransac = py_ransac_cls().cast<RANSACOptions>();
            return o;
        }))
        .def_readwrite("min_tri_angle", &EstimateTriangulationOptions::min_tri_angle,
                       "Minimum triangulation angle in radians.")
        .def_readwrite("ransac", &EstimateTriangulationOptions::ransac,
                       "RANSAC options; max_error is the angular error in radians.");
    MakeDataclass(PyTriOpts, {"min_tri_angle", "ransac"});
    const EstimateTriangulationOptions tri_defaults = PyTriOpts().cast<EstimateTriangulationOptions>();
    m.def(
        "estimate_triangulation",
        [](const std::vector<TriPointData>& point_data, const std::vector<PyImage>& images,
           const std::vector<PyCamera>& cameras, const EstimateTriangulationOptions& options) -> py::object {
            CheckSameSize(images.size(), cameras.size(), "images.size() == cameras.size()");
            CheckSameSize(images.size(), point_data.size(), "images.size() == point_data.size()");
            std::vector<std::array<double, 12>> poses;
            poses.reserve(images.size());
            for (const PyImage& im : images) poses.push_back(TriPoseMatrix(im.cam_from_world));
            return EstimateTriangulationTrack(point_data, poses, options);
        },
        "point_data"_a, "images"_a, "cameras"_a, "opions"_a = tri_defaults,
        "Robustly estimate 3D point from observations in multiple views using RANSAC");

    // ---- absolute_pose_estimation / pose_refinement (reference: pycolmap/estimators/absolute_pose.h; abspose_host.h) -
    py::class_<AbsolutePoseEstimationOptions> PyAbsEst(m, "AbsolutePoseEstimationOptions");
    PyAbsEst
        .def(py::init([py_ransac_cls]() {
            AbsolutePoseEstimationOptions o;  // pycolmap's RANSACOptions() with max_error = 12, as the binding builds it
            o.ransac = py_ransac_cls().cast<RANSACOptions>();
            o.ransac.max_error = 12.0;
            return o;
        }))
        .def_readwrite("estimate_focal_length", &AbsolutePoseEstimationOptions::estimate_focal_length)
        .def_readwrite("num_focal_length_samples", &AbsolutePoseEstimationOptions::num_focal_length_samples)
        .def_readwrite("min_focal_length_ratio", &AbsolutePoseEstimationOptions::min_focal_length_ratio)
        .def_readwrite("max_focal_length_ratio", &AbsolutePoseEstimationOptions::max_focal_length_ratio)
        .def_readwrite("ransac", &AbsolutePoseEstimationOptions::ransac);
    MakeDataclass(PyAbsEst, {"estimate_focal_length", "num_focal_length_samples", "min_focal_length_ratio",
                             "max_focal_length_ratio", "ransac"});
    const AbsolutePoseEstimationOptions abs_est_defaults = PyAbsEst().cast<AbsolutePoseEstimationOptions>();
    py::class_<AbsolutePoseRefinementOptions> PyAbsRef(m, "AbsolutePoseRefinementOptions");
    PyAbsRef.def(py::init<>())
        .def_readwrite("gradient_tolerance", &AbsolutePoseRefinementOptions::gradient_tolerance)
        .def_readwrite("max_num_iterations", &AbsolutePoseRefinementOptions::max_num_iterations)
        .def_readwrite("loss_function_scale", &AbsolutePoseRefinementOptions::loss_function_scale)
        .def_readwrite("refine_focal_length", &AbsolutePoseRefinementOptions::refine_focal_length,
                       "Not supported: True raises ValueError (DESIGN.md 12, A11).")
        .def_readwrite("refine_extra_params", &AbsolutePoseRefinementOptions::refine_extra_params,
                       "Not supported: True raises ValueError (DESIGN.md 12, A11).")
        .def_readwrite("print_summary", &AbsolutePoseRefinementOptions::print_summary,
                       "Accepted; has no effect (no solver report is printed).");
    MakeDataclass(PyAbsRef, {"gradient_tolerance", "max_num_iterations", "loss_function_scale", "refine_focal_length",
                             "refine_extra_params", "print_summary"});
    const AbsolutePoseRefinementOptions abs_ref_defaults = PyAbsRef().cast<AbsolutePoseRefinementOptions>();
    m.def("absolute_pose_estimation", &EstimateAndRefineAbsolutePose, "points2D"_a, "points3D"_a, "camera"_a,
          "estimation_options"_a = abs_est_defaults, "refinement_options"_a = abs_ref_defaults,
          "return_covariance"_a = false, "Absolute pose estimation with non-linear refinement.");
    m.def("pose_refinement", &RefineAbsolutePose, "cam_from_world"_a, "points2D"_a, "points3D"_a, "inlier_mask"_a,
          "camera"_a, "refinement_options"_a = abs_ref_defaults, "Non-linear refinement of absolute pose.");

    // ---- rig_absolute_pose_estimation (reference: pycolmap/estimators/generalized_absolute_pose.h; rigpose_host.h) -----
    // The reference's m.def attaches the keyword names "cameras", "camera_idxs", "cams_from_rig" to the positions of
    // camera_idxs, cams_from_rig, cameras: cameras= names the index slot.  Reproduced as it is.
    m.def("rig_absolute_pose_estimation", &EstimateAndRefineGeneralizedAbsolutePose, "points2D"_a, "points3D"_a,
          "cameras"_a, "camera_idxs"_a, "cams_from_rig"_a,
          "estimation_options"_a = py_ransac_cls().cast<RANSACOptions>(), "refinement_options"_a = abs_ref_defaults,
          "return_covariance"_a = false,
          "Absolute pose estimation with non-linear refinement for a multi-camera rig.\n\n"
          "Positional order: points2D, points3D, camera_idxs, cams_from_rig, cameras, estimation_options, "
          "refinement_options, return_covariance.  As in the reference binding, the keyword names of the third to "
          "fifth argument are shifted: cameras= takes the camera indices, camera_idxs= the cams_from_rig list and "
          "cams_from_rig= the cameras.");

    // ---- undistort_images (reference: pycolmap/pipeline/images.h:96-148, 203-261; undistort_host.h) ------------------------
    py::class_<UndistortCameraOptions> PyUndistOpts(m, "UndistortCameraOptions");
    PyUndistOpts.def(py::init<>())
        .def_readwrite("blank_pixels", &UndistortCameraOptions::blank_pixels,
                       "The amount of blank pixels in the undistorted image in the range [0, 1].")
        .def_readwrite("min_scale", &UndistortCameraOptions::min_scale,
                       "Minimum scale change of camera used to satisfy the blank pixel constraint.")
        .def_readwrite("max_scale", &UndistortCameraOptions::max_scale,
                       "Maximum scale change of camera used to satisfy the blank pixel constraint.")
        .def_readwrite("max_image_size", &UndistortCameraOptions::max_image_size,
                       "Maximum image size in terms of width or height of the undistorted camera.")
        .def_readwrite("roi_min_x", &UndistortCameraOptions::roi_min_x)
        .def_readwrite("roi_min_y", &UndistortCameraOptions::roi_min_y)
        .def_readwrite("roi_max_x", &UndistortCameraOptions::roi_max_x)
        .def_readwrite("roi_max_y", &UndistortCameraOptions::roi_max_y);
    MakeDataclass(PyUndistOpts, {"blank_pixels", "min_scale", "max_scale", "max_image_size", "roi_min_x", "roi_min_y",
                                 "roi_max_x", "roi_max_y"});
    py::enum_<CopyType> PyCopyType(m, "CopyType");
    PyCopyType.value("copy", CopyType::COPY).value("soft-link", CopyType::SOFT_LINK).value("hard-link", CopyType::HARD_LINK);
    PyCopyType.def(py::init([](const std::string& s) {
        if (s == "copy") return CopyType::COPY;
        if (s == "soft-link") return CopyType::SOFT_LINK;
        if (s == "hard-link") return CopyType::HARD_LINK;
        throw py::value_error("Invalid string value " + s + " for enum CopyType");
    }));
    py::implicitly_convertible<std::string, CopyType>();
    m.def("undistort_camera", &UndistortCameraPy, "options"_a, "camera"_a,
          "Undistort camera: the PINHOLE camera of the undistorted image (pycolmap_amd extension under a later release's name).");
    m.def("undistort_image", &UndistortImagePy, "options"_a, "image"_a, "camera"_a,
          "Undistort an H x W or H x W x 3 uint8 image: (undistorted image, undistorted camera).");
    auto plan_camera = [](const ModelCamera& c) {
        PyCamera out;
        out.camera_id = c.camera_id;
        out.model = c.model;
        out.width = c.width;
        out.height = c.height;
        out.params = c.params;
        return out;
    };
    m.def(
        "_undistort_plan",
        [plan_camera](const py::object& input_path, const std::vector<std::string>& image_list,
                      const UndistortCameraOptions& options) {
            const SparseModel model = ReadSparseModel(PathToString(input_path));
            const std::vector<UndistortPlanItem> plan =
                UndistortPlan(model, image_list, options, [](const std::string& msg) {
                    Logging::Write(Logging::WARNING, "undistort_images", 0, msg);
                });
            py::list out;
            for (const UndistortPlanItem& it : plan)
                out.append(py::dict("name"_a = it.name, "image_id"_a = it.image_id, "camera"_a = plan_camera(it.camera),
                                    "undistorted_camera"_a = FromAmcCam(it.undistorted, it.camera.camera_id, false),
                                    "copy"_a = it.copy));
            return out;
        },
        "input_path"_a, "image_list"_a = std::vector<std::string>(), "undistort_options"_a = UndistortCameraOptions(),
        "Per image of an undistort_images call: name, image_id, camera, undistorted_camera, copy (test hook)");
    m.def(
        "_write_undistorted_model",
        [](const py::object& input_path, const py::object& output_path, const UndistortCameraOptions& options) {
            const SparseModel model = ReadSparseModel(PathToString(input_path));
            WriteSparseModelBin(PathToString(output_path), UndistortModel(model, options));
            return py::make_tuple(model.cameras.size(), model.images.size(), model.points3D.size());
        },
        "input_path"_a, "output_path"_a, "undistort_options"_a = UndistortCameraOptions(),
        "Read the sparse model at input_path, undistort it, write cameras / images / points3D .bin into output_path");

    // ---- Database, DatabaseTransaction (bind_database.cc) ----
    BindDatabase(m);

    // ---- single-pair estimators (estimators.h) ----------------------------------------------------
    BindEstimators(m);

    // ---- pipeline entry points ----------------------------------------------------------------
    m.def("_parse_gpu_index", &ParseGpuIndex, "gpu_index"_a, "SiftMatchingOptions.gpu_index -> device list (test hook)");
    auto run_pipeline = [](const py::object& database_path, const SiftMatchingOptions& sift,
                           const TwoViewGeometryOptions& tvg, Device device,
                           const std::function<void(MatchController&)>& body) {
        const std::string db_path = PathToString(database_path);
        AMC_THROW_CHECK_FILE_EXISTS(db_path);
        RequireAccelerator(device);
        const auto t0 = std::chrono::steady_clock::now();
        auto since = [](std::chrono::steady_clock::time_point t) {
            return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
        };
        auto ctrl = std::make_unique<MatchController>(db_path, sift, tvg, ParseGpuIndex(sift.gpu_index));
        RunInterruptible(*ctrl, [&] {
            ctrl->Setup();
            body(*ctrl);
        });
        py::dict st = StatsDict(ctrl->stats);
        const auto t1 = std::chrono::steady_clock::now();
        {
            py::gil_scoped_release release;
            ctrl.reset();  // closes the database (WAL again), frees the arena and the contexts' buffers
        }
        st["teardown_ms"] = since(t1);
        st["call_ms"] = since(t0);  // the whole call as the caller's clock sees it
        SetLastStats(st);
    };

    m.def(
        "match_exhaustive",
        [run_pipeline](const py::object& database_path, const SiftMatchingOptions& sift,
                       const ExhaustiveMatchingOptions& mo, const TwoViewGeometryOptions& tvg, Device device) {
            run_pipeline(database_path, sift, tvg, device, [&](MatchController& c) { RunExhaustive(c, mo); });
        },
        "database_path"_a, "sift_options"_a = SiftMatchingOptions(),
        "matching_options"_a = ExhaustiveMatchingOptions(), "verification_options"_a = TwoViewGeometryOptions(),
        "device"_a = Device::AUTO, "Exhaustive feature matching");
    m.def(
        "match_sequential",
        [run_pipeline](const py::object& database_path, const SiftMatchingOptions& sift,
                       const SequentialMatchingOptions& mo, const TwoViewGeometryOptions& tvg, Device device) {
            // options of COLMAP's vocabulary-tree retrieval that have no counterpart in the feature-voting retrieval
            // used here (controller.cc): accepted for drop-in compatibility, and said out loud when they are set
            const SequentialMatchingOptions def;
            if (mo.loop_detection && (!mo.vocab_tree_path.empty() ||
                                      mo.loop_detection_num_nearest_neighbors != def.loop_detection_num_nearest_neighbors ||
                                      mo.loop_detection_num_checks != def.loop_detection_num_checks ||
                                      mo.loop_detection_num_images_after_verification != def.loop_detection_num_images_after_verification))
                Logging::Write(Logging::WARNING, "match_sequential", 0,
                               "vocab_tree_path / loop_detection_num_nearest_neighbors / _num_checks / "
                               "_num_images_after_verification are ignored: loop closure candidates come from exact feature "
                               "voting on the first loop_detection_max_num_features descriptors, not from a vocabulary tree");
            run_pipeline(database_path, sift, tvg, device, [&](MatchController& c) { RunSequential(c, mo); });
        },
        "database_path"_a, "sift_options"_a = SiftMatchingOptions(),
        "matching_options"_a = SequentialMatchingOptions(), "verification_options"_a = TwoViewGeometryOptions(),
        "device"_a = Device::AUTO, "Sequential feature matching");
    m.def(
        "match_spatial",
        [run_pipeline](const py::object& database_path, const SiftMatchingOptions& sift,
                       const SpatialMatchingOptions& mo, const TwoViewGeometryOptions& tvg, Device device) {
            run_pipeline(database_path, sift, tvg, device, [&](MatchController& c) { RunSpatial(c, mo); });
        },
        "database_path"_a, "sift_options"_a = SiftMatchingOptions(),
        "matching_options"_a = SpatialMatchingOptions(), "verification_options"_a = TwoViewGeometryOptions(),
        "device"_a = Device::AUTO, "Spatial feature matching");
    m.def(
        "verify_matches",
        [run_pipeline](const py::object& database_path, const py::object& pairs_path,
                       const TwoViewGeometryOptions& tvg) {
            const std::string pp = PathToString(pairs_path);
            const std::string dbp = PathToString(database_path);
            AMC_THROW_CHECK_FILE_EXISTS(dbp);
            AMC_THROW_CHECK_FILE_EXISTS(pp);
            run_pipeline(database_path, SiftMatchingOptions(), tvg, Device::AUTO,
                         [&](MatchController& c) { RunImagePairs(c, pp); });
        },
        "database_path"_a, "pairs_path"_a, "options"_a = TwoViewGeometryOptions(),
        "Run geometric verification of the matches");
    auto unsupported = [](const char* what) {
        return [what](const py::args&, const py::kwargs&) {
            throw py::value_error(std::string(what) +
                                  " needs a FLANN vocabulary-tree file and is outside pycolmap_amd's scope "
                                  "(SURVEY.md section 8f); use match_exhaustive, match_sequential, match_spatial or verify_matches.");
        };
    };
    m.def("_exhaustive_blocks", &ExhaustiveBlocks, "image_ids"_a, "block_size"_a,
          "Pair blocks of ExhaustiveFeatureMatcher::Run (test hook)");
    m.def("_sequential_blocks", &SequentialBlocks, "ordered_image_ids"_a, "overlap"_a, "quadratic_overlap"_a,
          "Pair blocks of SequentialFeatureMatcher::Run (test hook)");
    m.def("_spatial_blocks", &SpatialBlocks, "image_ids"_a, "priors"_a, "options"_a,
          "Pair blocks of SpatialFeatureMatcher::Run (test hook)");
    m.def("_ell_to_xyz", &EllToXYZ, "lat_lon_alt"_a, "GPSTransform(WGS84)::EllToXYZ of one point (test hook)");
    m.def("match_vocabtree", unsupported("match_vocabtree"));
    m.attr("_last_stats") = py::dict();
    m.def("last_run_stats", []() { return py::module_::import("pycolmap_amd._pycolmap").attr("_last_stats"); },
          "Timing / counters of the most recent match_* / verify_matches / extract_features / undistort_images call\n"
          "(pycolmap_amd extension).");
}
