// module.cc — the Python-visible host layer: a C++/pybind11 extension with pycolmap's API
// surface for the match + verify path, implemented over libamc.so (C ABI) + SQLite.
//
// Mirrors (names, argument meaning, error behaviour):
//   match_exhaustive / match_sequential / match_spatial / verify_matches    /root/reference/pycolmap/pipeline/match_features.h:22-68, 219-260
//   SiftMatchingOptions / ExhaustiveMatchingOptions / SequentialMatchingOptions      ...:71-152
//   TwoViewGeometryOptions / TwoViewGeometryConfiguration / TwoViewGeometry
//                                                           /root/reference/pycolmap/estimators/two_view_geometry.h:41-93
//   RANSACOptions (Python-side defaults)                    /root/reference/pycolmap/optim/bindings.h:10-25
//   Device enum + GPU parameter check                       /root/reference/pycolmap/utils.h:9-31, main.cc:102-106
//   option "dataclass" protocol (summary/todict/mergedict, dict/kwargs ctors, implicit dict
//   conversion, copy, pickle)                               /root/reference/pycolmap/helpers.h:217-283
//   interruptible blocking wait                             /root/reference/pycolmap/helpers.h:306-347
//   Database                                                /root/reference/pycolmap/scene/database.h:9-46
//   Camera, *_matrix_estimation, estimate_two_view_geometry, squared_sampson_error -> estimators.h
#include <pybind11/numpy.h>
#include <cctype>

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <iostream>
#include <ctime>
#include <cstdio>
#include <mutex>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <exception>
#include <fstream>
#include <functional>
#include <sstream>
#include <thread>
#include <unordered_set>

#include "controller.h"
#include "py_types.h"
#include "estimators.h"
#include "sift_host.h"
#include "tri_host.h"
#include "abspose_host.h"
#include "rigpose_host.h"
#include "undistort_host.h"
#include "ba_config_host.h"
#include "ba_host.h"
#include "initial_pair_host.h"
#include "mapper_host.h"
#include "reconstruction.h"
#include "retriangulate_host.h"
#include "track_ops_host.h"
#include "triangulator_host.h"

namespace py = pybind11;
using namespace pybind11::literals;
using namespace amchost;

namespace {

enum class Device { AUTO = -1, CPU = 0, CUDA = 1 };

std::string PathToString(const py::object& p) {
    return py::module_::import("os").attr("fspath")(p).cast<std::string>();
}
// THROW_CHECK_FILE_EXISTS (/root/reference/pycolmap/log_exceptions.h:54-76, 123-125): ValueError,
// "[file:line] Check Failed: ExistsFile(path) : File <path> does not exist."
#define AMC_THROW_CHECK_FILE_EXISTS(path)                                                                        \
    do {                                                                                                         \
        std::ifstream f_(path);                                                                                  \
        if (!f_.good())                                                                                          \
            throw py::value_error(CheckMessage(__FILE__, __LINE__, "ExistsFile(" #path ")",                      \
                                               std::string("File ") + (path) + " does not exist."));             \
    } while (0)
// VerifyGPUParams analogue.  This package is the accelerator path only.
void RequireAccelerator(Device d) {
    if (d == Device::CPU)
        throw py::value_error(
            "pycolmap_amd implements the accelerated (MI355X) matcher only and has no CPU fallback; "
            "set device='auto' or device='cuda', or use the reference pycolmap for device='cpu'.");
}

// ---- option "dataclass" protocol --------------------------------------------------------------
void MergeDict(py::object self, const py::dict& d, const std::vector<std::string>& fields) {
    for (auto item : d) {
        const std::string key = py::str(item.first);
        if (std::find(fields.begin(), fields.end(), key) == fields.end()) {
            std::string known;
            for (const auto& f : fields) known += (known.empty() ? "" : ", ") + f;
            throw py::value_error(py::str(self.attr("__class__").attr("__name__")).cast<std::string>() +
                                  ": unknown option '" + key + "' (valid: " + known + ")");
        }
        py::object cur = self.attr(key.c_str());
        py::object val = py::reinterpret_borrow<py::object>(item.second);
        if (py::isinstance<py::dict>(val) && py::hasattr(cur, "mergedict")) {
            cur.attr("mergedict")(val);  // nested options: recursive merge into the defaults
            self.attr(key.c_str()) = cur;
        } else {
            self.attr(key.c_str()) = val;
        }
    }
}
py::dict ToDict(const py::object& self, const std::vector<std::string>& fields, bool recursive = true) {
    py::dict d;
    for (const auto& f : fields) {
        py::object v = self.attr(f.c_str());
        d[py::str(f)] = (recursive && py::hasattr(v, "todict")) ? v.attr("todict")() : v;
    }
    return d;
}
// CreateSummary (/root/reference/pycolmap/helpers.h:159-214): "Name:" then one line per attribute,
// "    attr = value" ("    attr: type = value" with write_type), nested option objects as "    attr: <their summary>"
// indented by four more spaces; long sequences abbreviated like the reference does.
std::string Summary(const py::object& self, const std::vector<std::string>& fields, bool write_type) {
    std::ostringstream ss;
    const std::string prefix = "    ";
    ss << py::str(self.attr("__class__").attr("__name__")).cast<std::string>() << ":";
    for (const auto& f : fields) {
        py::object v = self.attr(f.c_str());
        ss << "\n" << prefix << f;
        if (py::hasattr(v, "summary")) {
            std::string sub = v.attr("summary")(write_type).cast<std::string>();
            std::string ind;
            for (char ch : sub) {
                ind.push_back(ch);
                if (ch == '\n') ind += prefix;
            }
            ss << ": " << ind;
        } else {
            if (write_type) ss << ": " << py::str(py::type::of(v).attr("__name__")).cast<std::string>();
            std::string value = py::str(v).cast<std::string>();
            if (value.size() > 80 && py::hasattr(v, "__len__")) {
                const int n = v.attr("__len__")().cast<int>();
                value = std::string(1, value.front()) + " ... " + std::to_string(n) + " elements ... " + std::string(1, value.back());
            }
            ss << " = " << value;
        }
    }
    return ss.str();
}
// AddDefaultsToDocstrings (/root/reference/pycolmap/helpers.h:217-240): every option's docstring ends in
// "(type, default: value)", taken from a default-constructed instance
void AddDefaultsToDocstrings(const py::object& cls, const std::vector<std::string>& fields) {
    py::object obj = cls();
    for (const auto& f : fields) {
        py::object member = obj.attr(f.c_str());
        py::object prop = cls.attr(f.c_str());
        const std::string doc = py::str(prop.attr("__doc__")).cast<std::string>();
        const std::string type_name = py::str(py::type::of(member).attr("__name__")).cast<std::string>();
        std::string def = py::str(member).cast<std::string>();
        if (py::hasattr(member, "summary")) def = py::str(member.attr("__class__").attr("__name__")).cast<std::string>() + "()";
        try {
            prop.attr("__doc__") = py::str((doc == "None" ? std::string() : doc + " ") + "(" + type_name + ", default: " + def + ")");
        } catch (const py::error_already_set&) {
            PyErr_Clear();  // a read-only docstring: leave it
        }
    }
}

template <typename T>
void MakeDataclass(py::class_<T>& cls, const std::vector<std::string>& fields) {
    // dict / kwargs construction starts from the class's *Python-side* default constructor (for
    // RANSACOptions that is pycolmap's defaults, not the C++ struct's), then merges
    // (/root/reference/pycolmap/helpers.h:258-268)
    const py::object cls_obj = cls;
    cls.def(py::init([fields, cls_obj](const py::dict& d) {
        py::object self = cls_obj();
        MergeDict(self, d, fields);
        return self.cast<T>();
    }));
    cls.def(py::init([fields, cls_obj](const py::kwargs& kw) {
        py::object self = cls_obj();
        MergeDict(self, py::dict(kw), fields);
        return self.cast<T>();
    }));
    py::implicitly_convertible<py::dict, T>();
    py::implicitly_convertible<py::kwargs, T>();
    AddDefaultsToDocstrings(cls_obj, fields);
    cls.def("mergedict", [fields](py::object self, const py::dict& d) { MergeDict(self, d, fields); });
    cls.def("todict", [fields](py::object self, bool recursive) { return ToDict(self, fields, recursive); },
            "recursive"_a = true);
    cls.def("summary", [fields](py::object self, bool write_type) { return Summary(self, fields, write_type); },
            "write_type"_a = false);
    cls.def("__repr__", [fields](py::object self) { return Summary(self, fields, false); });
    cls.def("__copy__", [](const T& self) { return T(self); });
    cls.def("__deepcopy__", [](const T& self, const py::dict&) { return T(self); });
    cls.def(py::pickle([fields](py::object self) { return ToDict(self, fields, /*recursive=*/false); },
                       [fields, cls_obj](const py::dict& d) {
                           py::object self = cls_obj();
                           MergeDict(self, d, fields);
                           return self.cast<T>();
                       }));
}

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

// ---- pycolmap.logging (/root/reference/pycolmap/main.cc:39-89): the glog front end the reference exposes -
// flags, per-severity destinations, info / warning / error / fatal stamped with the Python call site.  There is no
// glog here; the few lines it amounts to for this surface are written out: glog's line format, severity filtering
// by minloglevel / stderrthreshold, optional files.  fatal raises (glog aborts the process).
struct Logging {
    enum Level { INFO = 0, WARNING = 1, ERROR = 2, FATAL = 3 };
    static int minloglevel, stderrthreshold;
    static std::string log_dir;
    static bool logtostderr, alsologtostderr;
    static std::string destination[4];
    static std::mutex mu;
    static void Write(Level lv, const std::string& where, int line, const std::string& msg) {
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
};
int Logging::minloglevel = 0;
int Logging::stderrthreshold = 2;
std::string Logging::log_dir;
bool Logging::logtostderr = false;
bool Logging::alsologtostderr = true;   // the reference sets FLAGS_alsologtostderr = true at import
std::string Logging::destination[4];
std::mutex Logging::mu;

static std::pair<std::string, int> PythonCallFrame() {
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

    // ---- Camera (estimators.h), Image ---------------------------------------------------------
    BindCamera(m);
    // Image: the database-facing part of /root/reference/pycolmap/scene/image.h:74-130 (identifiers, name, pose and pose
    // prior, the keypoints it was constructed with); the reconstruction bookkeeping (points3D, observations) belongs
    // to COLMAP's mapper and is not part of this library
    struct PyPoint2D {
        std::array<double, 2> xy{{0.0, 0.0}};
        uint64_t point3D_id = kInvalidPoint3DId;
    };
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
    auto image_from_row = [](const ImageRow& r) {
        PyImage im;
        im.image_id = r.image_id;
        im.camera_id = r.camera_id;
        im.name = r.name;
        im.cam_from_world_prior.rotation.xyzw = {{r.prior_q[1], r.prior_q[2], r.prior_q[3], r.prior_q[0]}};
        im.cam_from_world_prior.translation = r.prior_t;
        return im;
    };
    auto row_from_image = [](const PyImage& im) {
        ImageRow r;
        r.image_id = im.image_id;
        r.camera_id = im.camera_id;
        r.name = im.name;
        const auto& q = im.cam_from_world_prior.rotation.xyzw;
        r.prior_q = {{q[3], q[0], q[1], q[2]}};
        r.prior_t = im.cam_from_world_prior.translation;
        return r;
    };
    auto camera_from_row = [](const CameraRow& r) {
        PyCamera c;
        c.camera_id = r.camera_id;
        c.model = r.model_id;
        c.width = r.width;
        c.height = r.height;
        c.params = r.params;
        c.has_prior_focal_length = r.has_prior_focal_length;
        return c;
    };
    auto row_from_camera = [](const PyCamera& c) {
        c.CheckParams();
        CameraRow r;
        r.camera_id = c.camera_id;
        r.model_id = c.model;
        r.width = c.width;
        r.height = c.height;
        r.params = c.params;
        r.has_prior_focal_length = c.has_prior_focal_length;
        return r;
    };
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

    // ---- Reconstruction, bundle_adjustment (/root/reference/pycolmap/scene/reconstruction.h, pipeline/sfm.h:95-103,
    // 259-362): the minimal subset.  The three maps are Python dicts of Camera / Image / Point3D objects
    // in file order, so they have reference semantics; every operation converts them to model_io's structs
    // (reconstruction.h, ba_host.h do the work) and writes the outcome back into the same objects. ----------------------
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

    struct PyReconstruction {
        py::dict cameras, images, points3D;
    };
    // the dicts as a plain model; a key that is not its object's id is a ValueError
    auto to_model = [](const PyReconstruction& r) {
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
    };
    // a model read from files as fresh objects
    auto from_model = [](PyReconstruction& r, const SparseModel& m) {
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
    };
    // the outcome of an operation on to_model(r) back into r's own objects: camera parameters, poses, the points2D's
    // point ids, the points' positions and tracks; points the operation deleted leave the dict
    auto update_from_model = [](PyReconstruction& r, const SparseModel& m) {
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
    };
    auto checked_model = [to_model](const PyReconstruction& r) {
        SparseModel m = to_model(r);
        const std::string bad = CheckModel(m);
        if (!bad.empty()) throw py::value_error("Reconstruction: " + bad);
        return m;
    };
    // update_from_model plus the points' errors (the point filter and update_point3D_errors write them; bundle_adjustment
    // does not)
    auto update_with_errors = [update_from_model](PyReconstruction& r, const SparseModel& m) {
        update_from_model(r, m);
        for (const ModelPoint3D& mp : m.points3D) r.points3D[py::int_(mp.point3D_id)].cast<PyPoint3D&>().error = mp.error;
    };
    // One amc_filter_points3d call on the checked model: ids == nullptr filters every point.  Nothing
    // of r changes unless the call succeeds.  Without a device the call raises pycolmap_amd._capi.AmcError.
    auto filter_model = [checked_model, update_with_errors](PyReconstruction& r, const std::vector<uint64_t>* ids, const std::vector<uint32_t>* image_ids,
                                                            double max_reproj_error, double min_tri_angle, bool errors_only) -> size_t {
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
        amc_filter_result res{};
        int rc = AMC_OK;
        std::string err;
        {
            py::gil_scoped_release release;
            EstimatorCtx& E = TheEstimatorCtx();
            std::lock_guard<std::mutex> lock(E.mu);
            amc_ctx* ctx = nullptr;
            try {
                ctx = E.Get();
            } catch (const std::runtime_error& e) {
                rc = AMC_E_HIP;
                err = e.what();
            }
            if (ctx) {
                rc = amc_filter_points3d(ctx, &pb, &opts, &res);
                if (rc != AMC_OK) err = std::string("amc_filter_points3d: ") + amc_last_error();
            }
        }
        if (rc == AMC_E_INVALID) throw std::invalid_argument(err);
        if (rc != AMC_OK) {
            const py::object cls = py::module_::import("pycolmap_amd._capi").attr("AmcError");
            const py::object exc = cls(rc, err);
            PyErr_SetObject(cls.ptr(), exc.ptr());
            throw py::error_already_set();
        }
        // the result's scalars are copied and its arrays freed before anything else can throw
        const amc_filter_result stats = res;
        size_t count = 0;
        try {
            if (errors_only)
                ApplyPointErrors(flat, res.point_error, &model);
            else
                count = ApplyFilterResult(flat, res.point_verdict, res.obs_deleted, res.point_error, &model);
        } catch (...) {
            amc_filter_result_free(&res);
            throw;
        }
        amc_filter_result_free(&res);
        const uint64_t by_library = stats.num_filtered;
        const double device_ms = stats.device_ms;
        py::dict st;
        st["call"] = errors_only ? "update_point3D_errors" : "filter_points3D";
        st["num_points"] = stats.num_points;
        st["num_observations"] = stats.num_observations;
        st["num_filtered"] = stats.num_filtered;
        st["num_batches"] = stats.num_batches;
        st["device_ms"] = stats.device_ms;
        st["kernel_ms"] = stats.kernel_ms;
        st["copy_ms"] = stats.copy_ms;
        if (!errors_only && by_library != count) throw std::runtime_error("filter_points3D: the library counted " + std::to_string(by_library) + ", the write-back " + std::to_string(count));
        update_with_errors(r, model);
        st["host_ms"] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - device_ms;
        py::module_::import("pycolmap_amd._pycolmap").attr("_last_stats") = st;
        return count;
    };
    auto summary = [checked_model](const PyReconstruction& r) {
        const SparseModel m = checked_model(r);
        const size_t nobs = ComputeNumObservations(m);
        std::ostringstream ss;
        ss << "Reconstruction:\n\tnum_reg_images = " << m.images.size() << "\n\tnum_cameras = " << m.cameras.size()
           << "\n\tnum_points3D = " << m.points3D.size() << "\n\tnum_observations = " << nobs
           << "\n\tmean_track_length = " << ComputeMeanTrackLength(m) << "\n\tmean_observations_per_image = "
           << (m.images.empty() ? 0.0 : static_cast<double>(nobs) / static_cast<double>(m.images.size()));
        return ss.str();
    };
    auto read_into = [from_model](PyReconstruction& r, const std::string& path, int how) {
        const SparseModel m = how == 0 ? ReadSparseModel(path) : how == 1 ? ReadSparseModelBin(path) : ReadSparseModelTxt(path);
        const std::string bad = CheckModel(m);
        if (!bad.empty()) throw py::value_error(path + ": " + bad);
        from_model(r, m);
    };
    auto deep_copy = [](const PyReconstruction& r) {
        const py::object deepcopy = py::module_::import("copy").attr("deepcopy");
        PyReconstruction c;
        c.cameras = deepcopy(r.cameras);
        c.images = deepcopy(r.images);
        c.points3D = deepcopy(r.points3D);
        return c;
    };
    py::class_<PyReconstruction>(m, "Reconstruction")
        .def(py::init<>())
        .def(py::init([read_into](const std::string& path) {
                 PyReconstruction r;
                 read_into(r, path, 0);
                 return r;
             }),
             "path"_a)
        .def("read", [read_into](PyReconstruction& r, const std::string& path) { read_into(r, path, 0); }, "path"_a,
             "Read the model from `path`: the three .bin files when all exist, else the three .txt files.")
        .def("read_binary", [read_into](PyReconstruction& r, const std::string& path) { read_into(r, path, 1); }, "path"_a)
        .def("read_text", [read_into](PyReconstruction& r, const std::string& path) { read_into(r, path, 2); }, "path"_a)
        .def("write", [checked_model](const PyReconstruction& r, const std::string& path) { WriteSparseModelBin(path, checked_model(r)); },
             "path"_a, "Write cameras.bin, images.bin and points3D.bin into the existing directory `path`, in the maps' order.")
        .def("write_binary", [checked_model](const PyReconstruction& r, const std::string& path) { WriteSparseModelBin(path, checked_model(r)); },
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
        .def("compute_num_observations", [checked_model](const PyReconstruction& r) { return ComputeNumObservations(checked_model(r)); })
        .def("compute_mean_track_length", [checked_model](const PyReconstruction& r) { return ComputeMeanTrackLength(checked_model(r)); })
        .def("filter_observations_with_negative_depth", [checked_model, update_from_model](PyReconstruction& r) {
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
        .def("delete_point3D", [checked_model, update_with_errors](PyReconstruction& r, uint64_t point3D_id) {
                 SparseModel m = checked_model(r);
                 DeletePoint3D(&m, point3D_id);
                 update_with_errors(r, m);
             }, "point3D_id"_a, "Delete a 3D point, and all its references in the observed images.")
        .def("delete_observation", [checked_model, update_with_errors](PyReconstruction& r, uint32_t image_id, uint32_t point2D_idx) {
                 SparseModel m = checked_model(r);
                 DeleteObservation(&m, image_id, point2D_idx);
                 update_with_errors(r, m);
             }, "image_id"_a, "point2D_idx"_a,
             "Delete one observation from an image and the corresponding 3D point.\n"
             "Note that this deletes the entire 3D point, if the track has two elements\n"
             "prior to calling this method.")
        .def("filter_points3D", [filter_model](PyReconstruction& r, double max_reproj_error, double min_tri_angle, const std::unordered_set<uint64_t>& point3D_ids) {
                 const std::vector<uint64_t> ids(point3D_ids.begin(), point3D_ids.end());
                 return filter_model(r, &ids, nullptr, max_reproj_error, min_tri_angle, false);
             }, "max_reproj_error"_a, "min_tri_angle"_a, "point3D_ids"_a,
             "Filter 3D points with large reprojection error, negative depth, or\n"
             "insufficient triangulation angle.\n\n"
             "@param max_reproj_error    The maximum reprojection error.\n"
             "@param min_tri_angle       The minimum triangulation angle.\n"
             "@param point3D_ids         The points to be filtered.\n\n"
             "@return                    The number of filtered observations.")
        .def("filter_points3D_in_images", [filter_model](PyReconstruction& r, double max_reproj_error, double min_tri_angle, const std::unordered_set<uint32_t>& image_ids) {
                 const std::vector<uint32_t> ids(image_ids.begin(), image_ids.end());
                 return filter_model(r, nullptr, &ids, max_reproj_error, min_tri_angle, false);
             }, "max_reproj_error"_a, "min_tri_angle"_a, "image_ids"_a,
             "Filter 3D points with large reprojection error, negative depth, or\n"
             "insufficient triangulation angle.\n\n"
             "@param max_reproj_error    The maximum reprojection error.\n"
             "@param min_tri_angle       The minimum triangulation angle.\n"
             "@param image_ids           The the image ids in which the points3D are filtered.\n\n"
             "@return                    The number of filtered observations.")
        .def("filter_all_points3D", [filter_model](PyReconstruction& r, double max_reproj_error, double min_tri_angle) {
                 return filter_model(r, nullptr, nullptr, max_reproj_error, min_tri_angle, false);
             }, "max_reproj_error"_a, "min_tri_angle"_a,
             "Filter 3D points with large reprojection error, negative depth, or\n"
             "insufficient triangulation angle.\n\n"
             "@param max_reproj_error    The maximum reprojection error.\n"
             "@param min_tri_angle       The minimum triangulation angle.\n\n"
             "@return                    The number of filtered observations.")
        .def("update_point3D_errors", [filter_model](PyReconstruction& r) { filter_model(r, nullptr, nullptr, 0.0, 0.0, true); },
             "Set every 3D point's error to the mean reprojection error over its track, on the GPU (DESIGN.md section 16).")
        .def("update_point_3d_errors", [filter_model](PyReconstruction& r) { filter_model(r, nullptr, nullptr, 0.0, 0.0, true); },
             "Later pycolmap's spelling of update_point3D_errors.")
        .def("compute_mean_observations_per_reg_image", [checked_model](const PyReconstruction& r) { return ComputeMeanObservationsPerRegImage(checked_model(r)); })
        .def("compute_mean_reprojection_error", [checked_model](const PyReconstruction& r) { return ComputeMeanReprojectionError(checked_model(r)); })
        .def("summary", summary)
        .def("__repr__", [checked_model](const PyReconstruction& r) {
            const SparseModel m = checked_model(r);
            return "Reconstruction(num_reg_images=" + std::to_string(m.images.size()) + ", num_cameras=" + std::to_string(m.cameras.size()) +
                   ", num_points3D=" + std::to_string(m.points3D.size()) + ", num_observations=" + std::to_string(ComputeNumObservations(m)) + ")";
        })
        .def("__copy__", deep_copy)
        .def("__deepcopy__", [deep_copy](const PyReconstruction& r, const py::dict&) { return deep_copy(r); });

    enum class LossFunctionType { TRIVIAL = 0, SOFT_L1 = 1, CAUCHY = 2 };
    py::enum_<LossFunctionType> PyLoss(m, "LossFunctionType");
    PyLoss.value("TRIVIAL", LossFunctionType::TRIVIAL).value("SOFT_L1", LossFunctionType::SOFT_L1).value("CAUCHY", LossFunctionType::CAUCHY);
    PyLoss.def(py::init([](const std::string& s) {
        if (s == "TRIVIAL") return LossFunctionType::TRIVIAL;
        if (s == "SOFT_L1") return LossFunctionType::SOFT_L1;
        if (s == "CAUCHY") return LossFunctionType::CAUCHY;
        throw py::value_error("Invalid string value " + s + " for enum LossFunctionType");
    }));
    py::implicitly_convertible<std::string, LossFunctionType>();
    struct CeresSolverOptions {
        double function_tolerance = 0.0, gradient_tolerance = 0.0, parameter_tolerance = 0.0;  // COLMAP's BundleAdjustmentOptions
        int max_num_iterations = 100, max_linear_solver_iterations = 200, max_num_consecutive_invalid_steps = 10,
            max_consecutive_nonmonotonic_steps = 10;
        bool minimizer_progress_to_stdout = false;
        int num_threads = -1;
    };
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
    struct BundleAdjustmentOptions {
        LossFunctionType loss_function_type = LossFunctionType::TRIVIAL;
        double loss_function_scale = 1.0;
        bool refine_focal_length = true, refine_principal_point = false, refine_extra_params = true, refine_extrinsics = true,
             print_summary = true;
        int min_num_residuals_for_multi_threading = 50000;
        CeresSolverOptions solver_options;
    };
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
    // the flat problem bundle_adjustment hands to amc_bundle_adjust, after the controller's filter (a test hook: the GPU
    // tests run Context.bundle_adjust on it)
    auto flat_problem = [checked_model](const PyReconstruction& r, const BundleAdjustmentOptions& o) {
        SparseModel model = checked_model(r);
        FilterObservationsWithNegativeDepth(&model);
        size_t skipped = 0;
        const BaRefineFlags flags{o.refine_focal_length, o.refine_principal_point, o.refine_extra_params, o.refine_extrinsics};
        const FlatBa f = FlattenForBundleAdjustment(model, flags, &skipped);
        auto arr = [](const auto& v, py::ssize_t cols) {
            using T = typename std::decay<decltype(v)>::type::value_type;
            py::array_t<T> a({static_cast<py::ssize_t>(v.size()) / cols, cols});
            std::copy(v.begin(), v.end(), a.mutable_data());
            return a;
        };
        py::dict d;
        d["camera_models"] = arr(f.camera_models, 1);
        d["camera_params"] = arr(f.camera_params, 12);
        d["camera_const"] = arr(f.camera_const, 12);
        d["image_cameras"] = arr(f.image_cameras, 1);
        d["qvec"] = arr(f.qvec, 4);
        d["tvec"] = arr(f.tvec, 3);
        d["pose_const"] = arr(f.pose_const, 6);
        d["xyz"] = arr(f.xyz, 3);
        d["obs_image"] = arr(f.obs_image, 1);
        d["obs_point"] = arr(f.obs_point, 1);
        d["obs_xy"] = arr(f.obs_xy, 2);
        return d;
    };
    m.def("_bundle_adjustment_problem", flat_problem, "reconstruction"_a, "options"_a = BundleAdjustmentOptions(),
          "The flat problem bundle_adjustment solves (test hook).");
    m.def(
        "bundle_adjustment",
        [checked_model, update_from_model](PyReconstruction& r, const BundleAdjustmentOptions& o) {
            const auto t0 = std::chrono::steady_clock::now();
            if (r.images.size() < 2) {
                const auto f = PythonCallFrame();
                Logging::Write(Logging::ERROR, f.first, f.second, "Need at least two views.");
                return;
            }
            SparseModel model = checked_model(r);
            const size_t filtered = FilterObservationsWithNegativeDepth(&model);
            size_t skipped = 0;
            const BaRefineFlags flags{o.refine_focal_length, o.refine_principal_point, o.refine_extra_params, o.refine_extrinsics};
            FlatBa flat = FlattenForBundleAdjustment(model, flags, &skipped);
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
            amc_ba_problem pb = flat.Problem();
            amc_ba_result res{};
            {
                py::gil_scoped_release release;
                EstimatorCtx& E = TheEstimatorCtx();
                std::lock_guard<std::mutex> lock(E.mu);
                EstCheck(amc_bundle_adjust(E.Get(), &pb, &opts, &res), "amc_bundle_adjust");
            }
            WriteBackBundleAdjustment(flat, &model);
            update_from_model(r, model);
            static const char* const kTermination[] = {"FUNCTION_TOLERANCE", "PARAMETER_TOLERANCE", "GRADIENT_TOLERANCE", "MAX_ITERATIONS",
                                                       "MIN_RADIUS", "INVALID_STEPS", "NOTHING_TO_REFINE"};
            py::dict st;
            st["call"] = "bundle_adjustment";
            st["num_images"] = res.num_images;
            st["num_points"] = res.num_points;
            st["num_observations"] = res.num_observations;
            st["num_variable_parameters"] = res.num_variable_parameters;
            st["num_filtered_observations"] = filtered;
            st["num_skipped_points"] = skipped;
            st["initial_cost"] = res.initial_cost;
            st["final_cost"] = res.final_cost;
            st["num_successful_steps"] = res.num_successful_steps;
            st["num_unsuccessful_steps"] = res.num_unsuccessful_steps;
            st["num_pcg_iterations"] = res.num_pcg_iterations;
            st["termination"] = kTermination[res.termination >= 0 && res.termination < 7 ? res.termination : 5];
            st["device_ms"] = res.device_ms;
            st["kernel_ms"] = res.kernel_ms;
            st["host_ms"] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - res.device_ms;
            py::module_::import("pycolmap_amd._pycolmap").attr("_last_stats") = st;
        },
        "reconstruction"_a, "options"_a = BundleAdjustmentOptions(),
        "Jointly refine every pose, point and camera of the reconstruction on the GPU, in place (DESIGN.md section 15).");

    // ---- BundleAdjustmentConfig and BundleAdjuster (COLMAP 3.9.1's classes under the names later pycolmap releases
    // bind; ba_config_host.h does the work): the adjustment of a part of the model. ----
    py::class_<BundleAdjustmentConfig>(m, "BundleAdjustmentConfig")
        .def(py::init<>())
        .def("num_images", &BundleAdjustmentConfig::NumImages)
        .def("num_points", &BundleAdjustmentConfig::NumPoints)
        .def("num_constant_cam_intrinsics", &BundleAdjustmentConfig::NumConstantCamIntrinsics)
        .def("num_constant_cam_poses", &BundleAdjustmentConfig::NumConstantCamPoses)
        .def("num_constant_cam_positions", &BundleAdjustmentConfig::NumConstantCamPositions)
        .def("num_variable_points", &BundleAdjustmentConfig::NumVariablePoints)
        .def("num_constant_points", &BundleAdjustmentConfig::NumConstantPoints)
        .def("num_residuals", [checked_model](const BundleAdjustmentConfig& c, const PyReconstruction& r) { return c.NumResiduals(checked_model(r)); },
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
    struct PyBundleAdjuster {
        BundleAdjustmentOptions options;
        BundleAdjustmentConfig config;
        py::dict summary;
    };
    auto adjuster_flat = [checked_model](const PyBundleAdjuster& a, const PyReconstruction& r, SparseModel* model) {
        *model = checked_model(r);
        const BundleAdjustmentOptions& o = a.options;
        const BaRefineFlags flags{o.refine_focal_length, o.refine_principal_point, o.refine_extra_params, o.refine_extrinsics};
        return FlattenForBundleAdjuster(*model, a.config, flags);
    };
    auto adjuster_dict = [](const FlatBaConfig& fc) {
        auto arr = [](const auto& v, py::ssize_t cols) {
            using T = typename std::decay<decltype(v)>::type::value_type;
            py::array_t<T> a({static_cast<py::ssize_t>(v.size()) / cols, cols});
            std::copy(v.begin(), v.end(), a.mutable_data());
            return a;
        };
        const FlatBa& f = fc.flat;
        py::dict d;
        d["camera_models"] = arr(f.camera_models, 1);
        d["camera_params"] = arr(f.camera_params, 12);
        d["camera_const"] = arr(f.camera_const, 12);
        d["image_cameras"] = arr(f.image_cameras, 1);
        d["qvec"] = arr(f.qvec, 4);
        d["tvec"] = arr(f.tvec, 3);
        d["pose_const"] = arr(f.pose_const, 6);
        d["xyz"] = arr(f.xyz, 3);
        d["obs_image"] = arr(f.obs_image, 1);
        d["obs_point"] = arr(f.obs_point, 1);
        d["obs_xy"] = arr(f.obs_xy, 2);
        d["point_const"] = arr(fc.point_const, 1);
        d["camera_at"] = arr(fc.camera_at, 1);
        d["image_at"] = arr(fc.image_at, 1);
        d["point_at"] = arr(fc.point_at, 1);
        d["num_skipped_points"] = fc.skipped_points;
        return d;
    };
    // Solve: one amc_bundle_adjust_masked call on the config's part of the checked model.  Nothing of r
    // changes unless the call succeeds.  Without a device the call raises pycolmap_amd._capi.AmcError.
    // solver: None, or a callable that stands in for the library (a test hook: the CPU tests pass the reference): it takes
    // the flat problem as a dict of arrays with the options and returns camera_params, qvec, tvec, xyz and the statistics.
    auto adjuster_solve = [adjuster_flat, adjuster_dict, update_from_model](PyBundleAdjuster& a, PyReconstruction& r, const py::object& solver) -> bool {
        const auto t0 = std::chrono::steady_clock::now();
        SparseModel model;
        FlatBaConfig fc = adjuster_flat(a, r, &model);
        FlatBa& flat = fc.flat;
        if (flat.obs_image.empty()) return false;  // COLMAP: "No residuals" — nothing to solve
        const BundleAdjustmentOptions& o = a.options;
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
        static const char* const kTermination[] = {"FUNCTION_TOLERANCE", "PARAMETER_TOLERANCE", "GRADIENT_TOLERANCE", "MAX_ITERATIONS",
                                                   "MIN_RADIUS", "INVALID_STEPS", "NOTHING_TO_REFINE"};
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
            int rc = AMC_OK;
            std::string err;
            {
                py::gil_scoped_release release;
                EstimatorCtx& E = TheEstimatorCtx();
                std::lock_guard<std::mutex> lock(E.mu);
                amc_ctx* ctx = nullptr;
                try {
                    ctx = E.Get();
                } catch (const std::runtime_error& e) {
                    rc = AMC_E_HIP;
                    err = e.what();
                }
                if (ctx) {
                    rc = amc_bundle_adjust_masked(ctx, &pb, fc.point_const.data(), &opts, &res);
                    if (rc != AMC_OK) err = std::string("amc_bundle_adjust_masked: ") + amc_last_error();
                }
            }
            if (rc == AMC_E_INVALID) throw std::invalid_argument(err);
            if (rc != AMC_OK) {
                const py::object cls = py::module_::import("pycolmap_amd._capi").attr("AmcError");
                const py::object exc = cls(rc, err);
                PyErr_SetObject(cls.ptr(), exc.ptr());
                throw py::error_already_set();
            }
            st["num_variable_parameters"] = res.num_variable_parameters;
            st["initial_cost"] = res.initial_cost;
            st["final_cost"] = res.final_cost;
            st["num_successful_steps"] = res.num_successful_steps;
            st["num_unsuccessful_steps"] = res.num_unsuccessful_steps;
            st["num_pcg_iterations"] = res.num_pcg_iterations;
            st["termination"] = kTermination[res.termination >= 0 && res.termination < 7 ? res.termination : 5];
            st["device_ms"] = res.device_ms;
            st["kernel_ms"] = res.kernel_ms;
        }
        WriteBackBundleAdjuster(fc, &model);
        update_from_model(r, model);
        st["host_ms"] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - st["device_ms"].cast<double>();
        a.summary = st;
        py::module_::import("pycolmap_amd._pycolmap").attr("_last_stats") = st;
        return true;
    };
    py::class_<PyBundleAdjuster>(m, "BundleAdjuster")
        .def(py::init([](const BundleAdjustmentOptions& options, const BundleAdjustmentConfig& config) {
                 return PyBundleAdjuster{options, config, py::dict()};
             }), "options"_a, "config"_a)
        .def("solve", [adjuster_solve](PyBundleAdjuster& a, PyReconstruction& r) { return adjuster_solve(a, r, py::none()); }, "reconstruction"_a,
             "Refine the config's part of the reconstruction on the GPU, in place (DESIGN.md 15.12).  False when the\n"
             "config gives no residual.")
        .def("_solve_with", adjuster_solve, "reconstruction"_a, "solver"_a, "solve with a callable in the library's place (test hook).")
        .def("_problem", [adjuster_flat, adjuster_dict](const PyBundleAdjuster& a, const PyReconstruction& r) {
                 SparseModel model;
                 return adjuster_dict(adjuster_flat(a, r, &model));
             }, "reconstruction"_a, "The flat problem solve hands to amc_bundle_adjust_masked (test hook).")
        .def_property_readonly("options", [](const PyBundleAdjuster& a) { return a.options; })
        .def_property_readonly("config", [](const PyBundleAdjuster& a) { return a.config; })
        .def_property_readonly("summary", [](const PyBundleAdjuster& a) { return a.summary; });

    // ---- CorrespondenceGraph and IncrementalTriangulator (the reference's pycolmap/scene/correspondence_graph.h and
    // pycolmap/sfm/incremental_triangulator.h; correspondence_graph.h, triangulator_host.h) ----
    py::class_<Correspondence>(m, "Correspondence")
        .def(py::init<>())
        .def(py::init<uint32_t, uint32_t>(), "image_id"_a, "point2D_idx"_a)
        .def_readwrite("image_id", &Correspondence::image_id)
        .def_readwrite("point2D_idx", &Correspondence::point2D_idx)
        .def("__copy__", [](const Correspondence& c) { return Correspondence(c); })
        .def("__deepcopy__", [](const Correspondence& c, const py::dict&) { return Correspondence(c); })
        .def("__repr__", [](const Correspondence& c) {
            return "Correspondence(image_id=" + std::to_string(c.image_id) + ", point2D_idx=" + std::to_string(c.point2D_idx) + ")";
        });
    py::class_<CorrespondenceGraph, std::shared_ptr<CorrespondenceGraph>>(m, "CorrespondenceGraph")
        .def(py::init<>())
        .def("num_images", &CorrespondenceGraph::NumImages)
        .def("num_image_pairs", &CorrespondenceGraph::NumImagePairs)
        .def("exists_image", &CorrespondenceGraph::ExistsImage, "image_id"_a)
        .def("num_observations_for_image", &CorrespondenceGraph::NumObservationsForImage, "image_id"_a)
        .def("num_correspondences_for_image", &CorrespondenceGraph::NumCorrespondencesForImage, "image_id"_a)
        .def("num_correspondences_between_images", &CorrespondenceGraph::NumCorrespondencesBetweenImages, "image_id1"_a, "image_id2"_a)
        .def("finalize", &CorrespondenceGraph::Finalize)
        .def("add_image", &CorrespondenceGraph::AddImage, "image_id"_a, "num_points2D"_a)
        .def("add_correspondences", [](CorrespondenceGraph& g, uint32_t image_id1, uint32_t image_id2, const py::object& matches) {
                 const auto arr = py::array_t<uint32_t, py::array::c_style | py::array::forcecast>::ensure(matches);
                 if (!arr) throw py::value_error("add_correspondences: matches must be convertible to an N x 2 uint32 array");
                 if (!(arr.ndim() == 2 && arr.shape(1) == 2) && arr.size() != 0)
                     throw py::value_error("add_correspondences: expected an N x 2 array of point2D indices");
                 const auto frame = PythonCallFrame();
                 for (const std::string& w : g.AddCorrespondences(image_id1, image_id2, arr.data(), static_cast<size_t>(arr.size() / 2)))
                     Logging::Write(Logging::WARNING, frame.first, frame.second, w);
             }, "image_id1"_a, "image_id2"_a, "correspondences"_a)
        .def("extract_correspondences", [](const CorrespondenceGraph& g, uint32_t image_id, uint32_t point2D_idx) {
                 return g.ExtractCorrespondences(image_id, point2D_idx);
             }, "image_id"_a, "point2D_idx"_a)
        .def("extract_transitive_correspondences", [](const CorrespondenceGraph& g, uint32_t image_id, uint32_t point2D_idx, size_t transitivity) {
                 std::vector<Correspondence> found;
                 g.ExtractTransitiveCorrespondences(image_id, point2D_idx, transitivity, &found);
                 return found;
             }, "image_id"_a, "point2D_idx"_a, "transitivity"_a)
        .def("find_correspondences_between_images", [](const CorrespondenceGraph& g, uint32_t image_id1, uint32_t image_id2) {
                 const std::vector<uint32_t> v = g.FindCorrespondencesBetweenImages(image_id1, image_id2);
                 py::array_t<uint32_t> a({static_cast<py::ssize_t>(v.size() / 2), static_cast<py::ssize_t>(2)});
                 std::copy(v.begin(), v.end(), a.mutable_data());
                 return a;
             }, "image_id1"_a, "image_id2"_a)
        .def("has_correspondences", &CorrespondenceGraph::HasCorrespondences, "image_id"_a, "point2D_idx"_a)
        .def("is_two_view_observation", &CorrespondenceGraph::IsTwoViewObservation, "image_id"_a, "point2D_idx"_a)
        .def("__copy__", [](const CorrespondenceGraph& g) { return std::make_shared<CorrespondenceGraph>(g); })
        .def("__deepcopy__", [](const CorrespondenceGraph& g, const py::dict&) { return std::make_shared<CorrespondenceGraph>(g); })
        .def("__repr__", [](const CorrespondenceGraph& g) {
            return "CorrespondenceGraph(num_images=" + std::to_string(g.NumImages()) + ", num_image_pairs=" + std::to_string(g.NumImagePairs()) + ")";
        });

    py::class_<TriangulatorOptions> PyTrgOpts(m, "IncrementalTriangulatorOptions");
    PyTrgOpts.def(py::init<>())
        .def_readwrite("max_transitivity", &TriangulatorOptions::max_transitivity, "Maximum transitivity to search for correspondences.")
        .def_readwrite("create_max_angle_error", &TriangulatorOptions::create_max_angle_error, "Maximum angular error to create new triangulations.")
        .def_readwrite("continue_max_angle_error", &TriangulatorOptions::continue_max_angle_error, "Maximum angular error to continue existing triangulations.")
        .def_readwrite("merge_max_reproj_error", &TriangulatorOptions::merge_max_reproj_error, "Maximum reprojection error in pixels to merge triangulations.")
        .def_readwrite("complete_max_reproj_error", &TriangulatorOptions::complete_max_reproj_error, "Maximum reprojection error to complete an existing triangulation.")
        .def_readwrite("complete_max_transitivity", &TriangulatorOptions::complete_max_transitivity, "Maximum transitivity for track completion.")
        .def_readwrite("re_max_angle_error", &TriangulatorOptions::re_max_angle_error, "Maximum angular error to re-triangulate under-reconstructed image pairs.")
        .def_readwrite("re_min_ratio", &TriangulatorOptions::re_min_ratio, "Minimum ratio of common triangulations between an image pair over the number of correspondences between that image pair to be considered as under-reconstructed.")
        .def_readwrite("re_max_trials", &TriangulatorOptions::re_max_trials, "Maximum number of trials to re-triangulate an image pair.")
        .def_readwrite("min_angle", &TriangulatorOptions::min_angle, "Minimum pairwise triangulation angle for a stable triangulation.")
        .def_readwrite("ignore_two_view_tracks", &TriangulatorOptions::ignore_two_view_tracks, "Whether to ignore two-view tracks.")
        .def_readwrite("min_focal_length_ratio", &TriangulatorOptions::min_focal_length_ratio, "Thresholds for bogus camera parameters: images with bogus camera parameters are ignored in triangulation.")
        .def_readwrite("max_focal_length_ratio", &TriangulatorOptions::max_focal_length_ratio)
        .def_readwrite("max_extra_param", &TriangulatorOptions::max_extra_param);
    MakeDataclass(PyTrgOpts, {"max_transitivity", "create_max_angle_error", "continue_max_angle_error", "merge_max_reproj_error",
                              "complete_max_reproj_error", "complete_max_transitivity", "re_max_angle_error", "re_min_ratio",
                              "re_max_trials", "min_angle", "ignore_two_view_tracks", "min_focal_length_ratio",
                              "max_focal_length_ratio", "max_extra_param"});

    // keeps the caller's graph and reconstruction alive and works on that reconstruction in place
    struct PyTriangulator {
        py::object graph, reconstruction;
        std::set<uint64_t> modified;
        RetriTrials re_trials;  // retriangulate's per-pair trial counters
    };
    // the outcome of triangulate_image back into r: the created points as new objects first, then update_with_errors
    auto update_with_new_points = [update_with_errors](PyReconstruction& r, const SparseModel& m) {
        for (const ModelPoint3D& mp : m.points3D) {
            if (r.points3D.contains(py::int_(mp.point3D_id))) continue;
            PyPoint3D p;
            p.color = {{mp.rgb[0], mp.rgb[1], mp.rgb[2]}};
            r.points3D[py::int_(mp.point3D_id)] = py::cast(p);
        }
        update_with_errors(r, m);
    };
    // TriangulateImage: one amc_triangulate_observations call per run of points2D.  Nothing of
    // the reconstruction or of the modified set changes unless every call succeeds.  Without a device the call raises
    // pycolmap_amd._capi.AmcError.
    // solver: None, or a callable that stands in for the library (a test hook: the CPU tests pass the reference): it
    // takes the flat problem as a dict of arrays and returns continued, cand_round, round_offsets and round_xyz.
    auto triangulate_image_with = [checked_model, update_with_new_points](PyTriangulator& t, const TriangulatorOptions& o, uint32_t image_id,
                                                                          const py::object& solver) -> size_t {
        const auto t0 = std::chrono::steady_clock::now();
        const std::string bad = o.Check();
        if (!bad.empty()) throw py::value_error(CheckMessage(__FILE__, __LINE__, bad));
        PyReconstruction& r = t.reconstruction.cast<PyReconstruction&>();
        const CorrespondenceGraph& graph = t.graph.cast<const CorrespondenceGraph&>();
        SparseModel model = checked_model(r);
        ModelIndex ix(model, o);
        const auto self = ix.image.find(image_id);
        if (self == ix.image.end()) throw py::value_error(CheckMessage(__FILE__, __LINE__, "reconstruction.exists_image(image_id)", "image_id=" + std::to_string(image_id)));
        (void)graph.NumPoints2D(image_id);  // an image the graph does not hold: the graph's ValueError
        std::set<uint64_t> modified = t.modified;
        TriobsApplied total;
        uint64_t items = 0, observations = 0, calls = 0;
        double device_ms = 0, kernel_ms = 0, copy_ms = 0;
        if (!ix.image_bogus[self->second]) {
            FlatTriobs flat = FlattenModelForTriobs(model, ix);
            amc_triobs_opts opts;
            amc_triobs_opts_default(&opts);
            opts.create_max_angle_error = o.create_max_angle_error;
            opts.continue_max_angle_error = o.continue_max_angle_error;
            opts.min_angle = o.min_angle;
            const size_t npoints2D = model.images[self->second].points2D.size();
            for (size_t begin = 0; begin < npoints2D;) {
                begin = PlanTriangulationRun(graph, model, ix, o, image_id, begin, &flat);
                if (flat.NumItems() == 0) continue;
                if (!solver.is_none()) {
                    auto arr = [](const auto& v, py::ssize_t cols) {
                        using T = typename std::decay<decltype(v)>::type::value_type;
                        py::array_t<T> a({static_cast<py::ssize_t>(v.size()) / cols, cols});
                        std::copy(v.begin(), v.end(), a.mutable_data());
                        return a;
                    };
                    py::dict d;
                    d["camera_models"] = arr(flat.camera_models, 1);
                    d["camera_params"] = arr(flat.camera_params, 12);
                    d["image_cameras"] = arr(flat.image_cameras, 1);
                    d["qvec"] = arr(flat.qvec, 4);
                    d["tvec"] = arr(flat.tvec, 3);
                    d["item_offsets"] = arr(flat.item_offsets, 1);
                    d["cand_image"] = arr(flat.cand_image, 1);
                    d["cand_xy"] = arr(flat.cand_xy, 2);
                    d["cand_has_point"] = arr(flat.cand_has_point, 1);
                    d["cand_xyz"] = arr(flat.cand_xyz, 3);
                    d["no_create_two_view"] = arr(flat.no_create_two_view, 1);
                    d["create_max_angle_error"] = o.create_max_angle_error;
                    d["continue_max_angle_error"] = o.continue_max_angle_error;
                    d["min_angle"] = o.min_angle;
                    const py::dict out = solver(d);
                    const auto cont = py::array_t<int32_t, py::array::c_style | py::array::forcecast>::ensure(out["continued"]);
                    const auto rnd = py::array_t<uint32_t, py::array::c_style | py::array::forcecast>::ensure(out["cand_round"]);
                    const auto roff = py::array_t<uint64_t, py::array::c_style | py::array::forcecast>::ensure(out["round_offsets"]);
                    const auto rxyz = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(out["round_xyz"]);
                    if (!cont || !rnd || !roff || !rxyz || static_cast<size_t>(cont.size()) != flat.NumItems() ||
                        static_cast<size_t>(rnd.size()) != flat.cand_image.size() || static_cast<size_t>(roff.size()) != flat.NumItems() + 1 ||
                        static_cast<uint64_t>(rxyz.size()) != 3 * roff.data()[flat.NumItems()])
                        throw py::value_error("triangulate_image: the solver's result does not have the problem's shape");
                    items += flat.NumItems();
                    observations += flat.cand_image.size();
                    calls += 1;
                    const TriobsApplied a = ApplyTriobsResult(flat, cont.data(), rnd.data(), roff.data(), rxyz.data(), &model, &ix, &modified);
                    total.num_tris += a.num_tris;
                    total.num_created += a.num_created;
                    total.num_continued += a.num_continued;
                    continue;
                }
                const amc_triobs_problem pb = flat.Problem();
                amc_triobs_result res{};
                int rc = AMC_OK;
                std::string err;
                {
                    py::gil_scoped_release release;
                    EstimatorCtx& E = TheEstimatorCtx();
                    std::lock_guard<std::mutex> lock(E.mu);
                    amc_ctx* ctx = nullptr;
                    try {
                        ctx = E.Get();
                    } catch (const std::runtime_error& e) {
                        rc = AMC_E_HIP;
                        err = e.what();
                    }
                    if (ctx) {
                        rc = amc_triangulate_observations(ctx, &pb, &opts, &res);
                        if (rc != AMC_OK) err = std::string("amc_triangulate_observations: ") + amc_last_error();
                    }
                }
                if (rc == AMC_E_INVALID) throw std::invalid_argument(err);
                if (rc != AMC_OK) {
                    const py::object cls = py::module_::import("pycolmap_amd._capi").attr("AmcError");
                    const py::object exc = cls(rc, err);
                    PyErr_SetObject(cls.ptr(), exc.ptr());
                    throw py::error_already_set();
                }
                items += res.num_items;
                observations += res.num_candidates;
                calls += 1;
                device_ms += res.device_ms;
                kernel_ms += res.kernel_ms;
                copy_ms += res.copy_ms;
                try {
                    const TriobsApplied a = ApplyTriobsResult(flat, res.continued, res.cand_round, res.round_offsets, res.round_xyz, &model, &ix, &modified);
                    total.num_tris += a.num_tris;
                    total.num_created += a.num_created;
                    total.num_continued += a.num_continued;
                } catch (...) {
                    amc_triobs_result_free(&res);
                    throw;
                }
                amc_triobs_result_free(&res);
            }
        }
        update_with_new_points(r, model);
        t.modified.swap(modified);
        py::dict st;
        st["call"] = "triangulate_image";
        st["num_items"] = items;
        st["num_observations"] = observations;
        st["num_created_points"] = total.num_created;
        st["num_continued_observations"] = total.num_continued;
        st["num_device_calls"] = calls;
        st["device_ms"] = device_ms;
        st["kernel_ms"] = kernel_ms;
        st["copy_ms"] = copy_ms;
        st["host_ms"] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - device_ms;
        py::module_::import("pycolmap_amd._pycolmap").attr("_last_stats") = st;
        return total.num_tris;
    };
    py::class_<PyTriangulator>(m, "IncrementalTriangulator")
        .def(py::init([](const py::object& graph, const py::object& reconstruction) {
                 if (!py::isinstance<CorrespondenceGraph>(graph) || !py::isinstance<PyReconstruction>(reconstruction))
                     throw py::type_error("IncrementalTriangulator(correspondence_graph: CorrespondenceGraph, reconstruction: Reconstruction)");
                 return PyTriangulator{graph, reconstruction, {}, {}};
             }), "correspondence_graph"_a, "reconstruction"_a)
        .def("_triangulate_image_with", triangulate_image_with, "options"_a, "image_id"_a, "solver"_a,
             "triangulate_image with a callable in the library's place (test hook).")
        .def("triangulate_image", [triangulate_image_with](PyTriangulator& t, const TriangulatorOptions& o, uint32_t image_id) {
                 return triangulate_image_with(t, o, image_id, py::none());
             }, "options"_a, "image_id"_a,
             "Triangulate observations of image: continue the tracks its correspondences carry and create new ones, on the\n"
             "GPU (DESIGN.md section 17).  Returns the number of triangulated observations.")
        .def("add_modified_point3D", [](PyTriangulator& t, uint64_t point3D_id) { t.modified.insert(point3D_id); }, "point3D_id"_a)
        .def("clear_modified_points3D", [](PyTriangulator& t) { t.modified.clear(); })
        .def("get_modified_points3D", [](const PyTriangulator& t) {
                 const PyReconstruction& r = t.reconstruction.cast<const PyReconstruction&>();
                 py::set ids;
                 for (uint64_t id : t.modified)
                     if (r.points3D.contains(py::int_(id))) ids.add(py::int_(id));
                 return ids;
             }, "The recorded ids of changed points that still exist.")
        .def_property_readonly("correspondence_graph", [](const PyTriangulator& t) { return t.graph; })
        .def_property_readonly("reconstruction", [](const PyTriangulator& t) { return t.reconstruction; })
        .def("__copy__", [](const PyTriangulator& t) { return PyTriangulator(t); })
        .def("__deepcopy__", [](const PyTriangulator& t, const py::dict& memo) {
                 const py::object deepcopy = py::module_::import("copy").attr("deepcopy");
                 return PyTriangulator{deepcopy(t.graph, memo), deepcopy(t.reconstruction, memo), t.modified, t.re_trials};
             })
        .def("__repr__", [](const PyTriangulator& t) {
            const PyReconstruction& r = t.reconstruction.cast<const PyReconstruction&>();
            return "IncrementalTriangulator(num_images=" + std::to_string(r.images.size()) + ", num_points3D=" + std::to_string(r.points3D.size()) +
                   ", num_modified_points3D=" + std::to_string(t.modified.size()) + ")";
        });

    // ---- complete_tracks, complete_all_tracks (track_ops_host.h) ----
    // IncrementalTriangulator::CompleteTracks / CompleteAllTracks as module-level functions with the triangulator first:
    // tests pin that the class has no such methods.  One amc_complete_tracks call on the superset closures (18.3), then
    // the sequential walk on the host.  Nothing of the reconstruction or of the modified set changes unless everything
    // succeeds.  Without a device the call raises pycolmap_amd._capi.AmcError.
    // ids: None = every point of the reconstruction.  solver: None, or a callable that stands in for the library (a test
    // hook): it takes the flat problem as a dict of arrays and returns a dict with cand_pass.
    // 18.0: the listed ids as a set, which is processed in ascending order; None = every point of the model
    auto listed_point3D_ids = [](const SparseModel& model, const py::object& ids) {
        std::set<uint64_t> listed;
        if (ids.is_none()) {
            for (const ModelPoint3D& p : model.points3D) listed.insert(p.point3D_id);
            return listed;
        }
        for (const py::handle& id : py::iter(ids)) {
            try {
                listed.insert(id.cast<uint64_t>());
            } catch (const py::cast_error&) {
                throw py::type_error("point3D_ids: expected an iterable of non-negative ints");
            }
        }
        return listed;
    };
    auto complete_tracks_with = [checked_model, update_with_errors, listed_point3D_ids](PyTriangulator& t, const TriangulatorOptions& o, const py::object& ids,
                                                                    const py::object& solver) -> size_t {
        const auto t0 = std::chrono::steady_clock::now();
        const std::string bad = o.Check();
        if (!bad.empty()) throw py::value_error(CheckMessage(__FILE__, __LINE__, bad));
        PyReconstruction& r = t.reconstruction.cast<PyReconstruction&>();
        const CorrespondenceGraph& graph = t.graph.cast<const CorrespondenceGraph&>();
        SparseModel model = checked_model(r);
        const ModelIndex ix(model, o);
        const std::set<uint64_t> listed = listed_point3D_ids(model, ids);
        const FlatComplete flat = PlanCompletion(graph, model, ix, o, listed);
        std::set<uint64_t> modified = t.modified;
        CompletionApplied applied;
        uint64_t calls = 0;
        double device_ms = 0, kernel_ms = 0, copy_ms = 0;
        if (flat.NumItems() != 0 && !solver.is_none()) {
            auto arr = [](const auto& v, py::ssize_t cols) {
                using T = typename std::decay<decltype(v)>::type::value_type;
                py::array_t<T> a({static_cast<py::ssize_t>(v.size()) / cols, cols});
                std::copy(v.begin(), v.end(), a.mutable_data());
                return a;
            };
            py::dict d;
            d["camera_models"] = arr(flat.camera_models, 1);
            d["camera_params"] = arr(flat.camera_params, 12);
            d["image_cameras"] = arr(flat.image_cameras, 1);
            d["qvec"] = arr(flat.qvec, 4);
            d["tvec"] = arr(flat.tvec, 3);
            d["item_xyz"] = arr(flat.item_xyz, 3);
            d["item_offsets"] = arr(flat.item_offsets, 1);
            d["cand_image"] = arr(flat.cand_image, 1);
            d["cand_xy"] = arr(flat.cand_xy, 2);
            d["complete_max_reproj_error"] = o.complete_max_reproj_error;
            const py::dict out = solver(d);
            const auto pass = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>::ensure(out["cand_pass"]);
            if (!pass || static_cast<size_t>(pass.size()) != flat.NumCandidates())
                throw py::value_error("complete_tracks: the solver's result does not have the problem's shape");
            calls = 1;
            applied = ApplyCompletion(flat, pass.data(), graph, o, &model, ix, &modified);
        } else if (flat.NumItems() != 0) {
            amc_complete_opts opts;
            amc_complete_opts_default(&opts);
            opts.complete_max_reproj_error = o.complete_max_reproj_error;
            const amc_complete_problem pb = flat.Problem();
            amc_complete_result res{};
            int rc = AMC_OK;
            std::string err;
            {
                py::gil_scoped_release release;
                EstimatorCtx& E = TheEstimatorCtx();
                std::lock_guard<std::mutex> lock(E.mu);
                amc_ctx* ctx = nullptr;
                try {
                    ctx = E.Get();
                } catch (const std::runtime_error& e) {
                    rc = AMC_E_HIP;
                    err = e.what();
                }
                if (ctx) {
                    rc = amc_complete_tracks(ctx, &pb, &opts, &res);
                    if (rc != AMC_OK) err = std::string("amc_complete_tracks: ") + amc_last_error();
                }
            }
            if (rc == AMC_E_INVALID) throw std::invalid_argument(err);
            if (rc != AMC_OK) {
                const py::object cls = py::module_::import("pycolmap_amd._capi").attr("AmcError");
                const py::object exc = cls(rc, err);
                PyErr_SetObject(cls.ptr(), exc.ptr());
                throw py::error_already_set();
            }
            calls = 1;
            device_ms = res.device_ms;
            kernel_ms = res.kernel_ms;
            copy_ms = res.copy_ms;
            try {
                applied = ApplyCompletion(flat, res.cand_pass, graph, o, &model, ix, &modified);
            } catch (...) {
                amc_complete_result_free(&res);
                throw;
            }
            amc_complete_result_free(&res);
        }
        if (applied.num_completed != 0) update_with_errors(r, model);
        t.modified.swap(modified);
        py::dict st;
        st["call"] = ids.is_none() ? "complete_all_tracks" : "complete_tracks";
        st["num_items"] = flat.NumItems();
        st["num_candidates_tested"] = flat.NumCandidates();
        st["num_candidates_visited"] = applied.num_visited;
        st["num_completed_observations"] = applied.num_completed;
        st["num_device_calls"] = solver.is_none() ? calls : 0;
        st["device_ms"] = device_ms;
        st["kernel_ms"] = kernel_ms;
        st["copy_ms"] = copy_ms;
        st["host_ms"] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - device_ms;
        py::module_::import("pycolmap_amd._pycolmap").attr("_last_stats") = st;
        return applied.num_completed;
    };
    m.def("_complete_tracks_with", complete_tracks_with, "triangulator"_a, "options"_a, "point3D_ids"_a, "solver"_a,
          "complete_tracks (point3D_ids=None: complete_all_tracks) with a callable in the library's place (test hook).");
    m.def("complete_tracks", [complete_tracks_with](PyTriangulator& t, const TriangulatorOptions& o, const py::iterable& point3D_ids) {
              return complete_tracks_with(t, o, point3D_ids, py::none());
          }, "triangulator"_a, "options"_a, "point3D_ids"_a,
          "Complete the tracks of the given points3D: attach the observations their correspondences lead to, up to\n"
          "complete_max_transitivity steps away, that have no point yet and reproject within complete_max_reproj_error, on\n"
          "the GPU (DESIGN.md section 18).  The ids are a set, taken in ascending order.  Returns the number of added\n"
          "observations.");
    m.def("complete_all_tracks", [complete_tracks_with](PyTriangulator& t, const TriangulatorOptions& o) {
              return complete_tracks_with(t, o, py::none(), py::none());
          }, "triangulator"_a, "options"_a, "Complete the tracks of all points3D of the reconstruction (DESIGN.md section 18).");

    // ---- merge_tracks, merge_all_tracks (track_ops_host.h) ----
    // One amc_merge_tracks call on the connected components of the listed points, then the merge logs applied root by
    // root in ascending id order.  The solver stands in for the library as above and returns root_return,
    // root_merge_offsets, merge_current, merge_other and merge_xyz.
    auto merge_tracks_with = [checked_model, update_with_new_points, listed_point3D_ids](PyTriangulator& t, const TriangulatorOptions& o, const py::object& ids,
                                                                     const py::object& solver) -> size_t {
        const auto t0 = std::chrono::steady_clock::now();
        const std::string bad = o.Check();
        if (!bad.empty()) throw py::value_error(CheckMessage(__FILE__, __LINE__, bad));
        PyReconstruction& r = t.reconstruction.cast<PyReconstruction&>();
        const CorrespondenceGraph& graph = t.graph.cast<const CorrespondenceGraph&>();
        SparseModel model = checked_model(r);
        const ModelIndex ix(model, o);
        const std::set<uint64_t> listed = listed_point3D_ids(model, ids);
        const FlatMerge flat = PlanMerge(graph, model, ix, listed);
        std::set<uint64_t> modified = t.modified;
        MergeApplied applied;
        uint64_t calls = 0, pairs_tried = 0;
        double device_ms = 0, kernel_ms = 0, copy_ms = 0;
        if (flat.NumComponents() != 0 && !solver.is_none()) {
            auto arr = [](const auto& v, py::ssize_t cols) {
                using T = typename std::decay<decltype(v)>::type::value_type;
                py::array_t<T> a({static_cast<py::ssize_t>(v.size()) / cols, cols});
                std::copy(v.begin(), v.end(), a.mutable_data());
                return a;
            };
            py::dict d;
            d["camera_models"] = arr(flat.camera_models, 1);
            d["camera_params"] = arr(flat.camera_params, 12);
            d["image_cameras"] = arr(flat.image_cameras, 1);
            d["qvec"] = arr(flat.qvec, 4);
            d["tvec"] = arr(flat.tvec, 3);
            d["comp_point_offsets"] = arr(flat.comp_point_offsets, 1);
            d["comp_root_offsets"] = arr(flat.comp_root_offsets, 1);
            d["roots"] = arr(flat.roots, 1);
            d["point_xyz"] = arr(flat.point_xyz, 3);
            d["point_obs_offsets"] = arr(flat.point_obs_offsets, 1);
            d["obs_image"] = arr(flat.obs_image, 1);
            d["obs_xy"] = arr(flat.obs_xy, 2);
            d["obs_corr_offsets"] = arr(flat.obs_corr_offsets, 1);
            d["corr_obs"] = arr(flat.corr_obs, 1);
            d["merge_max_reproj_error"] = o.merge_max_reproj_error;
            const py::dict out = solver(d);
            const auto ret = py::array_t<uint32_t, py::array::c_style | py::array::forcecast>::ensure(out["root_return"]);
            const auto moff = py::array_t<uint64_t, py::array::c_style | py::array::forcecast>::ensure(out["root_merge_offsets"]);
            const auto cur = py::array_t<uint32_t, py::array::c_style | py::array::forcecast>::ensure(out["merge_current"]);
            const auto oth = py::array_t<uint32_t, py::array::c_style | py::array::forcecast>::ensure(out["merge_other"]);
            const auto mxyz = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(out["merge_xyz"]);
            const size_t nroots = flat.roots.size();
            bool fits = ret && moff && cur && oth && mxyz && static_cast<size_t>(ret.size()) == nroots && static_cast<size_t>(moff.size()) == nroots + 1;
            if (fits) {
                for (size_t k = 0; k < nroots; ++k) fits = fits && moff.data()[k] <= moff.data()[k + 1];
                const uint64_t nm = moff.data()[nroots];
                fits = fits && moff.data()[0] == 0 && static_cast<uint64_t>(cur.size()) == nm && static_cast<uint64_t>(oth.size()) == nm &&
                       static_cast<uint64_t>(mxyz.size()) == 3 * nm;
            }
            if (!fits) throw py::value_error("merge_tracks: the solver's result does not have the problem's shape");
            calls = 1;
            applied = ApplyMergeResult(flat, ret.data(), moff.data(), cur.data(), oth.data(), mxyz.data(), &model, &modified);
        } else if (flat.NumComponents() != 0) {
            amc_merge_opts opts;
            amc_merge_opts_default(&opts);
            opts.merge_max_reproj_error = o.merge_max_reproj_error;
            const amc_merge_problem pb = flat.Problem();
            amc_merge_result res{};
            int rc = AMC_OK;
            std::string err;
            {
                py::gil_scoped_release release;
                EstimatorCtx& E = TheEstimatorCtx();
                std::lock_guard<std::mutex> lock(E.mu);
                amc_ctx* ctx = nullptr;
                try {
                    ctx = E.Get();
                } catch (const std::runtime_error& e) {
                    rc = AMC_E_HIP;
                    err = e.what();
                }
                if (ctx) {
                    rc = amc_merge_tracks(ctx, &pb, &opts, &res);
                    if (rc != AMC_OK) err = std::string("amc_merge_tracks: ") + amc_last_error();
                }
            }
            if (rc == AMC_E_INVALID) throw std::invalid_argument(err);
            if (rc != AMC_OK) {
                const py::object cls = py::module_::import("pycolmap_amd._capi").attr("AmcError");
                const py::object exc = cls(rc, err);
                PyErr_SetObject(cls.ptr(), exc.ptr());
                throw py::error_already_set();
            }
            calls = 1;
            pairs_tried = res.num_pairs_tried;
            device_ms = res.device_ms;
            kernel_ms = res.kernel_ms;
            copy_ms = res.copy_ms;
            try {
                applied = ApplyMergeResult(flat, res.root_return, res.root_merge_offsets, res.merge_current, res.merge_other, res.merge_xyz, &model, &modified);
            } catch (...) {
                amc_merge_result_free(&res);
                throw;
            }
            amc_merge_result_free(&res);
        }
        if (applied.num_merges != 0) update_with_new_points(r, model);
        t.modified.swap(modified);
        py::dict st;
        st["call"] = ids.is_none() ? "merge_all_tracks" : "merge_tracks";
        st["num_components"] = flat.NumComponents();
        st["largest_component"] = flat.largest_component;
        st["num_pairs_tried"] = pairs_tried;
        st["num_merges"] = applied.num_merges;
        st["num_device_calls"] = solver.is_none() ? calls : 0;
        st["device_ms"] = device_ms;
        st["kernel_ms"] = kernel_ms;
        st["copy_ms"] = copy_ms;
        st["host_ms"] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - device_ms;
        py::module_::import("pycolmap_amd._pycolmap").attr("_last_stats") = st;
        return applied.num_merged;
    };
    m.def("_merge_tracks_with", merge_tracks_with, "triangulator"_a, "options"_a, "point3D_ids"_a, "solver"_a,
          "merge_tracks (point3D_ids=None: merge_all_tracks) with a callable in the library's place (test hook).");
    m.def("merge_tracks", [merge_tracks_with](PyTriangulator& t, const TriangulatorOptions& o, const py::iterable& point3D_ids) {
              return merge_tracks_with(t, o, point3D_ids, py::none());
          }, "triangulator"_a, "options"_a, "point3D_ids"_a,
          "Merge the given points3D with the points their correspondences carry, wherever every observation of both\n"
          "reprojects within merge_max_reproj_error of the weighted mean position, on the GPU (DESIGN.md section 18).  The ids\n"
          "are a set, taken in ascending order.  Returns the number of merged observations.");
    m.def("merge_all_tracks", [merge_tracks_with](PyTriangulator& t, const TriangulatorOptions& o) {
              return merge_tracks_with(t, o, py::none(), py::none());
          }, "triangulator"_a, "options"_a, "Merge the tracks of all points3D of the reconstruction (DESIGN.md section 18).");

    // ---- retriangulate (retriangulate_host.h) ----
    // IncrementalTriangulator::Retriangulate as a module-level function with the triangulator first: tests pin that the
    // class has no such method.  The host colours the statically eligible pairs into rounds, one
    // amc_retriangulate_pairs call runs every round on the device, and the host replays the result in the sequential
    // order.  Nothing of the reconstruction, of the modified set or of the trial counters changes unless everything
    // succeeds.  Without a device the call raises pycolmap_amd._capi.AmcError.
    // solver: None, or a callable that stands in for the library (a test hook): it takes the flat problem as a dict of
    // arrays and returns a dict with pair_ran, corr_action, created_offsets and created_xyz.  max_correspondences: the
    // bound above which the call is refused (the library's; tests pass a smaller one).
    auto retriangulate_with = [checked_model, update_with_new_points](PyTriangulator& t, const TriangulatorOptions& o, const py::object& solver,
                                                                      uint64_t max_correspondences) -> size_t {
        const auto t0 = std::chrono::steady_clock::now();
        const std::string bad = o.Check();
        if (!bad.empty()) throw py::value_error(CheckMessage(__FILE__, __LINE__, bad));
        PyReconstruction& r = t.reconstruction.cast<PyReconstruction&>();
        const CorrespondenceGraph& graph = t.graph.cast<const CorrespondenceGraph&>();
        SparseModel model = checked_model(r);
        ModelIndex ix(model, o);
        const FlatRetri flat = PlanRetriangulation(graph, model, ix, o, t.re_trials, max_correspondences);
        std::set<uint64_t> modified = t.modified;
        RetriTrials trials = t.re_trials;
        RetriApplied applied;
        uint64_t calls = 0;
        double device_ms = 0, kernel_ms = 0, copy_ms = 0;
        if (flat.NumPairs() == 0) {
            applied = ApplyRetriResult(flat, nullptr, nullptr, nullptr, nullptr, &model, &ix, &modified, &trials);
        } else if (!solver.is_none()) {
            auto arr = [](const auto& v, py::ssize_t cols) {
                using T = typename std::decay<decltype(v)>::type::value_type;
                py::array_t<T> a({static_cast<py::ssize_t>(v.size()) / cols, cols});
                std::copy(v.begin(), v.end(), a.mutable_data());
                return a;
            };
            py::dict d;
            d["camera_models"] = arr(flat.camera_models, 1);
            d["camera_params"] = arr(flat.camera_params, 12);
            d["image_cameras"] = arr(flat.image_cameras, 1);
            d["qvec"] = arr(flat.qvec, 4);
            d["tvec"] = arr(flat.tvec, 3);
            d["obs_image"] = arr(flat.obs_image, 1);
            d["obs_xy"] = arr(flat.obs_xy, 2);
            d["obs_point"] = arr(flat.obs_point, 1);
            d["point_xyz"] = arr(flat.point_xyz, 3);
            d["pair_images"] = arr(flat.pair_images, 2);
            d["pair_offsets"] = arr(flat.pair_offsets, 1);
            d["corr_obs"] = arr(flat.corr_obs, 2);
            d["corr_two_view"] = arr(flat.corr_two_view, 1);
            d["round_offsets"] = arr(flat.round_offsets, 1);
            d["create_max_angle_error"] = o.create_max_angle_error;
            d["re_max_angle_error"] = o.re_max_angle_error;
            d["min_angle"] = o.min_angle;
            d["re_min_ratio"] = o.re_min_ratio;
            const py::dict out = solver(d);
            const auto ran = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>::ensure(out["pair_ran"]);
            const auto act = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>::ensure(out["corr_action"]);
            const auto coff = py::array_t<uint64_t, py::array::c_style | py::array::forcecast>::ensure(out["created_offsets"]);
            const auto cxyz = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(out["created_xyz"]);
            if (!ran || !act || !coff || !cxyz || static_cast<size_t>(ran.size()) != flat.NumPairs() || static_cast<size_t>(act.size()) != flat.NumCorrs() ||
                static_cast<size_t>(coff.size()) != flat.NumPairs() + 1 || static_cast<uint64_t>(cxyz.size()) != 3 * coff.data()[flat.NumPairs()])
                throw py::value_error("retriangulate: the solver's result does not have the problem's shape");
            applied = ApplyRetriResult(flat, ran.data(), act.data(), coff.data(), cxyz.data(), &model, &ix, &modified, &trials);
        } else {
            amc_retri_opts opts;
            amc_retri_opts_default(&opts);
            opts.create_max_angle_error = o.create_max_angle_error;
            opts.re_max_angle_error = o.re_max_angle_error;
            opts.min_angle = o.min_angle;
            opts.re_min_ratio = o.re_min_ratio;
            const amc_retri_problem pb = flat.Problem();
            amc_retri_result res{};
            int rc = AMC_OK;
            std::string err;
            {
                py::gil_scoped_release release;
                EstimatorCtx& E = TheEstimatorCtx();
                std::lock_guard<std::mutex> lock(E.mu);
                amc_ctx* ctx = nullptr;
                try {
                    ctx = E.Get();
                } catch (const std::runtime_error& e) {
                    rc = AMC_E_HIP;
                    err = e.what();
                }
                if (ctx) {
                    rc = amc_retriangulate_pairs(ctx, &pb, &opts, &res);
                    if (rc != AMC_OK) err = std::string("amc_retriangulate_pairs: ") + amc_last_error();
                }
            }
            if (rc == AMC_E_INVALID) throw std::invalid_argument(err);
            if (rc != AMC_OK) {
                const py::object cls = py::module_::import("pycolmap_amd._capi").attr("AmcError");
                const py::object exc = cls(rc, err);
                PyErr_SetObject(cls.ptr(), exc.ptr());
                throw py::error_already_set();
            }
            calls = 1;
            device_ms = res.device_ms;
            kernel_ms = res.kernel_ms;
            copy_ms = res.copy_ms;
            try {
                applied = ApplyRetriResult(flat, res.pair_ran, res.corr_action, res.created_offsets, res.created_xyz, &model, &ix, &modified, &trials);
            } catch (...) {
                amc_retri_result_free(&res);
                throw;
            }
            amc_retri_result_free(&res);
        }
        if (applied.num_tris != 0) update_with_new_points(r, model);
        t.modified.swap(modified);
        t.re_trials.swap(trials);
        py::dict st;
        st["call"] = "retriangulate";
        st["num_pairs"] = flat.NumPairs();
        st["num_pairs_run"] = applied.num_pairs_run;
        st["num_rounds"] = flat.NumRounds();
        st["num_correspondences"] = flat.NumCorrs();
        st["num_continued_observations"] = applied.num_continued;
        st["num_created_points"] = applied.num_created;
        st["num_device_calls"] = calls;
        st["device_ms"] = device_ms;
        st["kernel_ms"] = kernel_ms;
        st["copy_ms"] = copy_ms;
        st["host_ms"] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - device_ms;
        py::module_::import("pycolmap_amd._pycolmap").attr("_last_stats") = st;
        return applied.num_tris;
    };
    m.def("_retriangulate_with", retriangulate_with, "triangulator"_a, "options"_a, "solver"_a,
          "max_correspondences"_a = static_cast<uint64_t>(AMC_RETRI_MAX_CORRS),
          "retriangulate with a callable in the library's place, or None for the library (test hook).");
    m.def("retriangulate", [retriangulate_with](PyTriangulator& t, const TriangulatorOptions& o) {
              return retriangulate_with(t, o, py::none(), AMC_RETRI_MAX_CORRS);
          }, "triangulator"_a, "options"_a,
          "Retriangulate the under-reconstructed image pairs: for every pair of the correspondence graph whose share of\n"
          "correspondences with a common point3D is below re_min_ratio and that has trials left, continue tracks within\n"
          "re_max_angle_error and create two-view points, on the GPU (DESIGN.md section 19).  Returns the number of\n"
          "triangulated observations.");
    m.def("_retriangulate_trials", [](const PyTriangulator& t) {
              py::dict d;
              for (const auto& kv : t.re_trials)
                  d[py::make_tuple(static_cast<uint32_t>(kv.first >> 32), static_cast<uint32_t>(kv.first))] = kv.second;
              return d;
          }, "triangulator"_a, "The trial counters of retriangulate, {(image_id1, image_id2): trials} (test hook, a copy).");
    m.def("_retriangulate_rounds", [](const std::vector<std::pair<uint32_t, uint32_t>>& pairs) { return ColourRetriRounds(pairs); },
          "pairs"_a, "The round of every image pair under retriangulate's greedy colouring, pairs in the given order (test hook).");

    // ---- IncrementalMapper (mapper_host.h) ----
    // The three steps in front of triangulate_image: which candidate to register next, the registration itself and the
    // images of the local adjustment after it.  The graph and the reconstruction are the triangulator's.  An image that
    // is not registered is not in the reconstruction (R1), so the mapper keeps its candidates itself.  Every method
    // takes a device first: without one it raises pycolmap_amd._capi.AmcError and changes nothing.  The `_with`
    // variants put a callable in the library's place (test hooks: the CPU tests pass the references).
    py::enum_<ImageSelectionMethod> PySelection(m, "ImageSelectionMethod");
    PySelection.value("MAX_VISIBLE_POINTS_NUM", ImageSelectionMethod::MAX_VISIBLE_POINTS_NUM)
        .value("MAX_VISIBLE_POINTS_RATIO", ImageSelectionMethod::MAX_VISIBLE_POINTS_RATIO)
        .value("MIN_UNCERTAINTY", ImageSelectionMethod::MIN_UNCERTAINTY);
    PySelection.def(py::init([](const std::string& s) {
        if (s == "MAX_VISIBLE_POINTS_NUM") return ImageSelectionMethod::MAX_VISIBLE_POINTS_NUM;
        if (s == "MAX_VISIBLE_POINTS_RATIO") return ImageSelectionMethod::MAX_VISIBLE_POINTS_RATIO;
        if (s == "MIN_UNCERTAINTY") return ImageSelectionMethod::MIN_UNCERTAINTY;
        throw py::value_error("Invalid string value " + s + " for enum ImageSelectionMethod");
    }));
    py::implicitly_convertible<std::string, ImageSelectionMethod>();
    py::class_<MapperOptions> PyMapOpts(m, "IncrementalMapperOptions");
    PyMapOpts.def(py::init<>())
        .def_readwrite("init_min_num_inliers", &MapperOptions::init_min_num_inliers, "Minimum number of inliers for initial image pair.")
        .def_readwrite("init_max_error", &MapperOptions::init_max_error, "Maximum error in pixels for two-view geometry estimation for initial image pair.")
        .def_readwrite("init_max_forward_motion", &MapperOptions::init_max_forward_motion, "Maximum forward motion for initial image pair.")
        .def_readwrite("init_min_tri_angle", &MapperOptions::init_min_tri_angle, "Minimum triangulation angle for initial image pair.")
        .def_readwrite("init_max_reg_trials", &MapperOptions::init_max_reg_trials, "Maximum number of trials to use an image for initialization.")
        .def_readwrite("abs_pose_max_error", &MapperOptions::abs_pose_max_error, "Maximum reprojection error in absolute pose estimation.")
        .def_readwrite("abs_pose_min_num_inliers", &MapperOptions::abs_pose_min_num_inliers, "Minimum number of inliers in absolute pose estimation.")
        .def_readwrite("abs_pose_min_inlier_ratio", &MapperOptions::abs_pose_min_inlier_ratio, "Minimum inlier ratio in absolute pose estimation.")
        .def_readwrite("abs_pose_refine_focal_length", &MapperOptions::abs_pose_refine_focal_length, "Whether to estimate the focal length in absolute pose estimation.")
        .def_readwrite("abs_pose_refine_extra_params", &MapperOptions::abs_pose_refine_extra_params, "Whether to estimate the extra parameters in absolute pose estimation.")
        .def_readwrite("local_ba_num_images", &MapperOptions::local_ba_num_images, "Number of images to optimize in local bundle adjustment.")
        .def_readwrite("local_ba_min_tri_angle", &MapperOptions::local_ba_min_tri_angle, "Minimum triangulation for images to be chosen in local bundle adjustment.")
        .def_readwrite("min_focal_length_ratio", &MapperOptions::min_focal_length_ratio, "The threshold used to filter and ignore images with degenerate intrinsics.")
        .def_readwrite("max_focal_length_ratio", &MapperOptions::max_focal_length_ratio, "The threshold used to filter and ignore images with degenerate intrinsics.")
        .def_readwrite("max_extra_param", &MapperOptions::max_extra_param, "The threshold used to filter and ignore images with degenerate intrinsics.")
        .def_readwrite("filter_max_reproj_error", &MapperOptions::filter_max_reproj_error, "Maximum reprojection error in pixels for observations.")
        .def_readwrite("filter_min_tri_angle", &MapperOptions::filter_min_tri_angle, "Minimum triangulation angle in degrees for stable 3D points.")
        .def_readwrite("max_reg_trials", &MapperOptions::max_reg_trials, "Maximum number of trials to register an image.")
        .def_readwrite("fix_existing_images", &MapperOptions::fix_existing_images, "If reconstruction is provided as input, fix the existing image poses.")
        .def_readwrite("num_threads", &MapperOptions::num_threads, "Number of threads.")
        .def_readwrite("image_selection_method", &MapperOptions::image_selection_method, "Method to find and select next best image to register.");
    MakeDataclass(PyMapOpts, {"init_min_num_inliers", "init_max_error", "init_max_forward_motion", "init_min_tri_angle", "init_max_reg_trials",
                              "abs_pose_max_error", "abs_pose_min_num_inliers", "abs_pose_min_inlier_ratio", "abs_pose_refine_focal_length",
                              "abs_pose_refine_extra_params", "local_ba_num_images", "local_ba_min_tri_angle", "min_focal_length_ratio",
                              "max_focal_length_ratio", "max_extra_param", "filter_max_reproj_error", "filter_min_tri_angle", "max_reg_trials",
                              "fix_existing_images", "num_threads", "image_selection_method"});

    struct PyMapper {
        py::object triangulator;
        MapperCandidates candidates;
        std::map<uint32_t, py::object> candidate_images;  // a copy of what add_candidate was given, for the reconstruction
        MapperTrials trials;
        size_t num_total_reg_images = 0;
        py::dict last;  // last_registration()
        // the registered images in COLMAP's reg_image_ids_ order, the images the model held when the mapper
        // was made (existing_image_ids_), the images filter_images removed (filtered_images_)
        std::vector<uint32_t> reg_image_ids;
        std::set<uint32_t> existing_image_ids, filtered_images;
        py::dict last_pair;  // last_initial_pair()
    };
    // one library call under the estimator context's lock with the GIL released; fn == nullptr only takes the device
    auto call_library = [](const std::function<int(amc_ctx*)>& fn, const char* name) {
        int rc = AMC_OK;
        std::string err;
        {
            py::gil_scoped_release release;
            EstimatorCtx& E = TheEstimatorCtx();
            std::lock_guard<std::mutex> lock(E.mu);
            amc_ctx* ctx = nullptr;
            try {
                ctx = E.Get();
            } catch (const std::runtime_error& e) {
                rc = AMC_E_HIP;
                err = e.what();
            }
            if (ctx && fn) {
                rc = fn(ctx);
                if (rc != AMC_OK) err = std::string(name) + ": " + amc_last_error();
            }
        }
        if (rc == AMC_E_INVALID) throw std::invalid_argument(err);
        if (rc != AMC_OK) {
            const py::object cls = py::module_::import("pycolmap_amd._capi").attr("AmcError");
            const py::object exc = cls(rc, err);
            PyErr_SetObject(cls.ptr(), exc.ptr());
            throw py::error_already_set();
        }
    };
    auto np_array = [](const auto& v, py::ssize_t cols) {
        using T = typename std::decay<decltype(v)>::type::value_type;
        py::array_t<T> a({static_cast<py::ssize_t>(v.size()) / cols, cols});
        std::copy(v.begin(), v.end(), a.mutable_data());
        return a;
    };
    auto checked_mapper_options = [](const MapperOptions& o) {
        const std::string bad = o.Check();
        if (!bad.empty()) throw py::value_error(CheckMessage(__FILE__, __LINE__, bad));
    };
    auto find_next_images_with = [checked_model, call_library, np_array, checked_mapper_options](PyMapper& mp, const MapperOptions& o, const py::object& solver) {
        const auto t0 = std::chrono::steady_clock::now();
        checked_mapper_options(o);
        if (solver.is_none()) call_library(nullptr, "");
        PyTriangulator& t = mp.triangulator.cast<PyTriangulator&>();
        const CorrespondenceGraph& graph = t.graph.cast<const CorrespondenceGraph&>();
        const SparseModel model = checked_model(t.reconstruction.cast<PyReconstruction&>());
        const ModelIndex ix(model, o.BogusThresholds());
        const FlatVisibility flat = PlanVisibility(graph, model, ix, mp.candidates);
        std::vector<uint32_t> ranked;
        double device_ms = 0, kernel_ms = 0, copy_ms = 0;
        uint64_t calls = 0;
        const size_t nc = flat.cand_ids.size();
        if (nc == 0) {
        } else if (!solver.is_none()) {
            py::dict d;
            d["image_point_offsets"] = np_array(flat.image_point_offsets, 1);
            d["point2D_point3D"] = np_array(flat.point2D_point3D, 1);
            d["cand_width"] = np_array(flat.cand_width, 1);
            d["cand_height"] = np_array(flat.cand_height, 1);
            d["cand_point_offsets"] = np_array(flat.cand_point_offsets, 1);
            d["cand_xy"] = np_array(flat.cand_xy, 2);
            d["corr_offsets"] = np_array(flat.corr_offsets, 1);
            d["corr_image"] = np_array(flat.corr_image, 1);
            d["corr_point2D"] = np_array(flat.corr_point2D, 1);
            const py::dict out = solver(d);
            const auto nobs = py::array_t<uint32_t, py::array::c_style | py::array::forcecast>::ensure(out["num_observations"]);
            const auto nvis = py::array_t<uint32_t, py::array::c_style | py::array::forcecast>::ensure(out["num_visible_points3D"]);
            const auto score = py::array_t<uint64_t, py::array::c_style | py::array::forcecast>::ensure(out["score"]);
            if (!nobs || !nvis || !score || static_cast<size_t>(nobs.size()) != nc || static_cast<size_t>(nvis.size()) != nc || static_cast<size_t>(score.size()) != nc)
                throw py::value_error("find_next_images: the solver's result does not have the problem's shape");
            ranked = RankNextImages(flat, nobs.data(), nvis.data(), score.data(), o, mp.trials, &mp.filtered_images);
        } else {
            const amc_visibility_problem pb = flat.Problem();
            amc_visibility_result res{};
            call_library([&](amc_ctx* ctx) { return amc_image_visibility(ctx, &pb, &res); }, "amc_image_visibility");
            calls = 1;
            device_ms = res.device_ms;
            kernel_ms = res.kernel_ms;
            copy_ms = res.copy_ms;
            try {
                ranked = RankNextImages(flat, res.num_observations, res.num_visible_points3D, res.score, o, mp.trials, &mp.filtered_images);
            } catch (...) {
                amc_visibility_result_free(&res);
                throw;
            }
            amc_visibility_result_free(&res);
        }
        py::dict st;
        st["call"] = "find_next_images";
        st["num_candidates"] = nc;
        st["num_ranked"] = ranked.size();
        st["num_correspondences"] = flat.corr_image.size();
        st["num_device_calls"] = calls;
        st["device_ms"] = device_ms;
        st["kernel_ms"] = kernel_ms;
        st["copy_ms"] = copy_ms;
        st["host_ms"] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - device_ms;
        py::module_::import("pycolmap_amd._pycolmap").attr("_last_stats") = st;
        return ranked;
    };
    auto register_next_image_with = [checked_model, update_from_model, call_library, np_array, checked_mapper_options](
                                        PyMapper& mp, const MapperOptions& o, uint32_t image_id, const py::object& solver) -> bool {
        const auto t0 = std::chrono::steady_clock::now();
        checked_mapper_options(o);
        if (solver.is_none()) call_library(nullptr, "");
        PyTriangulator& t = mp.triangulator.cast<PyTriangulator&>();
        PyReconstruction& r = t.reconstruction.cast<PyReconstruction&>();
        const CorrespondenceGraph& graph = t.graph.cast<const CorrespondenceGraph&>();
        const auto cand = mp.candidates.find(image_id);
        if (cand == mp.candidates.end() || r.images.contains(py::int_(image_id)))
            throw py::value_error(CheckMessage(__FILE__, __LINE__, "!image.IsRegistered() && IsCandidate(image_id)", "image_id=" + std::to_string(image_id)));
        const MapperCandidate& c = cand->second;
        SparseModel model = checked_model(r);
        ModelIndex ix(model, o.BogusThresholds());
        const auto cam = ix.camera.find(c.camera_id);
        if (cam == ix.camera.end()) throw py::value_error("register_next_image: candidate " + std::to_string(image_id) + " names a camera the reconstruction does not hold");
        const RegistrationPairs pairs = CollectRegistrationPairs(graph, model, ix, c);
        PyCamera& pycam = r.cameras[py::int_(c.camera_id)].cast<PyCamera&>();
        pycam.CheckParams();
        const RegistrationRule rule = PlanRegistration(model, model.cameras[cam->second], pycam.has_prior_focal_length, o);
        // everything that can refuse the call has: from here on the trial counts
        mp.trials[image_id] += 1;
        py::dict last;
        last["image_id"] = image_id;
        last["success"] = false;
        last["num_visible_points3D"] = pairs.num_visible;
        last["num_pairs"] = pairs.size();
        last["num_inliers"] = 0;
        last["focal_factor"] = 1.0;
        last["estimate_focal_length"] = rule.estimate_focal_length;
        last["would_refine_focal_length"] = rule.refine_focal_length;
        last["would_refine_extra_params"] = rule.refine_extra_params;
        double device_ms = 0, kernel_ms = 0;
        uint64_t calls = 0;
        bool ok = pairs.num_visible >= static_cast<size_t>(o.abs_pose_min_num_inliers) && pairs.size() >= static_cast<size_t>(o.abs_pose_min_num_inliers);
        if (ok) {
            amc_abspose_opts eo;
            amc_abspose_opts_default(&eo);
            eo.estimate_focal_length = rule.estimate_focal_length ? 1 : 0;
            eo.num_focal_length_samples = 30;
            eo.min_focal_length_ratio = o.min_focal_length_ratio;
            eo.max_focal_length_ratio = o.max_focal_length_ratio;
            eo.max_error = o.abs_pose_max_error;
            eo.min_inlier_ratio = o.abs_pose_min_inlier_ratio;
            eo.confidence = 0.99999;
            eo.dyn_num_trials_multiplier = 3.0;
            eo.min_num_trials = 100;
            eo.max_num_trials = 10000;
            amc_abspose_refine_opts ro;
            amc_abspose_refine_opts_default(&ro);  // AbsolutePoseRefinementOptions(); intrinsics are never refined (J5)
            const std::array<double, 12> prm = CameraParams12(pycam);
            const int32_t cmodel = pycam.model;
            const size_t n = pairs.size();
            bool success = false;
            size_t num_inliers = 0;
            double focal_factor = 1.0, q[4] = {0, 0, 0, 1}, tv[3] = {0, 0, 0};
            std::vector<uint8_t> mask(n, 0);
            if (!solver.is_none()) {
                py::dict d, est;
                d["camera_model"] = cmodel;
                d["camera_params"] = np_array(std::vector<double>(prm.begin(), prm.end()), 12);
                d["points2D"] = np_array(pairs.points2D, 2);
                d["points3D"] = np_array(pairs.points3D, 3);
                est["estimate_focal_length"] = rule.estimate_focal_length;
                est["num_focal_length_samples"] = eo.num_focal_length_samples;
                est["min_focal_length_ratio"] = eo.min_focal_length_ratio;
                est["max_focal_length_ratio"] = eo.max_focal_length_ratio;
                est["max_error"] = eo.max_error;
                est["min_inlier_ratio"] = eo.min_inlier_ratio;
                est["confidence"] = eo.confidence;
                est["dyn_num_trials_multiplier"] = eo.dyn_num_trials_multiplier;
                est["min_num_trials"] = eo.min_num_trials;
                est["max_num_trials"] = eo.max_num_trials;
                d["estimation"] = est;
                const py::dict out = solver(d);
                const auto sq = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(out["qvec"]);
                const auto stv = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(out["tvec"]);
                const auto sm = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>::ensure(out["inlier_mask"]);
                if (!sq || !stv || !sm || sq.size() != 4 || stv.size() != 3 || static_cast<size_t>(sm.size()) != n)
                    throw py::value_error("register_next_image: the solver's result does not have the problem's shape");
                success = out["success"].cast<bool>();
                num_inliers = out["num_inliers"].cast<size_t>();
                focal_factor = out["focal_factor"].cast<double>();
                std::copy(sq.data(), sq.data() + 4, q);
                std::copy(stv.data(), stv.data() + 3, tv);
                std::copy(sm.data(), sm.data() + n, mask.begin());
            } else {
                const uint64_t off[2] = {0, n};
                amc_abspose_result res{};
                call_library([&](amc_ctx* ctx) {
                    return amc_estimate_absolute_poses(ctx, off, 1, &cmodel, prm.data(), pairs.points2D.data(), pairs.points3D.data(), &eo, &ro, 0, &res);
                }, "amc_estimate_absolute_poses");
                calls = 1;
                device_ms = res.device_ms;
                kernel_ms = res.kernel_ms;
                success = res.success[0] != 0;
                num_inliers = res.num_inliers[0];
                focal_factor = res.focal_factor[0];
                std::copy(res.qvec, res.qvec + 4, q);
                std::copy(res.tvec, res.tvec + 3, tv);
                std::copy(res.inlier_mask, res.inlier_mask + n, mask.begin());
                amc_abspose_result_free(&res);
            }
            last["num_inliers"] = num_inliers;
            last["focal_factor"] = focal_factor;
            ok = success && num_inliers >= static_cast<size_t>(o.abs_pose_min_num_inliers);
            if (ok) {
                std::set<uint64_t> modified = t.modified;
                ApplyRegistration(c, pairs, mask.data(), q, tv, rule.estimate_focal_length, focal_factor, &model, &ix, &modified);
                r.images[py::int_(image_id)] = py::module_::import("copy").attr("copy")(mp.candidate_images.at(image_id));
                update_from_model(r, model);
                t.modified.swap(modified);
                mp.num_total_reg_images += 1;
                mp.reg_image_ids.push_back(image_id);
                mp.candidate_images.erase(image_id);
                mp.candidates.erase(cand);
            }
        }
        last["success"] = ok;
        mp.last = last;
        py::dict st;
        st["call"] = "register_next_image";
        st["num_pairs"] = pairs.size();
        st["num_device_calls"] = calls;
        st["device_ms"] = device_ms;
        st["kernel_ms"] = kernel_ms;
        st["copy_ms"] = 0.0;
        st["host_ms"] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - device_ms;
        py::module_::import("pycolmap_amd._pycolmap").attr("_last_stats") = st;
        return ok;
    };
    auto find_local_bundle_with = [checked_model, call_library, np_array, checked_mapper_options](PyMapper& mp, const MapperOptions& o, uint32_t image_id,
                                                                                               const py::object& solver, uint64_t max_pair_points) {
        const auto t0 = std::chrono::steady_clock::now();
        checked_mapper_options(o);
        if (solver.is_none()) call_library(nullptr, "");
        PyTriangulator& t = mp.triangulator.cast<PyTriangulator&>();
        const SparseModel model = checked_model(t.reconstruction.cast<PyReconstruction&>());
        const ModelIndex ix(model, o.BogusThresholds());
        const FlatBundle flat = PlanLocalBundle(model, ix, o, image_id, max_pair_points);
        std::vector<uint32_t> bundle;
        double device_ms = 0, kernel_ms = 0, copy_ms = 0;
        uint64_t calls = 0;
        if (flat.NumPairs() == 0) {
            bundle = SelectLocalBundle(flat, o, nullptr);
        } else if (!solver.is_none()) {
            py::dict d;
            d["qvec"] = np_array(flat.qvec, 4);
            d["tvec"] = np_array(flat.tvec, 3);
            d["point_xyz"] = np_array(flat.point_xyz, 3);
            d["pair_images"] = np_array(flat.pair_images, 2);
            d["pair_offsets"] = np_array(flat.pair_offsets, 1);
            d["shared_points"] = np_array(flat.shared_points, 1);
            d["percentile"] = 75.0;
            const py::dict out = solver(d);
            const auto angle = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(out["angle"]);
            if (!angle || static_cast<size_t>(angle.size()) != flat.NumPairs())
                throw py::value_error("find_local_bundle: the solver's result does not have the problem's shape");
            bundle = SelectLocalBundle(flat, o, angle.data());
        } else {
            const amc_pair_angle_problem pb = flat.Problem();
            amc_pair_angle_opts po;
            amc_pair_angle_opts_default(&po);
            amc_pair_angle_result res{};
            call_library([&](amc_ctx* ctx) { return amc_shared_point_angles(ctx, &pb, &po, &res); }, "amc_shared_point_angles");
            calls = 1;
            device_ms = res.device_ms;
            kernel_ms = res.kernel_ms;
            copy_ms = res.copy_ms;
            try {
                bundle = SelectLocalBundle(flat, o, res.angle);
            } catch (...) {
                amc_pair_angle_result_free(&res);
                throw;
            }
            amc_pair_angle_result_free(&res);
        }
        py::dict st;
        st["call"] = "find_local_bundle";
        st["num_overlapping_images"] = flat.overlapping.size();
        st["num_pairs"] = flat.NumPairs();
        st["num_shared_points"] = flat.shared_points.size();
        st["num_device_calls"] = calls;
        st["device_ms"] = device_ms;
        st["kernel_ms"] = kernel_ms;
        st["copy_ms"] = copy_ms;
        st["host_ms"] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - device_ms;
        py::module_::import("pycolmap_amd._pycolmap").attr("_last_stats") = st;
        return bundle;
    };

    // ---- the initial pair, the global adjustment and the image filter (initial_pair_host.h) ----
    // Module-level functions that take the mapper first, as complete_tracks takes the triangulator: existing tests pin
    // that the class has no such methods.
    // reg_image_ids against a reconstruction that changed behind the mapper's back (K2): ids that left the model leave
    // the list, model images the list lacks join it in ascending id
    auto sync_reg_image_ids = [](PyMapper& mp) {
        const PyReconstruction& r = mp.triangulator.cast<PyTriangulator&>().reconstruction.cast<const PyReconstruction&>();
        std::vector<uint32_t> kept, extra;
        std::set<uint32_t> seen;
        for (uint32_t id : mp.reg_image_ids)
            if (r.images.contains(py::int_(id)) && seen.insert(id).second) kept.push_back(id);
        for (auto item : r.images)
            if (!seen.count(item.first.cast<uint32_t>())) extra.push_back(item.first.cast<uint32_t>());
        std::sort(extra.begin(), extra.end());
        kept.insert(kept.end(), extra.begin(), extra.end());
        mp.reg_image_ids.swap(kept);
    };
    // RegisterInitialImagePair (21.1, 21.2).  two_view_solver: None, or a callable (camera1, points1, camera2, points2,
    // matches, options) -> dict of the geometry after the pose step (pose_ok, config, inlier_matches (K, 2), qvec x y z w,
    // tvec, tri_angle) in the place of estimate_calibrated_two_view_geometry and estimate_two_view_geometry_pose; pair_solver: None, or a callable that takes
    // the flat problem of amc_triangulate_pairs as a dict of arrays and returns accepted, xyz and tri_angle.
    auto register_initial_image_pair_with = [checked_model, update_with_new_points, call_library, np_array, checked_mapper_options](
                                                PyMapper& mp, const MapperOptions& o, uint32_t id1, uint32_t id2, const py::object& two_view_solver,
                                                const py::object& pair_solver) -> bool {
        const auto t0 = std::chrono::steady_clock::now();
        checked_mapper_options(o);
        if (two_view_solver.is_none() || pair_solver.is_none()) call_library(nullptr, "");
        PyTriangulator& t = mp.triangulator.cast<PyTriangulator&>();
        PyReconstruction& r = t.reconstruction.cast<PyReconstruction&>();
        const CorrespondenceGraph& graph = t.graph.cast<const CorrespondenceGraph&>();
        const auto cand1 = mp.candidates.find(id1), cand2 = mp.candidates.find(id2);
        if (id1 == id2 || cand1 == mp.candidates.end() || cand2 == mp.candidates.end() || r.images.contains(py::int_(id1)) || r.images.contains(py::int_(id2)))
            throw py::value_error(CheckMessage(__FILE__, __LINE__, "image_id1 != image_id2 && IsCandidate(image_id1) && IsCandidate(image_id2)",
                                               "image_id1=" + std::to_string(id1) + ", image_id2=" + std::to_string(id2)));
        const MapperCandidate& c1 = cand1->second;
        const MapperCandidate& c2 = cand2->second;
        SparseModel model = checked_model(r);
        ModelIndex ix(model, o.BogusThresholds());
        const auto cam1 = ix.camera.find(c1.camera_id), cam2 = ix.camera.find(c2.camera_id);
        if (cam1 == ix.camera.end() || cam2 == ix.camera.end()) throw py::value_error("register_initial_image_pair: a candidate names a camera the reconstruction does not hold");
        const py::object pycam1 = r.cameras[py::int_(c1.camera_id)], pycam2 = r.cameras[py::int_(c2.camera_id)];
        pycam1.cast<PyCamera&>().CheckParams();
        pycam2.cast<PyCamera&>().CheckParams();
        if (graph.NumPoints2D(id1) != c1.NumPoints2D() || graph.NumPoints2D(id2) != c2.NumPoints2D())
            throw py::value_error("register_initial_image_pair: a candidate's number of points2D differs from the graph's");
        const std::vector<uint32_t> matches = graph.FindCorrespondencesBetweenImages(id1, id2);
        const double identity_q[4] = {0, 0, 0, 1}, zero_t[3] = {0, 0, 0};
        FlatInitialPair flat = PlanInitialPair(model.cameras[cam1->second], model.cameras[cam2->second], c1, c2, matches, identity_q, zero_t);
        // EstimateInitialTwoViewGeometry
        TwoViewGeometryOptions tvo;
        tvo.ransac_options.min_num_trials = 30;
        tvo.ransac_options.max_error = o.init_max_error;
        const py::object pts1 = np_array(c1.xy, 2), pts2 = np_array(c2.xy, 2), marr = MatchesArray(matches);
        PyTwoViewGeometry G;
        bool pose_ok = false;
        if (two_view_solver.is_none()) {
            const py::module_ mod = py::module_::import("pycolmap_amd._pycolmap");
            const py::object geometry = mod.attr("estimate_calibrated_two_view_geometry")(pycam1, pts1, pycam2, pts2, marr, tvo);
            pose_ok = mod.attr("estimate_two_view_geometry_pose")(pycam1, pts1, pycam2, pts2, geometry).cast<bool>();
            G = geometry.cast<PyTwoViewGeometry>();
        } else {
            const py::dict out = two_view_solver(pycam1, pts1, pycam2, pts2, marr, tvo);
            const auto im = py::array_t<uint32_t, py::array::c_style | py::array::forcecast>::ensure(out["inlier_matches"]);
            const auto sq = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(out["qvec"]);
            const auto stv = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(out["tvec"]);
            if (!im || !sq || !stv || im.size() % 2 != 0 || sq.size() != 4 || stv.size() != 3)
                throw py::value_error("register_initial_image_pair: the two-view solver's result does not have the expected shape");
            pose_ok = out["pose_ok"].cast<bool>();
            G.config = out["config"].cast<int>();
            G.inlier_matches.assign(im.data(), im.data() + im.size());
            std::copy(sq.data(), sq.data() + 4, G.cam2_from_cam1.rotation.xyzw.begin());
            std::copy(stv.data(), stv.data() + 3, G.cam2_from_cam1.translation.begin());
            G.tri_angle = out["tri_angle"].cast<double>();
        }
        // everything that can refuse the call has: from here on the trials count
        mp.trials[id1] += 1;
        mp.trials[id2] += 1;
        const size_t num_inliers = G.inlier_matches.size() / 2;
        const double tz = G.cam2_from_cam1.translation[2];
        bool ok = InitialPairAccepted(pose_ok, num_inliers, tz, G.tri_angle, o);
        py::dict last;
        last["image_id1"] = id1;
        last["image_id2"] = id2;
        last["success"] = false;
        last["num_correspondences"] = flat.NumCorrs();
        last["num_inliers"] = num_inliers;
        last["tri_angle"] = G.tri_angle;
        last["translation_z"] = tz;
        last["config"] = G.config;
        last["num_points3D"] = 0;
        double device_ms = 0, kernel_ms = 0, copy_ms = 0;
        uint64_t calls = 0;
        if (ok) {
            for (int k = 0; k < 4; ++k) flat.qvec[4 + k] = G.cam2_from_cam1.rotation.xyzw[k];
            for (int k = 0; k < 3; ++k) flat.tvec[3 + k] = G.cam2_from_cam1.translation[k];
            const size_t n = flat.NumCorrs();
            const double min_tri_angle = kMapperDegToRad * o.init_min_tri_angle;
            std::vector<uint8_t> accepted(n, 0);
            std::vector<double> xyz(3 * n, 0.0);
            if (!pair_solver.is_none()) {
                py::dict d;
                d["camera_models"] = np_array(flat.camera_models, 1);
                d["camera_params"] = np_array(flat.camera_params, 12);
                d["image_cameras"] = np_array(flat.image_cameras, 1);
                d["qvec"] = np_array(flat.qvec, 4);
                d["tvec"] = np_array(flat.tvec, 3);
                d["pair_images"] = np_array(flat.pair_images, 2);
                d["pair_offsets"] = np_array(flat.pair_offsets, 1);
                d["corr_xy1"] = np_array(flat.corr_xy1, 2);
                d["corr_xy2"] = np_array(flat.corr_xy2, 2);
                d["min_tri_angle"] = min_tri_angle;
                const py::dict out = pair_solver(d);
                const auto sa = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>::ensure(out["accepted"]);
                const auto sx = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(out["xyz"]);
                if (!sa || !sx || static_cast<size_t>(sa.size()) != n || static_cast<size_t>(sx.size()) != 3 * n)
                    throw py::value_error("register_initial_image_pair: the solver's result does not have the problem's shape");
                std::copy(sa.data(), sa.data() + n, accepted.begin());
                std::copy(sx.data(), sx.data() + 3 * n, xyz.begin());
            } else {
                const amc_pair_tri_problem pb = flat.Problem();
                amc_pair_tri_opts po;
                amc_pair_tri_opts_default(&po);
                po.min_tri_angle = min_tri_angle;
                amc_pair_tri_result res{};
                call_library([&](amc_ctx* ctx) { return amc_triangulate_pairs(ctx, &pb, &po, &res); }, "amc_triangulate_pairs");
                calls = 1;
                device_ms = res.device_ms;
                kernel_ms = res.kernel_ms;
                copy_ms = res.copy_ms;
                std::copy(res.accepted, res.accepted + n, accepted.begin());
                std::copy(res.xyz, res.xyz + 3 * n, xyz.begin());
                amc_pair_tri_result_free(&res);
            }
            const size_t created = ApplyInitialPair(c1, c2, flat, accepted.data(), xyz.data(), &model, &ix);
            const py::object copy = py::module_::import("copy").attr("copy");
            r.images[py::int_(id1)] = copy(mp.candidate_images.at(id1));
            r.images[py::int_(id2)] = copy(mp.candidate_images.at(id2));
            update_with_new_points(r, model);  // (the created points do not enter the triangulator's modified set, as in COLMAP)
            last["num_points3D"] = created;
            mp.num_total_reg_images += 2;
            mp.reg_image_ids.push_back(id1);
            mp.reg_image_ids.push_back(id2);
            mp.candidate_images.erase(id1);
            mp.candidate_images.erase(id2);
            mp.candidates.erase(id1);
            mp.candidates.erase(id2);
        }
        last["success"] = ok;
        mp.last_pair = last;
        py::dict st;
        st["call"] = "register_initial_image_pair";
        st["num_correspondences"] = flat.NumCorrs();
        st["num_device_calls"] = calls;
        st["device_ms"] = device_ms;
        st["kernel_ms"] = kernel_ms;
        st["copy_ms"] = copy_ms;
        st["host_ms"] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - device_ms;
        py::module_::import("pycolmap_amd._pycolmap").attr("_last_stats") = st;
        return ok;
    };
    // AdjustGlobalBundle with Reconstruction::Normalize (21.3).  solver: None, or BundleAdjuster._solve_with's callable.
    auto adjust_global_bundle_with = [checked_model, update_from_model, adjuster_solve, call_library, checked_mapper_options, sync_reg_image_ids](
                                         PyMapper& mp, const MapperOptions& o, const BundleAdjustmentOptions& ba_options, const py::object& solver) -> bool {
        checked_mapper_options(o);
        sync_reg_image_ids(mp);
        if (mp.reg_image_ids.size() < 2) throw py::value_error(CheckMessage(__FILE__, __LINE__, "reg_image_ids.size() >= 2", "adjust_global_bundle"));
        if (solver.is_none()) call_library(nullptr, "");
        PyReconstruction& r = mp.triangulator.cast<PyTriangulator&>().reconstruction.cast<PyReconstruction&>();
        {
            SparseModel m = checked_model(r);  // "avoid degeneracies in bundle adjustment"
            FilterObservationsWithNegativeDepth(&m);
            update_from_model(r, m);
        }
        PyBundleAdjuster adjuster{ba_options, GlobalBundleConfig(mp.reg_image_ids, mp.existing_image_ids, o.fix_existing_images), py::dict()};
        if (!adjuster_solve(adjuster, r, solver)) return false;
        const py::object stats = py::module_::import("pycolmap_amd._pycolmap").attr("_last_stats");
        SparseModel m = checked_model(r);
        const NormalizeResult nr = NormalizeModel(&m, mp.reg_image_ids);
        update_from_model(r, m);
        py::dict st(stats.attr("copy")());
        st["call"] = "adjust_global_bundle";
        st["normalize_scale"] = nr.scale;
        py::module_::import("pycolmap_amd._pycolmap").attr("_last_stats") = st;
        return true;
    };
    // FilterImages (21.4): host code, no device
    auto filter_images = [checked_model, update_from_model, checked_mapper_options, sync_reg_image_ids](PyMapper& mp, const MapperOptions& o) -> size_t {
        checked_mapper_options(o);
        sync_reg_image_ids(mp);
        PyTriangulator& t = mp.triangulator.cast<PyTriangulator&>();
        PyReconstruction& r = t.reconstruction.cast<PyReconstruction&>();
        SparseModel m = checked_model(r);
        const std::vector<uint32_t> gone = PlanFilterImages(m, mp.reg_image_ids, o);
        if (gone.empty()) return 0;
        for (uint32_t id : gone) DeRegisterImage(&m, id);
        const py::object copy = py::module_::import("copy").attr("copy");
        for (uint32_t id : gone) {
            // the image becomes a candidate again, none of its points2D carrying a point3D
            py::object image = copy(r.images[py::int_(id)]);
            PyImage& im = image.cast<PyImage&>();
            MapperCandidate c;
            c.image_id = id;
            c.camera_id = im.camera_id;
            for (PyPoint2D& p : im.points2D) {
                p.point3D_id = kInvalidPoint3DId;
                c.xy.push_back(p.xy[0]);
                c.xy.push_back(p.xy[1]);
            }
            mp.candidate_images[id] = image;
            mp.candidates[id] = std::move(c);
            mp.filtered_images.insert(id);
            r.images.attr("pop")(py::int_(id));
        }
        update_from_model(r, m);
        std::set<uint64_t> modified;  // points that left the model leave the triangulator's modified set
        for (uint64_t pid : t.modified)
            if (r.points3D.contains(py::int_(pid))) modified.insert(pid);
        t.modified.swap(modified);
        sync_reg_image_ids(mp);
        return gone.size();
    };
    py::class_<PyMapper>(m, "IncrementalMapper")
        .def(py::init([](const py::object& triangulator) {
                 if (!py::isinstance<PyTriangulator>(triangulator)) throw py::type_error("IncrementalMapper(triangulator: IncrementalTriangulator)");
                 PyMapper mp;
                 mp.triangulator = triangulator;
                 // BeginReconstruction: every image the model holds already counts as registered
                 const PyReconstruction& r = triangulator.cast<PyTriangulator&>().reconstruction.cast<PyReconstruction&>();
                 mp.num_total_reg_images = r.images.size();
                 for (auto item : r.images) mp.existing_image_ids.insert(item.first.cast<uint32_t>());
                 mp.reg_image_ids.assign(mp.existing_image_ids.begin(), mp.existing_image_ids.end());
                 return mp;
             }), "triangulator"_a)
        .def("add_candidate", [](PyMapper& mp, const py::object& image) {
                 const PyImage& im = image.cast<const PyImage&>();
                 PyTriangulator& t = mp.triangulator.cast<PyTriangulator&>();
                 const PyReconstruction& r = t.reconstruction.cast<const PyReconstruction&>();
                 const CorrespondenceGraph& graph = t.graph.cast<const CorrespondenceGraph&>();
                 if (im.image_id == 0xFFFFFFFFu) throw py::value_error("add_candidate: the image has no image_id");
                 if (r.images.contains(py::int_(im.image_id))) throw py::value_error("add_candidate: image " + std::to_string(im.image_id) + " is in the reconstruction");
                 if (mp.candidates.count(im.image_id)) throw py::value_error("add_candidate: image " + std::to_string(im.image_id) + " is a candidate already");
                 if (!r.cameras.contains(py::int_(im.camera_id))) throw py::value_error("add_candidate: the reconstruction has no camera " + std::to_string(im.camera_id));
                 if (graph.NumPoints2D(im.image_id) != im.points2D.size())  // an image the graph does not hold: the graph's ValueError
                     throw py::value_error("add_candidate: image " + std::to_string(im.image_id) + " has " + std::to_string(im.points2D.size()) +
                                           " points2D, the graph gives it " + std::to_string(graph.NumPoints2D(im.image_id)));
                 MapperCandidate c;
                 c.image_id = im.image_id;
                 c.camera_id = im.camera_id;
                 for (const PyPoint2D& p : im.points2D) {
                     if (p.point3D_id != kInvalidPoint3DId) throw py::value_error("add_candidate: a point2D of image " + std::to_string(im.image_id) + " carries a point3D");
                     c.xy.push_back(p.xy[0]);
                     c.xy.push_back(p.xy[1]);
                 }
                 mp.candidate_images[im.image_id] = py::module_::import("copy").attr("copy")(image);
                 mp.candidates[im.image_id] = std::move(c);
             }, "image"_a, "An image that may be registered: an Image with points2D, none carrying a point3D, whose camera the reconstruction holds and whose id the graph knows.")
        .def_property_readonly("candidates", [](const PyMapper& mp) {
                 std::vector<uint32_t> ids;
                 for (const auto& kv : mp.candidates) ids.push_back(kv.first);
                 return ids;
             }, "The ids of the candidates, ascending.")
        .def("num_reg_trials", [](const PyMapper& mp, uint32_t image_id) {
                 const auto it = mp.trials.find(image_id);
                 return it == mp.trials.end() ? 0 : it->second;
             }, "image_id"_a)
        .def("num_total_reg_images", [](const PyMapper& mp) { return mp.num_total_reg_images; })
        .def("last_registration", [](const PyMapper& mp) { return py::dict(mp.last.attr("copy")()); },
             "What the last register_next_image call saw: image_id, success, num_visible_points3D, num_pairs, num_inliers, focal_factor,\n"
             "estimate_focal_length, and the two refinement flags COLMAP would have set (the refinement here never refines intrinsics).")
        .def("find_next_images", [find_next_images_with](PyMapper& mp, const MapperOptions& o) { return find_next_images_with(mp, o, py::none()); }, "options"_a,
             "The candidates worth trying next, best first: never-tried ones before the others, each group by descending rank\n"
             "(visible points, their ratio or the visibility pyramid score), on the GPU (DESIGN.md section 20).")
        .def("_find_next_images_with", find_next_images_with, "options"_a, "solver"_a, "find_next_images with a callable in the library's place (test hook).")
        .def("register_next_image", [register_next_image_with](PyMapper& mp, const MapperOptions& o, uint32_t image_id) {
                 return register_next_image_with(mp, o, image_id, py::none());
             }, "options"_a, "image_id"_a,
             "Estimate the pose of a candidate from its 2D-3D correspondences on the GPU, add it to the reconstruction and\n"
             "continue the tracks of its inliers (DESIGN.md section 20).  False changes nothing but the trial count.")
        .def("_register_next_image_with", register_next_image_with, "options"_a, "image_id"_a, "solver"_a,
             "register_next_image with a callable in the library's place (test hook).")
        .def("find_local_bundle", [find_local_bundle_with](PyMapper& mp, const MapperOptions& o, uint32_t image_id) {
                 return find_local_bundle_with(mp, o, image_id, py::none(), AMC_MAPPER_MAX_PAIR_POINTS);
             }, "options"_a, "image_id"_a,
             "The images of the local bundle adjustment around a model image: its most overlapping images with a sufficient\n"
             "75th-percentile triangulation angle, on the GPU (DESIGN.md section 20).  The image itself is not in the list.")
        .def("_find_local_bundle_with", find_local_bundle_with, "options"_a, "image_id"_a, "solver"_a,
             "max_pair_points"_a = static_cast<uint64_t>(AMC_MAPPER_MAX_PAIR_POINTS), "find_local_bundle with a callable in the library's place (test hook).")
        .def_property_readonly("triangulator", [](const PyMapper& mp) { return mp.triangulator; })
        .def_property_readonly("reconstruction", [](const PyMapper& mp) { return mp.triangulator.cast<PyTriangulator&>().reconstruction; })
        .def_property_readonly("correspondence_graph", [](const PyMapper& mp) { return mp.triangulator.cast<PyTriangulator&>().graph; })
        .def("__copy__", [](const PyMapper& mp) {
                 PyMapper c(mp);
                 c.last = py::dict(mp.last.attr("copy")());
                 c.last_pair = py::dict(mp.last_pair.attr("copy")());
                 return c;
             })
        .def("__deepcopy__", [](const PyMapper& mp, const py::dict& memo) {
                 const py::object deepcopy = py::module_::import("copy").attr("deepcopy");
                 PyMapper c(mp);
                 c.triangulator = deepcopy(mp.triangulator, memo);
                 for (auto& kv : c.candidate_images) kv.second = deepcopy(kv.second, memo);
                 c.last = py::dict(mp.last.attr("copy")());
                 c.last_pair = py::dict(mp.last_pair.attr("copy")());
                 return c;
             })
        .def("last_initial_pair", [](const PyMapper& mp) { return py::dict(mp.last_pair.attr("copy")()); },
             "What the last register_initial_image_pair call saw: image_id1, image_id2, success, num_correspondences, num_inliers,\n"
             "tri_angle, translation_z, config and num_points3D (DESIGN.md section 21); empty before the first call.")
        .def_property_readonly("reg_image_ids", [sync_reg_image_ids](PyMapper& mp) {
                 sync_reg_image_ids(mp);
                 return mp.reg_image_ids;
             }, "The registered images in COLMAP's order: those the model held when the mapper was made, ascending, then every\n"
                "registered image in registration order (DESIGN.md section 21).")
        .def_property_readonly("filtered_images", [](const PyMapper& mp) { return std::vector<uint32_t>(mp.filtered_images.begin(), mp.filtered_images.end()); },
             "The ids of the images filter_images removed from the model, ascending.")
        .def("__repr__", [](const PyMapper& mp) {
            const PyReconstruction& r = mp.triangulator.cast<PyTriangulator&>().reconstruction.cast<const PyReconstruction&>();
            return "IncrementalMapper(num_reg_images=" + std::to_string(r.images.size()) + ", num_candidates=" + std::to_string(mp.candidates.size()) +
                   ", num_total_reg_images=" + std::to_string(mp.num_total_reg_images) + ")";
        });

    m.def("register_initial_image_pair", [register_initial_image_pair_with](PyMapper& mp, const MapperOptions& o, uint32_t image_id1, uint32_t image_id2) {
              return register_initial_image_pair_with(mp, o, image_id1, image_id2, py::none(), py::none());
          }, "mapper"_a, "options"_a, "image_id1"_a, "image_id2"_a,
          "Start a model from two candidates of the mapper: estimate their calibrated two-view geometry and relative pose on\n"
          "the GPU, put image 1 at the identity and image 2 at cam2_from_cam1, and triangulate every correspondence the graph\n"
          "holds between them in one device call (DESIGN.md section 21).  False changes nothing but the two trial counts.");
    m.def("_register_initial_image_pair_with", register_initial_image_pair_with, "mapper"_a, "options"_a, "image_id1"_a, "image_id2"_a,
          "two_view_solver"_a, "pair_solver"_a, "register_initial_image_pair with callables in the library's place (test hook; DESIGN.md section 21).");
    m.def("adjust_global_bundle", [adjust_global_bundle_with](PyMapper& mp, const MapperOptions& o, const BundleAdjustmentOptions& ba_options) {
              return adjust_global_bundle_with(mp, o, ba_options, py::none());
          }, "mapper"_a, "options"_a, "ba_options"_a,
          "Adjust every registered image and the points they see on the GPU, the first image's pose and the second's x position\n"
          "held, after deleting the observations with negative depth; then normalise the scene to an extent of 10\n"
          "(DESIGN.md section 21).  False when the model gives no residual.");
    m.def("_adjust_global_bundle_with", adjust_global_bundle_with, "mapper"_a, "options"_a, "ba_options"_a, "solver"_a,
          "adjust_global_bundle with a callable in the library's place (test hook; DESIGN.md section 21).");
    m.def("filter_images", filter_images, "mapper"_a, "options"_a,
          "From 20 registered images on, remove every registered image that sees no point3D or whose camera has bogus\n"
          "parameters: it leaves the reconstruction with its observations and becomes a candidate again (DESIGN.md section 21).\n"
          "Returns the number of images removed.  Host code: it needs no GPU.");
    m.def("_normalize_model", [checked_model, update_from_model](PyReconstruction& r, const std::vector<uint32_t>& reg_image_ids, double extent, double p0, double p1) {
              SparseModel model = checked_model(r);
              const NormalizeResult nr = NormalizeModel(&model, reg_image_ids, extent, p0, p1);
              update_from_model(r, model);
              return py::make_tuple(nr.applied, nr.scale, std::array<double, 3>{{nr.centroid[0], nr.centroid[1], nr.centroid[2]}});
          }, "reconstruction"_a, "reg_image_ids"_a, "extent"_a = 10.0, "p0"_a = 0.1, "p1"_a = 0.9,
          "adjust_global_bundle's normalisation on its own: (applied, scale, centroid) (test hook; DESIGN.md section 21).");

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

    // ---- Database ---------------------------------------------------------------------------
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
        .def("read_camera", [camera_from_row](const Database& db, camera_t id) { return camera_from_row(db.ReadCamera(id)); },
             "camera_id"_a)
        .def("read_all_cameras",
             [camera_from_row](const Database& db) {
                 std::vector<PyCamera> out;
                 for (const CameraRow& r : db.ReadAllCameras()) out.push_back(camera_from_row(r));
                 return out;
             })
        .def("read_image", [image_from_row](const Database& db, image_t id) { return image_from_row(db.ReadImage(id)); },
             "image_id"_a)
        .def("read_image_with_name",
             [image_from_row](const Database& db, const std::string& name) { return image_from_row(db.ReadImageWithName(name)); },
             "name"_a)
        .def("read_all_images",
             [image_from_row](const Database& db) {
                 std::vector<PyImage> out;
                 for (const ImageRow& r : db.ReadAllImages()) out.push_back(image_from_row(r));
                 return out;
             })
        .def("write_camera",
             [row_from_camera](Database& db, const PyCamera& c, bool use_camera_id) {
                 return db.WriteCamera(row_from_camera(c), use_camera_id);
             },
             "camera"_a, "use_camera_id"_a = false, "Returns the camera_id of the new row.")
        .def("write_image",
             [row_from_image](Database& db, const PyImage& im, bool use_image_id) {
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
    py::class_<PyDbTransaction>(m, "DatabaseTransaction")
        .def(py::init<Database*>(), "database"_a, py::keep_alive<1, 2>())
        .def("__enter__", [](PyDbTransaction& t) -> PyDbTransaction& { return t; }, py::return_value_policy::reference)
        .def("__exit__", [](PyDbTransaction& t, const py::object& type, const py::object&, const py::object&) {
            t.End(type.is_none());
            return false;
        });

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
        py::module_::import("pycolmap_amd._pycolmap").attr("_last_stats") = st;
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
