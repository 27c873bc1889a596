// binding_support.h — what every binding file (module.cc, bind_*.cc) shares: path and device checks, the option
// "dataclass" protocol, vector -> numpy, the last-call statistics, the logging sink, the estimator context and the one
// path every library call of the scene bindings takes (CallLibrary).  Everything here is inline.
//
// Mirrors:
//   Device enum + GPU parameter check                       /root/reference/pycolmap/utils.h:9-31, main.cc:102-106
//   option "dataclass" protocol (summary/todict/mergedict, dict/kwargs ctors, implicit dict
//   conversion, copy, pickle)                               /root/reference/pycolmap/helpers.h:217-283
//   pycolmap.logging                                        /root/reference/pycolmap/main.cc:39-89
#pragma once
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <chrono>
#include <fstream>
#include <functional>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../../include/amc.h"
#include "py_types.h"
#include "result_guard.h"

namespace amchost {
using namespace pybind11::literals;

enum class Device { AUTO = -1, CPU = 0, CUDA = 1 };

inline std::string PathToString(const py::object& p) {
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
inline void RequireAccelerator(Device d) {
    if (d == Device::CPU)
        throw py::value_error(
            "pycolmap_amd implements the accelerated (MI355X) matcher only and has no CPU fallback; "
            "set device='auto' or device='cuda', or use the reference pycolmap for device='cpu'.");
}

// ---- option "dataclass" protocol --------------------------------------------------------------
inline void MergeDict(py::object self, const py::dict& d, const std::vector<std::string>& fields) {
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
inline py::dict ToDict(const py::object& self, const std::vector<std::string>& fields, bool recursive = true) {
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
inline std::string Summary(const py::object& self, const std::vector<std::string>& fields, bool write_type) {
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
inline void AddDefaultsToDocstrings(const py::object& cls, const std::vector<std::string>& fields) {
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

// ---- small things every entry point repeats ------------------------------------------------------
// a flat vector as a (size / cols) x cols array of its element type
template <typename V>
py::array_t<typename V::value_type> NpArray(const V& v, py::ssize_t cols) {
    py::array_t<typename V::value_type> a({static_cast<py::ssize_t>(v.size()) / cols, cols});
    std::copy(v.begin(), v.end(), a.mutable_data());
    return a;
}
// what last_run_stats() returns
inline void SetLastStats(const py::dict& st) { py::module_::import("pycolmap_amd._pycolmap").attr("_last_stats") = st; }
// the host's share of a call that began at t0: the wall time so far less the device's
inline double HostMs(std::chrono::steady_clock::time_point t0, double device_ms) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - device_ms;
}
// the timing tail of an entry point's statistics, in their order; then the statistics become last_run_stats()
inline void FinishStats(py::dict& st, std::chrono::steady_clock::time_point t0, double device_ms, double kernel_ms, double copy_ms) {
    st["device_ms"] = device_ms;
    st["kernel_ms"] = kernel_ms;
    st["copy_ms"] = copy_ms;
    st["host_ms"] = HostMs(t0, device_ms);
    SetLastStats(st);
}
// the cameras and poses every flat problem begins with, as the first entries of the dict a solver hook receives
template <typename Flat>
py::dict CamerasAndPosesDict(const Flat& flat) {
    py::dict d;
    d["camera_models"] = NpArray(flat.camera_models, 1);
    d["camera_params"] = NpArray(flat.camera_params, 12);
    d["image_cameras"] = NpArray(flat.image_cameras, 1);
    d["qvec"] = NpArray(flat.qvec, 4);
    d["tvec"] = NpArray(flat.tvec, 3);
    return d;
}

// ---- pycolmap.logging (/root/reference/pycolmap/main.cc:39-89): the glog front end the reference exposes -
// flags, per-severity destinations, info / warning / error / fatal stamped with the Python call site.  There is no
// glog here; the few lines it amounts to for this surface are written out in module.cc, which also defines the static
// members: glog's line format, severity filtering by minloglevel / stderrthreshold, optional files.
struct Logging {
    enum Level { INFO = 0, WARNING = 1, ERROR = 2, FATAL = 3 };
    static int minloglevel, stderrthreshold;
    static std::string log_dir;
    static bool logtostderr, alsologtostderr;
    static std::string destination[4];
    static std::mutex mu;
    static void Write(Level lv, const std::string& where, int line, const std::string& msg);
};
// "file:function" and the line of the Python frame that called into the module
std::pair<std::string, int> PythonCallFrame();

// ---- one lazily created context for the single calls (device 0) ------------------------------------
struct EstimatorCtx {
    std::mutex mu;
    amc_ctx* ctx = nullptr;
    amc_ctx* Get() {
        if (!ctx) {
            const int rc = amc_ctx_create(0, &ctx);
            if (rc != AMC_OK) throw std::runtime_error(std::string("amc_ctx_create: ") + amc_last_error());
            if (amc_ctx_reserve_slots(ctx, 2) != AMC_OK)
                throw std::runtime_error(std::string("amc_ctx_reserve_slots: ") + amc_last_error());
        }
        return ctx;
    }
};
// one inline function: every translation unit shares the one context and its mutex
inline EstimatorCtx& TheEstimatorCtx() {
    static EstimatorCtx* e = new EstimatorCtx();  // intentionally leaked: no HIP calls at interpreter exit
    return *e;
}
inline void EstCheck(int rc, const char* what) {
    if (rc == AMC_OK) return;
    const std::string msg = std::string(what) + ": " + amc_last_error();
    if (rc == AMC_E_INVALID) throw std::invalid_argument(msg);
    throw std::runtime_error(msg);
}
// One library call under the estimator context's lock with the GIL released; fn == nullptr only takes the device.
// AMC_E_INVALID becomes ValueError (through invalid_argument), every other failure, a missing device among them,
// pycolmap_amd._capi.AmcError.
inline void CallLibrary(const std::function<int(amc_ctx*)>& fn, const char* name) {
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
}

}  // namespace amchost
