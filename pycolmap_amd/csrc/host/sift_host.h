// sift_host.h — SiftExtractionOptions and the Sift extractor of the host layer, over libamc.so's amc_sift_* C ABI
// (include/amc_sift.h).  Mirrors /root/reference/pycolmap/feature/sift.h and pipeline/extract_features.h:71-138.
#pragma once
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <cstdint>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>

#include "../../../include/amc_sift.h"

namespace amchost {
namespace py = pybind11;

// COLMAP 3.9.1's SiftExtractionOptions with its defaults; every field is bound, the extractor reads those of
// amc_sift_opts and refuses the ones it does not implement (affine shape, domain-size pooling, darkness adaptivity)
struct SiftExtractionOptions {
    enum class Normalization { L1_ROOT = 0, L2 = 1 };
    int num_threads = -1;
    std::string gpu_index = "-1";
    int max_image_size = 3200;
    int max_num_features = 8192;
    int first_octave = -1;
    int num_octaves = 4;
    int octave_resolution = 3;
    double peak_threshold = 0.02 / 3;
    double edge_threshold = 10.0;
    bool estimate_affine_shape = false;
    int max_num_orientations = 2;
    bool upright = false;
    bool darkness_adaptivity = false;
    bool domain_size_pooling = false;
    double dsp_min_scale = 1.0 / 6.0;
    double dsp_max_scale = 3.0;
    int dsp_num_scales = 10;
    Normalization normalization = Normalization::L1_ROOT;

    // ValueError naming the first option the GPU extractor does not implement or an out-of-range value
    void Check() const {
        if (estimate_affine_shape) throw py::value_error("SiftExtractionOptions.estimate_affine_shape is not supported by pycolmap_amd's extractor");
        if (domain_size_pooling) throw py::value_error("SiftExtractionOptions.domain_size_pooling is not supported by pycolmap_amd's extractor");
        if (darkness_adaptivity) throw py::value_error("SiftExtractionOptions.darkness_adaptivity is not supported by pycolmap_amd's extractor");
        if (max_image_size < 1) throw py::value_error("SiftExtractionOptions.max_image_size must be positive");
        if (first_octave < -1) throw py::value_error("SiftExtractionOptions.first_octave must be >= -1");
        if (num_octaves < 1 || octave_resolution < 1) throw py::value_error("SiftExtractionOptions.num_octaves and octave_resolution must be positive");
        if (max_num_orientations < 1) throw py::value_error("SiftExtractionOptions.max_num_orientations must be positive");
        if (!(peak_threshold >= 0.0) || !(edge_threshold > 0.0)) throw py::value_error("SiftExtractionOptions.peak_threshold / edge_threshold out of range");
    }
    amc_sift_opts ToAmc() const {
        amc_sift_opts o;
        amc_sift_opts_default(&o);
        o.first_octave = first_octave;
        o.num_octaves = num_octaves;
        o.octave_resolution = octave_resolution;
        o.peak_threshold = peak_threshold;
        o.edge_threshold = edge_threshold;
        o.max_num_orientations = max_num_orientations;
        o.upright = upright ? 1 : 0;
        o.normalization = normalization == Normalization::L2 ? AMC_SIFT_L2 : AMC_SIFT_L1_ROOT;
        o.max_num_features = max_num_features;
        o.max_image_size = max_image_size;
        return o;
    }
};

// ImageReaderOptions (/root/reference/pycolmap/pipeline/images.h:158-201; COLMAP 3.9.1's defaults) and CameraMode (:151-156)
struct ImageReaderOptions {
    std::string camera_model = "SIMPLE_RADIAL";
    std::string mask_path;
    int existing_camera_id = -1;
    std::string camera_params;
    double default_focal_length_factor = 1.2;
    std::string camera_mask_path;
};
enum class CameraMode { AUTO = 0, SINGLE = 1, PER_FOLDER = 2, PER_IMAGE = 3 };

// The device a Sift object extracts on: gpu_index "-1" is device 0, otherwise the first listed index
inline int SiftDeviceIndex(const std::string& gpu_index) {
    const std::string first = gpu_index.substr(0, gpu_index.find(','));
    int d = 0;
    try {
        d = std::stoi(first);
    } catch (const std::exception&) {
        throw py::value_error("SiftExtractionOptions.gpu_index: '" + gpu_index + "' is not a list of device indices");
    }
    return d < 0 ? 0 : d;
}

class SiftExtractor {
   public:
    explicit SiftExtractor(SiftExtractionOptions options) : options_(std::move(options)) { options_.Check(); }
    ~SiftExtractor() {
        if (ctx_) amc_ctx_destroy(ctx_);
    }
    SiftExtractor(const SiftExtractor&) = delete;
    SiftExtractor& operator=(const SiftExtractor&) = delete;

    const SiftExtractionOptions& Options() const { return options_; }

    // (N x 4 float32 keypoints, N x 128 float32 descriptors = bytes / 512), as the reference's Sift::Extract
    py::tuple Extract(py::array_t<uint8_t, 0> image) {
        if (image.ndim() != 2) throw py::value_error("Sift.extract: the image must be 2-D (grey)");
        const py::ssize_t h = image.shape(0), w = image.shape(1);
        if (h > options_.max_image_size || w > options_.max_image_size)
            throw py::value_error("Sift.extract: the image is " + std::to_string(w) + " x " + std::to_string(h) +
                                  ", larger than max_image_size " + std::to_string(options_.max_image_size));
        // a copy with unit column stride (the C ABI takes a row pitch)
        py::array_t<uint8_t, py::array::c_style> img = py::array_t<uint8_t, py::array::c_style>::ensure(image);
        amc_sift_image im{img.data(), (int32_t)w, (int32_t)h, (int64_t)w};
        const amc_sift_opts o = options_.ToAmc();
        const int device = SiftDeviceIndex(options_.gpu_index);
        amc_sift_result r{};
        int rc;
        {
            py::gil_scoped_release release;
            std::lock_guard<std::mutex> lock(mu_);
            rc = EnsureCtx(device);
            if (rc == AMC_OK) rc = amc_sift_extract(ctx_, &im, h && w ? 1 : 0, &o, &r);
        }
        if (rc != AMC_OK) {
            const std::string msg = std::string("Sift.extract: ") + amc_last_error();
            if (rc == AMC_E_INVALID) throw py::value_error(msg);
            throw std::runtime_error(msg);
        }
        const size_t n = (h && w) ? (size_t)r.offsets[1] : 0;
        py::array_t<float> kp({(py::ssize_t)n, (py::ssize_t)4});
        py::array_t<float> desc({(py::ssize_t)n, (py::ssize_t)128});
        float* kd = kp.mutable_data();
        float* dd = desc.mutable_data();
        for (size_t i = 0; i < n * 4; ++i) kd[i] = r.keypoints[i];
        for (size_t i = 0; i < n * 128; ++i) dd[i] = (float)r.descriptors[i] / 512.0f;
        last_device_ms_ = r.device_ms;
        amc_sift_result_free(&r);
        return py::make_tuple(kp, desc);
    }

    // (image * 255).cast<uint8_t>() of the reference, defined for every input: NaN -> 0, clamped to [0, 255], then
    // truncated
    py::tuple ExtractFloat(py::array_t<float, 0> image) {
        if (image.ndim() != 2) throw py::value_error("Sift.extract: the image must be 2-D (grey)");
        const py::ssize_t h = image.shape(0), w = image.shape(1);
        py::array_t<uint8_t> u8({h, w});
        auto src = image.unchecked<2>();
        auto dst = u8.mutable_unchecked<2>();
        for (py::ssize_t y = 0; y < h; ++y)
            for (py::ssize_t x = 0; x < w; ++x) {
                const float v = src(y, x) * 255.0f;
                dst(y, x) = (uint8_t)(v >= 255.0f ? 255.0f : v > 0.0f ? v : 0.0f);
            }
        return Extract(u8);
    }

    double LastDeviceMs() const { return last_device_ms_; }

   private:
    int EnsureCtx(int device) {
        if (ctx_) return AMC_OK;
        return amc_ctx_create(device, &ctx_);
    }
    SiftExtractionOptions options_;
    amc_ctx* ctx_ = nullptr;
    std::mutex mu_;
    double last_device_ms_ = 0.0;
};

}  // namespace amchost
