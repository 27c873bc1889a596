// abspose_plan.h — the host half of absolute pose: option checks, the focal-length
// factors, the per-(query, factor) problems with their scaled cameras and thresholds, the lift of the pixels that needs
// host libm, the dynamic trial-count rows and the mt19937(0) sample stream.  Host libm only.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <mutex>
#include <random>
#include <string>
#include <vector>

#include "camera_math.h"
#include "../../include/amc_abspose.h"

namespace amc {
namespace ap {

constexpr uint64_t kNoRow = ~(uint64_t)0;
constexpr int kMinSamples = 3;  // P3P: ComputeNumTrials' kMinNumSamples (tvg_math.h)

// AbsolutePoseEstimationOptions::Check + RANSACOptions::Check; empty string = valid
inline std::string check_estimation(const amc_abspose_opts& o) {
    if (!(o.num_focal_length_samples > 0)) return "num_focal_length_samples > 0";
    if (!(o.min_focal_length_ratio > 0)) return "min_focal_length_ratio > 0";
    if (!(o.max_focal_length_ratio > 0)) return "max_focal_length_ratio > 0";
    if (!(o.min_focal_length_ratio < o.max_focal_length_ratio)) return "min_focal_length_ratio < max_focal_length_ratio";
    if (!(o.max_error > 0)) return "max_error > 0";
    if (!(o.min_inlier_ratio >= 0) || !(o.min_inlier_ratio <= 1)) return "0 <= min_inlier_ratio <= 1";
    if (!(o.confidence >= 0) || !(o.confidence <= 1)) return "0 <= confidence <= 1";
    if (o.min_num_trials < 0 || o.max_num_trials < 0 || o.min_num_trials > o.max_num_trials)
        return "0 <= min_num_trials <= max_num_trials";
    return std::string();
}
inline std::string check_refinement(const amc_abspose_refine_opts& o) {
    if (!(o.gradient_tolerance >= 0)) return "gradient_tolerance >= 0";
    if (o.max_num_iterations < 0) return "max_num_iterations >= 0";
    if (!(o.loss_function_scale >= 0)) return "loss_function_scale >= 0";
    if (o.refine_focal_length) return "refine_focal_length is not supported (DESIGN.md 12, A11)";
    if (o.refine_extra_params) return "refine_extra_params is not supported (DESIGN.md 12, A11)";
    return std::string();
}

// EstimateAbsolutePose's focal-length factors: the literal floating loop (host double arithmetic), or just 1
inline std::vector<double> focal_factors(const amc_abspose_opts& o) {
    std::vector<double> f;
    if (!o.estimate_focal_length) {
        f.push_back(1.0);
        return f;
    }
    for (double x = 0; x <= 1.0; x += 1.0 / o.num_focal_length_samples)
        f.push_back(o.min_focal_length_ratio + (o.max_focal_length_ratio - o.min_focal_length_ratio) * x * x);
    return f;
}

// the camera with its focal lengths multiplied by `factor` (kMaxParams doubles)
inline void scaled_params(int model, const double* p, double factor, double* out) {
    for (int i = 0; i < cam::kMaxParams; ++i) out[i] = i < cam::num_params(model) ? p[i] : 0.0;
    for (int i = 0; i < cam::num_focal(model); ++i) out[i] *= factor;
}

// the first `need` words of std::mt19937(0) (operator() output, tempered), kept and extended across calls
inline std::vector<uint32_t> sample_stream_words(size_t need) {
    static std::mutex mu;
    static std::vector<uint32_t> words;
    static std::mt19937 gen(0);
    std::lock_guard<std::mutex> lock(mu);
    while (words.size() < need) words.push_back(static_cast<uint32_t>(gen()));
    return std::vector<uint32_t>(words.begin(), words.begin() + need);
}

// the first stream length a call tries: three draws per trial for twice the trials a RANSAC can run before its
// minimum count binds, capped by the trial limit; an overrun reruns the batch on a table twice as long
inline size_t initial_stream_len(uint64_t min_trials, uint64_t max_trials) {
    const uint64_t t = std::min<uint64_t>(max_trials, std::max<uint64_t>(min_trials, 1000) * 2);
    return (size_t)(3 * t + 1024);
}

}  // namespace ap
}  // namespace amc
