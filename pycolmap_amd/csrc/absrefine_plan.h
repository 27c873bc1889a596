// absrefine_plan.h — the host half of the joint pose and camera refinement: the checks an entry makes
// before it touches the device, the split of a call into device batches, and each batch's launch classes (the queries
// of one column count NV, largest first).  Host C++ only, no HIP: tests/shim/absrefine_plan_fuzz.cc runs it under the
// sanitizers.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "camera_math.h"
#include "../../include/amc_absrefine.h"

namespace amc {
namespace apr {

constexpr uint64_t kMaxBatchQueries = (uint64_t)1 << 16;  // 12.11's bounds
constexpr uint64_t kMaxBatchCorr = (uint64_t)1 << 22;
constexpr int kMaxNV = 10;

// AbsolutePoseRefinementOptions::Check; the two flags are honoured here.  Empty string = valid
inline std::string check_refinement(const amc_abspose_refine_opts& o) {
    if (!(o.gradient_tolerance >= 0)) return "gradient_tolerance >= 0";
    if (o.max_num_iterations < 0) return "max_num_iterations >= 0";
    if (!(o.loss_function_scale >= 0)) return "loss_function_scale >= 0";
    return std::string();
}

// the arrays of a call; empty string = valid.  NaN and infinity in the data are not looked at: they fail a query.
inline std::string check_input(bool estimate, const uint64_t* offsets, size_t nq, const int32_t* models,
                               const double* cparams, const double* points2D, const double* points3D,
                               const double* init_q, const double* init_t, const uint8_t* mask) {
    char buf[128];
    if (!offsets) return "NULL argument";
    if (offsets[0] != 0) return "offsets[0] != 0";
    for (size_t i = 0; i < nq; ++i) {
        if (offsets[i + 1] < offsets[i]) {
            std::snprintf(buf, sizeof buf, "offsets decrease at query %zu", i);
            return buf;
        }
        if (offsets[i + 1] - offsets[i] > 0xffffffffull) {
            std::snprintf(buf, sizeof buf, "query %zu has more than 2^32 - 1 correspondences", i);
            return buf;
        }
    }
    const uint64_t ncorr = offsets[nq];
    if (nq && (!models || !cparams)) return "NULL cameras";
    if (ncorr && (!points2D || !points3D)) return "NULL points";
    if (!estimate && nq && (!init_q || !init_t)) return "NULL initial poses";
    if (!estimate && ncorr && !mask) return "NULL inlier mask";
    for (size_t i = 0; i < nq; ++i)
        if (models[i] < 0 || models[i] >= cam::kNumModels) {
            std::snprintf(buf, sizeof buf, "query %zu has camera model %d", i, (int)models[i]);
            return buf;
        }
    return std::string();
}

// the number of variable camera columns of a model under the two flags (25.1)
inline int num_variable(int model, bool refine_focal, bool refine_extra) {
    return (refine_focal ? cam::num_focal(model) : 0) +
           (refine_extra ? cam::num_params(model) - cam::num_focal(model) - 2 : 0);
}

// contiguous batches: at most max_queries queries and max_corr correspondences each, greedily; a larger query is a
// batch of its own.  Returns the first query of each batch, then nq.
inline std::vector<size_t> plan_batches(const uint64_t* offsets, size_t nq, uint64_t max_queries, uint64_t max_corr) {
    std::vector<size_t> start{0};
    for (size_t i = 0; i < nq;) {
        size_t j = i + 1;
        while (j < nq && j - i < max_queries && offsets[j + 1] - offsets[i] <= max_corr) ++j;
        start.push_back(j);
        i = j;
    }
    return start;
}

// one batch's launches: order holds the batch-local query indices class by class (NV ascending), each class's largest
// queries first (stable); begin[nv] .. begin[nv + 1] is class nv's stretch of it
struct BatchClasses {
    std::vector<uint32_t> order;
    std::array<uint32_t, kMaxNV + 2> begin{};
};
inline BatchClasses plan_classes(const uint64_t* offsets, const int32_t* models, size_t q0, size_t q1,
                                 bool refine_focal, bool refine_extra) {
    BatchClasses c;
    const size_t bq = q1 - q0;
    std::vector<int> nv(bq);
    for (size_t i = 0; i < bq; ++i) nv[i] = num_variable(models[q0 + i], refine_focal, refine_extra);
    c.order.resize(bq);
    for (size_t i = 0; i < bq; ++i) c.order[i] = (uint32_t)i;
    auto len = [&](uint32_t i) { return offsets[q0 + i + 1] - offsets[q0 + i]; };
    std::stable_sort(c.order.begin(), c.order.end(),
                     [&](uint32_t a, uint32_t b) { return nv[a] != nv[b] ? nv[a] < nv[b] : len(a) > len(b); });
    size_t at = 0;
    for (int k = 0; k <= kMaxNV; ++k) {
        c.begin[k] = (uint32_t)at;
        while (at < bq && nv[c.order[at]] == k) ++at;
    }
    c.begin[kMaxNV + 1] = (uint32_t)at;
    return c;
}

}  // namespace apr
}  // namespace amc
