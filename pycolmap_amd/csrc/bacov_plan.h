// bacov_plan.h — the host half of the bundle-adjustment covariance: the checks of amc_bacov_opts, the
// compact column map, the (point, owner) slots and, per destination block of the reduced matrix, the slot pairs whose
// terms it subtracts, in ascending point index.  The problem's own checks and orders are ba_plan.h's.  No HIP here:
// tests/shim/bacov_plan_fuzz.cc runs it under ASan + UBSan.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "ba_plan.h"
#include "../../include/amc_bacov.h"

namespace amc {
namespace bacov {

constexpr int kP = cam::kMaxParams;  // 12

struct Plan {
    ba::Plan ba;
    uint32_t m = 0;                             // columns
    uint32_t nown = 0;                          // owners: the images, then the cameras
    std::vector<uint32_t> ocol;                 // nown + 1: an owner's first column
    std::vector<uint32_t> col_owner, col_coord; // m each
    std::vector<int32_t> icol, ccol;            // 6 per image, 12 per camera: the coordinate's column, or -1
    // slots: per variable point, its owners that have a column: images in point order, then cameras ascending
    std::vector<uint32_t> spo;                  // npts + 1: a point's first slot
    std::vector<uint32_t> slot_owner, slot_point;
    // destination blocks (owner A >= owner B sharing a variable point), in ascending (A, B); a block's pairs of slots in
    // ascending point index
    std::vector<uint32_t> dest_a, dest_b, dest_off, pair_a, pair_b;
};

inline std::string check_options(const amc_bacov_opts& o) {
    if (o.loss_function_type < 0 || o.loss_function_type > 2) return "loss_function_type in 0 .. 2";
    if (!(o.loss_function_scale > 0.0) || !(o.loss_function_scale - o.loss_function_scale == 0.0))
        return "loss_function_scale > 0 and finite";
    if (!(o.damping >= 0.0) || !(o.damping - o.damping == 0.0)) return "damping >= 0 and finite";
    return std::string();
}

// Checks the problem (ba::make_plan) and fills the plan; returns what is wrong, or the empty string.  The slots and the
// destination blocks are left empty when m == 0 or m > AMC_BACOV_MAX_COLUMNS (the caller ends the call there).
inline std::string make_plan(const amc_ba_problem& pb, const uint8_t* point_const, Plan* plan) {
    Plan& p = *plan;
    p = Plan();
    std::string bad = ba::make_plan(pb, point_const, &p.ba);
    if (!bad.empty()) return bad;
    const size_t ncam = pb.num_cameras, nimg = pb.num_images, npts = pb.num_points;
    p.nown = (uint32_t)(nimg + ncam);
    p.ocol.assign(p.nown + 1, 0);
    p.icol.assign(6 * nimg, -1);
    p.ccol.assign(kP * ncam, -1);
    uint64_t m = 0;
    for (size_t i = 0; i < nimg; ++i) {
        p.ocol[i] = (uint32_t)m;
        for (int k = 0; k < 6; ++k)
            if (p.ba.ivar[6 * i + k]) ++m;
    }
    for (size_t c = 0; c < ncam; ++c) {
        p.ocol[nimg + c] = (uint32_t)m;
        for (int k = 0; k < kP; ++k)
            if (p.ba.cvar[kP * c + k]) ++m;
    }
    p.ocol[p.nown] = (uint32_t)m;
    p.m = (uint32_t)m;
    if (m == 0 || m > AMC_BACOV_MAX_COLUMNS) return std::string();
    p.col_owner.reserve(m);
    p.col_coord.reserve(m);
    for (size_t i = 0; i < nimg; ++i)
        for (int k = 0; k < 6; ++k)
            if (p.ba.ivar[6 * i + k]) {
                p.icol[6 * i + k] = (int32_t)p.col_owner.size();
                p.col_owner.push_back((uint32_t)i);
                p.col_coord.push_back((uint32_t)k);
            }
    for (size_t c = 0; c < ncam; ++c)
        for (int k = 0; k < kP; ++k)
            if (p.ba.cvar[kP * c + k]) {
                p.ccol[kP * c + k] = (int32_t)p.col_owner.size();
                p.col_owner.push_back((uint32_t)(nimg + c));
                p.col_coord.push_back((uint32_t)k);
            }
    // slots
    p.spo.assign(npts + 1, 0);
    std::vector<uint32_t> seen(p.nown, 0xffffffffu), cams;
    uint64_t npairs = 0;
    for (size_t j = 0; j < npts; ++j) {
        p.spo[j] = (uint32_t)p.slot_owner.size();
        if (!p.ba.pvar[j]) continue;
        cams.clear();
        for (uint32_t k = p.ba.poff[j]; k < p.ba.poff[j + 1]; ++k) {
            const uint32_t i = p.ba.oimg[p.ba.pobs[k]];
            const uint32_t c = (uint32_t)nimg + pb.image_cameras[i];
            if (seen[i] != j) {
                seen[i] = (uint32_t)j;
                if (p.ocol[i + 1] > p.ocol[i]) {
                    p.slot_owner.push_back(i);
                    p.slot_point.push_back((uint32_t)j);
                }
            }
            if (seen[c] != j) {
                seen[c] = (uint32_t)j;
                if (p.ocol[c + 1] > p.ocol[c]) cams.push_back(c);
            }
        }
        std::sort(cams.begin(), cams.end());
        for (uint32_t c : cams) {
            p.slot_owner.push_back(c);
            p.slot_point.push_back((uint32_t)j);
        }
        const uint64_t n = p.slot_owner.size() - p.spo[j];
        npairs += n * (n + 1) / 2;
        if (p.slot_owner.size() > 0x7fffffffu / 128 || npairs > 0x7fffffffu / 8)
            return "the problem is too large for 32-bit offsets";
    }
    p.spo[npts] = (uint32_t)p.slot_owner.size();
    // destination blocks: the pairs keyed by (A, B), a stable counting sort by key keeps the ascending point index
    struct Pair {
        uint64_t key;
        uint32_t a, b;
    };
    std::vector<Pair> pairs;
    pairs.reserve(npairs);
    for (size_t j = 0; j < npts; ++j)
        for (uint32_t x = p.spo[j]; x < p.spo[j + 1]; ++x)
            for (uint32_t y = p.spo[j]; y < p.spo[j + 1]; ++y) {
                const uint32_t A = p.slot_owner[x], B = p.slot_owner[y];
                if (A >= B) pairs.push_back({(uint64_t)A * p.nown + B, x, y});
            }
    std::stable_sort(pairs.begin(), pairs.end(), [](const Pair& l, const Pair& r) { return l.key < r.key; });
    p.pair_a.resize(pairs.size());
    p.pair_b.resize(pairs.size());
    for (size_t t = 0; t < pairs.size(); ++t) {
        if (t == 0 || pairs[t].key != pairs[t - 1].key) {
            p.dest_a.push_back((uint32_t)(pairs[t].key / p.nown));
            p.dest_b.push_back((uint32_t)(pairs[t].key % p.nown));
            p.dest_off.push_back((uint32_t)t);
        }
        p.pair_a[t] = pairs[t].a;
        p.pair_b[t] = pairs[t].b;
    }
    p.dest_off.push_back((uint32_t)pairs.size());
    return std::string();
}

}  // namespace bacov
}  // namespace amc
