// absrefine_plan_fuzz.cc — a stand-alone program for tests/test_pose_intrinsics_cpu.py (built with
// -fsanitize=address,undefined and run): the host half of the joint pose and camera refinement (csrc/absrefine_plan.h)
// on seeded random calls.  The arrays are heap blocks of exactly the stated sizes, so a read past an array's end is an
// ASan report.  Every valid call's plan is checked against DESIGN.md 25.4: the batches are contiguous, cover the queries
// once and keep the two bounds (a query above the correspondence bound is a batch of its own); a batch's order is a
// permutation of its queries, class by class in ascending column count, each class's longest queries first and equal
// lengths in input order.  Every corrupted call (offsets that do not start at zero or decrease, an unknown model, a
// missing array) is refused before anything is read through it.  Prints "ok <calls> <batches> <launches>".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

#include "../../pycolmap_amd/csrc/absrefine_plan.h"

namespace {

int fail(const char* what, int call) {
    std::printf("FAIL %s (call %d)\n", what, call);
    return 1;
}

}  // namespace

int main() {
    using namespace amc;
    std::mt19937 rng(7);
    long batches = 0, launches = 0;
    const int calls = 400;
    for (int c = 0; c < calls; ++c) {
        const size_t nq = rng() % 40;
        std::vector<uint64_t> off(nq + 1, 0);
        std::vector<int32_t> models(nq);
        for (size_t i = 0; i < nq; ++i) {
            off[i + 1] = off[i] + (rng() % 5 == 0 ? 0 : rng() % 70);
            models[i] = (int32_t)(rng() % cam::kNumModels);
        }
        const uint64_t n = off[nq];
        std::vector<double> prm(nq * 12 + 1, 1.0), p2(2 * n + 1), p3(3 * n + 1), q(4 * nq + 1), t(3 * nq + 1);
        std::vector<uint8_t> mask(n + 1, 1);
        const bool estimate = rng() % 2 != 0;
        if (!apr::check_input(estimate, off.data(), nq, models.data(), prm.data(), p2.data(), p3.data(), q.data(), t.data(),
                              mask.data()).empty())
            return fail("a valid call is refused", c);
        // corruptions
        if (nq > 0) {
            std::vector<uint64_t> bad = off;
            bad[0] = 1;
            if (apr::check_input(estimate, bad.data(), nq, models.data(), prm.data(), p2.data(), p3.data(), q.data(), t.data(),
                                 mask.data()).empty())
                return fail("offsets[0] != 0 accepted", c);
            if (n > 0) {
                bad = off;
                size_t i = nq - 1;  // the last query that has correspondences
                while (bad[i + 1] == bad[i]) --i;
                if (bad[i] > 0) bad[i + 1] = bad[i] - 1;
                if (bad[i + 1] < bad[i] &&
                    apr::check_input(estimate, bad.data(), nq, models.data(), prm.data(), p2.data(), p3.data(), q.data(),
                                     t.data(), mask.data()).empty())
                    return fail("decreasing offsets accepted", c);
            }
            std::vector<int32_t> bm = models;
            bm[rng() % nq] = rng() % 2 ? 11 : -1;
            if (apr::check_input(estimate, off.data(), nq, bm.data(), prm.data(), p2.data(), p3.data(), q.data(), t.data(),
                                 mask.data()).empty())
                return fail("an unknown model accepted", c);
            if (apr::check_input(estimate, off.data(), nq, nullptr, prm.data(), p2.data(), p3.data(), q.data(), t.data(),
                                 mask.data()).empty())
                return fail("NULL models accepted", c);
            if (!estimate && apr::check_input(false, off.data(), nq, models.data(), prm.data(), p2.data(), p3.data(), nullptr,
                                              t.data(), mask.data()).empty())
                return fail("NULL initial rotations accepted", c);
            if (!estimate && n > 0 && apr::check_input(false, off.data(), nq, models.data(), prm.data(), p2.data(), p3.data(),
                                                       q.data(), t.data(), nullptr).empty())
                return fail("a NULL mask accepted", c);
            if (n > 0 && apr::check_input(estimate, off.data(), nq, models.data(), prm.data(), nullptr, p3.data(), q.data(),
                                          t.data(), mask.data()).empty())
                return fail("NULL points accepted", c);
        }
        if (!apr::check_input(estimate, nullptr, nq, models.data(), prm.data(), p2.data(), p3.data(), q.data(), t.data(),
                              mask.data()).size())
            return fail("NULL offsets accepted", c);
        // the plan
        const uint64_t max_q = 1 + rng() % 9, max_c = 1 + rng() % 200;
        const bool rf = rng() % 2 != 0, re = rng() % 2 != 0;
        const std::vector<size_t> start = apr::plan_batches(off.data(), nq, max_q, max_c);
        if (start.front() != 0 || start.back() != nq) return fail("the batches do not cover the queries", c);
        for (size_t b = 0; b + 1 < start.size(); ++b) {
            const size_t q0 = start[b], q1 = start[b + 1];
            if (q1 <= q0) return fail("an empty batch", c);
            if (q1 - q0 > max_q) return fail("a batch above the query bound", c);
            if (q1 - q0 > 1 && off[q1] - off[q0] > max_c) return fail("a batch above the correspondence bound", c);
            const apr::BatchClasses cls = apr::plan_classes(off.data(), models.data(), q0, q1, rf, re);
            if (cls.order.size() != q1 - q0) return fail("the order's size", c);
            std::set<uint32_t> seen(cls.order.begin(), cls.order.end());
            if (seen.size() != q1 - q0 || *seen.rbegin() != q1 - q0 - 1) return fail("the order is no permutation", c);
            if (cls.begin[0] != 0 || cls.begin[apr::kMaxNV + 1] != q1 - q0) return fail("the classes do not cover the batch", c);
            for (int nv = 0; nv <= apr::kMaxNV; ++nv) {
                if (cls.begin[nv + 1] < cls.begin[nv]) return fail("class bounds decrease", c);
                launches += cls.begin[nv + 1] > cls.begin[nv] ? 1 : 0;
                for (uint32_t k = cls.begin[nv]; k < cls.begin[nv + 1]; ++k) {
                    const uint32_t i = cls.order[k];
                    if (apr::num_variable(models[q0 + i], rf, re) != nv) return fail("a query in another class", c);
                    if (k > cls.begin[nv]) {
                        const uint32_t p = cls.order[k - 1];
                        const uint64_t lp = off[q0 + p + 1] - off[q0 + p], li = off[q0 + i + 1] - off[q0 + i];
                        if (lp < li || (lp == li && p > i)) return fail("a class is not longest first and stable", c);
                    }
                }
            }
            ++batches;
        }
    }
    // the column counts of 25.1 for every model under both flags
    const int both[11] = {1, 2, 2, 3, 6, 6, 10, 3, 2, 3, 10};
    for (int m = 0; m < 11; ++m) {
        if (apr::num_variable(m, true, true) != both[m] || apr::num_variable(m, false, false) != 0) return fail("column counts", m);
        if (apr::num_variable(m, true, false) != cam::num_focal(m)) return fail("focal columns", m);
    }
    std::printf("ok %d %ld %ld\n", calls, batches, launches);
    return 0;
}
