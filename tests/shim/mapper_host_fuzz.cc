// mapper_host_fuzz.cc — a stand-alone program for tests/test_mapper_cpu.py (built with -fsanitize=address,undefined
// together with csrc/host/model_io.cc and reconstruction.cc): the host halves of the mapper (DESIGN.md 20,
// csrc/host/mapper_host.h).  Seeded models, graphs and candidates are planned: the flat visibility problem must be
// consistent (offsets, indices in range, heap arrays of the exact sizes) and a sequential count over it must rank to a
// list without repeats that honours the two drop rules; the 2D-3D pairs must name points2D of the candidate and points
// of the model once per point2D; a registration with a made-up mask must leave a model that passes CheckModel; the local
// bundle must hold the wanted number of distinct other images for made-up angles, NaN included.  Then the refusals: a
// candidate whose point count differs from the graph's, a camera the model lacks, a graph that names a point2D the model
// does not hold, an image outside the model, a pair above the bound, a registration of a model image.  Prints
// "ok <cases>".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>

#include "../../pycolmap_amd/csrc/host/mapper_host.h"
#include "../../pycolmap_amd/csrc/host/reconstruction.h"

using namespace amchost;

#define REQUIRE(cond)                                                      \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static uint64_t g_state = 20;
static uint32_t Rand(uint32_t n) {  // 0 .. n - 1
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>((g_state >> 33) % n);
}

template <class F>
static bool Throws(F f) {
    try {
        f();
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}

static const uint32_t kPoints2D = 9;

// nimg images (ids 20, 23, ..) of kPoints2D points2D, two cameras (one bogus when asked), points with tracks
static SparseModel RandomModel(uint32_t nimg, bool bogus) {
    SparseModel m;
    ModelCamera c;
    c.camera_id = 5;
    c.model = 2;
    c.width = 1000;
    c.height = 800;
    c.params = {800.0, 500.0, 400.0, 0.05};
    m.cameras.push_back(c);
    c.camera_id = 2;
    c.model = 4;
    c.params = {bogus ? 5.0 : 800.0, 810.0, 500.0, 400.0, 0.01, 0.0, 0.0, 0.0};
    m.cameras.push_back(c);
    for (uint32_t i = 0; i < nimg; ++i) {
        ModelImage im;
        im.image_id = 20 + 3 * i;
        im.camera_id = Rand(3) ? 5 : 2;
        im.tvec[0] = 0.1 * i;
        im.tvec[2] = 6.0;
        im.name = "i" + std::to_string(i);
        for (uint32_t k = 0; k < kPoints2D; ++k) {
            ModelPoint2D p;
            p.x = 10.0 * k + i;
            p.y = 5.0 * k;
            im.points2D.push_back(p);
        }
        m.images.push_back(im);
    }
    const uint32_t npts = 1 + Rand(14);
    for (uint32_t j = 0; j < npts; ++j) {
        ModelPoint3D p;
        p.point3D_id = 3 + 2 * j;
        p.xyz[0] = 0.1 * j;
        p.xyz[2] = 1.0 + 0.01 * j;
        const uint32_t len = 1 + Rand(5);
        for (uint32_t e = 0; e < len; ++e) {
            const uint32_t i = Rand(nimg), k = Rand(kPoints2D);
            if (m.images[i].points2D[k].point3D_id != kInvalidPoint3DId) continue;  // (one image may see a point twice)
            m.images[i].points2D[k].point3D_id = p.point3D_id;
            p.track.emplace_back(m.images[i].image_id, k);
        }
        if (!p.track.empty()) m.points3D.push_back(p);
    }
    return m;
}

static const uint32_t kCandidateIds[3] = {7, 500, 501};

static CorrespondenceGraph RandomGraph(const SparseModel& m, uint32_t extra_for_first = 0) {
    CorrespondenceGraph g;
    for (size_t i = 0; i < m.images.size(); ++i) g.AddImage(m.images[i].image_id, m.images[i].points2D.size() + (i == 0 ? extra_for_first : 0));
    for (uint32_t id : kCandidateIds) g.AddImage(id, kPoints2D);
    g.AddImage(999, 4);  // an image that is neither in the model nor a candidate
    std::vector<uint32_t> ids;
    for (const ModelImage& im : m.images) ids.push_back(im.image_id);
    for (uint32_t id : kCandidateIds) ids.push_back(id);
    ids.push_back(999);
    const uint32_t nlists = 4 + Rand(6 * static_cast<uint32_t>(ids.size()));
    for (uint32_t l = 0; l < nlists; ++l) {
        const uint32_t ida = ids[Rand(static_cast<uint32_t>(ids.size()))], idb = ids[Rand(static_cast<uint32_t>(ids.size()))];
        const uint32_t n = Rand(10);
        std::unique_ptr<uint32_t[]> matches(new uint32_t[2 * n + 1]);
        for (uint32_t k = 0; k < n; ++k) {
            matches[2 * k] = Rand(static_cast<uint32_t>(g.NumPoints2D(ida)));
            matches[2 * k + 1] = Rand(static_cast<uint32_t>(g.NumPoints2D(idb)));
        }
        g.AddCorrespondences(ida, idb, matches.get(), n);
    }
    return g;
}

static MapperCandidates Candidates() {
    MapperCandidates c;
    for (uint32_t id : kCandidateIds) {
        MapperCandidate x;
        x.image_id = id;
        x.camera_id = id == 500 ? 2 : 5;
        for (uint32_t k = 0; k < kPoints2D; ++k) {
            x.xy.push_back(id == 501 && k == 3 ? std::nan("") : 100.0 * k + id % 7);
            x.xy.push_back(k == 4 ? -5.0 : 90.0 * k);
        }
        c[id] = x;
    }
    return c;
}

// heap copies of the exact sizes, so that a read past an array is seen
template <class T>
static std::unique_ptr<T[]> Exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

int main() {
    size_t cases = 0;
    for (uint32_t round = 0; round < 400; ++round) {
        SparseModel m = RandomModel(2 + Rand(6), round % 5 == 0);
        REQUIRE(CheckModel(m).empty());
        const CorrespondenceGraph g = RandomGraph(m);
        MapperOptions o;
        o.abs_pose_min_num_inliers = 1 + static_cast<int>(Rand(3));
        o.max_reg_trials = 1 + static_cast<int>(Rand(2));
        o.local_ba_num_images = 2 + static_cast<int>(Rand(4));
        o.image_selection_method = static_cast<ImageSelectionMethod>(Rand(3));
        REQUIRE(o.Check().empty());
        ModelIndex ix(m, o.BogusThresholds());
        const MapperCandidates cands = Candidates();

        // ---- 20.1
        const FlatVisibility f = PlanVisibility(g, m, ix, cands);
        const amc_visibility_problem pb = f.Problem();
        REQUIRE(pb.num_candidates == 3 && f.cand_point_offsets.size() == 4 && f.cand_point_offsets.back() == 3 * kPoints2D);
        REQUIRE(f.corr_offsets.size() == f.cand_point_offsets.back() + 1 && f.corr_offsets.back() == f.corr_image.size());
        REQUIRE(f.image_point_offsets.back() == f.point2D_point3D.size() && f.cand_xy.size() == 2 * 3 * kPoints2D);
        const auto ipoff = Exact(f.image_point_offsets);
        const auto table = Exact(f.point2D_point3D);
        const auto coff = Exact(f.corr_offsets);
        const auto cimg = Exact(f.corr_image);
        const auto cp2 = Exact(f.corr_point2D);
        std::vector<uint32_t> nobs(3, 0), nvis(3, 0);
        std::vector<uint64_t> score(3, 0);
        for (size_t c = 0; c < 3; ++c) {
            for (uint64_t j = f.cand_point_offsets[c]; j < f.cand_point_offsets[c + 1]; ++j) {
                REQUIRE(coff[j] <= coff[j + 1]);
                bool vis = false;
                for (uint64_t k = coff[j]; k < coff[j + 1]; ++k) {
                    REQUIRE(cimg[k] < pb.num_graph_images && cp2[k] < ipoff[cimg[k] + 1] - ipoff[cimg[k]]);
                    vis = vis || table[ipoff[cimg[k]] + cp2[k]] != kInvalidPoint3DId;
                }
                nobs[c] += coff[j + 1] > coff[j];
                nvis[c] += vis;
            }
            score[c] = 4 * nvis[c] + Rand(3);
        }
        MapperTrials trials;
        if (Rand(2)) trials[kCandidateIds[Rand(3)]] = static_cast<int>(Rand(3));
        const std::vector<uint32_t> ranked = RankNextImages(f, nobs.data(), nvis.data(), score.data(), o, trials);
        REQUIRE(std::set<uint32_t>(ranked.begin(), ranked.end()).size() == ranked.size());
        bool seen_tried = false;
        for (uint32_t id : ranked) {
            const size_t c = std::find(f.cand_ids.begin(), f.cand_ids.end(), id) - f.cand_ids.begin();
            REQUIRE(c < 3 && nvis[c] >= static_cast<uint32_t>(o.abs_pose_min_num_inliers));
            const int tried = trials.count(id) ? trials[id] : 0;
            REQUIRE(tried < o.max_reg_trials);
            REQUIRE(!(seen_tried && tried == 0));  // the never-tried ones come first
            seen_tried = seen_tried || tried > 0;
        }
        cases += 1;

        // ---- 20.2
        const MapperCandidate& cand = cands.at(kCandidateIds[Rand(3)]);
        const RegistrationPairs pairs = CollectRegistrationPairs(g, m, ix, cand);
        REQUIRE(pairs.points2D.size() == 2 * pairs.size() && pairs.points3D.size() == 3 * pairs.size() && pairs.point3D_id.size() == pairs.size());
        std::set<std::pair<uint32_t, uint64_t>> once;
        for (size_t i = 0; i < pairs.size(); ++i) {
            REQUIRE(pairs.point2D_idx[i] < kPoints2D && ix.point.count(pairs.point3D_id[i]));
            REQUIRE(once.emplace(pairs.point2D_idx[i], pairs.point3D_id[i]).second);
            REQUIRE(i == 0 || pairs.point2D_idx[i - 1] <= pairs.point2D_idx[i]);
        }
        REQUIRE(pairs.num_visible <= kPoints2D);
        const RegistrationRule rule = PlanRegistration(m, m.cameras[ix.camera.at(cand.camera_id)], Rand(2) != 0, o);
        REQUIRE(!(rule.camera_in_use && !rule.camera_bogus) || (!rule.estimate_focal_length && !rule.refine_focal_length && !rule.refine_extra_params));
        std::vector<uint8_t> mask(pairs.size() + 1, 0);
        for (size_t i = 0; i < pairs.size(); ++i) mask[i] = Rand(3) != 0;
        const auto exact_mask = Exact(std::vector<uint8_t>(mask.begin(), mask.begin() + pairs.size()));
        const double q[4] = {0.0, 0.0, 0.0, 1.0}, t[3] = {0.5, 0.0, 6.0};
        std::set<uint64_t> modified;
        size_t before = 0, after = 0;
        for (const ModelPoint3D& p : m.points3D) before += p.track.size();
        const double f0 = m.cameras[ix.camera.at(cand.camera_id)].params[0];
        const size_t attached = ApplyRegistration(cand, pairs, exact_mask.get(), q, t, rule.estimate_focal_length, 1.5, &m, &ix, &modified);
        for (const ModelPoint3D& p : m.points3D) after += p.track.size();
        REQUIRE(after == before + attached && modified.size() <= attached && attached <= pairs.size());
        REQUIRE(m.cameras[ix.camera.at(cand.camera_id)].params[0] == (rule.estimate_focal_length ? 1.5 * f0 : f0));
        REQUIRE(CheckModel(m).empty() && m.images.back().image_id == cand.image_id && ix.image.at(cand.image_id) == m.images.size() - 1);
        REQUIRE(Throws([&] { ApplyRegistration(cand, pairs, exact_mask.get(), q, t, false, 1.0, &m, &ix, &modified); }));  // it is in the model now
        cases += 1;

        // ---- 20.3
        for (const ModelImage& im : std::vector<ModelImage>(m.images)) {
            const FlatBundle fb = PlanLocalBundle(m, ix, o, im.image_id);
            REQUIRE(fb.pair_offsets.size() == fb.NumPairs() + 1 && fb.pair_images.size() == 2 * fb.NumPairs() && fb.NumPairs() <= fb.overlapping.size());
            REQUIRE(fb.pair_offsets.back() == fb.shared_points.size());
            for (size_t i = 0; i + 1 < fb.overlapping.size(); ++i)
                REQUIRE(fb.overlapping[i].second > fb.overlapping[i + 1].second ||
                        (fb.overlapping[i].second == fb.overlapping[i + 1].second && fb.overlapping[i].first < fb.overlapping[i + 1].first));
            for (uint32_t s : fb.shared_points) REQUIRE(s < fb.point_xyz.size() / 3);
            for (uint32_t i : fb.pair_images) REQUIRE(i < fb.tvec.size() / 3);
            std::vector<double> angle(fb.NumPairs());
            for (double& a : angle) a = Rand(5) == 0 ? std::nan("") : 0.02 * Rand(20);
            const auto exact_angle = Exact(angle);
            const std::vector<uint32_t> bundle = SelectLocalBundle(fb, o, exact_angle.get());
            REQUIRE(bundle.size() == fb.num_eff_images && fb.num_eff_images <= static_cast<size_t>(o.local_ba_num_images - 1));
            REQUIRE(std::set<uint32_t>(bundle.begin(), bundle.end()).size() == bundle.size());
            for (uint32_t id : bundle) REQUIRE(id != im.image_id && ix.image.count(id));
            if (fb.NumPairs() && fb.shared_points.size() > 1)
                REQUIRE(Throws([&] { PlanLocalBundle(m, ix, o, im.image_id, 0); }));  // above the bound it is given
            cases += 1;
        }
        REQUIRE(Throws([&] { PlanLocalBundle(m, ix, o, 4242); }));

        // ---- refusals
        const uint32_t left = cand.image_id == 7 ? 500 : 7;  // a candidate that is still outside the model
        MapperCandidates wrong = Candidates();
        wrong[left].xy.resize(2 * (kPoints2D - 1));
        REQUIRE(Throws([&] { PlanVisibility(g, m, ix, wrong); }));
        REQUIRE(Throws([&] { CollectRegistrationPairs(g, m, ix, wrong.at(left)); }));
        wrong = Candidates();
        wrong[left].camera_id = 77;
        REQUIRE(Throws([&] { PlanVisibility(g, m, ix, wrong); }));
        REQUIRE(PlanVisibility(g, m, ix, cands).cand_ids.size() == 2);  // the registered one is no candidate any more
        MapperCandidates unknown;
        unknown[1234].image_id = 1234;
        unknown[1234].camera_id = 5;
        REQUIRE(Throws([&] { PlanVisibility(g, m, ix, unknown); }));  // the graph's own refusal
        cases += 1;
    }
    // a graph that gives a model image more points2D than the model holds, and a correspondence onto one of them
    for (uint32_t round = 0; round < 50; ++round) {
        SparseModel m = RandomModel(3, false);
        CorrespondenceGraph g = RandomGraph(m, 4);
        const uint32_t match[2] = {0, kPoints2D + 1};
        g.AddCorrespondences(501, m.images[0].image_id, match, 1);
        const MapperOptions o;
        const ModelIndex ix(m, o.BogusThresholds());
        const MapperCandidates cands = Candidates();
        bool named = false;
        for (const Correspondence& c : g.ExtractCorrespondences(501, 0)) named = named || (c.image_id == m.images[0].image_id && c.point2D_idx >= kPoints2D);
        if (!named) continue;  // (a duplicate: the graph dropped it)
        REQUIRE(Throws([&] { PlanVisibility(g, m, ix, cands); }));
        REQUIRE(Throws([&] { CollectRegistrationPairs(g, m, ix, cands.at(501)); }));
        cases += 1;
    }
    std::printf("ok %zu\n", cases);
    return 0;
}
