// track_ops_host_fuzz.cc — a stand-alone program for tests/test_tracks_cpu.py (built with -fsanitize=address,undefined
// together with csrc/host/model_io.cc and reconstruction.cc): the host half of track completion and track merging
// (DESIGN.md 18.3, 18.4).  Seeded models and graphs are planned for random id lists; the flat problems must pass
// tracks_plan.h's checks and batch plans; made-up pass bytes and merge logs are applied and the model is checked
// afterwards; then the corruptions: a graph without the model's images, merge logs with slots out of range, twice the
// same slot or a slot merged away, problems with offsets, indices and models out of range in heap arrays of the exact
// sizes - each refused, none read through.  Prints "ok <cases>".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>

#include "../../pycolmap_amd/csrc/tracks_plan.h"
#include "../../pycolmap_amd/csrc/host/reconstruction.h"
#include "../../pycolmap_amd/csrc/host/track_ops_host.h"

using namespace amchost;
namespace trk = amc::trk;

#define REQUIRE(cond)                                                      \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static uint64_t g_state = 7;
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

static const uint32_t kPoints2D = 8;

// nimg images (ids 20, 23, ..) of kPoints2D points2D, two cameras (one of them bogus when asked), points with tracks
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
    const uint32_t npts = 1 + Rand(8);
    for (uint32_t j = 0; j < npts; ++j) {
        ModelPoint3D p;
        p.point3D_id = 3 + 2 * j;
        p.xyz[0] = 0.1 * j;
        p.rgb[0] = static_cast<uint8_t>(10 * j);
        const uint32_t len = 1 + Rand(4);
        for (uint32_t e = 0; e < len; ++e) {
            const uint32_t i = Rand(nimg), k = Rand(kPoints2D);
            if (m.images[i].points2D[k].point3D_id != kInvalidPoint3DId) continue;
            m.images[i].points2D[k].point3D_id = p.point3D_id;
            p.track.emplace_back(m.images[i].image_id, k);
        }
        m.points3D.push_back(p);
    }
    return m;
}

static CorrespondenceGraph RandomGraph(const SparseModel& m) {
    CorrespondenceGraph g;
    for (const ModelImage& im : m.images) g.AddImage(im.image_id, im.points2D.size());
    g.AddImage(999, 4);  // an image the model does not hold
    const uint32_t nimg = static_cast<uint32_t>(m.images.size());
    const uint32_t nlists = 2 + Rand(4 * nimg);
    for (uint32_t l = 0; l < nlists; ++l) {
        const uint32_t a = Rand(nimg + 1), b = Rand(nimg + 1);
        const uint32_t ida = a == nimg ? 999 : m.images[a].image_id, idb = b == nimg ? 999 : m.images[b].image_id;
        const uint32_t n = Rand(8);
        std::unique_ptr<uint32_t[]> matches(new uint32_t[2 * n + 1]);
        for (uint32_t k = 0; k < 2 * n; ++k) matches[k] = Rand(ida == 999 || idb == 999 ? 4 : kPoints2D);
        g.AddCorrespondences(ida, idb, matches.get(), n);
    }
    // (not finalized: every image of the model stays in the graph, with or without correspondences)
    return g;
}

static std::set<uint64_t> RandomIds(const SparseModel& m) {
    std::set<uint64_t> ids;
    for (const ModelPoint3D& p : m.points3D)
        if (Rand(3)) ids.insert(p.point3D_id);
    ids.insert(1000 + Rand(5));  // an id the model does not hold
    return ids;
}

static size_t NumObservations(const SparseModel& m) {
    size_t n = 0;
    for (const ModelPoint3D& p : m.points3D) n += p.track.size();
    return n;
}

static uint64_t Completion(uint32_t round) {
    uint64_t cases = 0;
    SparseModel m = RandomModel(3 + Rand(5), round % 4 == 0);
    REQUIRE(CheckModel(m).empty());
    const CorrespondenceGraph g = RandomGraph(m);
    TriangulatorOptions o;
    o.complete_max_transitivity = static_cast<int>(Rand(4));
    const ModelIndex ix(m, o);
    const std::set<uint64_t> ids = RandomIds(m);
    const FlatComplete f = PlanCompletion(g, m, ix, o, ids);
    const amc_complete_problem pb = f.Problem();
    REQUIRE(trk::check_problem(pb).empty());
    REQUIRE(trk::candidate_items(pb).size() == f.NumCandidates());
    REQUIRE(o.complete_max_transitivity != 0 || f.NumItems() == 0);
    for (size_t i = 0; i < f.NumItems(); ++i) {
        REQUIRE(f.item_offsets[i + 1] > f.item_offsets[i]);
        REQUIRE(f.item_index[i].size() == f.item_offsets[i + 1] - f.item_offsets[i]);
        REQUIRE(ids.count(f.item_point3D[i]) != 0);
        REQUIRE(i == 0 || f.item_point3D[i - 1] < f.item_point3D[i]);
    }
    std::unique_ptr<uint8_t[]> pass(new uint8_t[f.NumCandidates() + 1]);
    for (size_t k = 0; k < f.NumCandidates(); ++k) pass[k] = Rand(3) != 0;
    const size_t before = NumObservations(m);
    std::set<uint64_t> modified;
    const CompletionApplied a = ApplyCompletion(f, pass.get(), g, o, &m, ix, &modified);
    REQUIRE(CheckModel(m).empty());
    REQUIRE(NumObservations(m) == before + a.num_completed);
    REQUIRE(a.num_visited >= a.num_completed && a.num_visited <= 4 * f.NumCandidates());
    REQUIRE((a.num_completed == 0) == modified.empty());
    for (const uint64_t id : modified) REQUIRE(ids.count(id) != 0);
    ++cases;
    // corruptions of the flat problem, in heap arrays of the exact sizes
    if (f.NumCandidates() != 0) {
        std::vector<uint32_t> cimg = f.cand_image;
        cimg[Rand(static_cast<uint32_t>(cimg.size()))] = static_cast<uint32_t>(f.image_cameras.size());
        amc_complete_problem bad = pb;
        bad.cand_image = cimg.data();
        REQUIRE(!trk::check_problem(bad).empty());
        std::vector<uint64_t> off = f.item_offsets;
        off[0] = 1;
        bad = pb;
        bad.item_offsets = off.data();
        REQUIRE(!trk::check_problem(bad).empty());
        std::vector<int32_t> models = f.camera_models;
        models[0] = 11;
        bad = pb;
        bad.camera_models = models.data();
        REQUIRE(!trk::check_problem(bad).empty());
        bad = pb;
        bad.cand_xy = nullptr;
        REQUIRE(!trk::check_problem(bad).empty());
        cases += 4;
    }
    amc_complete_opts co{-1.0, 0.0};
    REQUIRE(!trk::check_options(co).empty());
    // a graph that does not hold the model's images
    const CorrespondenceGraph none;
    bool has_track = false;
    for (const ModelPoint3D& p : m.points3D) has_track = has_track || (ids.count(p.point3D_id) && !p.track.empty());
    if (has_track && o.complete_max_transitivity > 0) {
        REQUIRE(Throws([&] { PlanCompletion(none, m, ix, o, ids); }));
        ++cases;
    }
    return cases;
}

static uint64_t Merging(uint32_t round) {
    uint64_t cases = 0;
    SparseModel m = RandomModel(3 + Rand(5), round % 4 == 0);
    const CorrespondenceGraph g = RandomGraph(m);
    const TriangulatorOptions o;
    const ModelIndex ix(m, o);
    const std::set<uint64_t> ids = RandomIds(m);
    const FlatMerge f = PlanMerge(g, m, ix, ids);
    const amc_merge_problem pb = f.Problem();
    REQUIRE(trk::check_merge_problem(pb).empty());
    const size_t nc = f.NumComponents();
    const std::vector<uint64_t> comp_obs = trk::component_obs_offsets(pb);
    for (size_t c = 0; c < nc; ++c) {
        REQUIRE(f.comp_point_offsets[c + 1] - f.comp_point_offsets[c] >= 2);
        REQUIRE(f.comp_root_offsets[c + 1] > f.comp_root_offsets[c]);
        REQUIRE(c == 0 || comp_obs[c] - comp_obs[c - 1] >= comp_obs[c + 1] - comp_obs[c]);  // largest first
        for (uint64_t p = f.comp_point_offsets[c] + 1; p < f.comp_point_offsets[c + 1]; ++p) REQUIRE(f.point3D_ids[p - 1] < f.point3D_ids[p]);
        for (uint64_t r = f.comp_root_offsets[c]; r < f.comp_root_offsets[c + 1]; ++r) REQUIRE(ids.count(f.point3D_ids[f.roots[r]]) != 0);
    }
    for (size_t first = 0; first < nc; first += 2) {  // batches of two components
        const size_t last = std::min(nc, first + 2);
        const trk::MergeBatchPlan b = trk::plan_merge_batch(pb, first, last);
        REQUIRE(b.comp_point.front() == 0 && b.comp_point.back() + 1 == b.point_obs.size());
        REQUIRE(b.point_obs.back() + 1 == b.obs_corr.size() && b.obs_corr.back() == b.corr_obs.size());
        for (const uint32_t v : b.corr_obs) REQUIRE(v + 1 < b.obs_corr.size());
        for (const uint32_t v : b.roots) REQUIRE(v + 1 < b.point_obs.size());
    }
    // a made-up result: every component's first root merges the slots 0 and 1, and when the component has a second
    // root and a third point, that root merges the new slot and slot 2
    const size_t nroots = f.roots.size();
    std::unique_ptr<uint32_t[]> ret(new uint32_t[nroots + 1]);
    std::unique_ptr<uint64_t[]> moff(new uint64_t[nroots + 1]);
    std::vector<uint32_t> cur, oth;
    std::vector<double> xyz;
    size_t expect_merges = 0;
    for (size_t c = 0; c < nc; ++c) {
        const uint64_t k = f.comp_point_offsets[c + 1] - f.comp_point_offsets[c];
        for (uint64_t r = f.comp_root_offsets[c]; r < f.comp_root_offsets[c + 1]; ++r) {
            moff[r] = cur.size();
            ret[r] = 0;
            const uint64_t nth = r - f.comp_root_offsets[c];
            if (nth == 0 || (nth == 1 && k >= 3)) {
                cur.push_back(nth == 0 ? 0 : static_cast<uint32_t>(k));
                oth.push_back(nth == 0 ? 1 : 2);
                for (int d = 0; d < 3; ++d) xyz.push_back(0.5 * d);
                ret[r] = 7;
                ++expect_merges;
            }
        }
    }
    moff[nroots] = cur.size();
    cur.push_back(0);  // (never empty: .data() below)
    oth.push_back(0);
    xyz.resize(xyz.size() + 3);
    SparseModel work = m;
    std::set<uint64_t> modified{f.point3D_ids.empty() ? 1 : f.point3D_ids[0]};
    uint64_t largest = 0;
    for (const ModelPoint3D& p : m.points3D) largest = std::max(largest, p.point3D_id);
    const MergeApplied a = ApplyMergeResult(f, ret.get(), moff.get(), cur.data(), oth.data(), xyz.data(), &work, &modified);
    REQUIRE(CheckModel(work).empty());
    REQUIRE(a.num_merges == expect_merges && a.num_merged == 7 * expect_merges);
    REQUIRE(work.points3D.size() + expect_merges == m.points3D.size());
    REQUIRE(NumObservations(work) == NumObservations(m));
    for (const ModelPoint3D& p : work.points3D) REQUIRE(p.point3D_id <= largest || (p.error == -1.0 && modified.count(p.point3D_id)));
    ++cases;
    if (expect_merges != 0) {  // logs that do not fit
        for (int kind = 0; kind < 3; ++kind) {
            std::vector<uint32_t> c2 = cur, o2 = oth;
            if (kind == 0) c2[0] = 1000;
            if (kind == 1) o2[0] = c2[0];
            std::unique_ptr<uint64_t[]> moff2(new uint64_t[nroots + 1]);
            std::copy(moff.get(), moff.get() + nroots + 1, moff2.get());
            if (kind == 2) {  // the first merge twice: its slots are gone the second time
                c2.insert(c2.begin(), c2[0]);
                o2.insert(o2.begin(), o2[0]);
                for (size_t r = 1; r <= nroots; ++r) moff2[r] += 1;
            }
            std::vector<double> x2(3 * c2.size(), 0.0);
            SparseModel w2 = m;
            std::set<uint64_t> mod2;
            REQUIRE(Throws([&] { ApplyMergeResult(f, ret.get(), moff2.get(), c2.data(), o2.data(), x2.data(), &w2, &mod2); }));
            ++cases;
        }
    }
    if (nc != 0) {  // corruptions of the flat problem, in heap arrays of the exact sizes
        amc_merge_problem bad = pb;
        std::vector<uint32_t> roots = f.roots;
        roots[0] = static_cast<uint32_t>(f.comp_point_offsets[1]);  // the first point after its component
        bad.roots = roots.data();
        REQUIRE(!trk::check_merge_problem(bad).empty());
        if (!f.corr_obs.empty()) {
            std::vector<uint32_t> corr = f.corr_obs;
            corr[0] = static_cast<uint32_t>(f.obs_image.size());
            bad = pb;
            bad.corr_obs = corr.data();
            REQUIRE(!trk::check_merge_problem(bad).empty());
            ++cases;
        }
        std::vector<uint64_t> poo = f.point_obs_offsets;
        poo[1] = poo[0];  // a point without observations
        bad = pb;
        bad.point_obs_offsets = poo.data();
        REQUIRE(!trk::check_merge_problem(bad).empty());
        std::vector<uint64_t> cpo = f.comp_point_offsets;
        cpo[1] = 0;  // a component without points
        bad = pb;
        bad.comp_point_offsets = cpo.data();
        REQUIRE(!trk::check_merge_problem(bad).empty());
        std::vector<uint32_t> oimg = f.obs_image;
        oimg.back() = static_cast<uint32_t>(f.image_cameras.size());
        bad = pb;
        bad.obs_image = oimg.data();
        REQUIRE(!trk::check_merge_problem(bad).empty());
        cases += 4;
        const CorrespondenceGraph none;
        REQUIRE(Throws([&] { PlanMerge(none, m, ix, ids); }));
        ++cases;
    }
    amc_merge_opts mo{-1.0, 0.0};
    REQUIRE(!trk::check_merge_options(mo).empty());
    return cases;
}

// a component of 4097 observations is refused by the plan and by the library's check
static uint64_t Bound() {
    for (const uint32_t nobs : {4096u, 4097u}) {
        SparseModel m;
        ModelCamera c;
        c.camera_id = 1;
        c.model = 0;
        c.width = 1000;
        c.height = 800;
        c.params = {800.0, 500.0, 400.0};
        m.cameras.push_back(c);
        CorrespondenceGraph g;
        for (uint32_t i = 0; i < 2; ++i) {
            ModelImage im;
            im.image_id = i + 1;
            im.camera_id = 1;
            im.points2D.resize(nobs);
            m.images.push_back(im);
            g.AddImage(i + 1, nobs);
        }
        // point 1 holds one observation in image 1, point 2 all but one point2D of image 2
        ModelPoint3D a, b;
        a.point3D_id = 1;
        b.point3D_id = 2;
        a.track.emplace_back(1, 0);
        m.images[0].points2D[0].point3D_id = 1;
        for (uint32_t k = 0; k + 1 < nobs; ++k) {
            b.track.emplace_back(2, k);
            m.images[1].points2D[k].point3D_id = 2;
        }
        m.points3D.push_back(a);
        m.points3D.push_back(b);
        REQUIRE(CheckModel(m).empty());
        const uint32_t match[2] = {0, 0};
        g.AddCorrespondences(1, 2, match, 1);  // point 1's observation corresponds to one of point 2's
        const TriangulatorOptions o;
        const ModelIndex ix(m, o);
        const std::set<uint64_t> ids{1};
        REQUIRE(NumObservations(m) == nobs);
        if (nobs <= AMC_MERGE_MAX_COMPONENT_OBS) {
            const FlatMerge f = PlanMerge(g, m, ix, ids);
            REQUIRE(f.NumComponents() == 1 && f.largest_component == nobs);
            REQUIRE(trk::check_merge_problem(f.Problem()).empty());
        } else {
            REQUIRE(Throws([&] { PlanMerge(g, m, ix, ids); }));
        }
    }
    return 2;
}

int main() {
    uint64_t cases = 0;
    for (uint32_t round = 0; round < 400; ++round) {
        cases += Completion(round);
        cases += Merging(round);
    }
    cases += Bound();
    std::printf("ok %llu\n", static_cast<unsigned long long>(cases));
    return 0;
}
