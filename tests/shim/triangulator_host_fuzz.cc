// triangulator_host_fuzz.cc — a stand-alone program for tests/test_triangulator_cpu.py (built with
// -fsanitize=address,undefined together with csrc/host/model_io.cc and reconstruction.cc): the host half of the
// incremental triangulator.  Seeded graphs take random match lists with self pairs, indices out
// of range and duplicates and are held to their counts and to the one-correspondence-per-image rule; walks of every
// transitivity are checked for duplicates and for the seed; seeded models are cut into runs, whose observation sets
// must be pairwise disjoint and whose flat problems must pass triobs_plan.h's checks and plan; made-up results are
// applied and the model is checked afterwards; then the corruptions: queries for images and points2D that do not exist,
// results that continue to a candidate without a point or give an observation two points, problems with offsets,
// indices and models out of range in heap arrays of the exact sizes - each refused, none read through.  Prints
// "ok <cases>".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>

#include "../../pycolmap_amd/csrc/triobs_plan.h"
#include "../../pycolmap_amd/csrc/host/reconstruction.h"
#include "../../pycolmap_amd/csrc/host/triangulator_host.h"

using namespace amchost;
namespace triobs = amc::triobs;

#define REQUIRE(cond)                                                      \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static uint64_t g_state = 1;
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

static const uint32_t kPoints2D = 10;

// nimg images (ids 20, 23, ..) of kPoints2D points2D, two cameras (one of them bogus when asked), some points
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
    const uint32_t npts = Rand(6);
    for (uint32_t j = 0; j < npts; ++j) {
        ModelPoint3D p;
        p.point3D_id = 3 + 2 * j;
        p.xyz[0] = 0.1 * j;
        const uint32_t len = 2 + Rand(3);
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

static CorrespondenceGraph RandomGraph(const SparseModel& m, uint64_t* cases) {
    CorrespondenceGraph g;
    for (const ModelImage& im : m.images) g.AddImage(im.image_id, im.points2D.size());
    g.AddImage(999, 4);  // an image the model does not hold
    const uint32_t nimg = static_cast<uint32_t>(m.images.size());
    const uint32_t nlists = 2 + Rand(3 * nimg);
    for (uint32_t l = 0; l < nlists; ++l) {
        const uint32_t a = Rand(nimg + 1), b = Rand(nimg + 1);
        const uint32_t ida = a == nimg ? 999 : m.images[a].image_id, idb = b == nimg ? 999 : m.images[b].image_id;
        const uint32_t n = Rand(8);
        std::unique_ptr<uint32_t[]> matches(new uint32_t[2 * n + 1]);
        for (uint32_t k = 0; k < 2 * n; ++k) matches[k] = Rand(kPoints2D + 2);  // two indices out of range
        const size_t before = g.NumCorrespondencesBetweenImages(ida, idb);
        g.AddCorrespondences(ida, idb, matches.get(), n);
        REQUIRE(g.NumCorrespondencesBetweenImages(ida, idb) <= before + n);
        REQUIRE(ida != idb || g.NumCorrespondencesBetweenImages(ida, idb) == 0);
        ++*cases;
    }
    g.Finalize();
    // the counts against the lists, and at most one correspondence per other image
    for (const ModelImage& im : m.images) {
        if (!g.ExistsImage(im.image_id)) continue;
        size_t nobs = 0, ncorr = 0;
        for (uint32_t k = 0; k < kPoints2D; ++k) {
            const std::vector<Correspondence>& c = g.ExtractCorrespondences(im.image_id, k);
            nobs += !c.empty();
            ncorr += c.size();
            std::set<uint32_t> into;
            for (const Correspondence& x : c) {
                REQUIRE(x.image_id != im.image_id && into.insert(x.image_id).second);
                bool back = false;
                for (const Correspondence& y : g.ExtractCorrespondences(x.image_id, x.point2D_idx))
                    back = back || (y.image_id == im.image_id && y.point2D_idx == k);
                REQUIRE(back);
            }
            REQUIRE(g.HasCorrespondences(im.image_id, k) == !c.empty());
        }
        REQUIRE(nobs > 0 && nobs == g.NumObservationsForImage(im.image_id) && ncorr == g.NumCorrespondencesForImage(im.image_id));
        ++*cases;
    }
    return g;
}

int main() {
    uint64_t cases = 0;
    for (uint32_t seed = 0; seed < 40; ++seed) {
        g_state = 1234 + seed;
        const uint32_t nimg = 2 + Rand(6);
        SparseModel m = RandomModel(nimg, seed % 7 == 3);
        REQUIRE(CheckModel(m).empty());
        const CorrespondenceGraph g = RandomGraph(m, &cases);
        // walks
        for (const ModelImage& im : m.images) {
            if (!g.ExistsImage(im.image_id)) {
                REQUIRE(Throws([&] { g.HasCorrespondences(im.image_id, 0); }));
                REQUIRE(Throws([&] { g.NumObservationsForImage(im.image_id); }));
                continue;
            }
            REQUIRE(Throws([&] { g.ExtractCorrespondences(im.image_id, kPoints2D); }));
            for (uint32_t k = 0; k < kPoints2D; ++k)
                for (size_t t = 0; t <= 5; ++t) {
                    std::vector<Correspondence> found;
                    g.ExtractTransitiveCorrespondences(im.image_id, k, t, &found);
                    std::set<std::pair<uint32_t, uint32_t>> seen;
                    for (const Correspondence& c : found) {
                        REQUIRE(seen.insert({c.image_id, c.point2D_idx}).second);
                        REQUIRE(!(c.image_id == im.image_id && c.point2D_idx == k));
                    }
                    REQUIRE(t != 0 || found.empty());
                    REQUIRE(t < 1 || found.size() >= g.ExtractCorrespondences(im.image_id, k).size());
                    ++cases;
                }
        }
        REQUIRE(Throws([&] { g.NumCorrespondencesForImage(12345); }));
        // runs
        TriangulatorOptions o;
        o.max_transitivity = 1 + static_cast<int>(seed % 3);
        o.ignore_two_view_tracks = seed % 2 == 0;
        REQUIRE(o.Check().empty());
        ModelIndex ix(m, o);
        FlatTriobs flat = FlattenModelForTriobs(m, ix);
        std::set<uint64_t> modified;
        for (size_t ii = 0; ii < m.images.size(); ++ii) {
            const uint32_t image_id = m.images[ii].image_id;
            if (!g.ExistsImage(image_id)) {
                REQUIRE(Throws([&] { PlanTriangulationRun(g, m, ix, o, image_id, 0, &flat); }));
                continue;
            }
            size_t runs = 0;
            for (size_t begin = 0; begin < kPoints2D;) {
                const size_t next = PlanTriangulationRun(g, m, ix, o, image_id, begin, &flat);
                REQUIRE(next > begin && next <= kPoints2D);
                REQUIRE(o.max_transitivity != 1 || next == kPoints2D);  // one batch per image (17.4)
                begin = next;
                ++runs;
                if (flat.NumItems() == 0) continue;
                const amc_triobs_problem pb = flat.Problem();
                REQUIRE(triobs::check_problem(pb).empty());
                std::vector<uint32_t> order, slots;
                triobs::plan_batch(pb.item_offsets, 0, pb.num_items, &order, &slots);
                REQUIRE(order.size() == pb.num_items && slots.size() == pb.num_items + 1);
                std::set<std::pair<uint32_t, uint32_t>> used;
                for (const Correspondence& c : flat.cand_obs) REQUIRE(used.insert({c.image_id, c.point2D_idx}).second);
                // a made-up result: continue to the first candidate with a point, one round of every candidate without
                std::vector<int32_t> cont(pb.num_items, -1);
                std::vector<uint32_t> round(flat.cand_image.size(), 0);
                std::vector<uint64_t> roff{0};
                std::vector<double> rxyz;
                for (size_t i = 0; i < pb.num_items; ++i) {
                    const uint64_t c0 = pb.item_offsets[i], n = pb.item_offsets[i + 1] - c0;
                    REQUIRE(flat.cand_obs[c0 + n - 1].image_id == image_id && flat.cand_obs[c0 + n - 1].point2D_idx == flat.item_point2D[i]);
                    bool ref_has = flat.cand_has_point[c0 + n - 1] != 0;
                    for (uint64_t k = 0; k + 1 < n && !ref_has; ++k)
                        if (flat.cand_has_point[c0 + k]) {
                            cont[i] = static_cast<int32_t>(k);
                            ref_has = true;
                        }
                    uint64_t free_obs = 0;
                    for (uint64_t k = 0; k < n; ++k) free_obs += !(k + 1 == n ? ref_has : flat.cand_has_point[c0 + k] != 0);
                    if (free_obs >= 2) {
                        for (uint64_t k = 0; k < n; ++k)
                            if (!(k + 1 == n ? ref_has : flat.cand_has_point[c0 + k] != 0)) round[c0 + k] = 1;
                        rxyz.insert(rxyz.end(), {1.0, 2.0, 3.0});
                    }
                    roff.push_back(rxyz.size() / 3);
                }
                // corrupted results are refused on a copy
                if (pb.num_items) {
                    SparseModel copy = m;
                    ModelIndex cix(copy, o);
                    std::set<uint64_t> cm;
                    std::vector<int32_t> bad = cont;
                    const uint64_t n0 = pb.item_offsets[1];
                    bad[0] = static_cast<int32_t>(n0 - 1);  // the reference observation itself
                    REQUIRE(Throws([&] { ApplyTriobsResult(flat, bad.data(), round.data(), roff.data(), rxyz.data(), &copy, &cix, &cm); }));
                    ++cases;
                }
                const size_t points_before = m.points3D.size();
                const TriobsApplied a = ApplyTriobsResult(flat, cont.data(), round.data(), roff.data(), rxyz.data(), &m, &ix, &modified);
                REQUIRE(m.points3D.size() == points_before + a.num_created);
                REQUIRE(a.num_tris >= a.num_continued + 2 * a.num_created);
                REQUIRE(CheckModel(m).empty());
                for (size_t j = points_before; j < m.points3D.size(); ++j) REQUIRE(m.points3D[j].error == -1.0 && modified.count(m.points3D[j].point3D_id));
                // the same result a second time gives observations a second point
                if (a.num_created) {
                    SparseModel copy = m;
                    ModelIndex cix(copy, o);
                    std::set<uint64_t> cm;
                    std::vector<int32_t> none(pb.num_items, -1);
                    REQUIRE(Throws([&] { ApplyTriobsResult(flat, none.data(), round.data(), roff.data(), rxyz.data(), &copy, &cix, &cm); }));
                }
                ++cases;
            }
            REQUIRE(runs >= 1);
        }
    }
    // problems out of range, in heap arrays of the exact sizes
    {
        std::unique_ptr<int32_t[]> models(new int32_t[1]{2});
        std::unique_ptr<double[]> params(new double[12]()), q(new double[4]{0, 0, 0, 1}), t(new double[3]()), xy(new double[4]()), X(new double[6]());
        std::unique_ptr<uint32_t[]> icam(new uint32_t[1]{0}), ci(new uint32_t[2]{0, 0});
        std::unique_ptr<uint64_t[]> off(new uint64_t[2]{0, 2});
        std::unique_ptr<uint8_t[]> has(new uint8_t[2]());
        amc_triobs_problem pb{};
        pb.num_cameras = 1;
        pb.camera_models = models.get();
        pb.camera_params = params.get();
        pb.num_images = 1;
        pb.image_cameras = icam.get();
        pb.qvec = q.get();
        pb.tvec = t.get();
        pb.num_items = 1;
        pb.item_offsets = off.get();
        pb.cand_image = ci.get();
        pb.cand_xy = xy.get();
        pb.cand_has_point = has.get();
        pb.cand_xyz = X.get();
        REQUIRE(triobs::check_problem(pb).empty());
        models[0] = 11;
        REQUIRE(!triobs::check_problem(pb).empty());
        models[0] = -1;
        REQUIRE(!triobs::check_problem(pb).empty());
        models[0] = 2;
        icam[0] = 1;
        REQUIRE(!triobs::check_problem(pb).empty());
        icam[0] = 0;
        ci[1] = 1;
        REQUIRE(!triobs::check_problem(pb).empty());
        ci[1] = 0;
        off[0] = 1;
        REQUIRE(!triobs::check_problem(pb).empty());
        off[0] = 0;
        off[1] = 0;  // an item without candidates
        REQUIRE(!triobs::check_problem(pb).empty());
        off[1] = AMC_TRIOBS_MAX_ITEM_CANDIDATES + 1;  // refused before anything is read through it
        REQUIRE(!triobs::check_problem(pb).empty());
        off[1] = 2;
        pb.cand_xyz = nullptr;
        REQUIRE(!triobs::check_problem(pb).empty());
        pb.cand_xyz = X.get();
        REQUIRE(triobs::check_problem(pb).empty());
        amc_triobs_opts op{2.0, 2.0, 1.5, 0.0};
        REQUIRE(triobs::check_options(op).empty());
        op.create_max_angle_error = 0.0;
        REQUIRE(!triobs::check_options(op).empty());
        op.create_max_angle_error = 2.0;
        op.min_angle = -1.0;
        REQUIRE(!triobs::check_options(op).empty());
        op.min_angle = std::nan("");
        REQUIRE(!triobs::check_options(op).empty());
        cases += 12;
    }
    std::printf("ok %llu\n", static_cast<unsigned long long>(cases));
    return 0;
}
