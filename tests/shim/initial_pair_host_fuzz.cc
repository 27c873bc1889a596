// initial_pair_host_fuzz.cc — a stand-alone program for tests/test_initial_pair_cpu.py (built with
// -fsanitize=address,undefined together with csrc/host/model_io.cc and reconstruction.cc): the host halves of the initial
// pair, the global adjustment and the image filter (csrc/host/initial_pair_host.h).  Seeded models, matches
// and candidates: the flat problem of a pair must be consistent (heap arrays of the exact sizes, offsets, indices in
// range); a made-up accepted mask must leave a model that passes CheckModel with one two-element track per accepted
// correspondence; the configuration of the global adjustment must hold the gauge; the normalisation must keep the model
// valid for any poses, NaN included, and be the identity below two images; FilterImages must do nothing below twenty
// images and otherwise leave a valid model without the removed images; the ranking must put a filtered candidate behind
// the untried ones.  Then the refusals.  Prints "ok <cases>".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>

#include "../../pycolmap_amd/csrc/host/initial_pair_host.h"
#include "../../pycolmap_amd/csrc/host/reconstruction.h"

using namespace amchost;

#define REQUIRE(cond)                                                      \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static uint64_t g_state = 21;
static uint32_t Rand(uint32_t n) {  // 0 .. n - 1
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>((g_state >> 33) % n);
}
static double Unit() { return (static_cast<double>(Rand(2001)) - 1000.0) / 250.0; }  // -4 .. 4

template <class F>
static bool Throws(F f) {
    try {
        f();
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}

template <class T>
static std::unique_ptr<T[]> Exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size() + 1]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

static const uint32_t kPoints2D = 7;

static ModelCamera Camera(uint32_t id, bool bogus) {
    ModelCamera c;
    c.camera_id = id;
    c.model = 2;
    c.width = 1000;
    c.height = 800;
    c.params = {bogus ? 5.0 : 800.0, 500.0, 400.0, 0.05};
    return c;
}

// nimg images (ids 10, 12, ..) of kPoints2D points2D; image `blind` (an index, or nimg for none) sees no point
static SparseModel RandomModel(uint32_t nimg, uint32_t blind, bool bogus_camera, bool nan_pose) {
    SparseModel m;
    m.cameras.push_back(Camera(1, false));
    m.cameras.push_back(Camera(2, bogus_camera));
    for (uint32_t i = 0; i < nimg; ++i) {
        ModelImage im;
        im.image_id = 10 + 2 * i;
        im.camera_id = i == 1 ? 2 : 1;
        const double q[4] = {1.0 + Unit(), Unit(), Unit(), Unit()};
        const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (int k = 0; k < 4; ++k) im.qvec[k] = n > 0 ? q[k] / n : (k == 0);
        for (int k = 0; k < 3; ++k) im.tvec[k] = Unit();
        if (nan_pose && i == 0) im.tvec[1] = std::nan("");
        im.name = "i" + std::to_string(i);
        im.points2D.resize(kPoints2D);
        m.images.push_back(im);
    }
    const uint32_t npts = Rand(3 * nimg + 1);
    for (uint32_t j = 0; j < npts; ++j) {
        ModelPoint3D p;
        p.point3D_id = 5 + 3 * j;
        for (int k = 0; k < 3; ++k) p.xyz[k] = Unit();
        const uint32_t len = 2 + Rand(4);
        for (uint32_t e = 0; e < len; ++e) {
            const uint32_t i = Rand(nimg), k = Rand(kPoints2D);
            if (i == blind || m.images[i].points2D[k].point3D_id != kInvalidPoint3DId) continue;
            m.images[i].points2D[k].point3D_id = p.point3D_id;
            p.track.emplace_back(m.images[i].image_id, k);
        }
        if (p.track.size() >= 2) {
            m.points3D.push_back(p);
        } else {
            for (const auto& e : p.track) m.images[(e.first - 10) / 2].points2D[e.second].point3D_id = kInvalidPoint3DId;
        }
    }
    return m;
}

static MapperCandidate Candidate(uint32_t id, uint32_t camera, uint32_t n) {
    MapperCandidate c;
    c.image_id = id;
    c.camera_id = camera;
    for (uint32_t k = 0; k < n; ++k) {
        c.xy.push_back(k == 2 ? std::nan("") : 50.0 * k + id);
        c.xy.push_back(40.0 * k);
    }
    return c;
}

int main() {
    size_t cases = 0;
    for (uint32_t round = 0; round < 600; ++round) {
        // ---- 21.1, 21.2: a pair into a model of 0 .. 3 images
        SparseModel m = RandomModel(Rand(4), 99, false, false);
        REQUIRE(CheckModel(m).empty());
        MapperOptions o;
        ModelIndex ix(m, o.BogusThresholds());
        const uint32_t n1 = 1 + Rand(9), n2 = 1 + Rand(9);
        const MapperCandidate c1 = Candidate(200, 1, n1), c2 = Candidate(100, 2, n2);
        std::vector<uint32_t> matches;
        std::set<uint32_t> used1, used2;
        for (uint32_t k = 0, n = Rand(12); k < n; ++k) {
            const uint32_t a = Rand(n1), b = Rand(n2);
            if (Rand(3) && (used1.count(a) || used2.count(b))) continue;  // (mostly one correspondence per point2D, as a graph pair gives)
            used1.insert(a);
            used2.insert(b);
            matches.push_back(a);
            matches.push_back(b);
        }
        const double q2[4] = {Unit(), Unit(), Unit(), Unit()}, t2[3] = {Unit(), Unit(), Unit()};
        const FlatInitialPair f = PlanInitialPair(m.cameras[0], m.cameras[1], c1, c2, matches, q2, t2);
        const amc_pair_tri_problem pb = f.Problem();
        REQUIRE(pb.num_cameras == 2 && pb.num_images == 2 && pb.num_pairs == 1 && f.camera_params.size() == 24);
        REQUIRE(f.pair_offsets.size() == 2 && f.pair_offsets[0] == 0 && f.pair_offsets[1] == matches.size() / 2);
        REQUIRE(f.corr_xy1.size() == matches.size() && f.corr_xy2.size() == matches.size());
        const auto xy1 = Exact(f.corr_xy1);
        const auto xy2 = Exact(f.corr_xy2);
        for (size_t k = 0; k < f.NumCorrs(); ++k) {
            REQUIRE(f.corrs[2 * k] < n1 && f.corrs[2 * k + 1] < n2);
            const double want = c1.xy[2 * f.corrs[2 * k] + 1];
            REQUIRE(xy1[2 * k + 1] == want && xy2[2 * k + 1] == c2.xy[2 * f.corrs[2 * k + 1] + 1]);
        }
        std::vector<uint8_t> accepted(f.NumCorrs() + 1, 0);
        std::vector<double> xyz(3 * f.NumCorrs() + 3, 0.0);
        for (size_t k = 0; k < f.NumCorrs(); ++k) {
            accepted[k] = Rand(3) != 0;
            for (int c = 0; c < 3; ++c) xyz[3 * k + c] = Rand(40) == 0 ? std::nan("") : Unit();
        }
        const auto acc = Exact(accepted);
        const auto X = Exact(xyz);
        const size_t before_images = m.images.size(), before_points = m.points3D.size();
        const size_t created = ApplyInitialPair(c1, c2, f, acc.get(), X.get(), &m, &ix);
        REQUIRE(CheckModel(m).empty());
        REQUIRE(m.images.size() == before_images + 2 && m.points3D.size() == before_points + created);
        size_t want_created = 0;
        {
            std::set<uint32_t> s1, s2;
            for (size_t k = 0; k < f.NumCorrs(); ++k)
                if (accepted[k] && !s1.count(f.corrs[2 * k]) && !s2.count(f.corrs[2 * k + 1])) {
                    s1.insert(f.corrs[2 * k]);
                    s2.insert(f.corrs[2 * k + 1]);
                    want_created += 1;
                }
        }
        REQUIRE(created == want_created);
        for (size_t j = before_points; j < m.points3D.size(); ++j)
            REQUIRE(m.points3D[j].track.size() == 2 && m.points3D[j].track[0].first == 200 && m.points3D[j].track[1].first == 100 && m.points3D[j].error == -1.0);
        REQUIRE(m.images[before_images].qvec[0] == 1.0 && m.images[before_images + 1].qvec[0] == q2[3] && m.images[before_images + 1].tvec[2] == t2[2]);
        REQUIRE(Throws([&] { ApplyInitialPair(c1, c2, f, acc.get(), X.get(), &m, &ix); }));  // already in the model
        if (n1 > 0) {
            std::vector<uint32_t> bad = matches;
            bad.push_back(n1);
            bad.push_back(0);
            REQUIRE(Throws([&] { PlanInitialPair(m.cameras[0], m.cameras[1], c1, c2, bad, q2, t2); }));
        }
        ModelCamera unknown = m.cameras[0];
        unknown.model = 77;
        REQUIRE(Throws([&] { PlanInitialPair(unknown, m.cameras[1], c1, c2, matches, q2, t2); }));
        cases += 1;

        // ---- 21.1: the verdict
        o.init_min_num_inliers = 10;
        REQUIRE(InitialPairAccepted(true, 10, 0.5, 0.5, o) && !InitialPairAccepted(false, 10, 0.5, 0.5, o) && !InitialPairAccepted(true, 9, 0.5, 0.5, o));
        REQUIRE(!InitialPairAccepted(true, 10, -0.95, 0.5, o) && !InitialPairAccepted(true, 10, 0.5, kMapperDegToRad * 16.0, o));
        REQUIRE(!InitialPairAccepted(true, 10, std::nan(""), 0.5, o) && !InitialPairAccepted(true, 10, 0.5, std::nan(""), o));

        // ---- 21.3: the configuration and the normalisation
        const uint32_t nimg = Rand(26);
        SparseModel g = RandomModel(nimg, nimg ? Rand(nimg + 1) : 0, round % 3 == 0, round % 7 == 0);
        REQUIRE(CheckModel(g).empty());
        std::vector<uint32_t> reg;
        for (const ModelImage& im : g.images) reg.push_back(im.image_id);
        for (size_t i = reg.size(); i > 1; --i) std::swap(reg[i - 1], reg[Rand(static_cast<uint32_t>(i))]);
        std::set<uint32_t> existing;
        for (uint32_t id : reg)
            if (Rand(2)) existing.insert(id);
        const bool fix = Rand(2) != 0;
        if (reg.size() < 2) {
            REQUIRE(Throws([&] { GlobalBundleConfig(reg, existing, fix); }));
        } else {
            const BundleAdjustmentConfig c = GlobalBundleConfig(reg, existing, fix);
            REQUIRE(c.NumImages() == reg.size() && c.HasConstantCamPose(reg[0]) && c.NumPoints() == 0);
            REQUIRE(c.HasConstantCamPose(reg[1]) != c.HasConstantCamPositions(reg[1]));
            REQUIRE(c.HasConstantCamPose(reg[1]) == (fix && existing.count(reg[1]) != 0));
            for (size_t i = 2; i < reg.size(); ++i) REQUIRE(c.HasConstantCamPose(reg[i]) == (fix && existing.count(reg[i]) != 0) && !c.HasConstantCamPositions(reg[i]));
        }
        const SparseModel before = g;
        const NormalizeResult nr = NormalizeModel(&g, reg);
        REQUIRE(nr.applied == (reg.size() >= 2));
        REQUIRE(g.images.size() == before.images.size() && g.points3D.size() == before.points3D.size());
        for (size_t i = 0; i < g.images.size(); ++i) {
            for (int k = 0; k < 4; ++k) REQUIRE(g.images[i].qvec[k] == before.images[i].qvec[k]);
            if (!nr.applied)
                for (int k = 0; k < 3; ++k) REQUIRE(g.images[i].tvec[k] == before.images[i].tvec[k] || before.images[i].tvec[k] != before.images[i].tvec[k]);
        }
        if (nr.applied && round % 7 != 0) REQUIRE(nr.scale > 0.0 && std::isfinite(nr.scale));
        REQUIRE(Throws([&] { NormalizeModel(&g, reg, 0.0); }) && Throws([&] { NormalizeModel(&g, reg, 10.0, 0.9, 0.1); }));
        {
            std::vector<uint32_t> stranger = reg;
            stranger.push_back(4242);
            stranger.push_back(4243);
            REQUIRE(Throws([&] { NormalizeModel(&g, stranger); }));
        }
        cases += 1;

        // ---- 21.4: FilterImages
        const std::vector<uint32_t> gone = PlanFilterImages(g, reg, o);
        if (reg.size() < kFilterImagesMinNumImages) REQUIRE(gone.empty());
        REQUIRE(std::set<uint32_t>(gone.begin(), gone.end()).size() == gone.size());
        const ModelIndex gx(g, o.BogusThresholds());
        for (uint32_t id : reg) {
            const ModelImage& im = g.images[gx.image.at(id)];
            bool any = false;
            for (const ModelPoint2D& p : im.points2D) any = any || p.point3D_id != kInvalidPoint3DId;
            const bool want = reg.size() >= kFilterImagesMinNumImages && (!any || gx.image_bogus[gx.image.at(id)]);
            REQUIRE((std::find(gone.begin(), gone.end(), id) != gone.end()) == want);
        }
        // (any image can be removed, filtered or not)
        std::vector<uint32_t> remove = gone;
        if (!reg.empty() && remove.empty()) remove.push_back(reg[Rand(static_cast<uint32_t>(reg.size()))]);
        for (uint32_t id : remove) {
            DeRegisterImage(&g, id);
            REQUIRE(CheckModel(g).empty());
            for (const ModelImage& im : g.images) REQUIRE(im.image_id != id);
            for (const ModelPoint3D& p : g.points3D) {
                REQUIRE(p.track.size() >= 2);
                for (const auto& e : p.track) REQUIRE(e.first != id);
            }
            REQUIRE(Throws([&] { DeRegisterImage(&g, id); }));
        }
        cases += 1;

        // ---- the second group of the ranking
        FlatVisibility fv;
        fv.cand_ids = {7, 8, 9};
        const uint32_t nobs[3] = {9, 9, 9}, nvis[3] = {5, 6, 7};
        const uint64_t score[3] = {50, 60, 70};
        o.abs_pose_min_num_inliers = 1;
        o.image_selection_method = ImageSelectionMethod::MIN_UNCERTAINTY;
        const std::set<uint32_t> filtered{9};
        const std::vector<uint32_t> plain = RankNextImages(fv, nobs, nvis, score, o, MapperTrials());
        const std::vector<uint32_t> ranked = RankNextImages(fv, nobs, nvis, score, o, MapperTrials(), &filtered);
        REQUIRE(plain.size() == 3 && plain[0] == 9 && plain[1] == 8 && plain[2] == 7);
        REQUIRE(ranked.size() == 3 && ranked[0] == 8 && ranked[1] == 7 && ranked[2] == 9);
        cases += 1;
    }
    std::printf("ok %zu\n", cases);
    return 0;
}
