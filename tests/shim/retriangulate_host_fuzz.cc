// retriangulate_host_fuzz.cc — a stand-alone program for tests/test_retriangulate_cpu.py (built with
// -fsanitize=address,undefined together with csrc/host/model_io.cc and reconstruction.cc): the host half of
// retriangulate.  Seeded models and graphs are planned; the flat problem must pass retri_plan.h's
// checks, its rounds must be image-disjoint and its launches must cover every pair once under any bound; a made-up but
// consistent result is applied and the model is checked afterwards; then the corruptions: results with unknown actions,
// a Continue without a point, a Create onto a point, created positions that do not fit, and problems with offsets,
// indices, rounds and lists out of order in heap arrays of the exact sizes - each refused, none read through.  Prints
// "ok <cases>".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>

#include "../../pycolmap_amd/csrc/retri_plan.h"
#include "../../pycolmap_amd/csrc/host/reconstruction.h"
#include "../../pycolmap_amd/csrc/host/retriangulate_host.h"

using namespace amchost;
namespace retri = amc::retri;

#define REQUIRE(cond)                                                      \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static uint64_t g_state = 11;
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
    return g;
}

static size_t NumObservations(const SparseModel& m) {
    size_t n = 0;
    for (const ModelPoint3D& p : m.points3D) n += p.track.size();
    return n;
}

// heap copies of the exact sizes, so that a read past an array is seen
template <class T>
static std::unique_ptr<T[]> Exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

// a result that fits the problem, made the way the device makes it: round by round on the state the rounds leave
struct Result {
    std::vector<uint8_t> ran, action;
    std::vector<uint64_t> created_offsets{0};
    std::vector<double> created_xyz;
};
static Result MakeResult(const FlatRetri& f) {
    Result r;
    std::vector<int64_t> point(f.obs_point.begin(), f.obs_point.end());
    r.action.assign(f.NumCorrs(), AMC_RETRI_NONE);
    for (size_t p = 0; p < f.NumPairs(); ++p) {
        r.ran.push_back(Rand(4) != 0);
        uint64_t made = 0;
        for (uint64_t k = f.pair_offsets[p]; k < f.pair_offsets[p + 1] && r.ran[p]; ++k) {
            const uint32_t o1 = f.corr_obs[2 * k], o2 = f.corr_obs[2 * k + 1];
            if (point[o1] >= 0 && point[o2] >= 0) continue;
            if (Rand(3) == 0) continue;
            if (point[o1] >= 0) {
                r.action[k] = AMC_RETRI_CONTINUE_1TO2;
                point[o2] = point[o1];
            } else if (point[o2] >= 0) {
                r.action[k] = AMC_RETRI_CONTINUE_2TO1;
                point[o1] = point[o2];
            } else {
                r.action[k] = AMC_RETRI_CREATED;
                point[o1] = point[o2] = static_cast<int64_t>(f.point3D_ids.size() + k);
                for (int d = 0; d < 3; ++d) r.created_xyz.push_back(0.5 * static_cast<double>(k) + d);
                made += 1;
            }
        }
        r.created_offsets.push_back(r.created_offsets.back() + made);
    }
    return r;
}

static uint64_t OneModel(uint32_t round) {
    uint64_t cases = 0;
    SparseModel m = RandomModel(3 + Rand(6), round % 4 == 0);
    REQUIRE(CheckModel(m).empty());
    const CorrespondenceGraph g = RandomGraph(m);
    TriangulatorOptions o;
    o.re_max_trials = static_cast<int>(Rand(3));
    o.re_min_ratio = 0.1 * Rand(11);
    o.ignore_two_view_tracks = Rand(2) != 0;
    ModelIndex ix(m, o);
    RetriTrials trials;
    for (const auto& pc : g.ImagePairs())
        if (Rand(4) == 0) trials[pc.first] = static_cast<int>(Rand(3));
    const FlatRetri f = PlanRetriangulation(g, m, ix, o, trials);
    const amc_retri_problem pb = f.Problem();
    REQUIRE(retri::check_problem(pb).empty());
    REQUIRE(f.obs_id.size() == f.obs_image.size() && f.corr_obs.size() == 2 * f.NumCorrs() && f.pair_offsets.back() == f.NumCorrs());
    // every pair is statically eligible, the rounds are image-disjoint and every pair sits in its lowest feasible round
    std::vector<std::set<uint32_t>> in_round(f.NumRounds());
    for (size_t r = 0; r < f.NumRounds(); ++r) {
        REQUIRE(f.round_offsets[r + 1] > f.round_offsets[r]);
        for (uint64_t p = f.round_offsets[r]; p < f.round_offsets[r + 1]; ++p) {
            const uint32_t a = f.pair_ids[p].first, b = f.pair_ids[p].second;
            REQUIRE(a < b && a != 999 && b != 999 && o.re_max_trials > 0);
            REQUIRE(!ix.image_bogus[ix.image.at(a)] && !ix.image_bogus[ix.image.at(b)]);
            REQUIRE(f.pair_offsets[p + 1] - f.pair_offsets[p] == g.NumCorrespondencesBetweenImages(a, b));
            const auto t = trials.find(RetriPairKey(a, b));
            REQUIRE(t == trials.end() || t->second < o.re_max_trials);
            REQUIRE(in_round[r].insert(a).second && in_round[r].insert(b).second);
            if (p > f.round_offsets[r]) REQUIRE(f.pair_ids[p - 1] < f.pair_ids[p]);
            for (size_t lower = 0; lower < r; ++lower) REQUIRE(in_round[lower].count(a) || in_round[lower].count(b));
        }
    }
    // the launches cover every pair once, in order, within rounds, under any bound
    for (const uint64_t bound : {uint64_t(1), uint64_t(1 + Rand(12)), retri::kMaxLaunchCorrs}) {
        uint64_t next = 0;
        for (const retri::Launch& l : retri::plan_launches(pb, bound)) {
            REQUIRE(l.first == next && l.last > l.first);
            REQUIRE(l.last == l.first + 1 || f.pair_offsets[l.last] - f.pair_offsets[l.first] <= bound);
            size_t r = 0;
            while (f.round_offsets[r + 1] <= l.first) ++r;
            REQUIRE(l.last <= f.round_offsets[r + 1]);
            next = l.last;
        }
        REQUIRE(next == f.NumPairs());
        cases += 1;
    }
    // the plan refuses a call above the bound it is given, naming the size, and plans one exactly at it
    if (f.NumCorrs() > 0) {
        std::string what;
        try {
            PlanRetriangulation(g, m, ix, o, trials, f.NumCorrs() - 1);
        } catch (const std::invalid_argument& e) {
            what = e.what();
        }
        REQUIRE(what.find("hold " + std::to_string(f.NumCorrs()) + " correspondences, more than " + std::to_string(f.NumCorrs() - 1)) != std::string::npos);
        REQUIRE(PlanRetriangulation(g, m, ix, o, trials, f.NumCorrs()).NumCorrs() == f.NumCorrs());
        cases += 2;
    }
    // a consistent result goes in
    const Result res = MakeResult(f);
    {
        SparseModel work = m;
        ModelIndex wix(work, o);
        std::set<uint64_t> modified;
        RetriTrials wt = trials;
        const auto ran = Exact(res.ran), act = Exact(res.action);
        const auto coff = Exact(res.created_offsets);
        const auto cxyz = Exact(res.created_xyz);
        const size_t before = NumObservations(m);
        const RetriApplied a = ApplyRetriResult(f, ran.get(), act.get(), coff.get(), cxyz.get(), &work, &wix, &modified, &wt);
        REQUIRE(CheckModel(work).empty());
        REQUIRE(NumObservations(work) == before + a.num_tris && a.num_tris == a.num_continued + 2 * a.num_created);
        REQUIRE(work.points3D.size() == m.points3D.size() + a.num_created && a.num_created == res.created_offsets.back());
        size_t spent = 0, had = 0;
        for (const auto& kv : wt) spent += kv.second;
        for (const auto& kv : trials) had += kv.second;
        REQUIRE(spent == had + a.num_pairs_run + f.bogus_spent.size());
        for (const auto& kv : wt) REQUIRE(kv.second <= std::max(o.re_max_trials, trials.count(kv.first) ? trials.at(kv.first) : 0));
        cases += 1;
    }
    // results that do not fit are refused
    auto refused = [&](const Result& bad) {
        SparseModel work = m;
        ModelIndex wix(work, o);
        std::set<uint64_t> modified;
        RetriTrials wt = trials;
        const auto ran = Exact(bad.ran), act = Exact(bad.action);
        const auto coff = Exact(bad.created_offsets);
        const auto cxyz = Exact(bad.created_xyz);
        return Throws([&] { ApplyRetriResult(f, ran.get(), act.get(), coff.get(), cxyz.get(), &work, &wix, &modified, &wt); });
    };
    for (uint64_t k = 0; k < f.NumCorrs(); ++k) {
        size_t p = 0;
        while (f.pair_offsets[p + 1] <= k) ++p;
        if (!res.ran[p]) continue;
        Result bad = res;
        bad.action[k] = 4 + Rand(250);
        REQUIRE(refused(bad));
        cases += 1;
        if (res.action[k] == AMC_RETRI_NONE && f.obs_point[f.corr_obs[2 * k]] >= 0 && f.obs_point[f.corr_obs[2 * k + 1]] >= 0) {
            for (const uint8_t a : {AMC_RETRI_CONTINUE_1TO2, AMC_RETRI_CONTINUE_2TO1, AMC_RETRI_CREATED}) {
                bad = res;
                bad.action[k] = a;  // onto a point (and for a Create without a position)
                REQUIRE(refused(bad));
                cases += 1;
            }
        }
        if (res.action[k] == AMC_RETRI_CREATED) {
            bad = res;
            bad.action[k] = AMC_RETRI_NONE;  // a position too many
            REQUIRE(refused(bad));
            bad = res;
            for (size_t q = p + 1; q < bad.created_offsets.size(); ++q) bad.created_offsets[q] -= 1;  // a position too few
            REQUIRE(refused(bad));
            cases += 2;
        }
    }
    // corrupted problems are refused before anything is read through them
    if (f.NumCorrs() > 0) {
        const auto check = [&](const FlatRetri& g2) {
            amc_retri_problem q = g2.Problem();
            const auto oi = Exact(g2.obs_image);
            const auto op = Exact(g2.obs_point);
            const auto pi = Exact(g2.pair_images);
            const auto po = Exact(g2.pair_offsets);
            const auto co = Exact(g2.corr_obs);
            const auto ro = Exact(g2.round_offsets);
            q.obs_image = oi.get();
            q.obs_point = op.get();
            q.pair_images = pi.get();
            q.pair_offsets = po.get();
            q.corr_obs = co.get();
            q.round_offsets = ro.get();
            return retri::check_problem(q);
        };
        REQUIRE(check(f).empty());
        FlatRetri b = f;
        b.corr_obs[Rand(static_cast<uint32_t>(b.corr_obs.size()))] = static_cast<uint32_t>(f.obs_image.size()) + Rand(3);
        REQUIRE(!check(b).empty());
        b = f;
        b.obs_point[Rand(static_cast<uint32_t>(b.obs_point.size()))] = static_cast<int32_t>(f.point3D_ids.size()) + static_cast<int32_t>(Rand(3));
        REQUIRE(!check(b).empty());
        b = f;
        b.obs_point[Rand(static_cast<uint32_t>(b.obs_point.size()))] = -2;
        REQUIRE(!check(b).empty());
        b = f;
        b.obs_image[Rand(static_cast<uint32_t>(b.obs_image.size()))] = static_cast<uint32_t>(m.images.size());
        REQUIRE(!check(b).empty());
        b = f;
        b.pair_images[Rand(static_cast<uint32_t>(b.pair_images.size()))] = static_cast<uint32_t>(m.images.size()) + 5;
        REQUIRE(!check(b).empty());
        b = f;
        b.pair_offsets[0] = 1;
        REQUIRE(!check(b).empty());
        b = f;  // more correspondences than a call may hold: refused by the count, before corr_obs is read
        b.pair_offsets.back() = AMC_RETRI_MAX_CORRS + 1;
        REQUIRE(check(b).find("more than 16777216") != std::string::npos);
        b = f;  // an observation and points that no correspondence can use
        b.obs_image.resize(2 * f.NumCorrs() + 1, 0);
        b.obs_point.resize(2 * f.NumCorrs() + 1, -1);
        REQUIRE(check(b).find("observations, more than two per correspondence") != std::string::npos);
        {
            amc_retri_problem q = f.Problem();
            static const double three[3] = {0.0, 0.0, 0.0};
            q.point_xyz = three;  // (far too short: the problem is refused by the count, before point_xyz is read)
            q.num_points = 2 * f.NumCorrs() + 1;
            REQUIRE(retri::check_problem(q).find("points, more than two per correspondence") != std::string::npos);
        }
        b = f;
        b.round_offsets.back() += 1;
        REQUIRE(!check(b).empty());
        b = f;
        b.round_offsets[0] = 1;
        REQUIRE(!check(b).empty());
        b = f;  // the first correspondence once more in its pair: an observation twice
        {
            size_t p = 0;
            while (f.pair_offsets[p + 1] == f.pair_offsets[p]) ++p;
            const uint64_t k = f.pair_offsets[p];
            b.corr_obs.insert(b.corr_obs.begin() + 2 * k, {f.corr_obs[2 * k], f.corr_obs[2 * k + 1]});
            b.corr_two_view.push_back(0);
            for (size_t q = p + 1; q < b.pair_offsets.size(); ++q) b.pair_offsets[q] += 1;
        }
        REQUIRE(check(b).find("twice") != std::string::npos);
        b = f;  // a correspondence turned round: observations of the other image
        std::swap(b.corr_obs[0], b.corr_obs[1]);
        REQUIRE(!check(b).empty());
        if (f.NumRounds() > 1) {
            // all pairs in one round: an image of round 2 is in round 1 too (the lowest feasible round was taken)
            b = f;
            b.round_offsets.assign({0, f.NumPairs()});
            REQUIRE(check(b).find("two pairs") != std::string::npos);
            cases += 1;
        }
        cases += 14;
    }
    amc_retri_opts bad_opts{2.0, 5.0, 1.5, 0.2};
    REQUIRE(retri::check_options(bad_opts).empty());
    bad_opts.create_max_angle_error = 0.0;
    REQUIRE(!retri::check_options(bad_opts).empty());
    bad_opts = {2.0, -1.0, 1.5, 0.2};
    REQUIRE(!retri::check_options(bad_opts).empty());
    bad_opts = {2.0, 5.0, 1.5, std::nan("")};
    REQUIRE(!retri::check_options(bad_opts).empty());
    // a graph that names a point2D the model does not hold
    if (f.NumCorrs() > 0) {
        SparseModel small = m;
        for (ModelImage& im : small.images)
            if (im.image_id == f.pair_ids[0].first) {
                for (ModelPoint3D& p : small.points3D)
                    p.track.erase(std::remove_if(p.track.begin(), p.track.end(), [&](const std::pair<uint32_t, uint32_t>& e) { return e.first == im.image_id; }), p.track.end());
                im.points2D.clear();
            }
        const ModelIndex six(small, o);
        bool non_empty = false;
        for (size_t p = 0; p < f.NumPairs(); ++p) non_empty = non_empty || (f.pair_ids[p].first == f.pair_ids[0].first && f.pair_offsets[p + 1] > f.pair_offsets[p]);
        if (non_empty) {
            REQUIRE(Throws([&] { PlanRetriangulation(g, small, six, o, trials); }));
            cases += 1;
        }
    }
    return cases;
}

int main() {
    uint64_t cases = 0;
    for (uint32_t round = 0; round < 300; ++round) cases += OneModel(round);
    // the colouring on its own: a star, a path and a complete graph
    {
        std::vector<std::pair<uint32_t, uint32_t>> star, path, full;
        for (uint32_t i = 2; i < 40; ++i) star.emplace_back(1, i);
        for (uint32_t i = 1; i < 40; ++i) path.emplace_back(i, i + 1);
        for (uint32_t a = 1; a <= 8; ++a)
            for (uint32_t b = a + 1; b <= 8; ++b) full.emplace_back(a, b);
        const std::vector<uint32_t> s = ColourRetriRounds(star), p = ColourRetriRounds(path), c = ColourRetriRounds(full);
        for (size_t i = 0; i < s.size(); ++i) REQUIRE(s[i] == i);
        for (size_t i = 0; i < p.size(); ++i) REQUIRE(p[i] == i % 2);
        REQUIRE(*std::max_element(c.begin(), c.end()) <= 2 * 7 - 2);
        REQUIRE(ColourRetriRounds({}).empty());
        cases += 4;
    }
    std::printf("ok %llu\n", static_cast<unsigned long long>(cases));
    return 0;
}
