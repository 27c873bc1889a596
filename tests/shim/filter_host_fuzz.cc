// filter_host_fuzz.cc — a stand-alone program for tests/test_filter_cpu.py (built with -fsanitize=address,undefined
// together with csrc/host/model_io.cc and reconstruction.cc): the host half of the point filter.
// Seeded models are flattened (every point, an id set, the ids of some images), the flat problem passes
// filter_plan.h's checks and gives the two classes; results with every verdict pattern are applied and the model
// afterwards is checked element by element, with the count of filter_plan.h; observations and points are deleted one
// by one down to the empty model.  Then the corruptions: offsets, indices and models out of range in heap arrays of the
// exact sizes, cross references that name nothing, a result for another model, an unknown verdict - each refused, none
// read through.  Prints "ok <cases>".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>

#include "../../pycolmap_amd/csrc/filter_plan.h"
#include "../../pycolmap_amd/csrc/host/reconstruction.h"

using namespace amchost;
namespace filt = amc::filt;

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

// a consistent model: 2 cameras, nimg images of 12 points2D each, points with tracks of 0 .. 8 elements (distinct points2D)
static SparseModel RandomModel(uint32_t seed) {
    g_state = 77 + seed;
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
    c.params = {800.0, 810.0, 500.0, 400.0, 0.01, 0.0, 0.0, 0.0};
    m.cameras.push_back(c);
    const uint32_t nimg = 2 + Rand(6);
    for (uint32_t i = 0; i < nimg; ++i) {
        ModelImage im;
        im.image_id = 20 + 3 * i;
        im.camera_id = Rand(2) ? 5 : 2;
        im.tvec[0] = 0.1 * i;
        im.tvec[2] = 6.0;
        for (int k = 0; k < 12; ++k) {
            ModelPoint2D p;
            p.x = 10.0 * k + i;
            p.y = 5.0 * k;
            im.points2D.push_back(p);
        }
        m.images.push_back(im);
    }
    const uint32_t npts = Rand(14);
    for (uint32_t j = 0; j < npts; ++j) {
        ModelPoint3D p;
        p.point3D_id = 1000 + 7 * j;
        p.xyz[0] = 0.1 * j;
        p.xyz[2] = 1.0;
        p.error = 0.25 * j;
        const uint32_t want = Rand(9);
        for (uint32_t k = 0; k < want; ++k) {
            const uint32_t i = Rand(nimg), idx = Rand(12);
            if (m.images[i].points2D[idx].point3D_id != kInvalidPoint3DId) continue;
            m.images[i].points2D[idx].point3D_id = p.point3D_id;
            p.track.emplace_back(m.images[i].image_id, idx);
        }
        m.points3D.push_back(p);
    }
    return m;
}

static std::map<uint64_t, ModelPoint3D> ById(const SparseModel& m) {
    std::map<uint64_t, ModelPoint3D> out;
    for (const ModelPoint3D& p : m.points3D) out[p.point3D_id] = p;
    return out;
}

// applies (verdict, deleted, error) and compares the model with what 16.5 says must come out
static void ApplyAndCheck(const SparseModel& model, const FlatFilter& f, const std::vector<uint8_t>& verdict,
                          const std::vector<uint8_t>& deleted, const std::vector<double>& error) {
    SparseModel m = model;
    const uint64_t want_count = filt::count_filtered(f.track_offsets.data(), f.point_ids.size(), verdict.data(), deleted.data());
    const size_t count = ApplyFilterResult(f, verdict.data(), deleted.data(), error.data(), &m);
    REQUIRE(count == want_count);
    REQUIRE(CheckModel(m).empty());
    const auto after = ById(m);
    size_t kept = 0;
    for (size_t j = 0; j < model.points3D.size(); ++j) {
        const ModelPoint3D& p = model.points3D[j];
        const auto it = after.find(p.point3D_id);
        if (verdict[j] == AMC_FILTER_NOT_SELECTED) {
            REQUIRE(it != after.end() && it->second.track == p.track && it->second.error == p.error);
            ++kept;
        } else if (verdict[j] == AMC_FILTER_KEPT) {
            REQUIRE(it != after.end() && it->second.error == error[j]);
            std::vector<std::pair<uint32_t, uint32_t>> want;
            for (size_t k = 0; k < p.track.size(); ++k)
                if (!deleted[f.track_offsets[j] + k]) want.push_back(p.track[k]);
            REQUIRE(it->second.track == want);
            ++kept;
        } else {
            REQUIRE(it == after.end());
        }
    }
    REQUIRE(kept == m.points3D.size());
    REQUIRE(ComputeNumObservations(m) + 0 <= ComputeNumObservations(model));
}

template <class T>
static std::unique_ptr<T[]> Exact(const std::vector<T>& v) {  // a heap array of exactly v.size() elements
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
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

int main() {
    size_t cases = 0;
    for (uint32_t seed = 0; seed < 150; ++seed) {
        const SparseModel model = RandomModel(seed);
        REQUIRE(CheckModel(model).empty());
        const size_t npts = model.points3D.size();
        // every point, an id set (with an id that does not exist), the ids of some images
        std::vector<uint64_t> ids = {999999};
        for (size_t j = 0; j < npts; j += 2) ids.push_back(model.points3D[j].point3D_id);
        const std::vector<uint64_t> in_images = Point3DIdsInImages(model, {model.images[0].image_id, model.images.back().image_id});
        const std::vector<uint64_t>* sets[3] = {nullptr, &ids, &in_images};
        for (const std::vector<uint64_t>* set : sets) {
            const FlatFilter f = FlattenForFilter(model, set);
            const amc_filter_problem pb = f.Problem();
            REQUIRE(filt::check_problem(pb).empty());
            REQUIRE(pb.num_points == npts && f.track_offsets.back() == ComputeNumObservations(model));
            REQUIRE(npts == 0 || (set == nullptr) == (pb.selected == nullptr));  // (without points there is nothing to select)
            size_t nsel = 0;
            for (size_t j = 0; j < npts; ++j) {
                REQUIRE(f.track_offsets[j + 1] - f.track_offsets[j] == model.points3D[j].track.size());
                const bool want = !set || std::find(set->begin(), set->end(), model.points3D[j].point3D_id) != set->end();
                REQUIRE(!set || (f.selected[j] != 0) == want);
                nsel += want;
            }
            std::vector<uint32_t> loc, opt, wave;
            filt::plan_batch(pb, 0, npts, 3, &loc, &opt, &wave);
            REQUIRE(opt.size() == f.obs_image.size() && loc.size() == npts + 1);
            for (size_t j = 0; j <= npts; ++j) REQUIRE(loc[j] == f.track_offsets[j]);
            size_t nwave = 0;
            for (size_t j = 0; j < npts; ++j)
                nwave += model.points3D[j].track.size() >= 3 && (!set || f.selected[j]);
            REQUIRE(wave.size() == nwave && nwave <= nsel);
            for (size_t o = 0; o < opt.size(); ++o) REQUIRE(f.track_offsets[opt[o]] <= o && o < f.track_offsets[opt[o] + 1]);
            ++cases;
        }
        const FlatFilter f = FlattenForFilter(model, nullptr);
        const size_t nobs = f.obs_image.size();
        // every verdict alone, then seeded mixtures
        for (int pattern = 0; pattern < 5 + 3; ++pattern) {
            std::vector<uint8_t> verdict(npts), deleted(nobs, 0);
            std::vector<double> error(npts);
            for (size_t j = 0; j < npts; ++j) {
                verdict[j] = static_cast<uint8_t>(pattern < 5 ? pattern : Rand(5));
                error[j] = 1.5 + j + pattern;
                if (verdict[j] == AMC_FILTER_KEPT || verdict[j] == AMC_FILTER_ANGLE)
                    for (uint64_t o = f.track_offsets[j]; o < f.track_offsets[j + 1]; ++o) deleted[o] = Rand(3) == 0;
            }
            ApplyAndCheck(model, f, verdict, deleted, error);
            if (npts) {
                std::vector<double> e(npts, 0.125);
                SparseModel m = model;
                ApplyPointErrors(f, e.data(), &m);
                REQUIRE(m.points3D[npts - 1].error == 0.125 && ComputeMeanReprojectionError(m) == 0.125);
            }
            ++cases;
        }
        // a result for another model, an unknown verdict
        if (npts) {
            std::vector<uint8_t> verdict(npts, AMC_FILTER_KEPT), deleted(nobs + 1, 0);
            std::vector<double> error(npts, 0.0);
            SparseModel fewer = model;
            fewer.points3D.pop_back();
            REQUIRE(Throws([&] { ApplyFilterResult(f, verdict.data(), deleted.data(), error.data(), &fewer); }));
            REQUIRE(Throws([&] { ApplyPointErrors(f, error.data(), &fewer); }));
            SparseModel longer = model;
            longer.points3D[0].track.emplace_back(model.images[0].image_id, 0);
            REQUIRE(Throws([&] { ApplyFilterResult(f, verdict.data(), deleted.data(), error.data(), &longer); }));
            verdict[npts - 1] = 5;
            SparseModel same = model;
            REQUIRE(Throws([&] { ApplyFilterResult(f, verdict.data(), deleted.data(), error.data(), &same); }));
            REQUIRE(same.points3D.size() == npts && CheckModel(same).empty());
            cases += 4;
        }
        // DeleteObservation and DeletePoint3D down to the empty model
        SparseModel m = model;
        while (!m.points3D.empty()) {
            const size_t j = Rand(static_cast<uint32_t>(m.points3D.size()));
            const ModelPoint3D p = m.points3D[j];
            const size_t before = m.points3D.size(), obs = ComputeNumObservations(m);
            if (p.track.empty() || Rand(3) == 0) {
                DeletePoint3D(&m, p.point3D_id);
                REQUIRE(m.points3D.size() == before - 1 && ComputeNumObservations(m) == obs - p.track.size());
                REQUIRE(Throws([&] { DeletePoint3D(&m, p.point3D_id); }));
            } else {
                const auto el = p.track[Rand(static_cast<uint32_t>(p.track.size()))];
                DeleteObservation(&m, el.first, el.second);
                if (p.track.size() <= 2) {
                    REQUIRE(m.points3D.size() == before - 1 && ComputeNumObservations(m) == obs - p.track.size());
                } else {
                    REQUIRE(m.points3D.size() == before && ComputeNumObservations(m) == obs - 1);
                    REQUIRE(m.points3D[j].track.size() == p.track.size() - 1);
                }
                REQUIRE(Throws([&] { DeleteObservation(&m, el.first, el.second); }));  // the point2D has no point now
            }
            REQUIRE(CheckModel(m).empty());
            ++cases;
        }
        REQUIRE(ComputeNumObservations(m) == 0 && ComputeMeanReprojectionError(m) == 0.0);
        REQUIRE(Throws([&] { DeleteObservation(&m, 9999, 0); }));
        REQUIRE(Throws([&] { DeleteObservation(&m, model.images[0].image_id, 12); }));
        // cross references that name nothing: the flattening refuses the model
        if (nobs) {
            size_t j = 0;
            while (model.points3D[j].track.empty()) ++j;
            SparseModel bad = model;
            bad.points3D[j].track[0].second = 4000;
            REQUIRE(Throws([&] { FlattenForFilter(bad, nullptr); }));
            bad = model;
            bad.points3D[j].track[0].first = 4000;
            REQUIRE(Throws([&] { FlattenForFilter(bad, nullptr); }));
            bad = model;
            bad.images[0].camera_id = 77;
            REQUIRE(Throws([&] { FlattenForFilter(bad, nullptr); }));
            bad = model;
            for (ModelImage& im : bad.images)
                for (ModelPoint2D& p2 : im.points2D)
                    if (p2.point3D_id == model.points3D[j].point3D_id) p2.point3D_id = 31337;
            REQUIRE(Throws([&] { FlattenForFilter(bad, nullptr); }));
            REQUIRE(Throws([&] { Point3DIdsInImages(model, {4000}); }));
            cases += 5;
        }
        // the flat problem's own checks, on heap arrays of the exact sizes
        {
            auto models = Exact(f.camera_models);
            auto icam = Exact(f.image_cameras);
            auto off = Exact(f.track_offsets);
            auto oimg = Exact(f.obs_image);
            amc_filter_problem pb = f.Problem();
            pb.camera_models = models.get();
            pb.image_cameras = icam.get();
            pb.track_offsets = off.get();
            pb.obs_image = oimg.get();
            REQUIRE(filt::check_problem(pb).empty());
            models[1] = 11;
            REQUIRE(!filt::check_problem(pb).empty());
            models[1] = -1;
            REQUIRE(!filt::check_problem(pb).empty());
            models[1] = 4;
            icam[0] = 2;
            REQUIRE(!filt::check_problem(pb).empty());
            icam[0] = 0;
            off[0] = 1;
            REQUIRE(!filt::check_problem(pb).empty());
            off[0] = 0;
            if (npts >= 2 && f.track_offsets[1] > 0) {
                off[1] = off[npts] + 1000;  // then it decreases, before anything is read at it
                REQUIRE(!filt::check_problem(pb).empty());
                off[1] = f.track_offsets[1];
            }
            if (nobs) {
                oimg[nobs - 1] = static_cast<uint32_t>(model.images.size());
                REQUIRE(!filt::check_problem(pb).empty());
                oimg[nobs - 1] = 0xFFFFFFFFu;
                REQUIRE(!filt::check_problem(pb).empty());
                oimg[nobs - 1] = 0;
                amc_filter_problem nul = pb;
                nul.obs_image = nullptr;
                REQUIRE(!filt::check_problem(nul).empty());
                nul = pb;
                nul.obs_xy = nullptr;
                REQUIRE(!filt::check_problem(nul).empty());
            }
            amc_filter_problem nul = pb;
            nul.track_offsets = nullptr;
            REQUIRE(!filt::check_problem(nul).empty());
            nul = pb;
            nul.qvec = nullptr;
            REQUIRE(!filt::check_problem(nul).empty());
            nul = pb;
            nul.camera_params = nullptr;
            REQUIRE(!filt::check_problem(nul).empty());
            REQUIRE(filt::check_problem(pb).empty());
            cases += 8;
        }
    }
    amc_filter_opts o{4.0, 1.5, 0, 0};
    REQUIRE(filt::check_options(o).empty());
    o.max_reproj_error = -1.0;
    REQUIRE(!filt::check_options(o).empty());
    o.max_reproj_error = std::strtod("nan", nullptr);
    REQUIRE(!filt::check_options(o).empty());
    o.max_reproj_error = 0.0;
    o.min_tri_angle = -0.0;
    REQUIRE(filt::check_options(o).empty());
    o.min_tri_angle = std::strtod("nan", nullptr);
    REQUIRE(!filt::check_options(o).empty());
    std::printf("ok %zu\n", cases);
    return 0;
}
