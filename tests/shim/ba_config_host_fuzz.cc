// ba_config_host_fuzz.cc — a stand-alone program for tests/test_ba_config_cpu.py (built with -fsanitize=address,undefined
// and run): the host half of BundleAdjuster (csrc/host/ba_config_host.h: the config, the set-up of DESIGN.md 15.12, the
// write-back) and the plan's checks with a point mask (csrc/ba_plan.h) on seeded random models and configs, valid and
// corrupted.  Valid: the flat problem is checked against the set-up's rules (every residual's image and point, the
// constant flags, the mask), make_plan accepts it with the mask and counts the variable columns without the constant
// points, and the write-back touches only what was in the problem.  Corrupted: a config id the model does not hold, a
// model whose cross references are broken, a mask that leaves a variable point with one observation or a constant point
// with none, each refused without a read past an array (the arrays are heap blocks of their exact sizes).
// Prints "ok <problems>" and returns 0.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../pycolmap_amd/csrc/ba_plan.h"
#include "../../pycolmap_amd/csrc/host/ba_config_host.h"

using namespace amchost;

namespace {

#define REQUIRE(cond)                                                      \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

template <class F>
bool throws(F f) {
    try {
        f();
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}

// ncam cameras, nimg images, npts points with tracks of length 1 .. 4 in distinct images; the ids descend
SparseModel random_model(std::mt19937& rng, size_t ncam, size_t nimg, size_t npts) {
    SparseModel m;
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    const int models[3] = {0, 2, 4};
    const size_t counts[3] = {3, 4, 8};
    for (size_t c = 0; c < ncam; ++c) {
        ModelCamera cam;
        cam.camera_id = static_cast<uint32_t>(10 + 3 * c);
        const int k = static_cast<int>(rng() % 3);
        cam.model = models[k];
        cam.width = 1000;
        cam.height = 800;
        cam.params.resize(counts[k]);
        for (double& v : cam.params) v = 500.0 + 100.0 * u(rng);
        m.cameras.push_back(cam);
    }
    for (size_t i = 0; i < nimg; ++i) {
        ModelImage im;
        im.image_id = static_cast<uint32_t>(100 + 7 * (nimg - 1 - i));  // descending: the model's order is not the ids'
        im.camera_id = m.cameras[rng() % ncam].camera_id;
        im.name = "image" + std::to_string(i);
        for (double& v : im.qvec) v = u(rng);
        for (double& v : im.tvec) v = u(rng);
        m.images.push_back(im);
    }
    for (size_t j = 0; j < npts; ++j) {
        ModelPoint3D p;
        p.point3D_id = 1000 + 11 * (npts - 1 - j);
        for (double& v : p.xyz) v = u(rng);
        const size_t len = std::min<size_t>(1 + rng() % 4, nimg);
        const size_t first = rng() % nimg;
        for (size_t k = 0; k < len; ++k) {
            ModelImage& im = m.images[(first + k) % nimg];
            if (rng() % 4 == 0) im.points2D.push_back(ModelPoint2D{u(rng), u(rng), kInvalidPoint3DId});  // a point2D without a point
            p.track.emplace_back(im.image_id, static_cast<uint32_t>(im.points2D.size()));
            im.points2D.push_back(ModelPoint2D{500.0 * u(rng), 400.0 * u(rng), p.point3D_id});
        }
        m.points3D.push_back(p);
    }
    return m;
}

BundleAdjustmentConfig random_config(std::mt19937& rng, const SparseModel& m) {
    BundleAdjustmentConfig c;
    for (const ModelImage& im : m.images)
        if (rng() % 2) {
            c.AddImage(im.image_id);
            const unsigned k = rng() % 4;
            if (k == 0) c.SetConstantCamPose(im.image_id);
            if (k == 1) c.SetConstantCamPositions(im.image_id, rng() % 2 ? std::vector<int>{0} : std::vector<int>{2, 1});
        }
    for (const ModelCamera& cam : m.cameras)
        if (rng() % 3 == 0) c.SetConstantCamIntrinsics(cam.camera_id);
    for (const ModelPoint3D& p : m.points3D) {
        const unsigned k = rng() % 6;
        if (k == 0) c.AddVariablePoint(p.point3D_id);
        if (k == 1) c.AddConstantPoint(p.point3D_id);
    }
    return c;
}

void check_flat(const SparseModel& m, const BundleAdjustmentConfig& cfg, const BaRefineFlags& f, const FlatBaConfig& fc) {
    const FlatBa& o = fc.flat;
    const size_t ncam = o.camera_models.size(), nimg = o.image_cameras.size(), npts = fc.point_at.size(), nobs = o.obs_image.size();
    REQUIRE(fc.camera_at.size() == ncam && fc.image_at.size() == nimg && o.xyz.size() == 3 * npts && fc.point_const.size() == npts);
    REQUIRE(o.camera_params.size() == 12 * ncam && o.camera_const.size() == 12 * ncam && o.qvec.size() == 4 * nimg &&
            o.tvec.size() == 3 * nimg && o.pose_const.size() == 6 * nimg && o.obs_point.size() == nobs && o.obs_xy.size() == 2 * nobs);
    std::vector<size_t> nres(npts, 0), per_image(nimg, 0);
    std::vector<char> cam_by_config(ncam, 0);
    for (size_t k = 0; k < nobs; ++k) {
        REQUIRE(o.obs_image[k] < nimg && o.obs_point[k] < npts);
        ++nres[o.obs_point[k]];
        ++per_image[o.obs_image[k]];
        // the residual is an element of the point's track in that image, at that pixel
        const ModelImage& im = m.images[fc.image_at[o.obs_image[k]]];
        const ModelPoint3D& p = m.points3D[fc.point_at[o.obs_point[k]]];
        bool found = false;
        for (const auto& el : p.track)
            found = found || (el.first == im.image_id && im.points2D[el.second].x == o.obs_xy[2 * k] && im.points2D[el.second].y == o.obs_xy[2 * k + 1]);
        REQUIRE(found);
        REQUIRE(p.track.size() >= 2);
        // an image outside the config carries residuals of listed points only
        if (!cfg.HasImage(im.image_id)) REQUIRE(cfg.HasPoint(p.point3D_id));
    }
    size_t constants = 0;
    for (size_t j = 0; j < npts; ++j) {
        const ModelPoint3D& p = m.points3D[fc.point_at[j]];
        REQUIRE(nres[j] >= 1 && nres[j] <= p.track.size());
        const bool constant = p.track.size() > nres[j] || cfg.HasConstantPoint(p.point3D_id);
        REQUIRE(fc.point_const[j] == (constant ? 1 : 0));
        REQUIRE(constant || nres[j] >= 2);
        constants += constant;
    }
    REQUIRE(constants == fc.num_constant_points);
    for (size_t i = 0; i < nimg; ++i) {
        const ModelImage& im = m.images[fc.image_at[i]];
        REQUIRE(per_image[i] >= 1);
        const bool inside = cfg.HasImage(im.image_id);
        if (inside) cam_by_config[o.image_cameras[i]] = 1;
        for (int k = 0; k < 6; ++k) {
            bool want = !inside || !f.refine_extrinsics || cfg.HasConstantCamPose(im.image_id);
            if (!want && k >= 3 && cfg.HasConstantCamPositions(im.image_id))
                for (int idx : cfg.ConstantCamPositions(im.image_id)) want = want || idx == k - 3;
            REQUIRE(o.pose_const[6 * i + k] == (want ? 1 : 0));
        }
        REQUIRE(m.cameras[fc.camera_at[o.image_cameras[i]]].camera_id == im.camera_id);
    }
    for (size_t c = 0; c < ncam; ++c) {
        const ModelCamera& cam = m.cameras[fc.camera_at[c]];
        const bool all_const = !cam_by_config[c] || cfg.IsConstantCamIntrinsics(cam.camera_id) ||
                               (!f.refine_focal_length && !f.refine_principal_point && !f.refine_extra_params);
        bool any_variable = false;
        for (int k = 0; k < 12; ++k) any_variable = any_variable || !o.camera_const[12 * c + k];
        REQUIRE(!all_const || !any_variable);
        for (size_t k = cam.params.size(); k < 12; ++k) REQUIRE(o.camera_const[12 * c + k] == 1);
    }
}

}  // namespace

int main() {
    std::mt19937 rng(11);
    int problems = 0, with_outside = 0, with_skipped = 0, with_constants = 0;
    for (int round = 0; round < 300; ++round) {
        const size_t ncam = 1 + rng() % 3, nimg = 2 + rng() % 6, npts = rng() % 30;
        SparseModel m = random_model(rng, ncam, nimg, npts);
        REQUIRE(CheckModel(m).empty());
        const BundleAdjustmentConfig cfg = random_config(rng, m);
        BaRefineFlags f;
        f.refine_focal_length = rng() % 2;
        f.refine_principal_point = rng() % 2;
        f.refine_extra_params = rng() % 2;
        f.refine_extrinsics = rng() % 4 != 0;
        FlatBaConfig fc = FlattenForBundleAdjuster(m, cfg, f);
        check_flat(m, cfg, f, fc);
        REQUIRE(cfg.NumResiduals(m) >= 2 * fc.flat.obs_image.size());
        ++problems;
        with_skipped += fc.skipped_points != 0;
        with_constants += fc.num_constant_points != 0;
        for (uint32_t i : fc.image_at) with_outside += !cfg.HasImage(m.images[i].image_id) ? 1 : 0;
        // the plan with the mask: accepted, and the constant points have no column
        amc_ba_problem pb = fc.flat.Problem();
        amc::ba::Plan plan;
        REQUIRE(amc::ba::make_plan(pb, fc.point_const.data(), &plan).empty());
        uint64_t nvar = 0;
        for (uint8_t v : plan.cvar) nvar += v;
        for (uint8_t v : plan.ivar) nvar += v;
        for (size_t j = 0; j < fc.point_const.size(); ++j) {
            REQUIRE(plan.pvar[j] == (fc.point_const[j] ? 0 : 1));
            nvar += fc.point_const[j] ? 0 : 3;
        }
        REQUIRE(plan.num_variable == nvar);
        // a mask that makes a point with a single residual variable is refused; so is a constant point without observations
        for (size_t j = 0; j < fc.point_const.size(); ++j) {
            size_t n = 0;
            for (uint32_t p : fc.flat.obs_point) n += p == j;
            if (n == 1) {
                std::vector<uint8_t> mask = fc.point_const;
                mask[j] = 0;
                REQUIRE(!amc::ba::make_plan(pb, mask.data(), &plan).empty());
                REQUIRE(!amc::ba::make_plan(pb, nullptr, &plan).empty());
                ++problems;
                break;
            }
        }
        if (!fc.point_const.empty()) {
            FlatBa more = fc.flat;
            more.xyz.insert(more.xyz.end(), {0.0, 0.0, 0.0});
            std::vector<uint8_t> mask = fc.point_const;
            mask.push_back(1);
            amc_ba_problem pm = more.Problem();
            REQUIRE(!amc::ba::make_plan(pm, mask.data(), &plan).empty());
            ++problems;
        }
        // the write-back touches only what was in the problem
        SparseModel w = m;
        for (double& v : fc.flat.xyz) v += 1.0;
        for (double& v : fc.flat.tvec) v += 1.0;
        WriteBackBundleAdjuster(fc, &w);
        std::vector<char> pin(m.points3D.size(), 0), iin(m.images.size(), 0);
        for (size_t j : fc.point_at) pin[j] = 1;
        for (uint32_t i : fc.image_at) iin[i] = 1;
        for (size_t j = 0; j < m.points3D.size(); ++j) REQUIRE((w.points3D[j].xyz[0] != m.points3D[j].xyz[0]) == (pin[j] != 0));
        for (size_t i = 0; i < m.images.size(); ++i) REQUIRE((w.images[i].tvec[0] != m.images[i].tvec[0]) == (iin[i] != 0));
        // corrupted input: ids the model does not hold, broken cross references, a write-back into another model
        {
            BundleAdjustmentConfig bad = cfg;
            bad.AddImage(99999);
            REQUIRE(throws([&] { FlattenForBundleAdjuster(m, bad, f); }));
            REQUIRE(throws([&] { (void)bad.NumResiduals(m); }));
            bad = cfg;
            bad.AddConstantPoint(5);
            if (!cfg.HasVariablePoint(5)) REQUIRE(throws([&] { FlattenForBundleAdjuster(m, bad, f); }));
            problems += 2;
        }
        if (!m.points3D.empty() && !m.points3D[0].track.empty()) {
            SparseModel b = m;
            b.points3D[0].track[0].second = 0x7fffffffu;
            REQUIRE(throws([&] { FlattenForBundleAdjuster(b, cfg, f); }));
            b = m;
            b.points3D[0].track[0].first = 424242;
            REQUIRE(throws([&] { FlattenForBundleAdjuster(b, cfg, f); }));
            b = m;
            b.images[0].camera_id = 7777;
            REQUIRE(throws([&] { FlattenForBundleAdjuster(b, cfg, f); }));
            problems += 3;
        }
        if (!fc.point_at.empty()) {
            SparseModel small;
            REQUIRE(throws([&] { WriteBackBundleAdjuster(fc, &small); }));
            ++problems;
        }
    }
    // the config's own checks
    BundleAdjustmentConfig c;
    c.AddImage(1);
    REQUIRE(throws([&] { c.SetConstantCamPose(2); }));
    REQUIRE(throws([&] { c.SetConstantCamPositions(2, {0}); }));
    REQUIRE(throws([&] { c.SetConstantCamPositions(1, {}); }));
    REQUIRE(throws([&] { c.SetConstantCamPositions(1, {0, 1, 2, 0}); }));
    REQUIRE(throws([&] { c.SetConstantCamPositions(1, {1, 1}); }));
    REQUIRE(throws([&] { c.SetConstantCamPositions(1, {3}); }));
    REQUIRE(throws([&] { c.SetConstantCamPositions(1, {-1}); }));
    REQUIRE(throws([&] { (void)c.ConstantCamPositions(1); }));
    c.SetConstantCamPositions(1, {2, 0});
    REQUIRE(throws([&] { c.SetConstantCamPose(1); }));
    c.RemoveConstantCamPositions(1);
    c.SetConstantCamPose(1);
    REQUIRE(throws([&] { c.SetConstantCamPositions(1, {0}); }));
    c.AddVariablePoint(4);
    REQUIRE(throws([&] { c.AddConstantPoint(4); }));
    c.AddConstantPoint(5);
    REQUIRE(throws([&] { c.AddVariablePoint(5); }));
    REQUIRE(with_outside >= 50 && with_skipped >= 50 && with_constants >= 100);
    std::printf("ok %d (%d outside images pulled in, %d models with skipped points, %d with constant points)\n", problems,
                with_outside, with_skipped, with_constants);
    return 0;
}
