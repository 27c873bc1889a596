// ba_plan_fuzz.cc — a stand-alone program for tests/test_ba_cpu.py (built with -fsanitize=address,undefined and run): the
// host half of bundle adjustment (csrc/ba_plan.h) on a valid problem, on every kind of invalid one (indices out of range
// in each array, a point seen once, values that are not finite, NULL arrays, an unknown model) and on seeded random
// problems, valid and corrupted; every third of them has an image without observations, every third a camera that no
// image uses (the empty segments of 15.2's orders), and the cameras' models are drawn one by one, so their parameter counts
// differ within a problem.  The arrays are heap blocks of exactly the stated sizes, so a read past an array's end
// or through an unchecked index is an ASan report.  A valid plan is checked: the three CSR orders are permutations with
// the orders DESIGN.md 15.2 states.  Prints "ok <problems>" and returns 0.
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <random>

#include "../../pycolmap_amd/csrc/ba_plan.h"

namespace {

struct Owned {
    std::vector<int32_t> models;
    std::vector<double> cparams, q, t, X, xy;
    std::vector<uint8_t> cconst, pconst;
    std::vector<uint32_t> icam, oi, op;
    amc_ba_problem view() {
        amc_ba_problem p{};
        p.num_cameras = models.size();
        p.camera_models = models.data();
        p.camera_params = cparams.data();
        p.camera_const = cconst.data();
        p.num_images = icam.size();
        p.image_cameras = icam.data();
        p.qvec = q.data();
        p.tvec = t.data();
        p.pose_const = pconst.data();
        p.num_points = X.size() / 3;
        p.xyz = X.data();
        p.num_observations = oi.size();
        p.obs_image = oi.data();
        p.obs_point = op.data();
        p.obs_xy = xy.data();
        return p;
    }
};

constexpr size_t kNone = ~(size_t)0;

// `empty_image` gets no observation, `unused_camera` no image (kNone: whatever the draws give)
Owned random_problem(std::mt19937& rng, size_t ncam, size_t nimg, size_t npts, size_t empty_image, size_t unused_camera) {
    Owned o;
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    for (size_t c = 0; c < ncam; ++c) o.models.push_back((int32_t)(rng() % 11));
    o.cparams.resize(12 * ncam);
    o.cconst.resize(12 * ncam);
    for (double& v : o.cparams) v = u(rng);
    for (uint8_t& v : o.cconst) v = rng() % 2;
    for (size_t i = 0; i < nimg; ++i) {
        uint32_t c = (uint32_t)(rng() % ncam);
        if (c == unused_camera) c = (c + 1) % (uint32_t)ncam;
        o.icam.push_back(c);
    }
    o.q.resize(4 * nimg);
    o.t.resize(3 * nimg);
    o.pconst.resize(6 * nimg);
    for (double& v : o.q) v = u(rng);
    for (double& v : o.t) v = u(rng);
    for (uint8_t& v : o.pconst) v = rng() % 2;
    o.X.resize(3 * npts);
    for (double& v : o.X) v = u(rng);
    for (size_t j = 0; j < npts; ++j) {
        const size_t n = 2 + rng() % 3;
        for (size_t k = 0; k < n; ++k) {
            uint32_t i = (uint32_t)(rng() % nimg);
            if (i == empty_image) i = (i + 1) % (uint32_t)nimg;
            o.oi.push_back(i);
            o.op.push_back((uint32_t)j);
        }
    }
    for (size_t k = o.oi.size(); k > 1; --k) {  // shuffle the observations
        const size_t a = k - 1, b = rng() % k;
        std::swap(o.oi[a], o.oi[b]);
        std::swap(o.op[a], o.op[b]);
    }
    o.xy.resize(2 * o.oi.size());
    for (double& v : o.xy) v = 500.0 * u(rng);
    return o;
}

#define REQUIRE(cond)                                                      \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

void check_plan(Owned& o, const amc::ba::Plan& p) {
    const size_t nimg = o.icam.size(), npts = o.X.size() / 3, nobs = o.oi.size(), ncam = o.models.size();
    REQUIRE(p.ioff.size() == nimg + 1 && p.poff.size() == npts + 1 && p.coff.size() == ncam + 1);
    REQUIRE(p.ioff[nimg] == nobs && p.poff[npts] == nobs && p.coff[ncam] == nimg);
    for (size_t i = 0; i < nimg; ++i)
        for (uint32_t k = p.ioff[i]; k < p.ioff[i + 1]; ++k) REQUIRE(p.oimg[k] == i);
    // image order keeps the input order within an image
    std::vector<size_t> next(nimg, 0);
    for (size_t i = 0; i < nimg; ++i) next[i] = p.ioff[i];
    for (size_t in = 0; in < nobs; ++in) {
        const size_t k = next[o.oi[in]]++;
        REQUIRE(p.opt[k] == o.op[in] && p.oxy[2 * k] == o.xy[2 * in] && p.oxy[2 * k + 1] == o.xy[2 * in + 1]);
    }
    std::vector<char> seen(nobs, 0);
    for (size_t j = 0; j < npts; ++j)
        for (uint32_t k = p.poff[j]; k < p.poff[j + 1]; ++k) {
            REQUIRE(p.pobs[k] < nobs && !seen[p.pobs[k]] && p.opt[p.pobs[k]] == j);
            REQUIRE(k == p.poff[j] || p.pobs[k - 1] < p.pobs[k]);
            seen[p.pobs[k]] = 1;
        }
    for (size_t c = 0; c < ncam; ++c)
        for (uint32_t k = p.coff[c]; k < p.coff[c + 1]; ++k) {
            REQUIRE(o.icam[p.cimg[k]] == c);
            REQUIRE(k == p.coff[c] || p.cimg[k - 1] < p.cimg[k]);
        }
    uint64_t nvar = 3 * npts;
    for (size_t c = 0; c < ncam; ++c)
        for (int k = 0; k < 12; ++k) {
            const bool var = k < amc::cam::num_params(o.models[c]) && !o.cconst[12 * c + k];
            REQUIRE(p.cvar[12 * c + k] == (var ? 1 : 0));
            nvar += var;
        }
    for (size_t k = 0; k < 6 * nimg; ++k) nvar += !o.pconst[k];
    REQUIRE(p.num_variable == nvar);
    uint32_t kc = 0;
    for (size_t c = 0; c < ncam; ++c) kc = std::max<uint32_t>(kc, (uint32_t)amc::cam::num_params(o.models[c]));
    REQUIRE(p.kc == kc);
    for (size_t c = 0; c < ncam; ++c)  // the slots past a narrower camera's parameters hold exact zeros
        for (int k = amc::cam::num_params(o.models[c]); k < 12; ++k) REQUIRE(p.cparams[12 * c + k] == 0.0);
}

// what the generator is asked to produce, counted over the valid plans
int g_empty_images = 0, g_unused_cameras = 0, g_mixed_counts = 0;

void count_edges(const Owned& o, const amc::ba::Plan& p, size_t empty_image, size_t unused_camera) {
    if (empty_image != kNone) {
        REQUIRE(p.ioff[empty_image] == p.ioff[empty_image + 1]);
        ++g_empty_images;
    }
    if (unused_camera != kNone) {
        REQUIRE(p.coff[unused_camera] == p.coff[unused_camera + 1]);
        ++g_unused_cameras;
    }
    for (size_t c = 1; c < o.models.size(); ++c)
        if (amc::cam::num_params(o.models[c]) != amc::cam::num_params(o.models[0])) {
            ++g_mixed_counts;
            break;
        }
}

}  // namespace

int main() {
    std::mt19937 rng(7);
    amc::ba::Plan plan;
    int problems = 0;
    for (int round = 0; round < 200; ++round) {
        const size_t ncam = (round % 3 == 1 ? 2 : 1) + rng() % 3, nimg = 2 + rng() % 5;
        const size_t empty_image = round % 3 == 0 ? rng() % nimg : kNone;
        const size_t unused_camera = round % 3 == 1 ? rng() % ncam : kNone;
        Owned o = random_problem(rng, ncam, nimg, 1 + rng() % 40, empty_image, unused_camera);
        amc_ba_problem v = o.view();
        REQUIRE(amc::ba::make_plan(v, &plan).empty());
        check_plan(o, plan);
        count_edges(o, plan, empty_image, unused_camera);
        ++problems;
        // one corruption per copy: each must be refused, none may be read through
        for (int kind = 0; kind < 9; ++kind) {
            Owned b = o;
            const size_t nobs = b.oi.size();
            switch (kind) {
                case 0: b.oi[rng() % nobs] = (uint32_t)b.icam.size() + (rng() % 2 ? 0u : 0x7fffffffu); break;
                case 1: b.op[rng() % nobs] = (uint32_t)(b.X.size() / 3) + (rng() % 2 ? 0u : 0x7fffffffu); break;
                case 2: b.icam[rng() % b.icam.size()] = (uint32_t)b.models.size(); break;
                case 3: b.models[rng() % b.models.size()] = rng() % 2 ? 11 : -1; break;
                case 4: b.X[rng() % b.X.size()] = NAN; break;
                case 5: b.xy[rng() % b.xy.size()] = INFINITY; break;
                case 6: b.q[rng() % b.q.size()] = -INFINITY; break;
                case 7: {  // a point left with one observation: drop all but one of point 0's
                    std::vector<uint32_t> oi, op;
                    std::vector<double> xy;
                    bool kept = false;
                    for (size_t k = 0; k < nobs; ++k) {
                        if (b.op[k] == 0 && kept) continue;
                        kept = kept || b.op[k] == 0;
                        oi.push_back(b.oi[k]);
                        op.push_back(b.op[k]);
                        xy.push_back(b.xy[2 * k]);
                        xy.push_back(b.xy[2 * k + 1]);
                    }
                    b.oi = oi;
                    b.op = op;
                    b.xy = xy;
                    break;
                }
                default: break;
            }
            amc_ba_problem w = b.view();
            if (kind == 8) w.obs_xy = nullptr;
            REQUIRE(!amc::ba::make_plan(w, &plan).empty());
            ++problems;
        }
    }
    amc_ba_opts opts{0, 100, 200, 10, 1.0, 0.0, 0.0, 0.0};
    REQUIRE(amc::ba::check_options(opts).empty());
    opts.loss_function_scale = 0.0;
    REQUIRE(!amc::ba::check_options(opts).empty());
    opts.loss_function_scale = NAN;
    REQUIRE(!amc::ba::check_options(opts).empty());
    Owned empty;
    amc_ba_problem e = empty.view();
    REQUIRE(amc::ba::make_plan(e, &plan).empty() && plan.num_variable == 0);
    REQUIRE(g_empty_images >= 60 && g_unused_cameras >= 60 && g_mixed_counts >= 60);
    std::printf("ok %d (%d with an image without observations, %d with an unused camera, %d with mixed parameter counts)\n",
                problems, g_empty_images, g_unused_cameras, g_mixed_counts);
    return 0;
}
