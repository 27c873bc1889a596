// bacov_plan_fuzz.cc — a stand-alone program for tests/test_ba_covariance_cpu.py (built with -fsanitize=address,undefined
// and run): the host half of the bundle-adjustment covariance (csrc/bacov_plan.h) on seeded random problems with constant
// points, images without observations, cameras without images and mixed camera models, valid and corrupted (indices out
// of range in each index array, an unknown model, values that are not finite, a variable point seen once, a constant
// point never seen).  The arrays are heap blocks of exactly the stated sizes, so a read past an array's end or through an
// unchecked index is an ASan report.  A valid plan is checked against DESIGN.md 24.1 and 24.3: the compact column map,
// the slots' owner order, and every destination block's pairs in ascending point index, each pair of a point's slots
// exactly once.  Prints "ok <problems>" and returns 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>

#include "../../pycolmap_amd/csrc/bacov_plan.h"

namespace {

struct Owned {
    std::vector<int32_t> models;
    std::vector<double> cparams, q, t, X, xy;
    std::vector<uint8_t> cconst, pconst, point_const;
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

Owned random_problem(std::mt19937& rng, size_t ncam, size_t nimg, size_t npts, int flavour) {
    Owned o;
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    for (size_t c = 0; c < ncam; ++c) o.models.push_back((int32_t)(rng() % 11));
    o.cparams.resize(12 * ncam);
    o.cconst.resize(12 * ncam);
    for (double& v : o.cparams) v = u(rng);
    for (uint8_t& v : o.cconst) v = flavour == 1 ? 1 : rng() % 2;  // flavour 1: every camera constant
    const size_t empty_image = flavour == 2 ? rng() % nimg : ~(size_t)0;
    for (size_t i = 0; i < nimg; ++i) o.icam.push_back((uint32_t)(rng() % ncam));
    o.q.resize(4 * nimg);
    o.t.resize(3 * nimg);
    o.pconst.resize(6 * nimg);
    for (double& v : o.q) v = u(rng);
    for (double& v : o.t) v = u(rng);
    for (uint8_t& v : o.pconst) v = flavour == 3 ? 1 : rng() % 3 == 0;  // flavour 3: every pose constant
    o.X.resize(3 * npts);
    for (double& v : o.X) v = u(rng);
    o.point_const.resize(npts);
    for (size_t j = 0; j < npts; ++j) {
        o.point_const[j] = flavour == 4 ? 1 : rng() % 3 == 0;  // flavour 4: every point constant
        const size_t n = (o.point_const[j] ? 1 : 2) + rng() % 4;  // (a point may meet an image twice)
        for (size_t k = 0; k < n; ++k) {
            uint32_t i = (uint32_t)(rng() % nimg);
            if (i == empty_image) i = (i + 1) % (uint32_t)nimg;
            o.oi.push_back(i);
            o.op.push_back((uint32_t)j);
        }
    }
    for (size_t k = o.oi.size(); k > 1; --k) {
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

int g_dest_blocks = 0, g_no_columns = 0, g_twice = 0;

void check_plan(Owned& o, const amc::bacov::Plan& p) {
    const size_t nimg = o.icam.size(), npts = o.X.size() / 3, ncam = o.models.size();
    // 24.1: the compact column map
    std::vector<uint32_t> owner, coord;
    for (size_t i = 0; i < nimg; ++i)
        for (uint32_t k = 0; k < 6; ++k)
            if (!o.pconst[6 * i + k]) {
                REQUIRE(p.icol[6 * i + k] == (int32_t)owner.size());
                owner.push_back((uint32_t)i);
                coord.push_back(k);
            } else {
                REQUIRE(p.icol[6 * i + k] == -1);
            }
    for (size_t c = 0; c < ncam; ++c)
        for (uint32_t k = 0; k < 12; ++k)
            if ((int)k < amc::cam::num_params(o.models[c]) && !o.cconst[12 * c + k]) {
                REQUIRE(p.ccol[12 * c + k] == (int32_t)owner.size());
                owner.push_back((uint32_t)(nimg + c));
                coord.push_back(k);
            } else {
                REQUIRE(p.ccol[12 * c + k] == -1);
            }
    REQUIRE(p.m == owner.size() && p.nown == nimg + ncam && p.ocol.size() == p.nown + 1 && p.ocol[p.nown] == p.m);
    if (p.m == 0) {
        ++g_no_columns;
        REQUIRE(p.slot_owner.empty() && p.dest_a.empty());
        return;
    }
    REQUIRE(p.col_owner == owner && p.col_coord == coord);
    for (uint32_t a = 0; a < p.nown; ++a)
        for (uint32_t k = p.ocol[a]; k < p.ocol[a + 1]; ++k) REQUIRE(owner[k] == a);
    // 24.3: slots: per variable point the images in point order (first meeting), then the cameras ascending
    REQUIRE(p.spo.size() == npts + 1 && p.spo[npts] == p.slot_owner.size() && p.slot_point.size() == p.slot_owner.size());
    std::map<std::pair<uint32_t, uint32_t>, std::vector<std::pair<uint32_t, uint32_t>>> want;  // (A, B) -> slot pairs
    for (size_t j = 0; j < npts; ++j) {
        std::vector<uint32_t> own;
        std::set<uint32_t> cams;
        if (!o.point_const[j])
            for (uint32_t k = p.ba.poff[j]; k < p.ba.poff[j + 1]; ++k) {
                const uint32_t i = p.ba.oimg[p.ba.pobs[k]], c = (uint32_t)nimg + o.icam[i];
                if (std::find(own.begin(), own.end(), i) != own.end()) ++g_twice;
                else if (p.ocol[i + 1] > p.ocol[i]) own.push_back(i);
                if (p.ocol[c + 1] > p.ocol[c]) cams.insert(c);
            }
        own.insert(own.end(), cams.begin(), cams.end());
        REQUIRE(p.spo[j + 1] - p.spo[j] == own.size());
        for (size_t s = 0; s < own.size(); ++s) REQUIRE(p.slot_owner[p.spo[j] + s] == own[s] && p.slot_point[p.spo[j] + s] == j);
        for (uint32_t x = p.spo[j]; x < p.spo[j + 1]; ++x)
            for (uint32_t y = p.spo[j]; y < p.spo[j + 1]; ++y)
                if (p.slot_owner[x] >= p.slot_owner[y]) want[{p.slot_owner[x], p.slot_owner[y]}].push_back({x, y});
    }
    // destination blocks: ascending (A, B), each block's pairs in ascending point index, every pair exactly once
    REQUIRE(p.dest_a.size() == want.size() && p.dest_b.size() == want.size() && p.dest_off.size() == want.size() + 1);
    size_t d = 0;
    for (const auto& kv : want) {
        REQUIRE(p.dest_a[d] == kv.first.first && p.dest_b[d] == kv.first.second);
        REQUIRE(p.dest_off[d + 1] - p.dest_off[d] == kv.second.size());
        for (size_t t = 0; t < kv.second.size(); ++t) {
            const uint32_t at = p.dest_off[d] + (uint32_t)t;
            REQUIRE(p.pair_a[at] == kv.second[t].first && p.pair_b[at] == kv.second[t].second);
            REQUIRE(t == 0 || p.slot_point[p.pair_a[at - 1]] < p.slot_point[p.pair_a[at]]);
        }
        ++d;
    }
    REQUIRE(p.dest_off[want.size()] == p.pair_a.size() && p.pair_a.size() == p.pair_b.size());
    g_dest_blocks += (int)want.size();
}

}  // namespace

int main() {
    std::mt19937 rng(11);
    amc::bacov::Plan plan;
    int problems = 0;
    for (int round = 0; round < 200; ++round) {
        const size_t ncam = 1 + rng() % 3, nimg = 2 + rng() % 6;
        const int flavour = round % 6;
        Owned o = random_problem(rng, ncam, nimg, 1 + rng() % 40, flavour);
        if (flavour == 5) {  // nothing variable in the reduced system: m == 0
            for (uint8_t& v : o.cconst) v = 1;
            for (uint8_t& v : o.pconst) v = 1;
        }
        amc_ba_problem v = o.view();
        REQUIRE(amc::bacov::make_plan(v, o.point_const.data(), &plan).empty());
        check_plan(o, plan);
        ++problems;
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
                case 6: b.t[rng() % b.t.size()] = -INFINITY; break;
                case 7:
                case 8: {  // point 0 left with one observation as a variable point (7), with none as a constant one (8)
                    std::vector<uint32_t> oi, op;
                    std::vector<double> xy;
                    bool kept = kind == 8;
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
                    b.point_const[0] = kind == 8;
                    break;
                }
            }
            amc_ba_problem bv = b.view();
            REQUIRE(!amc::bacov::make_plan(bv, b.point_const.data(), &plan).empty());
            ++problems;
        }
    }
    // the option checks
    amc_bacov_opts opts{0, 1, 1, 0, 1.0, 1e-8};
    REQUIRE(amc::bacov::check_options(opts).empty());
    for (int kind = 0; kind < 5; ++kind) {
        amc_bacov_opts b = opts;
        if (kind == 0) b.loss_function_type = 3;
        if (kind == 1) b.loss_function_scale = 0.0;
        if (kind == 2) b.loss_function_scale = INFINITY;
        if (kind == 3) b.damping = -1e-9;
        if (kind == 4) b.damping = NAN;
        REQUIRE(!amc::bacov::check_options(b).empty());
    }
    REQUIRE(g_dest_blocks > 1000 && g_no_columns >= 30 && g_twice > 50);
    std::printf("ok %d %d %d %d\n", problems, g_dest_blocks, g_no_columns, g_twice);
    return 0;
}
