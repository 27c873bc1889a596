// ba_host_fuzz.cc — a stand-alone program for tests/test_ba_cpu.py (built with -fsanitize=address,undefined together
// with csrc/host/model_io.cc and reconstruction.cc, and run with a scratch directory as its argument): the host code
// behind Reconstruction and bundle_adjustment on files.  It writes a small model, reads it back (.bin), checks, filters,
// flattens and writes back; then every one of the three files truncated at every length (a truncated file must throw
// std::invalid_argument or still give a model that CheckModel and the flattening accept or refuse, never a bad read);
// then ids out of range in every cross reference (camera ids, point3D ids, track image ids, point2D indices, duplicate
// ids), each of which CheckModel and FlattenForBundleAdjustment must refuse.  Prints "ok <cases>".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>

#include "../../pycolmap_amd/csrc/host/ba_host.h"
#include "../../pycolmap_amd/csrc/host/reconstruction.h"
#include "../../pycolmap_amd/csrc/ba_plan.h"

using namespace amchost;

#define REQUIRE(cond)                                                      \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static SparseModel SmallModel() {
    SparseModel m;
    ModelCamera c;
    c.camera_id = 7;
    c.model = 2;
    c.width = 1000;
    c.height = 800;
    c.params = {800.0, 500.0, 400.0, 0.05};
    m.cameras.push_back(c);
    c.camera_id = 3;
    c.model = 4;
    c.params = {800.0, 810.0, 500.0, 400.0, 0.01, 0.0, 0.0, 0.0};
    m.cameras.push_back(c);
    for (uint32_t i = 0; i < 4; ++i) {
        ModelImage im;
        im.image_id = 10 + i;
        im.camera_id = i == 3 ? 3 : 7;
        im.name = "image" + std::to_string(i) + ".png";
        im.tvec[0] = 0.3 * i;
        im.tvec[2] = i == 2 ? -30.0 : 6.0;  // image 12 sees everything behind it
        for (int k = 0; k < 6; ++k) {
            ModelPoint2D p;
            p.x = 400.0 + 20.0 * k + i;
            p.y = 300.0 + 10.0 * k;
            im.points2D.push_back(p);
        }
        m.images.push_back(im);
    }
    for (uint64_t j = 0; j < 5; ++j) {
        ModelPoint3D p;
        p.point3D_id = 100 + j;
        p.xyz[0] = 0.2 * j - 0.4;
        p.xyz[1] = 0.1 * j;
        p.xyz[2] = 1.0;
        p.error = 0.5;
        const uint32_t n = j == 4 ? 2 : 4;  // the last point: images 10 and 12 only, so the filter deletes it
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t img = j == 4 ? (i == 0 ? 0 : 2) : i;
            p.track.emplace_back(10 + img, static_cast<uint32_t>(j));
            m.images[img].points2D[j].point3D_id = p.point3D_id;
        }
        m.points3D.push_back(p);
    }
    return m;
}

static std::string Slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static void Dump(const std::string& path, const std::string& bytes) {
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    f.write(bytes.data(), static_cast<std::streamsize>(bytes.size()));
}

// everything bundle_adjustment does to a model before and after the solve; true when the model was accepted
static bool RunHost(SparseModel m) {
    if (!CheckModel(m).empty()) {
        bool threw = false;
        try {
            FlattenForBundleAdjustment(m, BaRefineFlags(), nullptr);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        REQUIRE(threw);
        return false;
    }
    (void)ComputeNumObservations(m);
    (void)ComputeMeanTrackLength(m);
    FilterObservationsWithNegativeDepth(&m);
    REQUIRE(CheckModel(m).empty());
    size_t skipped = 0;
    FlatBa flat = FlattenForBundleAdjustment(m, BaRefineFlags(), &skipped);
    amc_ba_problem pb = flat.Problem();
    amc::ba::Plan plan;
    (void)amc::ba::make_plan(pb, &plan);  // valid or refused (a non-finite value read from a damaged file), never a bad read
    WriteBackBundleAdjustment(flat, &m);
    return true;
}

int main(int argc, char** argv) {
    REQUIRE(argc == 2);
    const std::string dir = argv[1];
    int cases = 0;
    const SparseModel m0 = SmallModel();
    REQUIRE(CheckModel(m0).empty());
    WriteSparseModelBin(dir, m0);
    {
        SparseModel m = ReadSparseModelBin(dir);
        REQUIRE(CheckModel(m).empty() && m.images.size() == 4 && m.points3D.size() == 5 && m.cameras[0].camera_id == 7);
        REQUIRE(ComputeNumObservations(m) == 18);
        const size_t removed = FilterObservationsWithNegativeDepth(&m);
        REQUIRE(removed == 5 && m.points3D.size() == 4 && CheckModel(m).empty());  // 4 observations of image 12, and point 104
        for (const ModelPoint3D& p : m.points3D) REQUIRE(p.track.size() == 3);
        for (const ModelPoint2D& p : m.images[2].points2D) REQUIRE(p.point3D_id == kInvalidPoint3DId);
        REQUIRE(m.images[0].points2D[4].point3D_id == kInvalidPoint3DId);
        size_t skipped = 0;
        FlatBa flat = FlattenForBundleAdjustment(m, BaRefineFlags(), &skipped);
        REQUIRE(skipped == 0 && flat.obs_image.size() == 12 && flat.xyz.size() == 12 && flat.image_cameras[3] == 1);
        REQUIRE(flat.pose_const[0] && flat.pose_const[5] && flat.pose_const[9] && !flat.pose_const[8] && !flat.pose_const[12]);
        REQUIRE(!flat.camera_const[0] && flat.camera_const[1] && flat.camera_const[2] && !flat.camera_const[3] && flat.camera_const[4]);
        REQUIRE(RunHost(ReadSparseModelBin(dir)));
        ++cases;
    }
    // truncated files
    for (const char* name : {"cameras.bin", "images.bin", "points3D.bin"}) {
        const std::string path = dir + "/" + name, whole = Slurp(path);
        for (size_t len = 0; len < whole.size(); ++len) {
            Dump(path, whole.substr(0, len));
            try {
                RunHost(ReadSparseModelBin(dir));
            } catch (const std::invalid_argument&) {
            }
            ++cases;
        }
        // damaged counts and ids: every 8-byte word of the file replaced by a large value
        for (size_t at = 0; at + 8 <= whole.size(); at += 4) {
            std::string b = whole;
            for (int k = 0; k < 8; ++k) b[at + k] = static_cast<char>(k == 7 ? 0x7f : 0xff);
            Dump(path, b);
            try {
                RunHost(ReadSparseModelBin(dir));
            } catch (const std::invalid_argument&) {
            } catch (const std::length_error&) {
            } catch (const std::bad_alloc&) {
            }
            ++cases;
        }
        Dump(path, whole);
    }
    // ids out of range, in memory
    for (int kind = 0; kind < 8; ++kind) {
        SparseModel m = m0;
        switch (kind) {
            case 0: m.images[1].camera_id = 99; break;
            case 1: m.images[0].points2D[5].point3D_id = 12345; break;
            case 2: m.points3D[0].track[1].first = 77; break;
            case 3: m.points3D[0].track[1].second = 6; break;
            case 4: m.points3D[1].track[0].second = 0xffffffffu; break;
            case 5: m.images[2].image_id = 10; break;
            case 6: m.points3D[3].point3D_id = 100; break;
            case 7: m.cameras[0].params.pop_back(); break;
        }
        REQUIRE(!CheckModel(m).empty());
        REQUIRE(!RunHost(m));
        ++cases;
    }
    std::printf("ok %d\n", cases);
    return 0;
}
