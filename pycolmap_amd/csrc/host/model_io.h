// model_io.h — COLMAP 3.9's sparse model files (cameras / images / points3D, .bin and .txt) as plain structs: what
// undistort_images (/root/reference/pycolmap/pipeline/images.h:96-148) reads through Reconstruction::Read and writes
// through Reconstruction::Write.  No Python here; DESIGN.md 14.7 lists the layouts.
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace amchost {

constexpr uint64_t kInvalidPoint3DId = 0xFFFFFFFFFFFFFFFFull;

struct ModelCamera {
    uint32_t camera_id = 0;
    int model = -1;
    uint64_t width = 0, height = 0;
    std::vector<double> params;
};
struct ModelPoint2D {
    double x = 0, y = 0;
    uint64_t point3D_id = kInvalidPoint3DId;
};
struct ModelImage {
    uint32_t image_id = 0;
    double qvec[4] = {1, 0, 0, 0};  // w x y z
    double tvec[3] = {0, 0, 0};
    uint32_t camera_id = 0;
    std::string name;
    std::vector<ModelPoint2D> points2D;
};
struct ModelPoint3D {
    uint64_t point3D_id = 0;
    double xyz[3] = {0, 0, 0};
    uint8_t rgb[3] = {0, 0, 0};
    double error = 0;
    std::vector<std::pair<uint32_t, uint32_t>> track;  // (image id, point2D index)
};
// everything in file order
struct SparseModel {
    std::vector<ModelCamera> cameras;
    std::vector<ModelImage> images;
    std::vector<ModelPoint3D> points3D;
    const ModelCamera* FindCamera(uint32_t camera_id) const;
};

// number of parameters of a COLMAP camera model id, -1 for an unknown id; the id of a model name, -1 when unknown
int ModelNumParams(int model);
int ModelIdFromName(const std::string& name);

// Reconstruction::Read: the three .bin files when all of them exist, else the three .txt files.  Throws
// std::invalid_argument naming the file and what is wrong with it.
SparseModel ReadSparseModel(const std::string& dir);
// Reconstruction::ReadBinary / ReadText: one format, whatever else the directory holds
SparseModel ReadSparseModelBin(const std::string& dir);
SparseModel ReadSparseModelTxt(const std::string& dir);
// Reconstruction::WriteBinary into an existing directory
void WriteSparseModelBin(const std::string& dir, const SparseModel& model);

}  // namespace amchost
