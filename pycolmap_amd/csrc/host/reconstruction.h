// reconstruction.h — the operations of the minimal Reconstruction on model_io's plain structs: the
// consistency check of a model that came from files or from Python objects, the counts,
// FilterObservationsWithNegativeDepth, and the host half of the point filter: DeletePoint3D,
// DeleteObservation, the two means, the flat problem of include/amc_filter.h and the way its result goes back into the
// model.  No Python and no HIP here: tests/shim/ba_host_fuzz.cc and tests/shim/filter_host_fuzz.cc run it under ASan + UBSan.
#pragma once

#include <cstddef>
#include <string>
#include <vector>

#include "../../../include/amc_filter.h"
#include "model_io.h"

namespace amchost {

// What is wrong with the model's cross references, or the empty string: duplicate ids, an image without its camera, a
// camera whose parameter count is not its model's, a point2D naming a point that does not exist, a track element
// naming an image or a point2D index that does not exist or that does not name the point back.
std::string CheckModel(const SparseModel& m);

size_t ComputeNumObservations(const SparseModel& m);   // points2D with a point3D
double ComputeMeanTrackLength(const SparseModel& m);   // observations / points3D, 0 without points

// depth of world point xyz in the image: the third row of [R | t] (qvec w x y z) applied to it
double PointDepth(const ModelImage& im, const double* xyz);

// Reconstruction::FilterObservationsWithNegativeDepth on a checked model: an observation whose point's depth in its
// image is below DBL_EPSILON is removed; when the point's track has length <= 2 before that removal, the whole point is
// deleted.  Returns the number of removed observations (a deleted point's remaining observations are not counted).
size_t FilterObservationsWithNegativeDepth(SparseModel* m);

// Reconstruction::DeletePoint3D on a checked model: every point2D of the track loses its point, the point leaves.
// Throws std::invalid_argument for an id that does not exist.
void DeletePoint3D(SparseModel* m, uint64_t point3D_id);
// Reconstruction::DeleteObservation on a checked model: the whole point goes when its track has length <= 2 before the
// call; otherwise that one element leaves the track and the point2D loses its point.  Throws std::invalid_argument for
// an image that does not exist, an index past its points2D or a point2D without a point.
void DeleteObservation(SparseModel* m, uint32_t image_id, uint32_t point2D_idx);

// Reconstruction::ComputeMeanReprojectionError: the mean of the stored errors in ascending id order, 0 without points
double ComputeMeanReprojectionError(const SparseModel& m);
// Reconstruction::ComputeMeanObservationsPerRegImage: observations / images, 0 without images
double ComputeMeanObservationsPerRegImage(const SparseModel& m);

// the flat problem of amc_filter_points3d and the arrays it points into
struct FlatFilter {
    std::vector<int32_t> camera_models;
    std::vector<double> camera_params, qvec, tvec, xyz, obs_xy;
    std::vector<uint32_t> image_cameras, obs_image;
    std::vector<uint64_t> track_offsets{0};
    std::vector<uint8_t> selected;
    std::vector<uint64_t> point_ids;  // of the model's points, in its order
    amc_filter_problem Problem() const;
};
// Flattens a checked model (throws std::invalid_argument otherwise).  Cameras, images and points keep the model's
// order, the observations are the tracks' elements in track order.  ids == nullptr selects every point; an id that the
// model does not hold selects nothing (COLMAP skips it).
FlatFilter FlattenForFilter(const SparseModel& m, const std::vector<uint64_t>* ids);
// the ids that the points2D of the given images carry (FilterPoints3DInImages); an image that does not exist throws
std::vector<uint64_t> Point3DIdsInImages(const SparseModel& m, const std::vector<uint32_t>& image_ids);
// A filter result (arrays of the flat problem's sizes: verdicts and errors per point, marks per observation) back into
// the model it was flattened from: deleted points leave with their points2D cleared, marked elements leave their
// tracks, a point that stays takes its new error.  Returns the reference's count (16.3).  Throws
// std::invalid_argument when the model no longer has the flat problem's shape or a verdict is unknown.
size_t ApplyFilterResult(const FlatFilter& f, const uint8_t* point_verdict, const uint8_t* obs_deleted,
                         const double* point_error, SparseModel* m);
// update_point3D_errors: every point takes point_error
void ApplyPointErrors(const FlatFilter& f, const double* point_error, SparseModel* m);

}  // namespace amchost
