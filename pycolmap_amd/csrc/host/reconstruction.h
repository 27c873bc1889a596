// reconstruction.h — the operations of the minimal Reconstruction on model_io's plain structs: the
// consistency check of a model that came from files or from Python objects, the counts, and
// FilterObservationsWithNegativeDepth.  No Python and no HIP here: tests/shim/ba_host_fuzz.cc runs it under ASan + UBSan.
#pragma once

#include <cstddef>
#include <string>
#include <vector>

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

}  // namespace amchost
