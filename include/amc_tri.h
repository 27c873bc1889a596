/*
 * amc_tri.h — C ABI of libamc.so's track triangulation (gfx950): known poses and normalized observations in, one
 * LO-RANSAC per track, 3D points and inlier masks out.
 *
 * Additive to amc.h (AMC_ABI_VERSION is unchanged): a host that never triangulates never calls these.  The algorithm is
 * COLMAP 3.9.1's EstimateTriangulation with the angular residual, as the pycolmap 0.6 binding drives it, restated in
 * DESIGN.md section 11 with its deviations; the results are bit-identical to tests/tri_ref/tri_ref.cc.
 *
 * Reference surface (/root/reference/pycolmap/estimators/triangulation.h):
 *   EstimateTriangulationOptions{min_tri_angle, ransac: RANSACOptions}    amc_tri_opts
 *   PointData(point, point_normalized)                                     obs_xy (point_normalized only)
 *   images[i].CamFromWorld().ToMatrix()                                    poses (3 x 4 [R | t] each)
 *   estimate_triangulation(point_data, images, cameras, opions)
 *     -> None | {"xyz", "inliers"}                                         amc_triangulate_tracks, one track or a batch
 */
#ifndef AMC_TRI_H_
#define AMC_TRI_H_

#include "amc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct amc_tri_opts {
    double min_tri_angle;             /* radians, default 0 */
    double max_error;                 /* radians (the angular residual), default 4.0 (pycolmap's RANSACOptions()) */
    double min_inlier_ratio;          /* default 0.01 */
    double confidence;                /* default 0.9999 */
    double dyn_num_trials_multiplier; /* default 3.0 */
    int64_t min_num_trials;           /* default 1000 */
    int64_t max_num_trials;           /* default 100000 */
} amc_tri_opts;

/* Track i owns observations [offsets[i], offsets[i + 1]).  Arrays are host memory, owned by the library. */
typedef struct amc_tri_result {
    size_t ntracks;
    size_t nobs;
    double* xyz;           /* ntracks x 3: the final model; 0 where success is 0 */
    uint8_t* success;      /* ntracks: 1 when the RANSAC found at least 2 inliers */
    uint32_t* num_inliers; /* ntracks: the best support's inlier count */
    uint64_t* num_trials;  /* ntracks: report.num_trials as LORANSAC::Estimate leaves it */
    uint8_t* inlier_mask;  /* nobs: 1 = inlier of the final model; all 0 for a failed track */
    double device_ms;      /* first upload -> last result byte on the host (HIP events on ctx's stream) */
    double kernel_ms;      /* the triangulation kernels alone, summed over the batches (HIP events) */
    uint32_t num_batches;  /* device batches the call was split into */
    void* _priv;
} amc_tri_result;

void amc_tri_opts_default(amc_tri_opts* o);

/* Triangulate `ntracks` tracks on ctx's device and stream.
 *   poses          nposes x 12 doubles: cam_from_world as a row-major 3 x 4 [R | t]; the library adds the projection
 *                  centre -R^T t of each
 *   track_offsets  ntracks + 1 values, offsets[0] = 0, non-decreasing (CSR over the observations)
 *   obs_pose       offsets[ntracks] pose indices (< nposes)
 *   obs_xy         offsets[ntracks] x 2 doubles: normalized image coordinates (PointData.point_normalized)
 * A track with fewer than 2 observations comes back unsuccessful with 0 trials.  Results do not depend on the order
 * or the composition of the batch.  Fills *result (release it with amc_tri_result_free).  Errors: AMC_E_INVALID (NULL
 * arrays, bad offsets, a pose index out of range, invalid options), AMC_E_NOMEM, AMC_E_HIP. */
int amc_triangulate_tracks(amc_ctx* ctx, const double* poses, size_t nposes, const uint64_t* track_offsets,
                           size_t ntracks, const uint32_t* obs_pose, const double* obs_xy, const amc_tri_opts* opts,
                           amc_tri_result* result);

void amc_tri_result_free(amc_tri_result* result);

#ifdef __cplusplus
}
#endif

#endif /* AMC_TRI_H_ */
