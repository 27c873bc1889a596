/*
 * amc_abspose.h — C ABI of libamc.so's absolute pose (gfx950): 2D-3D correspondences and a camera in, one LO-RANSAC
 * per focal-length hypothesis and a robust refinement per query, camera poses and inlier masks out.
 *
 * Additive to amc.h (AMC_ABI_VERSION is unchanged): a host that never localises never calls these.  The algorithm is
 * COLMAP 3.9.1's EstimateAbsolutePose + RefineAbsolutePose as the pycolmap 0.6 binding drives them, restated in
 * DESIGN.md section 12 with its deviations A1-A12; the results are bit-identical to tests/abspose_ref.
 *
 * Reference surface (pycolmap/estimators/absolute_pose.h of the reference binding):
 *   AbsolutePoseEstimationOptions{estimate_focal_length, num_focal_length_samples, min_focal_length_ratio,
 *                                 max_focal_length_ratio, ransac: RANSACOptions (max_error = 12 px)}
 *                                                                          amc_abspose_opts
 *   AbsolutePoseRefinementOptions{gradient_tolerance, max_num_iterations, loss_function_scale, refine_focal_length,
 *                                 refine_extra_params, print_summary}      amc_abspose_refine_opts
 *   Camera (model id + params)                                             camera_models, camera_params
 *   absolute_pose_estimation(points2D, points3D, camera, estimation_options, refinement_options, return_covariance)
 *     -> None | {"cam_from_world", "num_inliers", "inliers"[, "covariance"]}
 *                                                                          amc_estimate_absolute_poses, one query or a
 *                                                                          batch
 *   pose_refinement(cam_from_world, points2D, points3D, inlier_mask, camera, refinement_options)
 *     -> None | {"cam_from_world"}                                         amc_refine_absolute_poses
 */
#ifndef AMC_ABSPOSE_H_
#define AMC_ABSPOSE_H_

#include "amc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct amc_abspose_opts {
    int32_t estimate_focal_length;    /* default 0 */
    int32_t num_focal_length_samples; /* default 30 */
    double min_focal_length_ratio;    /* default 0.1 */
    double max_focal_length_ratio;    /* default 10 */
    double max_error;                 /* pixels, default 12 */
    double min_inlier_ratio;          /* default 0.01 */
    double confidence;                /* default 0.9999 */
    double dyn_num_trials_multiplier; /* default 3.0 */
    int64_t min_num_trials;           /* default 1000 */
    int64_t max_num_trials;           /* default 100000 */
} amc_abspose_opts;

typedef struct amc_abspose_refine_opts {
    double gradient_tolerance;   /* default 1.0 */
    int64_t max_num_iterations;  /* default 100 */
    double loss_function_scale;  /* default 1.0 (CauchyLoss) */
    int32_t refine_focal_length; /* must be 0 */
    int32_t refine_extra_params; /* must be 0 */
    int32_t print_summary;       /* accepted, no effect */
} amc_abspose_refine_opts;

/* Query i owns correspondences [offsets[i], offsets[i + 1]).  Arrays are host memory, owned by the library. */
typedef struct amc_abspose_result {
    size_t nqueries;
    size_t ncorr;
    uint8_t* success;       /* nqueries: 1 = a pose (estimation and refinement both succeeded) */
    double* qvec;           /* nqueries x 4: cam_from_world rotation, Eigen order (x, y, z, w) */
    double* tvec;           /* nqueries x 3: cam_from_world translation */
    uint32_t* num_inliers;  /* nqueries: inliers of the chosen RANSAC (the input mask's count for refinement) */
    uint64_t* num_trials;   /* nqueries: report.num_trials of the chosen RANSAC (of the first when none succeeded) */
    double* focal_factor;   /* nqueries: the chosen focal-length factor (1 without focal estimation, 0 on failure) */
    double* covariance;     /* nqueries x 36 (row-major 6 x 6, rotation first) when asked, else NULL */
    uint8_t* inlier_mask;   /* ncorr: the chosen RANSAC's inlier mask (the input mask for refinement) */
    double device_ms;       /* first upload -> last result byte on the host (HIP events on ctx's stream) */
    double kernel_ms;       /* the kernels alone, summed over the batches (HIP events) */
    uint32_t num_batches;   /* device batches the call was split into */
    void* _priv;
} amc_abspose_result;

void amc_abspose_opts_default(amc_abspose_opts* o);
void amc_abspose_refine_opts_default(amc_abspose_refine_opts* o);

/* Estimate and refine the pose of `nqueries` queries on ctx's device and stream.
 *   offsets        nqueries + 1 values, offsets[0] = 0, non-decreasing (CSR over the correspondences)
 *   camera_models  nqueries COLMAP model ids (0 .. 10)
 *   camera_params  nqueries x 12 doubles: the model's parameters first, the rest ignored
 *   points2D       offsets[nqueries] x 2 doubles: pixels
 *   points3D       offsets[nqueries] x 3 doubles: world points
 * With estimate_focal_length the chosen focal_factor multiplies the camera's focal lengths (the caller's Camera is
 * scaled in place by the binding).  Results do not depend on the order or the composition of the batch.  Errors:
 * AMC_E_INVALID (NULL arrays, bad offsets, an unknown model, invalid or out-of-scope options), AMC_E_NOMEM, AMC_E_HIP. */
int amc_estimate_absolute_poses(amc_ctx* ctx, const uint64_t* offsets, size_t nqueries, const int32_t* camera_models,
                                const double* camera_params, const double* points2D, const double* points3D,
                                const amc_abspose_opts* estimation_options,
                                const amc_abspose_refine_opts* refinement_options, int return_covariance,
                                amc_abspose_result* result);

/* Refine given poses: the layout above plus init_qvec (nqueries x 4, x y z w), init_tvec (nqueries x 3) and
 * inlier_mask (offsets[nqueries] bytes, non-zero = use the correspondence). */
int amc_refine_absolute_poses(amc_ctx* ctx, const uint64_t* offsets, size_t nqueries, const int32_t* camera_models,
                              const double* camera_params, const double* points2D, const double* points3D,
                              const double* init_qvec, const double* init_tvec, const uint8_t* inlier_mask,
                              const amc_abspose_refine_opts* refinement_options, int return_covariance,
                              amc_abspose_result* result);

void amc_abspose_result_free(amc_abspose_result* result);

#ifdef __cplusplus
}
#endif

#endif /* AMC_ABSPOSE_H_ */
