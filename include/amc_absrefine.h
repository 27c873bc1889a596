/*
 * amc_absrefine.h — C ABI of libamc.so's absolute pose with a variable camera (gfx950): the pose of amc_abspose.h
 * refined together with the camera's focal lengths and distortion parameters.
 *
 * Additive to amc.h and amc_abspose.h (AMC_ABI_VERSION is unchanged).  The algorithm is COLMAP 3.9.1's
 * RefineAbsolutePose with refine_focal_length / refine_extra_params honoured, and the flow of its
 * EstimateAndRefineAbsolutePose use in IncrementalMapper::RegisterNextImage: LO-RANSAC per focal-length factor, then
 * one joint refinement from the RANSAC's own pose with the camera scaled by the chosen factor.  It is restated in
 * DESIGN.md section 25; the results are bit-identical to tests/absrefine_ref, and with both flags 0 to
 * amc_refine_absolute_poses.
 *
 * The layout is amc_abspose.h's: CSR offsets over the correspondences, camera_models, camera_params (nqueries x 12
 * doubles), and its two option structs, whose refine_focal_length / refine_extra_params these entries honour.
 */
#ifndef AMC_ABSREFINE_H_
#define AMC_ABSREFINE_H_

#include "amc_abspose.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What amc_abspose_result holds, plus the cameras.  Arrays are host memory, owned by the library. */
typedef struct amc_absrefine_result {
    size_t nqueries;
    size_t ncorr;
    uint8_t* success;       /* nqueries: 1 = a pose and a camera */
    double* qvec;           /* nqueries x 4: cam_from_world rotation (x, y, z, w) */
    double* tvec;           /* nqueries x 3 */
    uint32_t* num_inliers;  /* nqueries: inliers of the chosen RANSAC (the input mask's count for refinement) */
    uint64_t* num_trials;   /* nqueries: as amc_abspose_result (0 for refinement) */
    double* focal_factor;   /* nqueries: the chosen focal-length factor (1 for refinement, 0 when no RANSAC succeeded) */
    double* covariance;     /* nqueries x 36: the pose block of the joint covariance when asked, else NULL */
    uint8_t* inlier_mask;   /* ncorr */
    double* camera_params;  /* nqueries x 12: the refined camera of a successful query; of a failed one the input,
                               scaled by the focal factor where one was chosen */
    double device_ms;
    double kernel_ms;
    uint32_t num_batches;   /* device batches of the joint refinement */
    void* _priv;
} amc_absrefine_result;

/* The options' defaults are amc_abspose_opts_default and amc_abspose_refine_opts_default (both flags 0). */

/* Refine given poses and cameras: amc_refine_absolute_poses' arguments.  A camera's variable parameters are its focal
 * lengths iff refine_focal_length and its extra parameters iff refine_extra_params; the principal point is constant.
 * Errors: AMC_E_INVALID (NULL arrays, bad offsets, an unknown model, invalid options) before the device is used,
 * AMC_E_NOMEM, AMC_E_HIP.  NaN and infinity in the data are a failed query, not an error.  Results do not depend on
 * the order, the composition or the split of the batch (AMC_ABSREFINE_BATCH_QUERIES bounds a device batch's queries). */
int amc_refine_poses_and_cameras(amc_ctx* ctx, const uint64_t* offsets, size_t nqueries, const int32_t* camera_models,
                                 const double* camera_params, const double* points2D, const double* points3D,
                                 const double* init_qvec, const double* init_tvec, const uint8_t* inlier_mask,
                                 const amc_abspose_refine_opts* refinement_options, int return_covariance,
                                 amc_absrefine_result* result);

/* Estimate (amc_estimate_absolute_poses' LO-RANSAC per focal-length factor), then refine the RANSAC's pose and the
 * scaled camera jointly. */
int amc_estimate_poses_and_cameras(amc_ctx* ctx, const uint64_t* offsets, size_t nqueries,
                                   const int32_t* camera_models, const double* camera_params, const double* points2D,
                                   const double* points3D, const amc_abspose_opts* estimation_options,
                                   const amc_abspose_refine_opts* refinement_options, int return_covariance,
                                   amc_absrefine_result* result);

void amc_absrefine_result_free(amc_absrefine_result* result);

#ifdef __cplusplus
}
#endif

#endif /* AMC_ABSREFINE_H_ */
