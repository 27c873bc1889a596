/*
 * amc_rigpose.h — C ABI of libamc.so's absolute pose of a multi-camera rig (gfx950): 2D-3D correspondences seen by the
 * cameras of a rig in, one plain RANSAC of the generalised P3P with unique-point support and a robust refinement of
 * rig_from_world per query, rig poses and inlier masks out.
 *
 * Additive to amc.h and amc_abspose.h (AMC_ABI_VERSION is unchanged).  The algorithm is COLMAP 3.9.1's
 * EstimateGeneralizedAbsolutePose + RefineGeneralizedAbsolutePose as the pycolmap 0.6 binding drives them, restated in
 * DESIGN.md section 13 with its deviations R1-R9; the results are bit-identical to tests/rigpose_ref.
 *
 * Reference surface (pycolmap/estimators/generalized_absolute_pose.h of the reference binding):
 *   RANSACOptions                                                          amc_ransac_opts (amc.h)
 *   AbsolutePoseRefinementOptions                                          amc_abspose_refine_opts (amc_abspose.h)
 *   rig_absolute_pose_estimation(points2D, points3D, camera_idxs, cams_from_rig, cameras, estimation_options,
 *                                refinement_options, return_covariance)
 *     -> None | {"rig_from_world", "num_inliers", "inliers"[, "covariance"]}
 *                                                                          amc_estimate_rig_absolute_poses, one query
 *                                                                          or a batch
 */
#ifndef AMC_RIGPOSE_H_
#define AMC_RIGPOSE_H_

#include "amc.h"
#include "amc_abspose.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Query i owns correspondences [offsets[i], offsets[i + 1]) and cameras [camera_offsets[i], camera_offsets[i + 1]).
 * Arrays are host memory, owned by the library. */
typedef struct amc_rigpose_result {
    size_t nqueries;
    size_t ncorr;
    uint8_t* success;       /* nqueries: 1 = a pose (estimation and refinement both succeeded) */
    double* qvec;           /* nqueries x 4: rig_from_world rotation, Eigen order (x, y, z, w) */
    double* tvec;           /* nqueries x 3: rig_from_world translation */
    uint32_t* num_inliers;  /* nqueries: inliers with distinct 3D points (what the reference reports) */
    uint32_t* num_all_inliers; /* nqueries: the inlier mask's count */
    uint64_t* num_trials;   /* nqueries: report.num_trials of the RANSAC */
    double* covariance;     /* nqueries x 36 (row-major 6 x 6, rotation first) when asked, else NULL */
    uint8_t* inlier_mask;   /* ncorr: the RANSAC's inlier mask */
    double device_ms;       /* first upload -> last result byte on the host (HIP events on ctx's stream) */
    double kernel_ms;       /* the kernels alone, summed over the batches (HIP events) */
    uint32_t num_batches;   /* device batches the call was split into */
    void* _priv;
} amc_rigpose_result;

/* Estimate and refine rig_from_world of `nqueries` queries on ctx's device and stream.
 *   offsets         nqueries + 1 values, offsets[0] = 0, non-decreasing (CSR over the correspondences)
 *   camera_offsets  nqueries + 1 values, camera_offsets[0] = 0, non-decreasing (CSR over the cameras)
 *   camera_models   camera_offsets[nqueries] COLMAP model ids (0 .. 10)
 *   camera_params   camera_offsets[nqueries] x 12 doubles: the model's parameters first, the rest ignored
 *   cams_from_rig   camera_offsets[nqueries] x 7 doubles: rotation x y z w, translation x y z
 *   camera_idxs     offsets[nqueries] indices into the query's own cameras (0 .. its camera count - 1)
 *   points2D        offsets[nqueries] x 2 doubles: pixels
 *   points3D        offsets[nqueries] x 3 doubles: world points; correspondences of a query whose three doubles compare
 *                   equal are one point to the support count
 * Results do not depend on the order or the composition of the batch.  Errors: AMC_E_INVALID (NULL arrays, bad
 * offsets, an unknown model, a camera index out of its query's range, invalid or out-of-scope options), AMC_E_NOMEM,
 * AMC_E_HIP. */
int amc_estimate_rig_absolute_poses(amc_ctx* ctx, const uint64_t* offsets, size_t nqueries,
                                    const uint64_t* camera_offsets, const int32_t* camera_models,
                                    const double* camera_params, const double* cams_from_rig,
                                    const int32_t* camera_idxs, const double* points2D, const double* points3D,
                                    const amc_ransac_opts* ransac_options,
                                    const amc_abspose_refine_opts* refinement_options, int return_covariance,
                                    amc_rigpose_result* result);

void amc_rigpose_result_free(amc_rigpose_result* result);

#ifdef __cplusplus
}
#endif

#endif /* AMC_RIGPOSE_H_ */
