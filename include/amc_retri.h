/*
 * amc_retri.h — C ABI of libamc.so's pair retriangulator (gfx950): the arithmetic of COLMAP 3.9.1's
 * IncrementalTriangulator::Retriangulate for image pairs the host has already coloured into rounds.
 *
 * Additive to amc.h (AMC_ABI_VERSION is unchanged): a host that never retriangulates never calls these.  A pair is
 * two images and the one-to-one list of their correspondences, as observation indices.  The pairs of a round share no
 * image, so a round is one device step: the library tests every pair of the round for
 * under-reconstruction on the state the earlier rounds left, runs Continue or a two-observation Create for every
 * correspondence of the pairs that pass, applies the outcome to its own copy of the state and goes on to the next
 * round without returning to the host.  The results are bit-identical to tests/retri_ref and, correspondence by
 * correspondence, to amc_triangulate_observations on the equivalent two-candidate item.
 *
 * Reference surface (pycolmap/sfm/incremental_triangulator.h of the reference binding):
 *   IncrementalTriangulator.retriangulate     one call
 */
#ifndef AMC_RETRI_H_
#define AMC_RETRI_H_

#include "amc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A call with more correspondences is refused.  A problem may list at most two observations and two points per
 * correspondence, so the device working set is at most 168 bytes per correspondence (2.6 GiB at the bound) plus 13
 * bytes per pair, 188 per image, 100 per camera and 5 KiB of alignment, and a created point's slot,
 * num_points + the correspondence's index, fits an int32. */
#define AMC_RETRI_MAX_CORRS ((uint64_t)1 << 24)

/* what happened to a correspondence */
#define AMC_RETRI_NONE 0          /* its pair did not run, both observations had a point, or a test failed */
#define AMC_RETRI_CONTINUE_1TO2 1 /* observation 2 joined observation 1's point */
#define AMC_RETRI_CONTINUE_2TO1 2 /* observation 1 joined observation 2's point */
#define AMC_RETRI_CREATED 3       /* a new point on both observations */

typedef struct amc_retri_opts {
    double create_max_angle_error; /* degrees; default 2.0; the two-observation RANSAC's max_error */
    double re_max_angle_error;     /* degrees; default 5.0; Continue's bound */
    double min_angle;              /* degrees; default 1.5; the RANSAC's min_tri_angle */
    double re_min_ratio;           /* default 0.2; a pair runs when num_tri_corrs / num_corrs < re_min_ratio */
} amc_retri_opts;

/* Host arrays, owned by the caller; none of them is modified. */
typedef struct amc_retri_problem {
    size_t num_cameras;
    const int32_t* camera_models;  /* num_cameras COLMAP model ids (0 .. 10) */
    const double* camera_params;   /* num_cameras x 12: the model's parameters first, the rest ignored */
    size_t num_images;
    const uint32_t* image_cameras; /* num_images camera indices */
    const double* qvec;            /* num_images x 4: cam_from_world rotation, Eigen order (x, y, z, w) */
    const double* tvec;            /* num_images x 3 */
    size_t num_obs;
    const uint32_t* obs_image;     /* num_obs image indices */
    const double* obs_xy;          /* num_obs x 2 pixels */
    const int32_t* obs_point;      /* num_obs: the index of the point the observation carries, or -1 */
    size_t num_points;
    const double* point_xyz;       /* num_points x 3 */
    size_t num_pairs;
    const uint32_t* pair_images;   /* num_pairs x 2 image indices, different from one another */
    const uint64_t* pair_offsets;  /* num_pairs + 1: pair p's correspondences are pair_offsets[p] .. [p + 1); none is
                                      allowed */
    const uint32_t* corr_obs;      /* pair_offsets[num_pairs] x 2 observation indices: the first of the pair's first
                                      image, the second of its second; no observation twice in one pair */
    const uint8_t* corr_two_view;  /* pair_offsets[num_pairs]: non-zero = no Create for this correspondence (the host's
                                      ignore_two_view_tracks && IsTwoViewObservation of its first observation);
                                      NULL = all zero */
    size_t num_rounds;
    const uint64_t* round_offsets; /* num_rounds + 1: round r's pairs are round_offsets[r] .. [r + 1), ending at
                                      num_pairs; the pairs of a round share no image */
} amc_retri_problem;

/* The arrays belong to the result until amc_retri_result_free. */
typedef struct amc_retri_result {
    uint64_t num_pairs, num_corrs;
    uint64_t num_pairs_run; /* pairs whose ratio test passed */
    uint64_t num_continued; /* correspondences with a CONTINUE action */
    uint64_t num_created;   /* correspondences with the CREATED action */
    uint8_t* pair_ran;      /* num_pairs: 1 = under-reconstructed when its round came */
    uint32_t* pair_num_tri; /* num_pairs: the correspondences whose observations carried one point, as the test saw it */
    uint8_t* corr_action;   /* num_corrs: AMC_RETRI_* */
    uint64_t* created_offsets; /* num_pairs + 1: pair p created created_offsets[p + 1] - created_offsets[p] points */
    double* created_xyz;    /* num_created x 3, by pair and within a pair in correspondence order */
    uint32_t num_launches;  /* ratio / correspondence kernel pairs queued */
    uint32_t reserved;
    double host_ms;         /* the call's wall time less device_ms */
    double device_ms;       /* first upload -> last result byte on the host (HIP events on ctx's stream) */
    double kernel_ms;       /* the kernels alone (HIP event spans, launch gaps included) */
    double copy_ms;         /* the uploads and downloads alone; part of device_ms */
    double alloc_ms;        /* allocating the call's device working set, on the host clock; part of host_ms */
} amc_retri_result;

void amc_retri_opts_default(amc_retri_opts* o);

/* Retriangulate the pairs on ctx's device and stream, round by round.  Errors: AMC_E_INVALID (NULL arrays, offsets that
 * are not non-decreasing from 0 or do not end at the array's length, an index out of range, an observation of another
 * image than its pair's, an unknown model, two pairs of one round sharing an image, an observation twice in one pair's
 * list, more than two observations or two points per correspondence, an angle or ratio that is negative or NaN, a
 * create_max_angle_error of 0, more than AMC_RETRI_MAX_CORRS correspondences), AMC_E_NOMEM, AMC_E_HIP.  Pixels, poses and points that are not finite are computed, not refused.
 * On an error the result holds no arrays. */
int amc_retriangulate_pairs(amc_ctx* ctx, const amc_retri_problem* problem, const amc_retri_opts* options,
                            amc_retri_result* result);
void amc_retri_result_free(amc_retri_result* result);

#ifdef __cplusplus
}
#endif

#endif /* AMC_RETRI_H_ */
