/*
 * amc_filter.h — C ABI of libamc.so's point filter (gfx950): the observations of a sparse model in, per observation the
 * squared reprojection error and whether it goes, per point the verdict and the new mean error out.
 *
 * Additive to amc.h (AMC_ABI_VERSION is unchanged): a host that never filters a model never calls these.  The
 * algorithm is COLMAP 3.9.1's Reconstruction::FilterPoints3D (observations with a large reprojection error first, then
 * points that no pair of views sees under a sufficient angle) restated in DESIGN.md section 16 with its deviations
 * F1-F7; the results are bit-identical to tests/filter_ref.
 *
 * Reference surface (pycolmap/scene/reconstruction.h of the reference binding):
 *   Reconstruction.filter_points3D / filter_points3D_in_images / filter_all_points3D
 *                                              one call on the flattened model, `selected` carrying the id set
 *   Reconstruction.update_point3D_errors       the same call with errors_only
 */
#ifndef AMC_FILTER_H_
#define AMC_FILTER_H_

#include "amc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what became of a point (amc_filter_result.point_verdict) */
enum {
    AMC_FILTER_KEPT = 0,
    AMC_FILTER_NOT_SELECTED = 1, /* outside the selection: nothing of it was decided */
    AMC_FILTER_SHORT_TRACK = 2,  /* deleted: fewer than two observations */
    AMC_FILTER_REPROJECTION = 3, /* deleted: at most one observation within max_reproj_error */
    AMC_FILTER_ANGLE = 4         /* deleted: no pair of its remaining observations reaches min_tri_angle */
};

typedef struct amc_filter_opts {
    double max_reproj_error; /* pixels; default 4.0 */
    double min_tri_angle;    /* degrees; default 1.5 */
    int32_t errors_only;     /* non-zero: no thresholds, no verdicts; point_error = the mean over the whole track */
    int32_t reserved;
} amc_filter_opts;

/* Host arrays, owned by the caller; none of them is modified. */
typedef struct amc_filter_problem {
    size_t num_cameras;
    const int32_t* camera_models;  /* num_cameras COLMAP model ids (0 .. 10) */
    const double* camera_params;   /* num_cameras x 12: the model's parameters first, the rest ignored */
    size_t num_images;
    const uint32_t* image_cameras; /* num_images camera indices */
    const double* qvec;            /* num_images x 4: cam_from_world rotation, Eigen order (x, y, z, w) */
    const double* tvec;            /* num_images x 3 */
    size_t num_points;
    const double* xyz;             /* num_points x 3 */
    const uint64_t* track_offsets; /* num_points + 1: point j's observations are track_offsets[j] .. [j + 1), in track order */
    const uint32_t* obs_image;     /* track_offsets[num_points] image indices */
    const double* obs_xy;          /* track_offsets[num_points] x 2 pixels */
    const uint8_t* selected;       /* num_points, non-zero = the point is filtered; NULL = every point */
} amc_filter_problem;

/* The arrays belong to the result until amc_filter_result_free. */
typedef struct amc_filter_result {
    uint64_t num_points, num_observations;
    uint64_t num_filtered;  /* the reference's return value: deleted observations, counted by its rules */
    double* obs_sq_error;   /* num_observations: DBL_MAX for a depth below DBL_EPSILON */
    uint8_t* obs_deleted;   /* num_observations: 1 = over max_reproj_error in a selected point of two or more */
    uint8_t* point_verdict; /* num_points: AMC_FILTER_* above */
    double* point_error;    /* num_points: the new mean error where the verdict is KEPT or ANGLE, else 0 */
    uint32_t num_batches;
    uint32_t reserved;
    double host_ms;         /* the call's wall time less device_ms: validation, planning, the working set's
                               allocation, counting */
    double device_ms;       /* first upload -> last result byte on the host (HIP events on ctx's stream): copies and
                               kernels, nothing else */
    double kernel_ms;       /* the kernels alone (HIP event spans, launch gaps included) */
    double copy_ms;         /* the uploads and downloads alone (HIP event spans); part of device_ms */
    double alloc_ms;        /* allocating the call's device working set, on the host clock; part of host_ms */
} amc_filter_result;

void amc_filter_opts_default(amc_filter_opts* o);

/* Filter the problem on ctx's device and stream.  Errors: AMC_E_INVALID (NULL arrays, offsets that are not
 * non-decreasing from 0, an unknown model, an index out of range, a negative or NaN max_reproj_error or
 * min_tri_angle), AMC_E_NOMEM, AMC_E_HIP.  On an error the result holds no arrays. */
int amc_filter_points3d(amc_ctx* ctx, const amc_filter_problem* problem, const amc_filter_opts* options,
                        amc_filter_result* result);
void amc_filter_result_free(amc_filter_result* result);

#ifdef __cplusplus
}
#endif

#endif /* AMC_FILTER_H_ */
