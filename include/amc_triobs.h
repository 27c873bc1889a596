/*
 * amc_triobs.h — C ABI of libamc.so's observation triangulator (gfx950): the arithmetic of COLMAP 3.9.1's
 * IncrementalTriangulator::TriangulateImage for a batch of points2D whose correspondences the host has already found.
 *
 * Additive to amc.h (AMC_ABI_VERSION is unchanged): a host that never triangulates an image never calls these.  One
 * item is one reference point2D with the observations Find gave it; the library runs Continue, then the Create rounds
 * (one LO-RANSAC of DESIGN.md section 11 per round, on the observations no earlier round took), and reports what the
 * host has to apply to its model.  DESIGN.md section 17 restates the algorithm with its deviations; the results are
 * bit-identical to tests/triangulator_ref.
 *
 * Reference surface (pycolmap/sfm/incremental_triangulator.h of the reference binding):
 *   IncrementalTriangulator.triangulate_image     one call per run of points2D with disjoint observation sets
 */
#ifndef AMC_TRIOBS_H_
#define AMC_TRIOBS_H_

#include "amc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMC_TRIOBS_MAX_ITEM_CANDIDATES 4096 /* an item with more candidates is refused */

typedef struct amc_triobs_opts {
    double create_max_angle_error;   /* degrees; default 2.0; the RANSAC's max_error */
    double continue_max_angle_error; /* degrees; default 2.0 */
    double min_angle;                /* degrees; default 1.5; the RANSAC's min_tri_angle */
    double reserved;
} amc_triobs_opts;

/* Host arrays, owned by the caller; none of them is modified. */
typedef struct amc_triobs_problem {
    size_t num_cameras;
    const int32_t* camera_models;  /* num_cameras COLMAP model ids (0 .. 10) */
    const double* camera_params;   /* num_cameras x 12: the model's parameters first, the rest ignored */
    size_t num_images;
    const uint32_t* image_cameras; /* num_images camera indices */
    const double* qvec;            /* num_images x 4: cam_from_world rotation, Eigen order (x, y, z, w) */
    const double* tvec;            /* num_images x 3 */
    size_t num_items;
    const uint64_t* item_offsets;  /* num_items + 1: item i's candidates are item_offsets[i] .. [i + 1), the
                                      correspondences in Find's order, then the reference observation: at least one */
    const uint32_t* cand_image;    /* item_offsets[num_items] image indices */
    const double* cand_xy;         /* item_offsets[num_items] x 2 pixels */
    const uint8_t* cand_has_point; /* item_offsets[num_items]: non-zero = the observation carries a point3D */
    const double* cand_xyz;        /* item_offsets[num_items] x 3: that point; ignored where the flag is zero */
    const uint8_t* no_create_two_view; /* num_items: non-zero = the first Create round returns when it has exactly two
                                      observations (the host's ignore_two_view_tracks && IsTwoViewObservation of the
                                      first candidate without a point); NULL = all zero */
} amc_triobs_problem;

/* The arrays belong to the result until amc_triobs_result_free. */
typedef struct amc_triobs_result {
    uint64_t num_items, num_candidates;
    uint64_t num_created;   /* tracks created over all items */
    uint64_t num_continued; /* items whose reference observation joined an existing point */
    int32_t* continued;     /* num_items: the item-local index of the candidate whose point the reference observation
                               joins, or -1 */
    uint32_t* cand_round;   /* num_candidates: the Create round (1, 2, ..) whose track the candidate joined, or 0 */
    uint64_t* round_offsets;/* num_items + 1: item i created round_offsets[i + 1] - round_offsets[i] tracks */
    double* round_xyz;      /* num_created x 3, by item and within an item in round order */
    uint32_t num_batches;
    uint32_t reserved;
    double host_ms;         /* the call's wall time less device_ms */
    double device_ms;       /* first upload -> last result byte on the host (HIP events on ctx's stream) */
    double kernel_ms;       /* the kernels alone (HIP event spans, launch gaps included) */
    double copy_ms;         /* the uploads and downloads alone; part of device_ms */
    double alloc_ms;        /* allocating the call's device working set, on the host clock; part of host_ms */
} amc_triobs_result;

void amc_triobs_opts_default(amc_triobs_opts* o);

/* Triangulate the items on ctx's device and stream.  Errors: AMC_E_INVALID (NULL arrays, offsets that are not
 * non-decreasing from 0, an item without candidates or with more than AMC_TRIOBS_MAX_ITEM_CANDIDATES, an unknown
 * model, an index out of range, an angle option that is negative or NaN, a create_max_angle_error of 0), AMC_E_NOMEM,
 * AMC_E_HIP.  Pixels, poses and points that are not finite are computed, not refused.  On an error the result holds
 * no arrays. */
int amc_triangulate_observations(amc_ctx* ctx, const amc_triobs_problem* problem, const amc_triobs_opts* options,
                                 amc_triobs_result* result);
void amc_triobs_result_free(amc_triobs_result* result);

#ifdef __cplusplus
}
#endif

#endif /* AMC_TRIOBS_H_ */
