/*
 * amc_tracks.h — C ABI of libamc.so's track completion and track merging (gfx950): the arithmetic of COLMAP 3.9.1's
 * IncrementalTriangulator::CompleteTracks for a batch of points whose candidate observations the host has already
 * walked to, and the whole of IncrementalTriangulator::MergeTracks for a batch of connected components of points.
 *
 * Additive to amc.h (AMC_ABI_VERSION is unchanged): a host that never completes a track never calls these.  One item is
 * one point3D with the observations a completion walk from its track could test (the superset closure);
 * the library computes every candidate's squared reprojection error against the item's position (16.1) and whether it
 * passes the threshold.  Which of the passing candidates join the track is the host's sequential walk (18.1): the
 * library decides nothing that depends on the order.  The results are bit-identical to tests/tracks_ref.
 *
 * Reference surface (pycolmap/sfm/incremental_triangulator.h of the reference binding):
 *   IncrementalTriangulator.complete_tracks / complete_all_tracks     one amc_complete_tracks call each
 *   IncrementalTriangulator.merge_tracks / merge_all_tracks           one amc_merge_tracks call each
 *
 * Merging.  Two points are adjacent when an observation of one has a direct correspondence that
 * carries the other; merges never leave a connected component of that graph.  The host lays every component out
 * contiguously and the library runs Merge for the component's roots in their order, one lane per component, and reports
 * every root's return value and the log of its merges.  A component of k points has the slots 0 .. k - 1 for its points
 * in the problem's order and the slot k + j for the point its j-th merge makes.
 */
#ifndef AMC_TRACKS_H_
#define AMC_TRACKS_H_

#include "amc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMC_TRACKS_MAX_BATCH_CANDIDATES (1u << 23) /* a call with more candidates is split; the result is the same */
#define AMC_MERGE_MAX_COMPONENT_OBS 4096           /* a component with more observations is refused */

typedef struct amc_complete_opts {
    double complete_max_reproj_error; /* pixels; default 4.0 */
    double reserved;
} amc_complete_opts;

/* Host arrays, owned by the caller; none of them is modified. */
typedef struct amc_complete_problem {
    size_t num_cameras;
    const int32_t* camera_models;  /* num_cameras COLMAP model ids (0 .. 10) */
    const double* camera_params;   /* num_cameras x 12: the model's parameters first, the rest ignored */
    size_t num_images;
    const uint32_t* image_cameras; /* num_images camera indices */
    const double* qvec;            /* num_images x 4: cam_from_world rotation, Eigen order (x, y, z, w) */
    const double* tvec;            /* num_images x 3 */
    size_t num_items;
    const double* item_xyz;        /* num_items x 3: the points' positions */
    const uint64_t* item_offsets;  /* num_items + 1: item i's candidates are item_offsets[i] .. [i + 1); may be none */
    const uint32_t* cand_image;    /* item_offsets[num_items] image indices */
    const double* cand_xy;         /* item_offsets[num_items] x 2 pixels */
} amc_complete_problem;

/* The arrays belong to the result until amc_complete_result_free. */
typedef struct amc_complete_result {
    uint64_t num_items, num_candidates;
    uint64_t num_passed;    /* candidates whose pass byte is set */
    double* cand_sq_error;  /* num_candidates: 16.1's squared error; DBL_MAX for a depth below DBL_EPSILON */
    uint8_t* cand_pass;     /* num_candidates: !(error > complete_max_reproj_error^2), so a NaN error passes */
    uint32_t num_batches;
    uint32_t reserved;
    double host_ms;         /* the call's wall time less device_ms */
    double device_ms;       /* first upload -> last result byte on the host (HIP events on ctx's stream) */
    double kernel_ms;       /* the kernels alone (HIP event spans, launch gaps included) */
    double copy_ms;         /* the uploads and downloads alone; part of device_ms */
    double alloc_ms;        /* allocating the call's device working set, on the host clock; part of host_ms */
} amc_complete_result;

void amc_complete_opts_default(amc_complete_opts* o);

/* Test the candidates on ctx's device and stream.  Errors: AMC_E_INVALID (NULL arrays, offsets that are not
 * non-decreasing from 0, an unknown model, an index out of range, a complete_max_reproj_error that is negative or NaN),
 * AMC_E_NOMEM, AMC_E_HIP.  Pixels, poses and points that are not finite are computed, not refused.  A call without
 * candidates touches no device.  On an error the result holds no arrays. */
int amc_complete_tracks(amc_ctx* ctx, const amc_complete_problem* problem, const amc_complete_opts* options,
                        amc_complete_result* result);
void amc_complete_result_free(amc_complete_result* result);

typedef struct amc_merge_opts {
    double merge_max_reproj_error; /* pixels; default 4.0 */
    double reserved;
} amc_merge_opts;

/* Host arrays, owned by the caller; none of them is modified.  All indices are the call's, not the component's. */
typedef struct amc_merge_problem {
    size_t num_cameras;
    const int32_t* camera_models;        /* as in amc_complete_problem */
    const double* camera_params;
    size_t num_images;
    const uint32_t* image_cameras;
    const double* qvec;
    const double* tvec;
    size_t num_components;
    const uint64_t* comp_point_offsets;  /* num_components + 1: component c's points; at least one each */
    const uint64_t* comp_root_offsets;   /* num_components + 1: component c's roots */
    const uint32_t* roots;               /* comp_root_offsets[num_components] point indices, each inside its component */
    const double* point_xyz;             /* num_points x 3 */
    const uint64_t* point_obs_offsets;   /* num_points + 1: a point's observations in track order; at least one each */
    const uint32_t* obs_image;           /* num_observations image indices */
    const double* obs_xy;                /* num_observations x 2 pixels */
    const uint64_t* obs_corr_offsets;    /* num_observations + 1: an observation's correspondences that carry a point */
    const uint32_t* corr_obs;            /* the corresponding observations in the graph's list order, each inside the
                                            observation's component */
} amc_merge_problem;

/* The arrays belong to the result until amc_merge_result_free. */
typedef struct amc_merge_result {
    uint64_t num_components, num_points, num_observations, num_roots;
    uint64_t num_merges;          /* over all roots */
    uint64_t num_pairs_tried;     /* pairs of points whose merged position was tested */
    uint32_t* root_return;        /* num_roots: Merge's return value, the length of the root's last merged track or 0 */
    uint64_t* root_merge_offsets; /* num_roots + 1: root r logged the merges root_merge_offsets[r] .. [r + 1) */
    uint32_t* merge_current;      /* num_merges: the component's slot of `current` */
    uint32_t* merge_other;        /* num_merges: the slot of the point merged into it */
    double* merge_xyz;            /* num_merges x 3: the merged position */
    uint32_t num_batches;
    uint32_t reserved;
    double host_ms, device_ms, kernel_ms, copy_ms, alloc_ms; /* as in amc_complete_result */
} amc_merge_result;

void amc_merge_opts_default(amc_merge_opts* o);

/* Merge on ctx's device and stream.  Errors: AMC_E_INVALID (NULL arrays, offsets that are not non-decreasing from 0, a
 * component without points, a point without observations, a component of more than AMC_MERGE_MAX_COMPONENT_OBS
 * observations, a root or a correspondence outside its component, an unknown model, an index out of range, a
 * merge_max_reproj_error that is negative or NaN), AMC_E_NOMEM, AMC_E_HIP.  A call without components touches no
 * device.  On an error the result holds no arrays. */
int amc_merge_tracks(amc_ctx* ctx, const amc_merge_problem* problem, const amc_merge_opts* options,
                     amc_merge_result* result);
void amc_merge_result_free(amc_merge_result* result);

#ifdef __cplusplus
}
#endif

#endif /* AMC_TRACKS_H_ */
