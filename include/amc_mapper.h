/*
 * amc_mapper.h — C ABI of libamc.so's two image-level statistics of COLMAP 3.9.1's IncrementalMapper (gfx950), as
 * DESIGN.md section 20 restates them:
 *   amc_image_visibility     what COLMAP's Image keeps incrementally for an image that is not in the model yet: the
 *                            number of its points2D with a correspondence, the number with a correspondence that
 *                            carries a point3D, and the VisibilityPyramid score of the latter (FindNextImages, 20.1)
 *   amc_shared_point_angles  the percentile triangulation angle of an image pair over the points they share
 *                            (FindLocalBundle, 20.3)
 *
 * Additive to amc.h (AMC_ABI_VERSION is unchanged): a host that never maps never calls these.  Every output of the
 * first call is an integer and the second selects one of the angles it computed, so both are bit-identical to
 * tests/mapper_ref.
 *
 * Reference surface (later pycolmap releases; the 0.6 binding has the options only):
 *   IncrementalMapper.find_next_images, IncrementalMapper.find_local_bundle
 */
#ifndef AMC_MAPPER_H_
#define AMC_MAPPER_H_

#include "amc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* point2D_point3D's "none" */
#define AMC_MAPPER_NO_POINT3D UINT64_MAX
/* the pyramid: level l = 0 .. 5 has 2^(l + 1) x 2^(l + 1) cells, an occupied cell of it scores 4^(l + 1) */
#define AMC_MAPPER_PYRAMID_LEVELS 6
#define AMC_MAPPER_MAX_SCORE 17895696ull /* 16 + 256 + 4096 + 65536 + 1048576 + 16777216 */
/* A pair with more shared points is refused: the rank and the counts of the selection are 32-bit, and one wave walks
 * the pair's keys 64 times. */
#define AMC_MAPPER_MAX_PAIR_POINTS ((uint64_t)1 << 20)

/* Host arrays, owned by the caller; none of them is modified. */
typedef struct amc_visibility_problem {
    size_t num_graph_images;
    const uint64_t* image_point_offsets; /* num_graph_images + 1: graph image g's points2D are rows
                                            image_point_offsets[g] .. [g + 1) of point2D_point3D */
    const uint64_t* point2D_point3D;     /* per point2D of every graph image: its point3D id, or AMC_MAPPER_NO_POINT3D */
    size_t num_candidates;
    const uint32_t* cand_width;          /* num_candidates: the camera's width */
    const uint32_t* cand_height;         /* num_candidates */
    const uint64_t* cand_point_offsets;  /* num_candidates + 1: candidate c's points2D are cand_point_offsets[c] .. [c + 1) */
    const double* cand_xy;               /* 2 per candidate point2D: pixels; anything, NaN included, is computed (20.1) */
    const uint64_t* corr_offsets;        /* cand_point_offsets[num_candidates] + 1: the correspondences of a point2D */
    const uint32_t* corr_image;          /* per correspondence: a graph image index */
    const uint32_t* corr_point2D;        /* per correspondence: a point2D index of that image */
} amc_visibility_problem;

/* The arrays belong to the result until amc_visibility_result_free. */
typedef struct amc_visibility_result {
    uint64_t num_candidates;
    uint32_t* num_observations;     /* num_candidates: points2D with at least one correspondence */
    uint32_t* num_visible_points3D; /* num_candidates: points2D with at least one correspondence that carries a point3D */
    uint64_t* score;                /* num_candidates: the pyramid score of the visible points2D */
    uint64_t max_score;             /* AMC_MAPPER_MAX_SCORE */
    uint32_t num_batches;           /* kernel launches */
    uint32_t reserved;
    double host_ms;                 /* the call's wall time less device_ms */
    double device_ms;               /* first upload -> last result byte on the host (HIP events on ctx's stream) */
    double kernel_ms;               /* the kernels alone */
    double copy_ms;                 /* the uploads and downloads alone; part of device_ms */
    double alloc_ms;                /* allocating the call's device working set, on the host clock; part of host_ms */
} amc_visibility_result;

/* Errors: AMC_E_INVALID (NULL arguments or arrays, offsets that do not start at 0, decrease or, for corr_offsets, do
 * not have one entry per candidate point2D; a correspondence that names an image or a point2D the table does not hold;
 * a candidate of 2^32 or more points2D), AMC_E_NOMEM, AMC_E_HIP.  A call without candidates touches no device.  On an error
 * the result holds no arrays. */
int amc_image_visibility(amc_ctx* ctx, const amc_visibility_problem* problem, amc_visibility_result* result);
void amc_visibility_result_free(amc_visibility_result* result);

typedef struct amc_pair_angle_opts {
    double percentile; /* 0 .. 100; default 75; a pair of n points takes the element of rank
                          round(percentile / 100 * (n - 1)), half away from zero, in ascending order, NaN last */
} amc_pair_angle_opts;

typedef struct amc_pair_angle_problem {
    size_t num_images;
    const double* qvec;            /* num_images x 4: cam_from_world rotation, Eigen order (x, y, z, w) */
    const double* tvec;            /* num_images x 3 */
    size_t num_points;
    const double* point_xyz;       /* num_points x 3 */
    size_t num_pairs;
    const uint32_t* pair_images;   /* num_pairs x 2 image indices; they may be equal */
    const uint64_t* pair_offsets;  /* num_pairs + 1: pair p's shared points are pair_offsets[p] .. [p + 1); at least one
                                      and at most AMC_MAPPER_MAX_PAIR_POINTS */
    const uint32_t* shared_points; /* pair_offsets[num_pairs] point indices; a point may be listed more than once */
} amc_pair_angle_problem;

typedef struct amc_pair_angle_result {
    uint64_t num_pairs;
    double* angle;        /* num_pairs: radians; every NaN is the quiet NaN 0x7ff8000000000000 */
    uint32_t num_batches; /* angle kernel launches */
    uint32_t reserved;
    double host_ms, device_ms, kernel_ms, copy_ms, alloc_ms; /* as above */
} amc_pair_angle_result;

void amc_pair_angle_opts_default(amc_pair_angle_opts* o);
/* Errors: AMC_E_INVALID (NULL arguments or arrays, bad offsets, an index out of range, a pair without shared points or
 * with more than AMC_MAPPER_MAX_PAIR_POINTS, a percentile outside 0 .. 100 or NaN), AMC_E_NOMEM, AMC_E_HIP.  Poses and
 * points that are not finite are computed, not refused.  A call without pairs touches no device. */
int amc_shared_point_angles(amc_ctx* ctx, const amc_pair_angle_problem* problem, const amc_pair_angle_opts* options,
                            amc_pair_angle_result* result);
void amc_pair_angle_result_free(amc_pair_angle_result* result);

#ifdef __cplusplus
}
#endif

#endif /* AMC_MAPPER_H_ */
