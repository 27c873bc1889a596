/*
 * amc_initpair.h — C ABI of libamc.so's two-view triangulation of image pairs (gfx950): the loop over the
 * correspondences at the end of COLMAP 3.9.1's IncrementalMapper::RegisterInitialImagePair, as DESIGN.md section 21
 * restates it.  For every correspondence of every pair: both pixels to the normalised plane, TriangulatePoint's DLT,
 * the triangulation angle at the point, and the test
 *     tri_angle >= min_tri_angle && depth in view 1 >= DBL_EPSILON && depth in view 2 >= DBL_EPSILON.
 * The call takes many pairs, so that a search over candidate pairs can be one launch.
 *
 * Additive to amc.h (AMC_ABI_VERSION is unchanged): a host that never starts a model never calls these.  Every
 * correspondence is computed from its own two pixels and its pair's two images only; the results are bit-identical to
 * tests/initpair_ref.
 *
 * Reference surface (later pycolmap releases; the 0.6 binding has the options only):
 *   IncrementalMapper.register_initial_image_pair
 */
#ifndef AMC_INITPAIR_H_
#define AMC_INITPAIR_H_

#include "amc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A call with more correspondences is refused: the device indexes them with 32 bits, and a correspondence with its results takes
 * up to 101 bytes of device memory (6.3 GiB at the bound). */
#define AMC_INITPAIR_MAX_CORRS ((uint64_t)1 << 26)

typedef struct amc_pair_tri_opts {
    double min_tri_angle; /* radians (the host converts degrees once); default DegToRad(16); NaN accepts nothing */
    double reserved;
} amc_pair_tri_opts;

/* Host arrays, owned by the caller; none of them is modified. */
typedef struct amc_pair_tri_problem {
    size_t num_cameras;
    const int32_t* camera_models;  /* num_cameras COLMAP model ids (0 .. 10) */
    const double* camera_params;   /* num_cameras x 12: the model's parameters first, the rest ignored */
    size_t num_images;
    const uint32_t* image_cameras; /* num_images camera indices */
    const double* qvec;            /* num_images x 4: cam_from_world rotation, Eigen order (x, y, z, w) */
    const double* tvec;            /* num_images x 3 */
    size_t num_pairs;
    const uint32_t* pair_images;   /* num_pairs x 2 image indices; they may be equal */
    const uint64_t* pair_offsets;  /* num_pairs + 1: pair p's correspondences are pair_offsets[p] .. [p + 1); a pair
                                      may have none */
    const double* corr_xy1;        /* pair_offsets[num_pairs] x 2 pixels in the pair's first image */
    const double* corr_xy2;        /* pair_offsets[num_pairs] x 2 pixels in its second image */
} amc_pair_tri_problem;

/* The arrays belong to the result until amc_pair_tri_result_free. */
typedef struct amc_pair_tri_result {
    uint64_t num_pairs, num_corrs;
    uint64_t num_accepted;
    uint8_t* accepted;    /* num_corrs: 1 = the test above holds */
    double* xyz;          /* num_corrs x 3: the triangulated point, whatever the test says */
    double* tri_angle;    /* num_corrs: radians; every NaN is the quiet NaN 0x7ff8000000000000 */
    uint32_t num_batches; /* kernel launches over the correspondences */
    uint32_t reserved;
    double host_ms;       /* the call's wall time less device_ms */
    double device_ms;     /* first upload -> last result byte on the host (HIP events on ctx's stream) */
    double kernel_ms;     /* the kernels alone */
    double copy_ms;       /* the uploads and downloads alone; part of device_ms */
    double alloc_ms;      /* allocating the call's device working set, on the host clock; part of host_ms */
} amc_pair_tri_result;

void amc_pair_tri_opts_default(amc_pair_tri_opts* o);

/* Errors: AMC_E_INVALID (NULL arguments or arrays, offsets that do not start at 0 or decrease, an unknown model, an
 * index out of range, more than AMC_INITPAIR_MAX_CORRS correspondences), AMC_E_NOMEM, AMC_E_HIP.  Pixels, poses and a
 * min_tri_angle that are not finite are computed, not refused.  A call without correspondences touches no device.  On
 * an error the result holds no arrays.  AMC_INITPAIR_BATCH_CORRS (environment, read per call) bounds the
 * correspondences of one launch: a test hook, the result does not depend on it. */
int amc_triangulate_pairs(amc_ctx* ctx, const amc_pair_tri_problem* problem, const amc_pair_tri_opts* options,
                          amc_pair_tri_result* result);
void amc_pair_tri_result_free(amc_pair_tri_result* result);

#ifdef __cplusplus
}
#endif

#endif /* AMC_INITPAIR_H_ */
