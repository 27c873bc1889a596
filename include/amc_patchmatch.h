/*
 * amc_patchmatch.h — C ABI of libamc.so's PatchMatch stereo (gfx950): depth and normal maps of reference images from
 * their source images, after Schoenberger, Zheng, Pollefeys, Frahm, "Pixelwise View Selection for Unstructured Multi-View
 * Stereo" (ECCV 2016), as DESIGN.md section 22 restates it.  One call runs one pass (photometric, or geometric from the
 * maps of a photometric pass) over a list of problems; a problem is a reference image, 1 .. AMC_PATCHMATCH_MAX_SOURCES
 * source images and a depth range.  All images are 8-bit grey with a PINHOLE camera.
 *
 * Additive to amc.h (AMC_ABI_VERSION is unchanged): a host that never makes a depth map never calls these.  Every random
 * number is a hash of (seed, reference image, row, column, sweep, draw); the results are bit-identical to
 * tests/patchmatch_ref and do not depend on how the problems are spread over calls or launches.
 *
 * Reference surface: PatchMatchOptions, patch_match_stereo (pycolmap/pipeline/mvs.h, CUDA builds only).
 */
#ifndef AMC_PATCHMATCH_H_
#define AMC_PATCHMATCH_H_

#include "amc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMC_PATCHMATCH_MAX_SOURCES 32
#define AMC_PATCHMATCH_MAX_WINDOW_RADIUS 32
#define AMC_PATCHMATCH_MAX_PIXELS ((uint64_t)1 << 31) /* of one image */
#define AMC_PATCHMATCH_NO_MAP UINT64_MAX

typedef struct amc_patch_match_opts {
    int32_t window_radius;     /* 1 .. AMC_PATCHMATCH_MAX_WINDOW_RADIUS; default 5 */
    int32_t window_step;       /* 1 .. window_radius; default 1 */
    int32_t num_samples;       /* >= 1; default 15 */
    int32_t num_iterations;    /* >= 0, four sweeps each; default 5 */
    int32_t geom_consistency;  /* the geometric pass: the input maps initialise the state and price the hypotheses; default 0 */
    int32_t filter;            /* default 0 */
    int32_t filter_min_num_consistent; /* default 2 */
    int32_t want_costs;        /* fill amc_patch_match_result.costs; default 0 */
    uint32_t seed;             /* default 0 */
    uint32_t reserved;
    double sigma_spatial;      /* <= 0: window_radius; default -1 */
    double sigma_color;        /* default 0.2 */
    double ncc_sigma;          /* default 0.6 */
    double min_triangulation_angle; /* degrees; default 1 */
    double incident_angle_sigma;    /* default 0.9 */
    double geom_consistency_regularizer; /* default 0.3 */
    double geom_consistency_max_cost;    /* pixels; default 3 */
    double filter_min_ncc;               /* default 0.1 */
    double filter_min_triangulation_angle; /* degrees; default 3 */
    double filter_geom_consistency_max_cost; /* pixels; default 1 */
} amc_patch_match_opts;

/* Host arrays, owned by the caller; none of them is modified. */
typedef struct amc_patch_match_problem {
    size_t num_images;
    const uint8_t* pixels;          /* the images' grey bytes, row-major */
    const uint64_t* pixel_offsets;  /* num_images: where each image starts in `pixels` */
    const int32_t* widths;          /* num_images */
    const int32_t* heights;         /* num_images */
    const double* K;                /* num_images x 4: fx, fy, cx, cy */
    const double* R;                /* num_images x 9: cam_from_world rotation, row-major */
    const double* t;                /* num_images x 3 */
    size_t num_problems;
    const uint32_t* ref_images;     /* num_problems image indices */
    const uint64_t* src_offsets;    /* num_problems + 1: problem p's sources are src_images[src_offsets[p] .. [p + 1]) */
    const uint32_t* src_images;
    const double* depth_ranges;     /* num_problems x 2: depth_min, depth_max; 0 < min <= max */
    /* the maps of an earlier pass, or three NULLs: image i's depth map (h x w) starts at in_depth[in_map_offsets[i]], its
     * normal map (3 x h x w, planar) at in_normal[3 * in_map_offsets[i]]; AMC_PATCHMATCH_NO_MAP: the image has none */
    const float* in_depth;
    const float* in_normal;
    const uint64_t* in_map_offsets; /* num_images */
} amc_patch_match_problem;

/* The arrays belong to the result until amc_patch_match_result_free. */
typedef struct amc_patch_match_result {
    uint64_t num_problems, num_pixels, num_costs;
    uint64_t* map_offsets;   /* num_problems + 1: problem p's maps start at pixel map_offsets[p] */
    uint64_t* cost_offsets;  /* num_problems + 1: problem p's costs start at costs[cost_offsets[p]] */
    float* depth;            /* num_pixels; problem p's h x w map; 0 = filtered */
    float* normal;           /* 3 x num_pixels; problem p's 3 x h x w planar map at normal[3 * map_offsets[p]] */
    uint8_t* num_consistent; /* num_pixels: the consistent sources of the filter (saturating at 255); 0 without filter */
    float* costs;            /* num_costs, [sources][h][w] per problem: the final state's cost in every source (the initial
                                state's with num_iterations = 0); NULL unless want_costs */
    uint32_t num_batches;    /* groups of problems that were launched together */
    uint32_t num_launches;   /* kernel launches */
    double host_ms;          /* the call's wall time less device_ms */
    double device_ms;        /* first upload -> last result byte on the host (HIP events on ctx's stream) */
    double kernel_ms;        /* the kernels alone */
    double copy_ms;          /* the uploads and downloads alone; part of device_ms */
    double alloc_ms;         /* allocating the call's device working set, on the host clock; part of host_ms */
} amc_patch_match_result;

void amc_patch_match_opts_default(amc_patch_match_opts* o);

/* Errors: AMC_E_INVALID (NULL arguments or arrays, an option out of its range, a problem without sources or with more
 * than AMC_PATCHMATCH_MAX_SOURCES, an image without pixels or over AMC_PATCHMATCH_MAX_PIXELS, an index out of range, a
 * depth range that is not 0 < min <= max), AMC_E_NOMEM, AMC_E_HIP.  Nothing is refused for a pose or an intrinsic that is
 * not finite: such a source costs the maximum everywhere.  A call without problems touches no device.  On an error the
 * result holds no arrays.  AMC_PATCHMATCH_BATCH_BYTES (environment, read per call) bounds the state bytes of the
 * problems of one launch: a test hook, the result does not depend on it. */
int amc_patch_match(amc_ctx* ctx, const amc_patch_match_opts* opts, const amc_patch_match_problem* problem,
                    amc_patch_match_result* result);
void amc_patch_match_result_free(amc_patch_match_result* result);

#ifdef __cplusplus
}
#endif

#endif /* AMC_PATCHMATCH_H_ */
