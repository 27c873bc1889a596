/*
 * amc_fusion.h — C ABI of libamc.so's stereo fusion (gfx950): the depth and normal maps of a dense workspace fused into
 * one point cloud with normals, colours and visibility, after COLMAP's mvs::StereoFusion as DESIGN.md section 23 restates
 * it.  One call fuses one ordered list of images; all cameras are PINHOLE, all images 8-bit RGB.
 *
 * Additive to amc.h (AMC_ABI_VERSION is unchanged): a host that never fuses never calls these.  The results are
 * bit-identical to tests/fusion_ref and do not depend on how the seeds are spread over launches.
 *
 * Reference surface: StereoFusionOptions, stereo_fusion (pycolmap/pipeline/mvs.h).
 */
#ifndef AMC_FUSION_H_
#define AMC_FUSION_H_

#include "amc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMC_FUSION_MAX_NEIGHBOURS 64        /* of one image: a lane each */
#define AMC_FUSION_MAX_TRAVERSAL_DEPTH 128  /* the walk's stack */
#define AMC_FUSION_MAX_CLUSTER 256          /* members of one cluster: 48 bytes of LDS each (section 23.6) */
#define AMC_FUSION_MAX_PIXELS ((uint64_t)1 << 31) /* of one image */
#define AMC_FUSION_NO_MAP UINT64_MAX

typedef struct amc_fusion_opts {
    int32_t min_num_pixels;       /* >= 0; default 5 */
    int32_t max_num_pixels;       /* >= 1 and >= min_num_pixels; default 10000; above AMC_FUSION_MAX_CLUSTER that bound holds */
    int32_t max_traversal_depth;  /* 1 .. AMC_FUSION_MAX_TRAVERSAL_DEPTH; default 100 */
    int32_t reserved;
    double max_reproj_error;      /* pixels, >= 0; default 2 */
    double max_depth_error;       /* relative, >= 0; default 0.01 */
    double max_normal_error;      /* degrees, >= 0; default 10 */
    double bounding_box[6];       /* min x y z, max x y z; default: the lowest and the largest float32 */
} amc_fusion_opts;

/* Host arrays, owned by the caller; none of them is modified. */
typedef struct amc_fusion_problem {
    size_t num_images;
    const uint8_t* rgb;             /* the images' bytes, row-major, r g b per pixel */
    const uint64_t* rgb_offsets;    /* num_images: where each image starts in `rgb` */
    const int32_t* widths;          /* num_images */
    const int32_t* heights;         /* num_images */
    const double* K;                /* num_images x 4: fx, fy, cx, cy */
    const double* R;                /* num_images x 9: cam_from_world rotation, row-major */
    const double* t;                /* num_images x 3 */
    /* image i's depth map (h x w) starts at depth[map_offsets[i]], its normal map (3 x h x w, planar, in the camera's
     * frame) at normal[3 * map_offsets[i]]; AMC_FUSION_NO_MAP: the image has none */
    const float* depth;
    const float* normal;
    const uint64_t* map_offsets;    /* num_images */
    const uint64_t* nb_offsets;     /* num_images + 1: image i's neighbours are nb_images[nb_offsets[i] .. [i + 1]) */
    const uint32_t* nb_images;
} amc_fusion_problem;

/* The arrays belong to the result until amc_fusion_result_free. */
typedef struct amc_fusion_result {
    uint64_t num_points;
    float* xyz;              /* num_points x 3 */
    float* normal;           /* num_points x 3 */
    uint8_t* color;          /* num_points x 3: r g b */
    uint32_t* seed_image;    /* num_points: the seed's image ... */
    uint32_t* seed_pixel;    /* ... and pixel, row * width + col */
    uint32_t* num_fused;     /* num_points: the cluster's members */
    uint64_t* vis_offsets;   /* num_points + 1: point p is seen by vis_images[vis_offsets[p] .. [p + 1]), ascending */
    uint32_t* vis_images;
    uint64_t num_seeds;      /* clusters built, with and without a point */
    uint64_t num_truncated;  /* clusters that AMC_FUSION_MAX_CLUSTER cut short while max_num_pixels was larger */
    uint32_t num_batches;    /* cluster launches */
    uint32_t num_launches;   /* kernel launches of every kind */
    double host_ms;          /* the call's wall time less device_ms */
    double device_ms;        /* first upload -> last result byte on the host (HIP events on ctx's stream) */
    double kernel_ms;        /* the kernels alone */
    double copy_ms;          /* the uploads and downloads alone; part of device_ms */
    double alloc_ms;         /* allocating the call's device working set, on the host clock; part of host_ms */
} amc_fusion_result;

void amc_fusion_opts_default(amc_fusion_opts* o);

/* Errors: AMC_E_INVALID (NULL arguments or arrays, an option out of its range, an image with more than
 * AMC_FUSION_MAX_NEIGHBOURS neighbours, an image without pixels or over AMC_FUSION_MAX_PIXELS, an index out of range),
 * AMC_E_NOMEM, AMC_E_HIP.  Nothing is refused for a pose, an intrinsic or a map value that is not finite: such a pixel
 * joins no cluster.  A call without images touches no device.  On an error the result holds no arrays.
 * AMC_FUSION_BATCH_SEEDS (environment, read per call) bounds the seeds of one launch: a test hook, the result does not
 * depend on it. */
int amc_fuse_depth_maps(amc_ctx* ctx, const amc_fusion_opts* opts, const amc_fusion_problem* problem, amc_fusion_result* result);
void amc_fusion_result_free(amc_fusion_result* result);

#ifdef __cplusplus
}
#endif

#endif /* AMC_FUSION_H_ */
