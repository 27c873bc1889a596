/*
 * amc_sift.h — C ABI of libamc.so's SIFT extractor (gfx950): images in, keypoints and descriptors out.
 *
 * Additive to amc.h (AMC_ABI_VERSION is unchanged): a host that never extracts never calls these.  The algorithm is
 * VLFeat's SIFT as COLMAP's CPU extractor drives it, restated in DESIGN.md section 10 with its deviations; the results
 * are bit-identical to tests/sift_ref/sift_ref.cc.
 *
 * Reference surface (/root/reference/pycolmap/feature/sift.h, pipeline/extract_features.h):
 *   SiftExtractionOptions{first_octave, num_octaves, octave_resolution,
 *     peak_threshold, edge_threshold, max_num_orientations, upright,
 *     normalization, max_num_features, max_image_size}                  amc_sift_opts
 *   Sift.extract(image) -> (N x 4 keypoints, N x 128 descriptors / 512)  amc_sift_extract, one image or a batch
 */
#ifndef AMC_SIFT_H_
#define AMC_SIFT_H_

#include "amc.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { AMC_SIFT_L1_ROOT = 0, AMC_SIFT_L2 = 1 };

typedef struct amc_sift_opts {
    int32_t first_octave;         /* default -1 (x2 upsampling of the input) */
    int32_t num_octaves;          /* default 4 */
    int32_t octave_resolution;    /* default 3: levels per octave */
    double peak_threshold;        /* default 0.02 / 3 */
    double edge_threshold;        /* default 10 */
    int32_t max_num_orientations; /* default 2 */
    int32_t upright;              /* default 0: 1 gives every keypoint one feature at angle 0 */
    int32_t normalization;        /* AMC_SIFT_L1_ROOT (default) or AMC_SIFT_L2 */
    int32_t max_num_features;     /* default 8192: the cut of DESIGN.md section 10.1 (coarsest octaves kept) */
    int32_t max_image_size;       /* default 3200: an image larger in either dimension is refused (AMC_E_INVALID) */
} amc_sift_opts;

/* One 8-bit grey image: row y starts at pixels + y * pitch (pitch >= width bytes). */
typedef struct amc_sift_image {
    const uint8_t* pixels;
    int32_t width, height;
    int64_t pitch;
} amc_sift_image;

/* Image i owns features [offsets[i], offsets[i + 1]). */
typedef struct amc_sift_result {
    size_t nimages;
    uint64_t* offsets;     /* nimages + 1 */
    float* keypoints;      /* offsets[nimages] x 4: x, y (COLMAP convention: pixel centres at +0.5), scale (sigma in
                              input pixels), orientation (radians, (-pi, pi]) */
    uint8_t* descriptors;  /* offsets[nimages] x 128: min(255, round(512 x)) of the normalised descriptor */
    double device_ms;      /* first upload -> last result byte on the host: HIP events on the stream, host round trips
                              between stages included */
    double stage_ms[4];    /* stream time by stage between HIP events (host round trips included): scale space,
                              detection, orientation, descriptors */
    void* _priv;
} amc_sift_result;

void amc_sift_opts_default(amc_sift_opts* o);

/* Extract SIFT features from `nimages` images on ctx's device and stream.  Fills *result (release it with
 * amc_sift_result_free).  The device workspace is sized for the largest image of the call and freed before return. */
int amc_sift_extract(amc_ctx* ctx, const amc_sift_image* images, size_t nimages, const amc_sift_opts* opts,
                     amc_sift_result* result);

void amc_sift_result_free(amc_sift_result* result);

#ifdef __cplusplus
}
#endif

#endif /* AMC_SIFT_H_ */
