/*
 * amc_undistort.h — C ABI of libamc.so's image undistortion (gfx950): distorted photographs and their cameras in,
 * PINHOLE images out, for the dense workspace that undistort_images writes.
 *
 * Additive to amc.h (AMC_ABI_VERSION is unchanged): a host that never undistorts never calls these.  The rules are
 * COLMAP 3.9.1's UndistortCamera and WarpImageBetweenCameras, restated in DESIGN.md section 14 with their deviations;
 * the results are bit-identical to tests/undistort_ref/undistort_ref.cc.
 *
 * Reference surface (/root/reference/pycolmap/pipeline/images.h):
 *   UndistortCameraOptions{blank_pixels, min_scale, max_scale, max_image_size, roi_*}   (lines 203-240)  amc_undistort_opts
 *   undistort_images(output_path, input_path, image_path, ...)                          (lines 96-148, 242-261)
 *     per image: UndistortCamera + WarpImageBetweenCameras                              amc_undistort_camera,
 *                                                                                       amc_undistort_images
 */
#ifndef AMC_UNDISTORT_H_
#define AMC_UNDISTORT_H_

#include "amc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* UndistortCameraOptions (images.h:203-240) */
typedef struct amc_undistort_opts {
    double blank_pixels;    /* default 0.0: 0 keeps no blank pixel, 1 keeps every source pixel */
    double min_scale;       /* default 0.2 */
    double max_scale;       /* default 2.0 */
    int32_t max_image_size; /* default -1: no limit */
    int32_t _pad;
    double roi_min_x;       /* default 0 */
    double roi_min_y;       /* default 0 */
    double roi_max_x;       /* default 1 */
    double roi_max_y;       /* default 1 */
} amc_undistort_opts;

/* One camera: a COLMAP model id (0 .. 10), the sensor size and the model's parameters (the rest of params is ignored). */
typedef struct amc_undistort_cam {
    int32_t model;
    int32_t _pad;
    uint64_t width, height;
    double params[12];
} amc_undistort_cam;

/* One image of a batch (images.h:96-148 undistorts one image per reader thread).  src: height rows of width x channels
 * interleaved bytes, src_stride bytes apart (>= width x channels); src_camera has the source's width and height.
 * dst: dst_camera.height rows of dst_camera.width x channels bytes, tightly packed; dst_camera is PINHOLE. */
typedef struct amc_undistort_image {
    const uint8_t* src;
    uint64_t src_stride;
    int32_t channels; /* 1 or 3 */
    int32_t _pad;
    amc_undistort_cam src_camera;
    amc_undistort_cam dst_camera;
    uint8_t* dst;
} amc_undistort_image;

typedef struct amc_undistort_result {
    double device_ms;     /* first upload -> last result byte on the host (HIP events on ctx's stream) */
    double kernel_ms;     /* the resize and warp kernels alone, summed over the batches (HIP events) */
    uint32_t num_batches; /* device batches the call was split into */
    uint32_t num_resized; /* images that went through the anti-aliasing pre-pass */
} amc_undistort_result;

/* UndistortCameraOptions() (images.h:203-240) */
void amc_undistort_opts_default(amc_undistort_opts* o);

/* UndistortCamera (images.h:242-247 serves undistort_camera; COLMAP's undistortion.cc): the PINHOLE camera that sees
 * what `camera` sees, sized by the options.  A host computation: no context, no device.
 * Errors: AMC_E_INVALID (NULL, an unknown model, a zero size, options outside their ranges). */
int amc_undistort_camera(const amc_undistort_opts* opts, const amc_undistort_cam* camera, amc_undistort_cam* undistorted);

/* The model side of undistort_images (images.h:96-148 writes the undistorted sparse model): every point2D of an image
 * becomes undistorted.ImgFromCam(camera.CamFromImg(xy)).  n points, 2 doubles each; xy_out may be xy_in.  A host
 * computation.  Errors: AMC_E_INVALID (NULL, an unknown model, an undistorted camera that is not PINHOLE). */
int amc_undistort_points(const amc_undistort_cam* camera, const amc_undistort_cam* undistorted, size_t n,
                         const double* xy_in, double* xy_out);

/* WarpImageBetweenCameras for `nimages` images on ctx's device and stream (images.h:96-148), in device batches of
 * bounded bytes.  An image whose target has fewer pixels than its source is first resized to the target's size
 * (DESIGN.md 14.4).  Results do not depend on the order or the composition of the batch.  Errors: AMC_E_INVALID (NULL
 * pointers, a zero size or one above 2^31 pixels, channels other than 1 or 3, a stride below the row length, an unknown
 * source model, a target that is not PINHOLE, a parameter that is not finite), AMC_E_NOMEM, AMC_E_HIP. */
int amc_undistort_images(amc_ctx* ctx, size_t nimages, const amc_undistort_image* images, amc_undistort_result* result);

#ifdef __cplusplus
}
#endif

#endif /* AMC_UNDISTORT_H_ */
