/*
 * amc_ba.h — C ABI of libamc.so's bundle adjustment (gfx950): cameras, poses, points and observations in, the same
 * arrays refined in place by Levenberg-Marquardt with a matrix-free Schur-complement PCG as the linear step.
 *
 * Additive to amc.h (AMC_ABI_VERSION is unchanged): a host that never refines a model never calls these.  The
 * algorithm is COLMAP 3.9.1's BundleAdjuster problem (reprojection error through the eleven camera models, the
 * quaternion on Ceres' EigenQuaternionManifold, TRIVIAL / SOFT_L1 / CAUCHY loss) restated in DESIGN.md section 15 with
 * its deviations B1-B9; the results are bit-identical to tests/ba_ref.
 *
 * Reference surface (pycolmap/pipeline/sfm.h of the reference binding):
 *   BundleAdjustmentOptions{loss_function_type, loss_function_scale, refine_*, solver_options: CeresSolverOptions}
 *                                                                          amc_ba_opts + the constant masks
 *   bundle_adjustment(reconstruction, options)                             amc_bundle_adjust on the flattened model
 *   BundleAdjuster(options, config).Solve(&reconstruction)                 amc_bundle_adjust_masked on the config's part
 */
#ifndef AMC_BA_H_
#define AMC_BA_H_

#include "amc.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { AMC_BA_LOSS_TRIVIAL = 0, AMC_BA_LOSS_SOFT_L1 = 1, AMC_BA_LOSS_CAUCHY = 2 };

/* why the minimiser stopped */
enum {
    AMC_BA_FUNCTION_TOLERANCE = 0,
    AMC_BA_PARAMETER_TOLERANCE = 1,
    AMC_BA_GRADIENT_TOLERANCE = 2,
    AMC_BA_MAX_ITERATIONS = 3,
    AMC_BA_MIN_RADIUS = 4,
    AMC_BA_INVALID_STEPS = 5,   /* max_num_consecutive_invalid_steps in a row, or a cost that is not finite */
    AMC_BA_NOTHING_TO_REFINE = 6 /* no observation or no variable parameter */
};

typedef struct amc_ba_opts {
    int32_t loss_function_type;                /* default AMC_BA_LOSS_TRIVIAL */
    int32_t max_num_iterations;                /* default 100 */
    int32_t max_linear_solver_iterations;      /* default 200 */
    int32_t max_num_consecutive_invalid_steps; /* default 10 */
    double loss_function_scale;                /* default 1.0 */
    double function_tolerance;                 /* default 0 */
    double gradient_tolerance;                 /* default 0 */
    double parameter_tolerance;                /* default 0 */
} amc_ba_opts;

/* Host arrays, owned by the caller; poses, points and camera parameters are updated in place. */
typedef struct amc_ba_problem {
    size_t num_cameras;
    const int32_t* camera_models; /* num_cameras COLMAP model ids (0 .. 10) */
    double* camera_params;        /* num_cameras x 12: the model's parameters first, the rest ignored */
    const uint8_t* camera_const;  /* num_cameras x 12: non-zero = the parameter is constant */
    size_t num_images;
    const uint32_t* image_cameras; /* num_images camera indices */
    double* qvec;                 /* num_images x 4: cam_from_world rotation, Eigen order (x, y, z, w) */
    double* tvec;                 /* num_images x 3 */
    const uint8_t* pose_const;    /* num_images x 6 over the tangent (rotation 3, translation 3): non-zero = constant */
    size_t num_points;
    double* xyz;                  /* num_points x 3 */
    size_t num_observations;
    const uint32_t* obs_image;    /* num_observations image indices */
    const uint32_t* obs_point;    /* num_observations point indices */
    const double* obs_xy;         /* num_observations x 2 pixels */
} amc_ba_problem;

typedef struct amc_ba_result {
    uint64_t num_images, num_points, num_observations;
    uint64_t num_variable_parameters; /* tangent columns of the system */
    double initial_cost, final_cost;  /* 1/2 sum rho */
    uint32_t num_successful_steps, num_unsuccessful_steps; /* LM iterations */
    uint32_t num_pcg_iterations;      /* all linear solves together */
    uint32_t num_pcg_stops_residual;  /* linear solves ended by the residual rule */
    uint32_t num_pcg_stops_cap;       /* linear solves ended by max_linear_solver_iterations */
    int32_t termination;              /* AMC_BA_* above */
    double host_ms;                   /* sorting, validation, upload and download on the host clock */
    double device_ms;                 /* first upload -> last result byte on the host (HIP events on ctx's stream) */
    double kernel_ms;                 /* the kernels alone (HIP events) */
} amc_ba_result;

void amc_ba_opts_default(amc_ba_opts* o);

/* Refine the problem on ctx's device and stream.  Errors: AMC_E_INVALID (NULL arrays, an unknown model, an index out of
 * range, a value that is not finite, a point with fewer than two observations, invalid options), AMC_E_NOMEM,
 * AMC_E_HIP.  On an error the problem's arrays are unchanged. */
int amc_bundle_adjust(amc_ctx* ctx, amc_ba_problem* problem, const amc_ba_opts* options, amc_ba_result* result);

/* The same with constant points: point_const is num_points bytes, non-zero = the point is constant;
 * NULL = no constant point, which is amc_bundle_adjust.  A constant point has no column: its xyz comes back bit for bit,
 * its residuals still count in the cost and in the pose and camera blocks, it is left out of num_variable_parameters
 * and it needs one observation instead of two.  A problem without any variable parameter ends with
 * AMC_BA_NOTHING_TO_REFINE before the device is used (both costs 0). */
int amc_bundle_adjust_masked(amc_ctx* ctx, amc_ba_problem* problem, const uint8_t* point_const,
                             const amc_ba_opts* options, amc_ba_result* result);

#ifdef __cplusplus
}
#endif

#endif /* AMC_BA_H_ */
