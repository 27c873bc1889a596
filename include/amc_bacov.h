/*
 * amc_bacov.h — C ABI of libamc.so's bundle-adjustment covariance (gfx950): the flat problem of amc_ba.h in, the
 * covariance of its variable poses, camera parameters and points out, at the parameters given.  Nothing is refined
 * and the problem's arrays are never written.
 *
 * Additive to amc.h (AMC_ABI_VERSION is unchanged).  The definition is DESIGN.md section 24: the Schur complement of
 * the point blocks formed as a dense matrix over the variable columns, factored by Cholesky, inverted through the
 * triangular inverse, the point blocks propagated from it; deviations N1-N5 from COLMAP's EstimateBACovariance.  The
 * results are bit-identical to tests/bacov_ref.
 *
 * Reference surface (later pycolmap releases; the reference binding in the tree has none of it):
 *   BACovarianceOptions{params, damping}                       amc_bacov_opts + the constant masks of the problem
 *   estimate_ba_covariance(options, reconstruction, adjuster)  amc_ba_covariance on the adjuster's flattened problem
 */
#ifndef AMC_BACOV_H_
#define AMC_BACOV_H_

#include "amc_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMC_BACOV_MAX_COLUMNS 8192 /* three m x m doubles on the device, one on the host */

enum { AMC_BACOV_PHASES = 5 }; /* evaluation, formation, factor, inverse, points */

typedef struct amc_bacov_opts {
    int32_t loss_function_type; /* AMC_BA_LOSS_*, default TRIVIAL */
    int32_t want_points;        /* non-zero: the 3 x 3 block of every variable point; default 1 */
    int32_t want_matrix;        /* non-zero: the m x m matrix on the host; default 1 */
    int32_t reserved;           /* 0 */
    double loss_function_scale; /* default 1.0 */
    double damping;             /* added to the diagonal of every point block; default 1e-8 */
} amc_bacov_opts;

typedef struct amc_bacov_result {
    int32_t success;         /* 0: a pivot of the factorisation was not finite or not positive (no matrix, no blocks) */
    int32_t reserved;
    int64_t failed_column;   /* that pivot's column, or -1 */
    uint64_t num_columns;    /* m: the variable pose coordinates image by image, then the variable camera slots */
    uint64_t num_points;
    double min_pivot_ratio;  /* the smallest pivot / diagonal entry over the columns factored; 1 when m == 0 */
    uint32_t* column_owner;  /* m: an image index, or num_images + a camera index */
    uint32_t* column_coord;  /* m: the tangent coordinate 0 .. 5 (rotation first) or the parameter slot 0 .. 11 */
    double* matrix;          /* m x m row-major, both triangles; NULL without want_matrix or without success */
    uint8_t* point_present;  /* num_points: 1 = the point is variable and point_cov holds its block; NULL as above */
    double* point_cov;       /* num_points x 9 row-major; zeros where point_present is 0 */
    double host_ms;          /* validation, plans, upload and download on the host clock */
    double device_ms;        /* first upload -> last result byte on the host (HIP events on ctx's stream) */
    double kernel_ms;        /* the kernels alone: the sum of phase_ms */
    double copy_ms;          /* device_ms - kernel_ms */
    double phase_ms[AMC_BACOV_PHASES];
} amc_bacov_result;

void amc_bacov_opts_default(amc_bacov_opts* o);

/* The covariance of the problem's variable columns on ctx's device and stream.  point_const as
 * amc_bundle_adjust_masked's (NULL = no constant point).  Errors: AMC_E_INVALID (what amc_bundle_adjust_masked
 * refuses, invalid options, more than AMC_BACOV_MAX_COLUMNS columns: all before the device is used), AMC_E_NOMEM,
 * AMC_E_HIP.  A failed factorisation is not an error: AMC_OK with success == 0.  m == 0 succeeds without device use. */
int amc_ba_covariance(amc_ctx* ctx, const amc_ba_problem* problem, const uint8_t* point_const,
                      const amc_bacov_opts* options, amc_bacov_result* result);

void amc_bacov_result_free(amc_bacov_result* r);

#ifdef __cplusplus
}
#endif

#endif /* AMC_BACOV_H_ */
