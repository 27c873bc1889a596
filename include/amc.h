/*
 * amc.h — C ABI of libamc.so: the MI355X (gfx950) match + verify core.
 *
 * This is the drop-in boundary for pycolmap's exhaustive SIFT matching / two-view
 * verification hot path.  Plain C: `int` status codes, plain pointers and sizes, no torch or
 * C++ types.  The entry points stand in for exactly what the reference's binding layer
 * reaches through COLMAP's C++ API for this path:
 *
 *   reference call site (file:line)                              replaced by
 *   -----------------------------------------------------------  -------------------------------
 *   CreateExhaustiveFeatureMatcher / CreateSequentialFeature-    amc_ctx_create + amc_upload_*
 *     Matcher(opts, sift_opts, tvg_opts, db_path)->Start()        + amc_match_pairs (+ amc_verify_pairs)
 *     /root/reference/pycolmap/pipeline/match_features.h:45-47,    driven by the host scheduler
 *     :220, :229                                                   (pycolmap_amd/csrc/host)
 *   CreateImagePairsFeatureMatcher(...) in verify_matches        amc_verify_pairs
 *     /root/reference/pycolmap/pipeline/match_features.h:64-66
 *   SiftMatchingOptions{max_ratio,max_distance,cross_check}      amc_match_opts
 *     /root/reference/pycolmap/pipeline/match_features.h:73-98
 *   FeatureMatches <-> N x 2 uint32 row-major                    amc_match_result.matches
 *     /root/reference/pycolmap/estimators/two_view_geometry.h:19-38
 *
 * The operator-level seam inside COLMAP 3.9.1 that amc_match_pairs covers is
 * FeatureMatcher::Match(descriptors1, descriptors2, &matches) as called by
 * FeatureMatcherWorker::Run; semantics are those of
 * FindBestMatchesBruteForce and results are bit-identical to
 * oracle/match_oracle.c.
 *
 * Conventions
 *   - every function returns AMC_OK (0) or a negative AMC_E_* code; amc_last_error() returns a
 *     thread-local human-readable message for the last failure on the calling thread.
 *   - the library owns all device memory.  Host buffers passed in are caller-owned and may be
 *     freed as soon as the call returns.  Result buffers are library-allocated (pinned host
 *     memory) and released with the matching *_free.
 *   - calls are blocking unless stated otherwise; a ctx is thread-compatible (one thread at a
 *     time), different ctxs are independent.
 *   - there is NO CPU fallback: if no gfx950 device/kernel image is available the calls fail
 *     with AMC_E_HIP.
 */
#ifndef AMC_H_
#define AMC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMC_ABI_VERSION 5 /* 3: the multi-GPU exchange (amc_comm_*, amc_allgather_match_tables); 4: its verification half
                             (amc_allgather_pair_records, amc_allgather_inlier_tables); 5: amc_upload_matches and
                             amc_verify_pairs on the resident match table (matches = NULL) */
#define AMC_DESC_DIM 128 /* SIFT descriptor bytes; /root/reference/pycolmap/feature/sift.h:76-77 */

enum {
    AMC_OK = 0,
    AMC_E_INVALID = -1, /* bad argument (maps to ValueError, as THROW_CHECK does:
                           /root/reference/pycolmap/log_exceptions.h:54-76) */
    AMC_E_HIP = -2,     /* HIP runtime / kernel failure, or no device */
    AMC_E_NOMEM = -3,
    AMC_E_STATE = -4    /* e.g. slot not uploaded */
};

/* Which match kernel to run.  AUTO picks the int8-MFMA kernel (exact for any u8 values and any image size up to
 * 2^20 descriptors; beyond that, with cross_check on, the u8 dot4 kernel - see DESIGN.md "match kernels"). */
enum { AMC_KERNEL_AUTO = 0, AMC_KERNEL_MFMA = 1, AMC_KERNEL_DOT4 = 2 };

typedef struct amc_ctx amc_ctx;

/* Mirrors SiftMatchingOptions' matching fields
 * (/root/reference/pycolmap/pipeline/match_features.h:82-91).  Doubles, cast to float at the
 * comparison exactly as COLMAP does. */
typedef struct amc_match_opts {
    double max_ratio;    /* default 0.8 */
    double max_distance; /* default 0.7 */
    int32_t cross_check; /* default 1 */
    int32_t kernel;      /* AMC_KERNEL_* (default AUTO) */
} amc_match_opts;

/* CSR match table for a list of image pairs: pair p owns matches[2*offsets[p] ..
 * 2*offsets[p+1]) as (idx1, idx2) uint32 rows, ascending in idx1 — the layout of COLMAP's
 * `matches` blob and of pycolmap's N x 2 uint32 view. */
typedef struct amc_match_result {
    size_t npairs;
    uint64_t* offsets;   /* npairs + 1 */
    uint32_t* matches;   /* 2 * offsets[npairs] */
    uint64_t num_distances;   /* sum over pairs of n1*n2 (the BASELINE.json metric's unit) */
    uint64_t pairs_mfma;      /* pairs routed to the int8-MFMA kernel */
    uint64_t pairs_dot4;      /* pairs routed to the u8 dot4 kernel (guided: the dense filtered scan) */
    uint64_t pairs_guided_grid; /* guided pairs matched by candidate generation instead (match_guided.hip) */
    double device_ms;         /* first kernel launch -> last result byte on host, HIP events */
    double match_kernel_ms;   /* sum of one-way match-kernel launch durations (image 1 -> image 2
                                 scan), HIP events on the stream */
    double cross_kernel_ms;   /* candidate selection + reverse scan of candidate columns */
    uint32_t match_kernel_launches;
    uint32_t scan_run;        /* longest run of streamed images the call's forward scans kept X segments over (1: none) */
    void* _priv;
} amc_match_result;

const char* amc_last_error(void);
int amc_abi_version(void);

/* Number of visible HIP devices (>= 0), or AMC_E_HIP. */
int amc_device_count(void);

int amc_ctx_create(int device_id, amc_ctx** out);
void amc_ctx_destroy(amc_ctx* ctx);

/* Launch all of this ctx's work on `hip_stream` (a hipStream_t) instead of the ctx's own
 * stream; pass NULL to restore.  Lets a host that owns streams (e.g. torch) order/time us. */
int amc_ctx_set_stream(amc_ctx* ctx, void* hip_stream);

/* Release what the ctx keeps between calls for reuse and can re-allocate on demand: per-call device scratch (top-2
 * tables, the device-resident match table, verification workspaces), the pinned staging buffers and the pool of idle
 * result buffers (bounded on its own: three buffers, 1.5 GiB).  Uploaded images stay.  A host that runs one large job
 * per ctx (COLMAP's FeatureMatcherController::Match, /root/reference/pycolmap/pipeline/match_features.h:45-47) calls
 * this when the job is done; with gpu_index "-1" there is one ctx per device. */
int amc_ctx_trim(amc_ctx* ctx);

/* The match table of the LAST amc_match_pairs / amc_match_guided_pairs / amc_match_verify_pairs call on this ctx, where
 * the kernels left it in device memory: 2 * num_matches uint32 in the result's CSR order (amc_match_result.offsets
 * index it).  For a host that hands the table to a device-side consumer without a host round trip - the multi-GPU
 * exchange step (RCCL all-gather of the match tables, pycolmap_amd/distributed.py; the reference's multi-GPU surface is
 * SiftMatchingOptions.gpu_index, /root/reference/pycolmap/pipeline/match_features.h:76-81).  The pointer stays valid
 * until the next match call, amc_ctx_trim or amc_ctx_destroy on this ctx; NULL when the table is empty. */
int amc_ctx_resident_matches(amc_ctx* ctx, const uint32_t** dev_matches, uint64_t* num_matches);

/* Match rows from the HOST into that resident table: num_matches (idx1, idx2) uint32 rows in the CSR order of the pair
 * list they belong to - what verify_matches reads from the database's `matches` table before it verifies
 * (/root/reference/pycolmap/pipeline/match_features.h:51-68: CreateImagePairsFeatureMatcher on stored matches).  The
 * rows stay in device memory like uploaded descriptors and keypoints do, so that amc_verify_pairs(matches = NULL) -
 * once, or again with other options - reads them there instead of taking them over PCIe in every call.  Replaces
 * whatever the table held (a match call's rows); the next match call, amc_ctx_trim and amc_ctx_destroy drop it.
 * Blocking.  Errors: AMC_E_INVALID (NULL rows with num_matches > 0), AMC_E_HIP. */
int amc_upload_matches(amc_ctx* ctx, const uint32_t* matches, uint64_t num_matches);

/* ---- multi-GPU exchange -------------------------------------------------------------------
 * Image pairs shard over the GPUs of a node (one ctx per GPU: one process per GPU, or one thread per GPU of one
 * process); every rank matches its share and ONE exchange at the end gives every rank the whole match graph: an
 * all-gather of the per-rank CSR match tables over RCCL / xGMI.  The reference's surface for several GPUs is
 * SiftMatchingOptions.gpu_index (/root/reference/pycolmap/pipeline/match_features.h:76-81: COLMAP starts one matcher
 * thread per listed GPU and collects their outputs on the host); a host that binds this library calls
 * amc_allgather_match_tables where COLMAP's FeatureMatcherController joins its workers' output queues
 * (match_features.h:45-47).  INTEGRATION.md shows the binding.
 *
 * RCCL is loaded at the first amc_comm_* call (the librccl.so.1 already in the process - e.g. PyTorch's - or the
 * system's); the library has no link-time dependency on it.  Collectives run on the ctx's stream.
 *
 * amc_comm_unique_id: ncclGetUniqueId.  One rank calls it and hands the AMC_COMM_ID_BYTES to every rank by whatever
 * channel the host has (MPI, a key-value store, torch.distributed, shared memory between threads).
 * amc_comm_create: ncclCommInitRank on the ctx's device - collective: every rank calls it with the same id.
 * amc_comm_destroy: before the ctx it was created on (it owns device buffers of that ctx's device). */
#define AMC_COMM_ID_BYTES 128
typedef struct amc_comm amc_comm;
int amc_comm_unique_id(void* id);
int amc_comm_create(amc_ctx* ctx, int world_size, int rank, const void* id, amc_comm** out);
void amc_comm_destroy(amc_comm* comm);

/* The match graph of all ranks, in the global pair order: pair g owns rows offsets[g] .. offsets[g + 1]. */
typedef struct amc_gathered_tables {
    size_t npairs;                  /* pairs of all ranks */
    const uint64_t* offsets;        /* npairs + 1 (host) */
    const uint32_t* matches;        /* 2 * num_matches uint32 (pinned host), NULL unless `download` was set */
    const uint32_t* matches_device; /* the same table in this ctx's device memory: valid until the next gather on this
                                       comm or amc_comm_destroy */
    uint64_t num_matches;
    uint64_t rows_sent, rows_received;  /* match rows this rank sent to / received from other ranks (8 bytes each) */
    int32_t world_size, rank;
    /* wall clock of the phases on this rank (each ends with the stream drained): the (npairs, nmatches) sizes
     * [ncclAllGather], the per-pair (position, count) records and the match rows [grouped ncclSend / ncclRecv of
     * exactly each rank's rows, device memory to device memory], the reorder into the global CSR, the download */
    double sizes_ms, meta_ms, rows_ms, reorder_ms, download_ms, total_ms;
    void* _priv;
} amc_gathered_tables;

/* Collective: every rank of `comm` calls it once per exchange, after its match call.
 *   pair_index  global position of each of this rank's npairs_local pairs (the positions of all ranks together
 *               must be exactly 0 .. total - 1), or NULL: the ranks' lists are appended in rank order
 *   offsets     this rank's CSR (npairs_local + 1), e.g. amc_match_result.offsets
 *   matches     this rank's rows on the HOST, or NULL: the rows are taken from the ctx's device-resident match table
 *               (amc_ctx_resident_matches: where the last match call's kernels left them - no host round trip;
 *               offsets[npairs_local] must equal its row count)
 *   download    non-zero: this rank also wants the gathered rows on the host (the rank that feeds the SQLite writer)
 * Three steps, few and large: the sizes, the per-pair records (8 bytes per pair), the rows (8 bytes per match, each
 * rank sends exactly what it has to every other rank at once: xGMI is point to point, so all links carry data
 * at the same time).  Errors: AMC_E_INVALID (positions not a permutation, offsets / table disagree), AMC_E_HIP
 * (HIP or RCCL failure; amc_last_error names the call). */
int amc_allgather_match_tables(amc_ctx* ctx, amc_comm* comm, const uint64_t* pair_index, size_t npairs_local,
                               const uint64_t* offsets, const uint32_t* matches, int download,
                               amc_gathered_tables* out);
void amc_gathered_tables_free(amc_gathered_tables* t);

/* The verification half of the exchange (the payload of a sharded match + verify run is
 * [pair, count, matches, (config, F / E / H, inlier list)]; the reference's surface is the same
 * SiftMatchingOptions.gpu_index, /root/reference/pycolmap/pipeline/match_features.h:76-81 - COLMAP's verifier
 * threads hand FeatureMatcherData{matches, two_view_geometry} to ONE database writer).
 *
 * amc_allgather_pair_records: one fixed-size record per pair, all ranks, in the global pair order.
 *   records       this rank's npairs_local records of record_bytes each on the HOST (any plain struct: amc_tvg,
 *                 amc_pose, ...), or NULL: the amc_tvg records of the LAST amc_verify_pairs / amc_match_verify_pairs
 *                 call on this ctx, taken where the verification kernels left them in device memory (record_bytes must
 *                 be sizeof(amc_tvg), npairs_local that call's npairs)
 *   record_bytes  a multiple of 8, the same on every rank
 * Pairs no rank owns cannot occur: positions must be a permutation of 0 .. total - 1, as for the match tables.
 *
 * amc_allgather_inlier_tables: the inlier matches of the LAST verification call on this ctx (the rows of its input
 * matches whose inlier_mask byte is non-zero, ordered as ExtractInlierMatches orders them), compacted on the device
 * from the match table and the masks where they lie, and exchanged like the match tables: out->offsets / matches are
 * the `two_view_geometries.data` blobs of all pairs.  Same collective protocol and errors as
 * amc_allgather_match_tables; AMC_E_NOMEM when a rank cannot allocate its buffers (every rank returns it together). */
typedef struct amc_gathered_records {
    size_t npairs;               /* pairs of all ranks */
    size_t record_bytes;
    const void* records;         /* npairs * record_bytes (pinned host), NULL unless `download` was set */
    const void* records_device;  /* the same in this ctx's device memory: valid until the next record gather on this comm */
    uint64_t bytes_sent, bytes_received;
    int32_t world_size, rank;
    double total_ms;
    void* _priv;
} amc_gathered_records;
int amc_allgather_pair_records(amc_ctx* ctx, amc_comm* comm, const uint64_t* pair_index, size_t npairs_local,
                               const void* records, size_t record_bytes, int download, amc_gathered_records* out);
void amc_gathered_records_free(amc_gathered_records* r);
int amc_allgather_inlier_tables(amc_ctx* ctx, amc_comm* comm, const uint64_t* pair_index, size_t npairs_local,
                                int download, amc_gathered_tables* out);

/* Size the image-slot table. Slots are dense ids 0..num_slots-1 chosen by the caller (the host
 * layer maps COLMAP image_ids to slots). Discards previously uploaded data. */
int amc_ctx_reserve_slots(amc_ctx* ctx, uint32_t num_slots);
/* Append empty slots up to num_slots (>= the current count), keeping every uploaded image. */
int amc_ctx_grow_slots(amc_ctx* ctx, uint32_t num_slots);

/* Upload an image's descriptors: rows x 128 uint8 row-major (COLMAP FeatureDescriptors /
 * the `descriptors` blob).  rows may be 0.  The library copies. */
int amc_upload_descriptors(amc_ctx* ctx, uint32_t slot, const uint8_t* host_desc, uint32_t rows);

/* Same, but the source already lives in this device's memory (e.g. a torch uint8 tensor).
 * The library still makes its own prepared copy; the source may be freed after return. */
int amc_upload_descriptors_device(amc_ctx* ctx, uint32_t slot, const void* dev_desc,
                                  uint32_t rows);

/* Brute-force match every listed pair (slot1[p] = image 1 = match rows, slot2[p] = image 2).
 * Semantics: FindBestMatchesBruteForce.  Pairs with an empty image yield 0
 * matches.  Blocking.  `out` is filled on success and must be released with
 * amc_match_result_free. */
int amc_match_pairs(amc_ctx* ctx, const uint32_t* slot1, const uint32_t* slot2, size_t npairs,
                    const amc_match_opts* opts, amc_match_result* out);
void amc_match_result_free(amc_match_result* r);

/* Defaults identical to COLMAP's SiftMatchingOptions. */
void amc_match_opts_default(amc_match_opts* opts);

/* The host-built acosf table the thresholds use: lut[d] = acosf(min(d / 512^2, 1)),
 * d in [0, 262144].  Copies 262145 floats. (Test hook: must equal the oracle's table.) */
int amc_get_acos_lut(amc_ctx* ctx, float* out);

/* ------------------------------------------------------------------------------------------
 * Two-view geometric verification (COLMAP EstimateTwoViewGeometry)
 * ------------------------------------------------------------------------------------------ */

/* RANSACOptions (/root/reference/pycolmap/optim/bindings.h:19-25). */
typedef struct amc_ransac_opts {
    double max_error;
    double min_inlier_ratio;
    double confidence;
    double dyn_num_trials_multiplier;
    int64_t min_num_trials;
    int64_t max_num_trials; /* Every pair re-seeds std::mt19937, so all pairs read ONE table of its output words, laid out by
                             * the host for the worst case: 17 words per allowed trial (5 + 7 + 4 + 1 draws of the E / F / H /
                             * watermark RANSACs), 4 bytes each, per context - 0.3 MB at COLMAP's defaults, 0.7 GB at 1e7
                             * trials.  Trial caps that need more than 2^28 words (about 1.6e7 trials at the default
                             * min_inlier_ratio) return AMC_E_INVALID.  The table is rebuilt when the seed changes or it
                             * must grow; amc_ctx_trim releases one larger than 16 MB. */
} amc_ransac_opts;

/* TwoViewGeometryOptions (/root/reference/pycolmap/estimators/two_view_geometry.h:41-63). */
typedef struct amc_tvg_opts {
    int32_t min_num_inliers;
    int32_t detect_watermark;
    int32_t multiple_ignore_watermark;
    int32_t force_H_use;
    int32_t compute_relative_pose; /* EstimateTwoViewGeometryPose after the estimation: amc_verify_result.pose */
    int32_t multiple_models;       /* EstimateMultipleTwoViewGeometries: see amc_verify_result.inlier_mask */
    double min_E_F_inlier_ratio;
    double max_H_inlier_ratio;
    double watermark_min_inlier_ratio;
    double watermark_border_size;
    amc_ransac_opts ransac;
} amc_tvg_opts;

/* TwoViewGeometry::ConfigurationType, same values and order as
 * /root/reference/pycolmap/estimators/two_view_geometry.h:67-77. */
enum {
    AMC_TVG_UNDEFINED = 0, AMC_TVG_DEGENERATE = 1, AMC_TVG_CALIBRATED = 2, AMC_TVG_UNCALIBRATED = 3,
    AMC_TVG_PLANAR = 4, AMC_TVG_PANORAMIC = 5, AMC_TVG_PLANAR_OR_PANORAMIC = 6, AMC_TVG_WATERMARK = 7,
    AMC_TVG_MULTIPLE = 8
};

/* Camera models (ids and parameter vectors as in COLMAP 3.9.1 colmap/sensor/models.h, SURVEY.md A.1;
 * pycolmap.CameraModelId, /root/reference/pycolmap/scene/camera.h:40-49).  The calibrated path lifts
 * keypoints with Camera::CamFromImg of the image's model
 * (/root/reference/pycolmap/estimators/essential_matrix.h:33-46): all eleven are supported. */
enum {
    AMC_CAM_SIMPLE_PINHOLE = 0,        /* f, cx, cy */
    AMC_CAM_PINHOLE = 1,               /* fx, fy, cx, cy */
    AMC_CAM_SIMPLE_RADIAL = 2,         /* f, cx, cy, k */
    AMC_CAM_RADIAL = 3,                /* f, cx, cy, k1, k2 */
    AMC_CAM_OPENCV = 4,                /* fx, fy, cx, cy, k1, k2, p1, p2 */
    AMC_CAM_OPENCV_FISHEYE = 5,        /* fx, fy, cx, cy, k1, k2, k3, k4 */
    AMC_CAM_FULL_OPENCV = 6,           /* fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 */
    AMC_CAM_FOV = 7,                   /* fx, fy, cx, cy, omega */
    AMC_CAM_SIMPLE_RADIAL_FISHEYE = 8, /* f, cx, cy, k */
    AMC_CAM_RADIAL_FISHEYE = 9,        /* f, cx, cy, k1, k2 */
    AMC_CAM_THIN_PRISM_FISHEYE = 10    /* fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, sx1, sy1 */
};

/* One pair's TwoViewGeometry (/root/reference/pycolmap/estimators/two_view_geometry.h:79-93):
 * config, E/F/H row-major (the three RANSAC report models, as COLMAP stores them), the size of
 * the selected inlier set; plus diagnostics (trials of the E, F, H, watermark RANSACs and the
 * support of E, F, H). */
typedef struct amc_tvg {
    int32_t config;
    int32_t num_inliers;
    double E[9], F[9], H[9];
    int64_t num_trials[4];
    int64_t model_inliers[3];
} amc_tvg;

/* cam2_from_cam1 and tri_angle of a TwoViewGeometry (/root/reference/pycolmap/estimators/
 * two_view_geometry.h:85-92), as COLMAP 3.9.1 EstimateTwoViewGeometryPose leaves them: for CALIBRATED /
 * UNCALIBRATED the pose from E (DecomposeEssentialMatrix, cheirality of the inlier matches), for
 * PLANAR / PANORAMIC / PLANAR_OR_PANORAMIC the pose from H (DecomposeHomographyMatrix with both
 * calibration matrices), tri_angle = median triangulation angle of the points in front of both
 * cameras, and PLANAR_OR_PANORAMIC resolved to PANORAMIC (zero translation) or PLANAR.  Any other
 * config: ok = 0, identity rotation, zero translation, tri_angle 0 (the struct's defaults). */
typedef struct amc_pose {
    int32_t ok;            /* EstimateTwoViewGeometryPose's return value */
    int32_t config;        /* the geometry's config afterwards */
    double qvec[4];        /* cam2_from_cam1.rotation as (w, x, y, z): the `qvec` column of two_view_geometries */
    double tvec[3];        /* cam2_from_cam1.translation */
    double R[9];           /* the rotation matrix, row-major */
    double tri_angle;      /* radians */
    uint32_t num_points3D; /* inlier matches triangulated in front of both cameras */
    uint32_t pad_;
} amc_pose;

typedef struct amc_verify_result {
    size_t npairs;
    amc_tvg* tvg;          /* npairs */
    uint8_t* inlier_mask;  /* one byte per input match, same CSR offsets as the input: 0 = outlier,
                              g + 1 = inlier of the g-th estimated geometry (always 1 unless
                              multiple_models).  inlier_matches = the matches with a non-zero byte,
                              ordered by (byte, position): ExtractInlierMatches, and for a MULTIPLE
                              geometry the per-geometry lists one after the other */
    double device_ms;      /* first launch -> results on host */
    double kernel_ms;      /* verification kernel launches, HIP events on the stream */
    uint32_t kernel_launches;
    amc_pose* pose;        /* npairs when opts.compute_relative_pose (then tvg[p].config == pose[p].config),
                              else NULL */
    double pose_kernel_ms; /* the pose kernel's share of kernel_ms */
    /* Algorithmic work of the call, summed over its pairs and counted as COLMAP's sequential loops do it (every
     * model of every trial up to the stopping trial x all correspondences, ...), for the FP64 roofline of the
     * verification kernel (bench.py):
     *   [0] Sampson residuals  [1] homography transfer residuals  [2] translation residuals
     *   [3] 5-point minimal solves  [4] 7-point solves  [5] 4-point DLT solves
     *   [6] local 5-point solves  [7] local 8-point solves  [8] local DLT solves
     *   [9] inlier points summed over by the local solves  [10] 1-point (watermark) trials
     *   [11] FP64 flop of the residuals the kernels evaluated with the reference expression (33 / 20 / 7 per Sampson /
     *        transfer / translation residual): candidate re-scores, local-optimisation scores, inlier extraction, final
     *        masks.  [0] and [1] count the ALGORITHM's residuals; most of those are decided by the packed-FP32
     *        pre-filters of the counting loops and are not FP64 work. */
    uint64_t work[12];
    void* _priv;
} amc_verify_result;

/* C++ defaults of TwoViewGeometryOptions / its RANSACOptions member: what
 * pycolmap.TwoViewGeometryOptions() carries (py::init<>() of the C++ struct). */
void amc_tvg_opts_default(amc_tvg_opts* opts);

/* Keypoints of an image: rows x stride float32, x = [0], y = [1] (COLMAP `keypoints` blob has
 * 2, 4 or 6 columns).  Converted to double exactly as
 * FeatureKeypointsToPointsVector does. */
int amc_upload_keypoints(amc_ctx* ctx, uint32_t slot, const float* xy, uint32_t rows,
                         uint32_t stride_floats);

/* Image points in double precision, rows x 2 (x, y).  pycolmap's single-pair estimator bindings
 * take float64 N x 2 arrays (/root/reference/pycolmap/pybind11_extension.h:70-85) and COLMAP's
 * estimators work on them unchanged; this replaces the slot's float32 keypoints. */
int amc_upload_points_f64(amc_ctx* ctx, uint32_t slot, const double* xy, uint32_t rows);

/* Camera of an image (COLMAP Camera: model id, size, params, has_prior_focal_length).  num_params must be the
 * model's parameter count (Camera::VerifyParams), else AMC_E_INVALID. */
int amc_upload_camera(amc_ctx* ctx, uint32_t slot, int32_t model_id, uint64_t width,
                      uint64_t height, const double* params, int32_t num_params,
                      int32_t has_prior_focal_length);

/* Camera::CamFromImg for n image points (/root/reference/pycolmap/scene/camera.h:136-150: cam_from_img on an
 * N x 2 array): xy n x 2 pixels -> uv n x 2 normalised image-plane coordinates.  The same code that lifts an
 * image's keypoints for the calibrated path (device kernel for the pinhole and polynomial-distortion models; the
 * host libm for the fisheye family and FOV, whose distortion calls atan / tan / sin / cos). */
int amc_cam_from_img(amc_ctx* ctx, int32_t model_id, const double* params, int32_t num_params,
                     const double* xy, size_t n, double* uv);
/* Camera::ImgFromCam (/root/reference/pycolmap/scene/camera.h:166-196, "img_from_cam"): n points of the normalised image
 * plane (uv: n x 2) -> pixels (xy: n x 2), the inverse direction of amc_cam_from_img with the same split (device kernel
 * for the pinhole and polynomial-distortion models, host libm for the fisheye family and FOV). */
int amc_img_from_cam(amc_ctx* ctx, int32_t model_id, const double* params, int32_t num_params,
                     const double* uv, size_t n, double* xy);

/* EstimateTwoViewGeometry for every listed pair.  matches of pair p: uint32 (idx1, idx2) rows
 * matches[2*match_offsets[p] .. 2*match_offsets[p+1]).  The PRNG is re-seeded with `seed` at the
 * start of every pair (COLMAP's pipeline PRNG is thread_local and not reproducible across
 * pairs; pycolmap's single-pair estimators reseed with 0:
 * /root/reference/pycolmap/estimators/fundamental_matrix.h:21).  Blocking.
 * matches = NULL (with match_offsets[npairs] > 0): the rows are read from the ctx's resident match table - where the
 * last match call left them or amc_upload_matches put them; match_offsets[npairs] must equal its row count
 * (AMC_E_STATE otherwise).  Not with multiple_models (EstimateMultipleTwoViewGeometries shrinks the lists on the host:
 * AMC_E_INVALID). */
int amc_verify_pairs(amc_ctx* ctx, const uint32_t* slot1, const uint32_t* slot2, size_t npairs,
                     const uint64_t* match_offsets, const uint32_t* matches,
                     const amc_tvg_opts* opts, uint32_t seed, amc_verify_result* out);
void amc_verify_result_free(amc_verify_result* r);

/* FeatureMatcherWorker + VerifierWorker for one list of pairs (COLMAP's FeatureMatcherController::Match hands every
 * matched pair on to the verifier, /root/reference/pycolmap/pipeline/match_features.h:45-47): amc_match_pairs, then
 * amc_verify_pairs on every pair's matches - read by the verification kernel where the matcher left them in HBM,
 * without the host round trip of calling the two entry points one after the other.  Results are those of the two
 * calls: match_out as amc_match_pairs fills it; verify_out->tvg[p] / inlier_mask follow match_out->offsets (a pair
 * with fewer than min_num_inliers matches comes back DEGENERATE, as EstimateTwoViewGeometry returns it).  Both
 * images of every pair need descriptors, keypoints and a camera.  Free both results. */
int amc_match_verify_pairs(amc_ctx* ctx, const uint32_t* slot1, const uint32_t* slot2, size_t npairs,
                           const amc_match_opts* match_opts, const amc_tvg_opts* tvg_opts, uint32_t seed,
                           amc_match_result* match_out, amc_verify_result* verify_out);

/* Host-side timeline of the LAST amc_match_verify_pairs call on this ctx, milliseconds since the call was entered (what
 * the kernels' own spans in the two results do not show - VERDICT r5 asked where the milliseconds between them go):
 *   [0] verification set up (options, sample stream, image table, zeroed records)   [1] the match call returned
 *   [2] the verification slice closed (class lists, uploads) and launched            [3] verification results on the host
 *   [4] the call returned   [5] host time of the per-batch hand-over, hidden beside the scans (not a point in time)
 *   [6], [7] reserved (0).  All zero before the first such call. */
int amc_ctx_last_timeline(amc_ctx* ctx, double out_ms[8]);

/* EstimateTwoViewGeometryPose (/root/reference/pycolmap/estimators/two_view_geometry.h:153-159) on given
 * geometries: geoms[p] supplies config, E and H; inlier_matches (CSR, as amc_verify_pairs' matches)
 * are the geometry's inlier_matches.  Both images need points and a camera.
 * out: npairs records.  Also the cam2_from_cam1 of essential_matrix_estimation
 * (/root/reference/pycolmap/estimators/essential_matrix.h:63-83): config = AMC_TVG_CALIBRATED, E = the
 * report's model, inlier_matches = its inliers. */
int amc_pose_pairs(amc_ctx* ctx, const uint32_t* slot1, const uint32_t* slot2, size_t npairs,
                   const uint64_t* match_offsets, const uint32_t* inlier_matches, const amc_tvg* geoms,
                   amc_pose* out);

/* ---- guided matching (SiftMatchingOptions.guided_matching, /root/reference/pycolmap/pipeline/
 * match_features.h:95-98) ------------------------------------------------------------------------
 * COLMAP 3.9.1 FeatureMatcher::MatchGuided(max_error, keypoints1, keypoints2, descriptors1,
 * descriptors2, TwoViewGeometry*): after a successful verification the pair is matched again with
 * a float32 geometric filter on the distance matrix - squared Sampson error under F for
 * CALIBRATED / UNCALIBRATED, forward transfer error under H for PLANAR / PANORAMIC /
 * PLANAR_OR_PANORAMIC, rejected pairings score 0 - and the result replaces the geometry's
 * inlier_matches.  geoms[p] supplies config, F and H of pair p (any other configuration is
 * AMC_E_INVALID: COLMAP leaves those pairs alone); max_error is
 * TwoViewGeometryOptions.ransac_options.max_error.  Both images need their float32 keypoints
 * (amc_upload_keypoints), one per descriptor.  Same result layout as amc_match_pairs. */
int amc_match_guided_pairs(amc_ctx* ctx, const uint32_t* slot1, const uint32_t* slot2, size_t npairs,
                           const amc_tvg* geoms, double max_error, const amc_match_opts* opts,
                           amc_match_result* out);

/* ---- single LO-RANSAC per pair: the pycolmap estimator bindings ---------------------------------
 * AMC_RANSAC_F  LORANSAC<FundamentalMatrixSevenPointEstimator, FundamentalMatrixEightPointEstimator>
 *               (/root/reference/pycolmap/estimators/fundamental_matrix.h:17-39)
 * AMC_RANSAC_H  LORANSAC<HomographyMatrixEstimator, HomographyMatrixEstimator>
 *               (/root/reference/pycolmap/estimators/homography_matrix.h:16-37)
 * AMC_RANSAC_E  LORANSAC<EssentialMatrixFivePointEstimator, ...> on CamFromImg-normalised points
 *               with max_error = 0.5 * (e / f1 + e / f2)
 *               (/root/reference/pycolmap/estimators/essential_matrix.h:19-52); needs both cameras.
 * The correspondences of pair p are rows match_offsets[p] .. match_offsets[p+1] of `matches`
 * (indices into the two slots' points).  The PRNG is seeded with `seed` per pair (the bindings
 * call SetPRNGSeed(0)). */
enum { AMC_RANSAC_F = 0, AMC_RANSAC_H = 1, AMC_RANSAC_E = 2 };
typedef struct amc_ransac_report {
    int32_t success;      /* report.success */
    int32_t num_inliers;  /* report.support.num_inliers */
    int64_t num_trials;   /* report.num_trials */
    double model[9];      /* report.model, row-major */
} amc_ransac_report;
typedef struct amc_ransac_result {
    size_t npairs;
    amc_ransac_report* reports; /* npairs */
    uint8_t* inlier_mask;       /* one byte per input correspondence (report.inlier_mask; zeros on failure) */
    double device_ms;
    void* _priv;
} amc_ransac_result;
int amc_ransac_pairs(amc_ctx* ctx, int kind, const uint32_t* slot1, const uint32_t* slot2, size_t npairs,
                     const uint64_t* match_offsets, const uint32_t* matches,
                     const amc_ransac_opts* opts, uint32_t seed, amc_ransac_result* out);
void amc_ransac_result_free(amc_ransac_result* r);

/* ComputeSquaredSampsonError (/root/reference/pycolmap/estimators/two_view_geometry.h:161-175):
 * out[i] = (x2^T E x1)^2 / ((E x1)_0^2 + (E x1)_1^2 + (E^T x2)_0^2 + (E^T x2)_1^2), points n x 2. */
int amc_squared_sampson_error(amc_ctx* ctx, const double* points1, const double* points2, size_t n,
                              const double E[9], double* out);

/* PoseFromHomographyMatrix (/root/reference/pycolmap/geometry/homography_matrix.h:13-31, "homography_decomposition"):
 * the analytical decomposition of H (pixels; K1, K2 the calibration matrices, all 3 x 3 row-major) into its one
 * (pure rotation) or four (R, t, n) candidates, and of those the one that puts the most of the n correspondences
 * (points1 / points2: n x 2, camera coordinates) in front of both cameras - later candidates win ties.
 * points3D: room for n x 3; the winner's triangulated points in input order, *num_points3D of them. */
int amc_homography_decomposition(amc_ctx* ctx, const double H[9], const double K1[9], const double K2[9],
                                 const double* points1, const double* points2, size_t n, double R[9], double t[3],
                                 double normal[3], double* points3D, uint64_t* num_points3D);

#ifdef __cplusplus
}
#endif
#endif /* AMC_H_ */
