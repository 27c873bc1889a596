"""`import pycolmap` for code written against the reference package: every name of the match + verify path
(/root/reference/pycolmap/main.cc:91-118 registers them on the `pycolmap` module) and of SIFT feature extraction
(`extract_features`, `Sift`, `SiftExtractionOptions`, `Normalization`, `ImageReaderOptions`, `CameraMode`) and of
known-pose triangulation (`estimate_triangulation`, `PointData`, `EstimateTriangulationOptions`) and of absolute pose
(`absolute_pose_estimation`, `pose_refinement`, `AbsolutePoseEstimationOptions`, `AbsolutePoseRefinementOptions`,
`rig_absolute_pose_estimation`) and of image undistortion (`undistort_images`, `UndistortCameraOptions`, `CopyType`, with
the building blocks `undistort_camera` and `undistort_image`) and of bundle adjustment (`bundle_adjustment`,
`BundleAdjustmentOptions`, `CeresSolverOptions`, `LossFunctionType`, with the minimal `Reconstruction` and its `Point3D`,
`Track`, `TrackElement`, `Point2D`; `BundleAdjustmentConfig` and `BundleAdjuster` with `solve` for a part of the
model) and of incremental triangulation (`CorrespondenceGraph`, `Correspondence`,
`IncrementalTriangulator` with `triangulate_image`, `IncrementalTriangulatorOptions`)
resolves to pycolmap_amd's MI355X implementation.  Only what SURVEY.md section 8 and DESIGN.md sections 10 to 17 put in
scope exists;
anything else raises AttributeError naming this package, so that a script reaching for `import_images`, SfM or MVS
fails at the attribute, not later.  Track completion and merging (`complete_tracks`,
`complete_all_tracks`, `merge_tracks`, `merge_all_tracks`: module-level functions that take the `IncrementalTriangulator`
first) resolve too, and so does `retriangulate(triangulator, options)` for under-reconstructed image
pairs.  The three steps of the mapper in front of them resolve as well: `IncrementalMapper(triangulator)`
with `find_next_images`, `register_next_image` and `find_local_bundle`, `IncrementalMapperOptions` and
`ImageSelectionMethod`.  A model starts from verified matches alone with
`register_initial_image_pair(mapper, options, image_id1, image_id2)`, `adjust_global_bundle(mapper, options, ba_options)` and
`filter_images(mapper, options)`: module-level functions that take the `IncrementalMapper` first;
`find_initial_image_pair`, `adjust_local_bundle` and the drivers stay undefined.  The dense side reads the workspace of
`undistort_images` again: `PatchMatchController(options, workspace_path).run()` with `PatchMatchOptions` writes COLMAP's
photometric and geometric depth and normal maps, and `read_array` / `write_array` are this
package's helpers for COLMAP's array files; the function `patch_match_stereo` stays undefined, and so does
`stereo_fusion`.  The maps end in a point cloud: `StereoFusion(options, workspace_path).run()` with `FusionOptions` (the
thirteen fields of the reference's `StereoFusionOptions`) fuses them on the GPU into `fused_points` and
`fused_points_visibility`, and `write(output_path)` leaves what the reference's `stereo_fusion` leaves
(DESIGN.md section 23); the names `stereo_fusion` and `StereoFusionOptions` themselves stay undefined.  An adjustment's
uncertainty resolves as well: `estimate_ba_covariance(options, reconstruction, bundle_adjuster)` with
`BACovarianceOptions` and `BACovarianceOptionsParams` returns a `BACovariance` (or None) whose accessors give the pose,
camera, point, cross and relative-pose blocks by id.  A pose is refined together with its camera
by `refine_absolute_pose(cam_from_world, points2D, points3D, inlier_mask, camera, refinement_options)` and
`estimate_and_refine_absolute_pose(points2D, points3D, camera, estimation_options, refinement_options)`, which honour
`refine_focal_length` and `refine_extra_params` and update the camera in place, and a mapper registers an image that way
with `register_next_image_and_refine(mapper, options, image_id)`; `pose_refinement` and
`absolute_pose_estimation` keep refusing the two flags."""
import pycolmap_amd as _impl
from pycolmap_amd import *  # noqa: F401,F403
from pycolmap_amd import __version__  # noqa: F401

_PUBLIC = [n for n in dir(_impl) if not n.startswith("_")]
globals().update({n: getattr(_impl, n) for n in _PUBLIC})


def __getattr__(name):
    raise AttributeError(f"pycolmap.{name} is outside pycolmap_amd's scope (SIFT feature extraction, exhaustive / sequential "
                         f"matching + two-view verification, known-pose triangulation, absolute pose, image undistortion, bundle adjustment of a minimal Reconstruction behind the pycolmap API); available: {', '.join(sorted(_PUBLIC))}; also in scope: point filtering, and incremental triangulation of an image (CorrespondenceGraph, IncrementalTriangulator.triangulate_image), and the adjustment of a part of the model (BundleAdjustmentConfig, BundleAdjuster.solve), and track completion and merging (complete_tracks, complete_all_tracks, merge_tracks, merge_all_tracks with the triangulator as first argument), and retriangulation of under-reconstructed image pairs (retriangulate with the triangulator as first argument), and the mapper's image ranking, registration and local bundle (IncrementalMapper.find_next_images, register_next_image, find_local_bundle with IncrementalMapperOptions and ImageSelectionMethod), and the start of a model (register_initial_image_pair, adjust_global_bundle, filter_images with the mapper as first argument), and PatchMatch stereo on a dense workspace (PatchMatchController(options, workspace_path).run() with PatchMatchOptions, and read_array, write_array for its files; patch_match_stereo and stereo_fusion stay undefined), and stereo fusion of those maps (StereoFusion(options, workspace_path).run() and write(output_path) with FusionOptions, DESIGN.md section 23; the names stereo_fusion and StereoFusionOptions stay undefined), and the covariance of an adjustment (estimate_ba_covariance(options, reconstruction, bundle_adjuster) with BACovarianceOptions and BACovarianceOptionsParams, returning a BACovariance; DESIGN.md section 24), and the refinement of a pose together with its camera's focal length and distortion (refine_absolute_pose, estimate_and_refine_absolute_pose, and register_next_image_and_refine with the mapper as first argument; DESIGN.md section 25)")
