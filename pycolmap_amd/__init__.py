"""pycolmap_amd — MI355X-native exhaustive/sequential SIFT matching + two-view verification behind
the pycolmap API.

    import pycolmap_amd as pycolmap
    pycolmap.match_exhaustive(database_path)        # same signature as the reference
    pycolmap.verify_matches(database_path, pairs_path)
    pycolmap.fundamental_matrix_estimation(points2D1, points2D2)   # ... and the other estimator bindings

The compiled host layer (`_pycolmap`, C++/pybind11) drives `libamc.so` (HIP kernels behind a C ABI,
include/amc.h).  There is no CPU fallback: importing works anywhere, computing needs a gfx950 GPU.
"""
from __future__ import annotations

__version__ = "0.1.0"

try:  # the compiled host layer; absent only before `python -m pycolmap_amd.build`
    from ._pycolmap import (  # noqa: F401
        AbsolutePoseEstimationOptions, AbsolutePoseRefinementOptions, BundleAdjuster, BundleAdjustmentConfig, BundleAdjustmentOptions, Correspondence, CorrespondenceGraph, ImageSelectionMethod, IncrementalMapper, IncrementalMapperOptions, IncrementalTriangulator, IncrementalTriangulatorOptions, CeresSolverOptions, LossFunctionType, Point2D, Point3D, Reconstruction, Track, TrackElement, adjust_global_bundle, bundle_adjustment, complete_all_tracks, complete_tracks, COLMAP_build, COLMAP_version, Camera, CopyType, UndistortCameraOptions, undistort_camera, undistort_image, CameraMode, CameraModelId, Database, DatabaseTransaction, Device, EstimateTriangulationOptions, ExhaustiveMatchingOptions, Image, ImageReaderOptions, Normalization, PointData, RANSACOptions, Rigid3d,
        Rotation3d, Sift, SiftExtractionOptions,
        SequentialMatchingOptions, SiftMatchingOptions, SpatialMatchingOptions, TwoViewGeometry, TwoViewGeometryConfiguration,
        VocabTreeMatchingOptions,
        TwoViewGeometryOptions, absolute_pose_estimation, essential_matrix_estimation, estimate_calibrated_two_view_geometry,
        estimate_triangulation, estimate_two_view_geometry, estimate_two_view_geometry_pose, filter_images, fundamental_matrix_estimation, has_cuda,
        has_hip, homography_decomposition, homography_matrix_estimation, last_run_stats, logging, match_exhaustive, merge_all_tracks, merge_tracks, match_sequential,
        match_spatial, match_vocabtree, pose_refinement, register_initial_image_pair, retriangulate, rig_absolute_pose_estimation, squared_sampson_error, verify_matches,
    )
    from ._extraction import extract_features  # noqa: F401
    from ._undistortion import _undistort_plan, undistort_images  # noqa: F401
    from ._patch_match import PatchMatchController, PatchMatchOptions, read_array, write_array  # noqa: F401
    from ._fusion import FusionOptions, StereoFusion  # noqa: F401
    from ._ba_covariance import (  # noqa: F401
        BACovariance, BACovarianceOptions, BACovarianceOptionsParams, estimate_ba_covariance)
    from ._pose_intrinsics import (  # noqa: F401
        estimate_and_refine_absolute_pose, refine_absolute_pose, register_next_image_and_refine)
    _HOST_LAYER_ERROR = None
except ImportError as _e:  # pragma: no cover - exercised only on an unbuilt tree
    _HOST_LAYER_ERROR = _e

    def __getattr__(name):
        # submodules (`from pycolmap_amd import build`, `_capi`, `synth`, ...) must stay importable on an unbuilt tree:
        # the import machinery asks the package for the attribute first and imports the submodule on AttributeError
        import importlib.util
        if name.startswith("__") or importlib.util.find_spec(f"{__name__}.{name}") is not None:
            raise AttributeError(name)
        raise ImportError(
            f"pycolmap_amd.{name}: the compiled host layer is missing ({_HOST_LAYER_ERROR}); run "
            "`python -m pycolmap_amd.build` (needs hipcc + g++). pycolmap_amd has no Python/CPU fallback.")
