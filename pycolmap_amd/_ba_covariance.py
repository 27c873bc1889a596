"""Covariance of a bundle adjustment: BACovarianceOptions, estimate_ba_covariance and BACovariance, the names later
pycolmap releases bind for COLMAP 3.10's EstimateBACovariance (the reference binding in the tree, pycolmap 0.6, has none
of them; the spellings are COLMAP 3.10's as recollected).

The adjuster's own options and config flatten the model (BundleAdjuster._problem, FlattenForBundleAdjuster), so the gauge,
the refine_* flags and the constant points are those of the solve that produced the model; the flat problem goes through
Context.ba_covariance (libamc.so, csrc/bacov.hip) at the parameters the model holds.  Nothing is refined and the
reconstruction is never changed.  The propagation to a relative pose is host code here."""
from __future__ import annotations

import enum
import time

import numpy as np

from . import _capi, _pycolmap

FLAT_KEYS = ("camera_models", "camera_params", "camera_const", "image_cameras", "qvec", "tvec", "pose_const", "xyz",
             "obs_image", "obs_point", "obs_xy")


class BACovarianceOptionsParams(enum.IntEnum):
    """Which blocks the result serves.  The system is the same for all four: every variable column is in it."""
    POSES = 0
    POINTS = 1
    POSES_AND_POINTS = 2
    ALL = 3


_FIELDS = [  # name, default, doc
    ("params", BACovarianceOptionsParams.ALL, "For which parameters to serve the covariance."),
    ("damping", 1e-8, "Damping factor for the Hessian in the Schur complement solver. Enables to robustly deal with "
                      "poorly conditioned points."),
]
FIELD_NAMES = [f[0] for f in _FIELDS]


def _coerce(name, value):
    if name == "params":
        if isinstance(value, str):
            if value.upper() not in BACovarianceOptionsParams.__members__:
                raise ValueError(f"BACovarianceOptions.params: unknown value '{value}'")
            return BACovarianceOptionsParams[value.upper()]
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer, BACovarianceOptionsParams)):
            raise TypeError(f"BACovarianceOptions.params: a BACovarianceOptionsParams is needed, not {type(value).__name__}")
        return BACovarianceOptionsParams(int(value))
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise TypeError(f"BACovarianceOptions.damping: a float is needed, not {type(value).__name__}")
    return float(value)


class BACovarianceOptions:
    """COLMAP 3.10's BACovarianceOptions without experimental_custom_poses (N5), following the option protocol of this
    package: construction from a dict or keywords, mergedict, todict, summary, copy and pickle."""

    def __init__(self, *args, **kwargs):
        self._values = {name: default for name, default, _ in _FIELDS}
        if len(args) > 1 or (args and kwargs):
            raise TypeError("BACovarianceOptions(): at most one dict, or keywords")
        if args:
            if isinstance(args[0], BACovarianceOptions):
                self._values.update(args[0]._values)
            elif isinstance(args[0], dict):
                self.mergedict(args[0])
            else:
                raise TypeError(f"BACovarianceOptions(): a dict is needed, not {type(args[0]).__name__}")
        self.mergedict(kwargs)

    params = property(lambda self: self._values["params"], lambda self, v: self._values.__setitem__("params", _coerce("params", v)),
                      doc=_FIELDS[0][2] + " (BACovarianceOptionsParams, default: ALL)")
    damping = property(lambda self: self._values["damping"], lambda self, v: self._values.__setitem__("damping", _coerce("damping", v)),
                       doc=_FIELDS[1][2] + " (float, default: 1e-08)")

    def mergedict(self, d) -> None:
        for key, value in dict(d).items():
            if key not in self._values:
                raise ValueError(f"BACovarianceOptions: unknown option '{key}' (valid: {', '.join(FIELD_NAMES)})")
            setattr(self, key, value)

    def todict(self, recursive: bool = True) -> dict:
        return {name: self._values[name] for name in FIELD_NAMES}

    def summary(self, write_type: bool = False) -> str:
        lines = ["BACovarianceOptions:"]
        for name in FIELD_NAMES:
            v = self._values[name]
            shown = v.name if isinstance(v, enum.Enum) else v
            lines.append(f"    {name}{': ' + type(v).__name__ if write_type else ''} = {shown}")
        return "\n".join(lines)

    __repr__ = summary

    def __eq__(self, other):
        return isinstance(other, BACovarianceOptions) and self._values == other._values

    __hash__ = None

    def __copy__(self):
        return BACovarianceOptions(self)

    def __deepcopy__(self, memo):
        return BACovarianceOptions(self)

    def __getstate__(self):
        return {"params": int(self._values["params"]), "damping": self._values["damping"]}

    def __setstate__(self, state):
        self._values = {name: default for name, default, _ in _FIELDS}
        self.mergedict(state)

    def check(self) -> None:
        if not (self.damping >= 0.0 and np.isfinite(self.damping)):
            raise ValueError("BACovarianceOptions: damping >= 0 and finite")


def _rotation(q):
    """the rotation matrix of q = (x, y, z, w), normalised first"""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def relative_pose_jacobian(q1, t1, q2, t2):
    """d(cam2_from_cam1) / d(cam1_from_world, cam2_from_world), 6 x 12, every pose in the tangent of DESIGN.md 12.7's Plus
    (rotation first; Plus(q, d) = exp(d) q rotates by 2 |d| on the left), columns (d1, tau1, d2, tau2):
        R21 = R2 R1^T, t21 = t2 - R21 t1, u = R21 t1
        d21   = d2 - R21 d1
        tau21 = tau2 - R21 tau1 + 2 [u]x (d2 - R21 d1)"""
    R21 = _rotation(q2) @ _rotation(q1).T
    ux = _skew(R21 @ np.asarray(t1, np.float64))
    J = np.zeros((6, 12))
    J[:3, 0:3] = -R21
    J[:3, 6:9] = np.eye(3)
    J[3:, 0:3] = -2.0 * ux @ R21
    J[3:, 3:6] = -R21
    J[3:, 6:9] = 2.0 * ux
    J[3:, 9:12] = np.eye(3)
    return J


class BACovariance:
    """What estimate_ba_covariance returns: the blocks of the covariance by id.  An id that had no column gives None."""

    def __init__(self, result, flat, params, image_ids, camera_ids, point_ids):
        self._params = BACovarianceOptionsParams(params)
        poses = self._params != BACovarianceOptionsParams.POINTS
        points = self._params != BACovarianceOptionsParams.POSES
        cameras = self._params == BACovarianceOptionsParams.ALL
        m = int(result["num_columns"])
        owner, coord = np.asarray(result["column_owner"]), np.asarray(result["column_coord"])
        matrix = result["matrix"]
        # the flat problem names its images, cameras and points by their place in the model's maps
        image_at = [image_ids[int(v)] for v in np.asarray(flat["image_at"]).reshape(-1)]
        camera_at = [camera_ids[int(v)] for v in np.asarray(flat["camera_at"]).reshape(-1)]
        point_at = [point_ids[int(v)] for v in np.asarray(flat["point_at"]).reshape(-1)]
        nimg = len(image_at)
        self._matrix = matrix
        self._image_cols, self._camera_cols, self._poses = {}, {}, {}
        for k in range(m):
            if owner[k] < nimg:
                if poses:
                    self._image_cols.setdefault(image_at[owner[k]], []).append((k, int(coord[k])))
            elif cameras:
                self._camera_cols.setdefault(camera_at[owner[k] - nimg], []).append((k, int(coord[k])))
        q, t = np.asarray(flat["qvec"]).reshape(-1, 4), np.asarray(flat["tvec"]).reshape(-1, 3)
        for i, iid in enumerate(image_at):
            if iid in self._image_cols:
                self._poses[iid] = (q[i].copy(), t[i].copy())
        self._points = {}
        if points and result["point_present"] is not None:
            present, blocks = np.asarray(result["point_present"]), np.asarray(result["point_cov"])
            for j in np.flatnonzero(present):
                self._points[point_at[j]] = blocks[j].copy()
        self.summary = {"call": "estimate_ba_covariance", "params": self._params.name, "num_columns": m,
                        "num_pose_blocks": len(self._image_cols), "num_camera_blocks": len(self._camera_cols),
                        "num_point_blocks": len(self._points), "min_pivot_ratio": float(result["min_pivot_ratio"])}
        for k in ("host_ms", "device_ms", "kernel_ms", "copy_ms"):
            self.summary[k] = float(result.get(k, 0.0))
        self.summary["phase_ms"] = dict(result.get("phase_ms", {}))

    def _pose_block(self, id1, id2):
        out = np.zeros((6, 6))
        for r, a in self._image_cols[id1]:
            for c, b in self._image_cols[id2]:
                out[a, b] = self._matrix[r, c]
        return out

    def get_cam_from_world_cov(self, image_id):
        """6 x 6 over the pose's tangent, rotation first; a constant coordinate's row and column are zero."""
        return self._pose_block(image_id, image_id) if image_id in self._image_cols else None

    def get_cam_cross_cov(self, image_id1, image_id2):
        """The 6 x 6 block between two poses (rows image_id1, columns image_id2)."""
        if image_id1 not in self._image_cols or image_id2 not in self._image_cols:
            return None
        return self._pose_block(image_id1, image_id2)

    def get_cam2_from_cam1_cov(self, image_id1, image_id2):
        """The covariance of cam2_from_world * cam1_from_world.inverse() in the same tangent on the relative pose, by
        first-order propagation of the joint 12 x 12 through relative_pose_jacobian."""
        if image_id1 not in self._image_cols or image_id2 not in self._image_cols:
            return None
        joint = np.block([[self._pose_block(image_id1, image_id1), self._pose_block(image_id1, image_id2)],
                          [self._pose_block(image_id2, image_id1), self._pose_block(image_id2, image_id2)]])
        J = relative_pose_jacobian(*self._poses[image_id1], *self._poses[image_id2])
        return J @ joint @ J.T

    def variable_camera_param_idxs(self, camera_id):
        """The parameter slots of the camera that had a column, ascending."""
        return [c for _, c in self._camera_cols[camera_id]] if camera_id in self._camera_cols else None

    def get_camera_cov(self, camera_id):
        """k x k over variable_camera_param_idxs(camera_id)."""
        if camera_id not in self._camera_cols:
            return None
        cols = [k for k, _ in self._camera_cols[camera_id]]
        return self._matrix[np.ix_(cols, cols)].copy()

    def get_point_cov(self, point3D_id):
        block = self._points.get(point3D_id)
        return None if block is None else block.copy()

    def last_run_stats(self) -> dict:
        return dict(self.summary)


def _estimate(options, reconstruction, bundle_adjuster, solver):
    if not isinstance(options, BACovarianceOptions):
        options = BACovarianceOptions(options)
    options.check()
    t0 = time.perf_counter()
    flat = bundle_adjuster._problem(reconstruction)
    args = [np.asarray(flat[k]) for k in FLAT_KEYS]
    for k in (0, 3, 8, 9):
        args[k] = args[k].reshape(-1)
    if args[8].size == 0:
        _pycolmap.logging.warning("estimate_ba_covariance: the bundle adjuster's config gives no residual")
        return None
    ba = bundle_adjuster.options
    params = options.params
    opts = dict(loss_function_type=int(ba.loss_function_type), loss_function_scale=float(ba.loss_function_scale),
                damping=options.damping, want_points=int(params != BACovarianceOptionsParams.POSES),
                want_matrix=1)
    mask = np.asarray(flat["point_const"]).reshape(-1)
    if solver is None:
        with _capi.Context(0) as ctx:
            result = ctx.ba_covariance(*args, options=opts, point_const=mask)
    else:
        result = solver(dict(flat, options=opts))
    if not result["success"]:
        _pycolmap.logging.warning(
            f"estimate_ba_covariance: the Schur complement is rank deficient (the pivot of column "
            f"{result['failed_column']} of {result['num_columns']} is not positive); check the gauge of the config")
        return None
    cov = BACovariance(result, flat, params, list(reconstruction.images), list(reconstruction.cameras),
                       list(reconstruction.points3D))
    cov.summary["total_ms"] = (time.perf_counter() - t0) * 1e3
    _pycolmap._last_stats = dict(cov.summary)
    return cov


def estimate_ba_covariance(options, reconstruction, bundle_adjuster):
    """The covariance of the model's variable poses, camera parameters and points under the adjuster's options and
    config, on the GPU.  Returns a BACovariance, or None (with a warning through
    pycolmap.logging) when the factorisation fails.  The reconstruction is not changed.  Without a GPU it raises."""
    return _estimate(options, reconstruction, bundle_adjuster, None)


def _estimate_ba_covariance_with(options, reconstruction, bundle_adjuster, solver):
    """estimate_ba_covariance with a callable in the library's place (test hook, as BundleAdjuster._solve_with): it takes
    the flat problem as a dict of arrays with `options` and `point_const` and returns Context.ba_covariance's dict."""
    return _estimate(options, reconstruction, bundle_adjuster, solver)
