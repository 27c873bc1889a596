"""Stereo fusion over COLMAP's dense workspace: FusionOptions and StereoFusion, with the reference's option fields
(pycolmap/pipeline/mvs.h:193-243 of the reference) and COLMAP 3.9.1's defaults.

The workspace that undistort_images wrote and PatchMatchController filled (images/, sparse/, stereo/fusion.cfg,
stereo/depth_maps/ and stereo/normal_maps/) is read back, every image gets its neighbours (the images that share the most
points3D, _patch_match.auto_candidates), the maps are fused on the device through Context.fuse_depth_maps (libamc.so,
csrc/fusion.hip), and `write` leaves the points as a sparse model or as COLMAP's PLY and visibility files.  DESIGN.md
section 23 lists the rules and their deviations from COLMAP."""
from __future__ import annotations

import copy
import os
import struct
import time
from pathlib import Path

import numpy as np

from . import _capi, _pycolmap
from ._patch_match import auto_candidates, read_array
from ._undistortion import _check_message, read_image

FLOAT32_MAX = _capi.FLOAT32_MAX
POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                        ("r", "u1"), ("g", "u1"), ("b", "u1")])
INPUT_TYPES = ("photometric", "geometric")

_FIELDS = [  # name, COLMAP 3.9.1's default, the reference's docstring
    ("mask_path", "", "Path for PNG masks. Same format expected as ImageReaderOptions."),
    ("num_threads", -1, "The number of threads to use during fusion."),
    ("max_image_size", -1, "Maximum image size in either dimension."),
    ("min_num_pixels", 5, "Minimum number of fused pixels to produce a point."),
    ("max_num_pixels", 10000, "Maximum number of pixels to fuse into a single point."),
    ("max_traversal_depth", 100, "Maximum depth in consistency graph traversal."),
    ("max_reproj_error", 2.0, "Maximum relative difference between measured and projected pixel."),
    ("max_depth_error", 0.01, "Maximum relative difference between measured and projected depth."),
    ("max_normal_error", 10.0, "Maximum angular difference in degrees of normals of pixels to be fused."),
    ("check_num_images", 50, "Number of overlapping images to transitively check for fusing points."),
    ("use_cache", False, "Flag indicating whether to use LRU cache or pre-load all data"),
    ("cache_size", 32.0, "Cache size in gigabytes for fusion."),
    ("bounding_box", ((-FLOAT32_MAX,) * 3, (FLOAT32_MAX,) * 3), "Bounding box Tuple[min, max]"),
]
FIELD_NAMES = [f[0] for f in _FIELDS]


def _box(value):
    try:
        a = np.array(value, dtype=np.float64)
    except (TypeError, ValueError):
        a = None
    if a is None or a.shape != (2, 3):
        raise TypeError("FusionOptions.bounding_box: a pair of 3-vectors (min, max) is needed")
    return tuple(float(x) for x in a[0]), tuple(float(x) for x in a[1])


def _option_property(name, kind, doc, default):
    def get(self):
        return self._values[name]

    def set_(self, value):
        if kind is tuple:
            value = _box(value)
        elif kind is bool:
            if not isinstance(value, (bool, np.bool_)):
                raise TypeError(f"FusionOptions.{name}: a bool is needed, not {type(value).__name__}")
            value = bool(value)
        elif kind is int:
            if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
                raise TypeError(f"FusionOptions.{name}: an int is needed, not {type(value).__name__}")
            value = int(value)
        elif kind is float:
            if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
                raise TypeError(f"FusionOptions.{name}: a float is needed, not {type(value).__name__}")
            value = float(value)
        elif not isinstance(value, (str, os.PathLike)):
            raise TypeError(f"FusionOptions.{name}: a str is needed, not {type(value).__name__}")
        else:
            value = os.fspath(value)
        self._values[name] = value

    return property(get, set_, doc=f"{doc + ' ' if doc else ''}({kind.__name__}, default: {default})")


class FusionOptions:
    """The reference's StereoFusionOptions with COLMAP 3.9.1's defaults, following the option protocol of this package:
    construction from a dict or keywords, mergedict, todict, summary, copy and pickle."""

    def __init__(self, *args, **kwargs):
        self._values = {name: default for name, default, _ in _FIELDS}
        if len(args) > 1 or (args and kwargs):
            raise TypeError("FusionOptions(): at most one dict, or keywords")
        if args:
            if isinstance(args[0], FusionOptions):
                self._values.update(args[0]._values)
            elif isinstance(args[0], dict):
                self.mergedict(args[0])
            else:
                raise TypeError(f"FusionOptions(): a dict is needed, not {type(args[0]).__name__}")
        self.mergedict(kwargs)

    def mergedict(self, d) -> None:
        for key, value in dict(d).items():
            if key not in self._values:
                raise ValueError(f"FusionOptions: unknown option '{key}' (valid: {', '.join(FIELD_NAMES)})")
            setattr(self, key, value)

    def todict(self, recursive: bool = True) -> dict:
        return {name: self._values[name] for name in FIELD_NAMES}

    def summary(self, write_type: bool = False) -> str:
        lines = ["FusionOptions:"]
        for name in FIELD_NAMES:
            v = self._values[name]
            lines.append(f"    {name}{': ' + type(v).__name__ if write_type else ''} = {v}")
        return "\n".join(lines)

    __repr__ = summary

    def __eq__(self, other):
        return isinstance(other, FusionOptions) and self._values == other._values

    __hash__ = None

    def __copy__(self):
        return FusionOptions(self)

    def __deepcopy__(self, memo):
        return FusionOptions(self)

    def __getstate__(self):
        return self.todict()

    def __setstate__(self, state):
        self._values = {name: default for name, default, _ in _FIELDS}
        self.mergedict(state)

    def check(self) -> None:
        """COLMAP's StereoFusionOptions::Check(): the first condition that fails is a ValueError"""
        v = self._values
        conditions = [
            ("min_num_pixels >= 0", v["min_num_pixels"] >= 0),
            ("min_num_pixels <= max_num_pixels", v["min_num_pixels"] <= v["max_num_pixels"]),
            ("max_traversal_depth > 0", v["max_traversal_depth"] > 0),
            ("max_reproj_error >= 0", v["max_reproj_error"] >= 0),
            ("max_depth_error >= 0", v["max_depth_error"] >= 0),
            ("max_normal_error >= 0", v["max_normal_error"] >= 0),
            ("check_num_images > 0", v["check_num_images"] > 0),
            ("cache_size > 0", v["cache_size"] > 0),
        ]
        for text, holds in conditions:
            if not holds:
                raise ValueError(_check_message(f"Check Failed: {text}"))


for _name, _default, _doc in _FIELDS:
    setattr(FusionOptions, _name, _option_property(_name, type(_default), _doc, f'"{_default}"' if isinstance(_default, str) else _default))
del _name, _default, _doc


def _options(options) -> FusionOptions:
    if options is None:
        return FusionOptions()
    if isinstance(options, dict):
        return FusionOptions(options)
    if not isinstance(options, FusionOptions):
        raise TypeError(f"StereoFusion: options is a {type(options).__name__}, not FusionOptions or a dict")
    return copy.copy(options)


# ---- the host half: config, neighbours, the output files (no device) ----------------------------------------------------------
def parse_config(text: str, names):
    """stereo/fusion.cfg: an image name per line, in fusion order; empty lines and lines starting with # are skipped.  An
    unknown name or a name given twice is a ValueError."""
    known, out = set(names), []
    for line in text.splitlines():
        line = line.strip()
        if not line or line.startswith("#"):
            continue
        if line not in known:
            raise ValueError(f"fusion.cfg: the image {line} is not in the sparse model")
        if line in out:
            raise ValueError(f"fusion.cfg: {line} is listed twice")
        out.append(line)
    return out


def select_neighbours(order, seen, check_num_images: int):
    """Per image of `order` (image ids) the at most check_num_images images of `order` that share the most points3D with it,
    ties by image id, images that share none left out (_patch_match.auto_candidates), as positions in `order`; seen =
    {image id: its point3D ids}"""
    where = {iid: k for k, iid in enumerate(order)}
    sets = {iid: set(seen[iid]) for iid in order}
    out = []
    for iid in order:
        shared = {j: [p for p in seen[j] if p in sets[iid]] for j in order if j != iid}
        out.append([where[j] for j, _ in auto_candidates(iid, shared, check_num_images)])
    return out


def ply_bytes(points) -> bytes:
    """COLMAP's binary little-endian PLY of fused points (WriteBinaryPlyPoints with normals and colours)"""
    p = np.asarray(points, dtype=POINT_DTYPE)
    head = ("ply\nformat binary_little_endian 1.0\n" + f"element vertex {p.size}\n"
            "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    return head.encode() + p.tobytes()


def vis_bytes(visibility) -> bytes:
    """COLMAP's .vis file (WritePointsVisibility): a uint64 count, then per point a uint32 count and its uint32 image
    indices"""
    parts = [struct.pack("<Q", len(visibility))]
    for v in visibility:
        v = np.asarray(v, dtype="<u4")
        parts.append(struct.pack("<I", v.size) + v.tobytes())
    return b"".join(parts)


# ---- the class ----------------------------------------------------------------------------------------------------------------
class StereoFusion:
    """COLMAP's mvs::StereoFusion on a dense workspace: `run()` fuses the maps into `fused_points` (a structured array of
    x, y, z, nx, ny, nz, r, g, b) and `fused_points_visibility` (per point the image indices in fusion.cfg's order);
    `write(output_path)` does what the reference's stereo_fusion does with them."""

    def __init__(self, options=None, workspace_path="", workspace_format="COLMAP", pmvs_option_name="option-all", input_type="geometric"):
        self.options = _options(options)
        self.workspace_path = os.fspath(workspace_path)
        self.workspace_format = workspace_format
        self.pmvs_option_name = pmvs_option_name
        self.input_type = input_type
        self.summary = {}
        self._context_factory = _capi.Context  # (the tests put the CPU reference here)

    # what the options and the arguments rule out, before anything is read
    def _refuse(self):
        o = self.options
        fmt = str(self.workspace_format).lower()
        if fmt not in ("colmap", "pmvs"):
            raise ValueError("Invalid `workspace_format` - supported values are 'COLMAP' or 'PMVS'.")
        if fmt != "colmap":
            raise ValueError(f"workspace_format {self.workspace_format!r} is not supported by pycolmap_amd's StereoFusion: only "
                             "the 'COLMAP' workspace is read (DESIGN.md section 23)")
        if str(self.input_type).lower() not in INPUT_TYPES:
            raise ValueError("Invalid input type - supported values are 'photometric' and 'geometric'.")
        if o.mask_path:
            raise ValueError(f"mask_path={o.mask_path!r} is not supported by pycolmap_amd's StereoFusion: masks are not read "
                             "(DESIGN.md section 23)")
        o.check()
        if o.check_num_images > _capi.FUSION_MAX_NEIGHBOURS:
            raise ValueError(f"check_num_images={o.check_num_images} is more than {_capi.FUSION_MAX_NEIGHBOURS} "
                             "(AMC_FUSION_MAX_NEIGHBOURS): a lane of the kernel takes one neighbour (DESIGN.md section 23)")
        if o.max_traversal_depth > _capi.FUSION_MAX_TRAVERSAL_DEPTH:
            raise ValueError(f"max_traversal_depth={o.max_traversal_depth} is more than {_capi.FUSION_MAX_TRAVERSAL_DEPTH} "
                             "(AMC_FUSION_MAX_TRAVERSAL_DEPTH): the walk's stack is that deep (DESIGN.md section 23)")

    def _read_workspace(self):
        """everything the call needs, read and checked before a device is opened"""
        o = self.options
        ws = Path(self.workspace_path)
        for sub in ("sparse", "images", "stereo"):
            if not (ws / sub).is_dir():
                raise ValueError(_check_message(f"Check Failed: ExistsDir({sub}) : Directory {ws / sub} does not exist."))
        rec = _pycolmap.Reconstruction()
        rec.read(str(ws / "sparse"))
        images, cameras = dict(rec.images), dict(rec.cameras)
        for cid, cam in cameras.items():
            if str(getattr(cam.model, "name", cam.model)) != "PINHOLE":
                raise ValueError(f"camera {cid} of sparse/ is {getattr(cam.model, 'name', cam.model)}, not PINHOLE: "
                                 "StereoFusion reads the undistorted workspace that undistort_images writes")
            if o.max_image_size > 0 and max(cam.width, cam.height) > o.max_image_size:
                raise ValueError(f"max_image_size={o.max_image_size}: camera {cid} is {cam.width} x {cam.height}. StereoFusion "
                                 "does not rescale; make the workspace at the wanted size with "
                                 f"undistort_images(undistort_options=dict(max_image_size={o.max_image_size}))")
        by_name = {im.name: iid for iid, im in images.items()}
        with open(ws / "stereo" / "fusion.cfg") as f:
            names = parse_config(f.read(), by_name.keys())
        stage = str(self.input_type).lower()
        order, used, pix, dm, nm = [], [], [], [], []
        for pos, name in enumerate(names):
            dp = ws / "stereo" / "depth_maps" / f"{name}.{stage}.bin"
            npth = ws / "stereo" / "normal_maps" / f"{name}.{stage}.bin"
            if not (dp.exists() and npth.exists()):  # COLMAP leaves such an image out of the fusion
                continue
            iid = by_name[name]
            cam = cameras[images[iid].camera_id]
            a = read_image(str(ws / "images" / name))
            if a.ndim == 2:
                a = np.repeat(a[..., None], 3, axis=2)
            d, n = read_array(dp), read_array(npth)
            if a.shape[:2] != (cam.height, cam.width):
                raise ValueError(f"{name}: the image is {a.shape[1]} x {a.shape[0]}, its camera {cam.width} x {cam.height}")
            if d.shape != a.shape[:2] or n.shape != a.shape[:2] + (3,):
                raise ValueError(f"{name}: the image is {a.shape[1]} x {a.shape[0]}, its depth map {d.shape[1]} x {d.shape[0]}, "
                                 f"its normal map {n.shape[1]} x {n.shape[0]}")
            order.append(iid)
            used.append(pos)  # the image's index in fusion.cfg's order: what the visibility lists hold
            pix.append(np.ascontiguousarray(a[..., :3]))
            dm.append(d)
            nm.append(np.ascontiguousarray(np.transpose(n, (2, 0, 1))))
        seen = {iid: sorted({p.point3D_id for p in images[iid].points2D if p.has_point3D()}) for iid in order}
        nb = select_neighbours(order, seen, o.check_num_images)
        K = np.array([list(cameras[images[i].camera_id].params)[:4] for i in order], np.float64).reshape(-1, 4)
        R = np.array([np.asarray(images[i].cam_from_world.rotation.matrix(), np.float64) for i in order]).reshape(-1, 3, 3)
        t = np.array([np.asarray(images[i].cam_from_world.translation, np.float64) for i in order]).reshape(-1, 3)
        return (pix, K, R, t, dm, nm, nb), np.array(used, np.uint32), len(names) - len(used)

    def run(self) -> None:
        t_all = time.perf_counter()
        o = self.options
        self._refuse()
        args, used, missing = self._read_workspace()
        with self._context_factory(0) as ctx:  # no device: this raises, and fused_points stays unset
            res = ctx.fuse_depth_maps(*args, min_num_pixels=o.min_num_pixels, max_num_pixels=o.max_num_pixels,
                                      max_traversal_depth=o.max_traversal_depth, max_reproj_error=o.max_reproj_error,
                                      max_depth_error=o.max_depth_error, max_normal_error=o.max_normal_error,
                                      bounding_box=o.bounding_box)
        n = res["num_points"]
        pts = np.zeros(n, POINT_DTYPE)
        for k, name in enumerate(("x", "y", "z")):
            pts[name] = res["xyz"][:, k]
            pts["n" + name] = res["normal"][:, k]
        for k, name in enumerate(("r", "g", "b")):
            pts[name] = res["color"][:, k]
        off = res["vis_offsets"]
        self.fused_points = pts
        self.fused_points_visibility = [used[res["vis_images"][int(off[p]):int(off[p + 1])]] for p in range(n)]
        total_ms = (time.perf_counter() - t_all) * 1e3
        self.summary = {"num_images": len(args[0]), "images_without_maps": missing, "num_points": n,
                        "num_seeds": res["num_seeds"], "num_truncated": res["num_truncated"],
                        "num_batches": res.get("num_batches", 0), "num_launches": res.get("num_launches", 0),
                        "device_ms": res.get("device_ms", 0.0), "kernel_ms": res.get("kernel_ms", 0.0),
                        "copy_ms": res.get("copy_ms", 0.0), "host_ms": total_ms - res.get("device_ms", 0.0)}
        _pycolmap._last_stats = dict(self.summary, total_ms=total_ms)

    def last_run_stats(self) -> dict:
        return dict(self.summary)

    def write(self, output_path):
        """The reference's stereo_fusion after the fusion: the sparse model with its points3D replaced by the fused points
        (empty tracks), written as binary into `output_path` when that is an existing directory, else the points as
        `output_path` (.ply) and their visibility as `output_path`.vis.  Returns the Reconstruction."""
        if not hasattr(self, "fused_points"):
            raise ValueError("StereoFusion.write: run() has not fused anything yet")
        out = os.fspath(output_path)
        if not os.path.isdir(out) and not out.lower().endswith(".ply"):
            raise ValueError(_check_message(f"Check Failed: HasFileExtension({out}, .ply) : Path {out} does not match file extension .ply."))
        rec = _pycolmap.Reconstruction()
        rec.read(str(Path(self.workspace_path) / "sparse"))
        for image in dict(rec.images).values():  # ImportPLY: no observation keeps its point
            image.points2D = [_pycolmap.Point2D(list(map(float, p.xy))) for p in image.points2D]
        points = rec.points3D
        points.clear()
        for k, p in enumerate(self.fused_points):
            q = _pycolmap.Point3D()
            q.xyz = [float(p["x"]), float(p["y"]), float(p["z"])]
            q.color = [int(p["r"]), int(p["g"]), int(p["b"])]
            q.error = 0.0
            points[k + 1] = q
        if os.path.isdir(out):
            rec.write_binary(out)
        else:
            with open(out, "wb") as f:
                f.write(ply_bytes(self.fused_points))
            with open(out + ".vis", "wb") as f:
                f.write(vis_bytes(self.fused_points_visibility))
        return rec
