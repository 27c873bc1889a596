"""PatchMatch stereo over COLMAP's dense workspace: PatchMatchOptions and PatchMatchController, with the reference's
option fields (/root/reference/pycolmap/pipeline/mvs.h:96-180) and COLMAP 3.9.1's two stages.

The workspace that undistort_images wrote (images/, sparse/, stereo/patch-match.cfg) is read back: the model by the host
layer (csrc/host/model_io.cc), the images by _undistortion.read_image.  The config's entries become problems, `__auto__`
is resolved with Context.shared_point_angles, every problem gets its depth range, the passes run on the device through
Context.patch_match (libamc.so, csrc/patchmatch.hip) and the maps are written in COLMAP's array format.  DESIGN.md section
22 lists the rules and their deviations from COLMAP.  read_array / write_array are this package's helpers for that
format."""
from __future__ import annotations

import copy
import os
import time
from pathlib import Path

import numpy as np

from . import _capi, _pycolmap
from ._undistortion import _check_message, read_image

CALL_PROBLEMS = 64  # problems per device call (the call splits further by AMC_PATCHMATCH_BATCH_BYTES)
MAX_WINDOW_RADIUS = 32  # COLMAP's kMaxPatchMatchWindowRadius
AUTO, ALL = "__auto__", "__all__"


# ---- COLMAP's array files ---------------------------------------------------------------------------------------------
def write_array(path, array) -> int:
    """An H x W or H x W x C array as COLMAP's dense array file: the ASCII header "width&height&channels&", then
    little-endian float32 with the column varying fastest, then the row, then the channel.  Returns the bytes written."""
    a = np.asarray(array, dtype=np.float32)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3:
        raise ValueError(f"write_array: the array has {a.ndim} dimensions, not 2 or 3")
    h, w, c = a.shape
    data = f"{w}&{h}&{c}&".encode() + np.ascontiguousarray(np.transpose(a, (2, 0, 1))).astype("<f4").tobytes()
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def read_array(path) -> np.ndarray:
    """The array of a COLMAP dense array file: H x W for one channel, else H x W x C (float32)."""
    with open(path, "rb") as f:
        data = f.read()
    parts = data.split(b"&", 3)
    try:
        if len(parts) != 4:
            raise ValueError
        w, h, c = (int(p.decode()) for p in parts[:3])
        if w < 0 or h < 0 or c < 1 or len(parts[3]) != 4 * w * h * c:
            raise ValueError
    except ValueError:
        raise ValueError(f"{path}: not a COLMAP array file (width&height&channels& and float32 data)") from None
    a = np.frombuffer(parts[3], dtype="<f4").reshape(c, h, w).astype(np.float32)
    return a[0].copy() if c == 1 else np.ascontiguousarray(np.transpose(a, (1, 2, 0)))


# ---- the options --------------------------------------------------------------------------------------------------------
_FIELDS = [  # name, COLMAP 3.9.1's default, the reference's docstring
    ("max_image_size", -1, "Maximum image size in either dimension."),
    ("gpu_index", "-1", "Index of the GPU used for patch match. For multi-GPU usage, you should separate multiple GPU "
                        "indices by comma, e.g., \"0,1,2,3\"."),
    ("depth_min", -1.0, ""),
    ("depth_max", -1.0, ""),
    ("window_radius", 5, "Half window size to compute NCC photo-consistency cost."),
    ("window_step", 1, "Number of pixels to skip when computing NCC."),
    ("sigma_spatial", -1.0, "Spatial sigma for bilaterally weighted NCC."),
    ("sigma_color", 0.2, "Color sigma for bilaterally weighted NCC."),
    ("num_samples", 15, "Number of random samples to draw in Monte Carlo sampling."),
    ("ncc_sigma", 0.6, "Spread of the NCC likelihood function."),
    ("min_triangulation_angle", 1.0, "Minimum triangulation angle in degrees."),
    ("incident_angle_sigma", 0.9, "Spread of the incident angle likelihood function."),
    ("num_iterations", 5, "Number of coordinate descent iterations."),
    ("geom_consistency", True, "Whether to add a regularized geometric consistency term to the cost function. If true, the "
                               "`depth_maps` and `normal_maps` must not be null."),
    ("geom_consistency_regularizer", 0.3, "The relative weight of the geometric consistency term w.r.t. to the "
                                          "photo-consistency term."),
    ("geom_consistency_max_cost", 3.0, "Maximum geometric consistency cost in terms of the forward-backward reprojection "
                                       "error in pixels."),
    ("filter", True, "Whether to enable filtering."),
    ("filter_min_ncc", 0.1, "Minimum NCC coefficient for pixel to be photo-consistent."),
    ("filter_min_triangulation_angle", 3.0, "Minimum triangulation angle to be stable."),
    ("filter_min_num_consistent", 2, "Minimum number of source images have to be consistent for pixel not to be filtered."),
    ("filter_geom_consistency_max_cost", 1.0, "Maximum forward-backward reprojection error for pixel to be geometrically "
                                              "consistent."),
    ("cache_size", 32.0, "Cache size in gigabytes for patch match."),
    ("allow_missing_files", False, "Whether to tolerate missing images/maps in the problem setup"),
    ("write_consistency_graph", False, "Whether to write the consistency graph."),
]
FIELD_NAMES = [f[0] for f in _FIELDS]


def _option_property(name, kind, doc, default):
    def get(self):
        return self._values[name]

    def set_(self, value):
        if kind is bool:
            if not isinstance(value, (bool, np.bool_)):
                raise TypeError(f"PatchMatchOptions.{name}: a bool is needed, not {type(value).__name__}")
            value = bool(value)
        elif kind is int:
            if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
                raise TypeError(f"PatchMatchOptions.{name}: an int is needed, not {type(value).__name__}")
            value = int(value)
        elif kind is float:
            if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
                raise TypeError(f"PatchMatchOptions.{name}: a float is needed, not {type(value).__name__}")
            value = float(value)
        elif not isinstance(value, str):
            raise TypeError(f"PatchMatchOptions.{name}: a str is needed, not {type(value).__name__}")
        self._values[name] = value

    return property(get, set_, doc=f"{doc + ' ' if doc else ''}({kind.__name__}, default: {default})")


class PatchMatchOptions:
    """The reference's PatchMatchOptions with COLMAP 3.9.1's defaults, following the option protocol of this package:
    construction from a dict or keywords, mergedict, todict, summary, copy and pickle."""

    def __init__(self, *args, **kwargs):
        self._values = {name: default for name, default, _ in _FIELDS}
        if len(args) > 1 or (args and kwargs):
            raise TypeError("PatchMatchOptions(): at most one dict, or keywords")
        if args:
            if isinstance(args[0], PatchMatchOptions):
                self._values.update(args[0]._values)
            elif isinstance(args[0], dict):
                self.mergedict(args[0])
            else:
                raise TypeError(f"PatchMatchOptions(): a dict is needed, not {type(args[0]).__name__}")
        self.mergedict(kwargs)

    def mergedict(self, d) -> None:
        for key, value in dict(d).items():
            if key not in self._values:
                raise ValueError(f"PatchMatchOptions: unknown option '{key}' (valid: {', '.join(FIELD_NAMES)})")
            setattr(self, key, value)

    def todict(self, recursive: bool = True) -> dict:
        return {name: self._values[name] for name in FIELD_NAMES}

    def summary(self, write_type: bool = False) -> str:
        lines = ["PatchMatchOptions:"]
        for name in FIELD_NAMES:
            v = self._values[name]
            lines.append(f"    {name}{': ' + type(v).__name__ if write_type else ''} = {v}")
        return "\n".join(lines)

    __repr__ = summary

    def __eq__(self, other):
        return isinstance(other, PatchMatchOptions) and self._values == other._values

    __hash__ = None

    def __copy__(self):
        return PatchMatchOptions(self)

    def __deepcopy__(self, memo):
        return PatchMatchOptions(self)

    def __getstate__(self):
        return self.todict()

    def __setstate__(self, state):
        self._values = {name: default for name, default, _ in _FIELDS}
        self.mergedict(state)

    def check(self) -> None:
        """COLMAP's PatchMatchOptions::Check(): the first condition that fails is a ValueError"""
        v = self._values
        conditions = [
            ("depth_min <= depth_max", v["depth_min"] == -1 and v["depth_max"] == -1 or v["depth_min"] <= v["depth_max"]),
            ("depth_min >= 0", v["depth_min"] == -1 and v["depth_max"] == -1 or v["depth_min"] >= 0),
            ("window_radius <= kMaxPatchMatchWindowRadius", v["window_radius"] <= MAX_WINDOW_RADIUS),
            ("sigma_color > 0", v["sigma_color"] > 0),
            ("window_radius > 0", v["window_radius"] > 0),
            ("window_step > 0", v["window_step"] > 0),
            ("window_step <= 2", v["window_step"] <= 2),
            ("num_samples > 0", v["num_samples"] > 0),
            ("ncc_sigma > 0", v["ncc_sigma"] > 0),
            ("min_triangulation_angle >= 0", v["min_triangulation_angle"] >= 0),
            ("min_triangulation_angle < 180", v["min_triangulation_angle"] < 180),
            ("incident_angle_sigma > 0", v["incident_angle_sigma"] > 0),
            ("num_iterations > 0", v["num_iterations"] > 0),
            ("geom_consistency_regularizer >= 0", v["geom_consistency_regularizer"] >= 0),
            ("geom_consistency_max_cost >= 0", v["geom_consistency_max_cost"] >= 0),
            ("filter_min_ncc >= -1", v["filter_min_ncc"] >= -1),
            ("filter_min_ncc <= 1", v["filter_min_ncc"] <= 1),
            ("filter_min_triangulation_angle >= 0", v["filter_min_triangulation_angle"] >= 0),
            ("filter_min_triangulation_angle <= 180", v["filter_min_triangulation_angle"] < 180),
            ("filter_min_num_consistent >= 0", v["filter_min_num_consistent"] >= 0),
            ("filter_geom_consistency_max_cost >= 0", v["filter_geom_consistency_max_cost"] >= 0),
            ("cache_size > 0", v["cache_size"] > 0),
        ]
        for text, holds in conditions:
            if not holds:
                raise ValueError(_check_message(f"Check Failed: {text}"))


for _name, _default, _doc in _FIELDS:
    setattr(PatchMatchOptions, _name, _option_property(_name, type(_default), _doc, f'"{_default}"' if isinstance(_default, str) else _default))
del _name, _default, _doc


def _options(options) -> PatchMatchOptions:
    if options is None:
        return PatchMatchOptions()
    if isinstance(options, dict):
        return PatchMatchOptions(options)
    if not isinstance(options, PatchMatchOptions):
        raise TypeError(f"PatchMatchController: options is a {type(options).__name__}, not PatchMatchOptions or a dict")
    return copy.copy(options)


# ---- the host half: config, source selection, depth ranges (no device) ----------------------------------------------------
def parse_config(text: str, names, allow_missing: bool = False):
    """stereo/patch-match.cfg: pairs of lines, an image name and then `__all__`, `__auto__, N` or a comma-separated list of
    names; empty lines and lines starting with # are skipped.  Returns [(reference name, spec)] with spec ("all",),
    ("auto", N) or ("list", [names]).  An unknown name or an image that lists itself is a ValueError; with allow_missing
    an entry with an unknown reference is dropped, and unknown sources and the image itself are left out of a list."""
    known = set(names)
    lines = [ln.strip() for ln in text.splitlines()]
    lines = [ln for ln in lines if ln and not ln.startswith("#")]
    if len(lines) % 2:
        raise ValueError(f"patch-match.cfg: {len(lines)} lines, not pairs of an image name and its sources")
    out, seen = [], set()
    for k in range(0, len(lines), 2):
        ref, spec = lines[k], lines[k + 1]
        if ref in seen:
            raise ValueError(f"patch-match.cfg: {ref} has two entries")
        seen.add(ref)
        if ref not in known:
            if allow_missing:
                continue
            raise ValueError(f"patch-match.cfg: the reference image {ref} is not in the sparse model")
        parts = [p.strip() for p in spec.split(",")]
        if parts[0] == ALL:
            if len(parts) != 1:
                raise ValueError(f"patch-match.cfg: {ref}: `{ALL}` takes no argument")
            out.append((ref, ("all",)))
        elif parts[0] == AUTO:
            try:
                if len(parts) != 2:
                    raise ValueError
                n = int(parts[1])
            except ValueError:
                raise ValueError(f"patch-match.cfg: {ref}: `{AUTO}, N` needs one integer") from None
            if n < 1:
                raise ValueError(f"patch-match.cfg: {ref}: `{AUTO}, {n}` asks for no source images")
            out.append((ref, ("auto", n)))
        else:
            srcs = []
            for p in parts:
                if not p:
                    raise ValueError(f"patch-match.cfg: {ref}: an empty source name")
                if p == ref:
                    if allow_missing:
                        continue
                    raise ValueError(f"patch-match.cfg: {ref} lists itself as a source")
                if p not in known:
                    if allow_missing:
                        continue
                    raise ValueError(f"patch-match.cfg: {ref}: the source image {p} is not in the sparse model")
                if p in srcs:
                    raise ValueError(f"patch-match.cfg: {ref} lists {p} twice")
                srcs.append(p)
            out.append((ref, ("list", srcs)))
    return out


def auto_candidates(ref_id: int, shared: dict, n: int):
    """The n images that share the most points3D with ref_id (ties by image id): [(image id, [point3D ids])], shared =
    {image id: [point3D ids shared with ref_id]}"""
    order = sorted((i for i in shared if i != ref_id and shared[i]), key=lambda i: (-len(shared[i]), i))
    return [(i, shared[i]) for i in order[:n]]


def auto_select(candidates, angles_deg, min_triangulation_angle: float):
    """Of auto_candidates' images those whose 75th-percentile triangulation angle (degrees) reaches the minimum"""
    return [i for (i, _), a in zip(candidates, angles_deg) if a >= min_triangulation_angle]


def depth_range(depths, depth_min: float = -1.0, depth_max: float = -1.0):
    """The options' range when both are set; else from the sorted depths of the image's points3D: the 1st percentile
    times 0.75 and the 99th percentile times 1.25 (entry int(n * p) of the n sorted depths).  No depths: ValueError."""
    if depth_min > 0 and depth_max > 0:
        return float(depth_min), float(depth_max)
    d = np.sort(np.asarray(depths, np.float64).reshape(-1))
    d = d[d > 0]
    if d.size == 0:
        raise ValueError("no points3D in front of the image and no depth_min / depth_max: the depth range is unknown")
    lo = d[min(d.size - 1, int(d.size * 0.01))] * 0.75
    hi = d[min(d.size - 1, int(d.size * 0.99))] * 1.25
    return float(lo), float(hi)


def _grey(a: np.ndarray) -> np.ndarray:
    if a.ndim == 2:
        return a
    return np.floor(a.astype(np.float64) @ [0.2126, 0.7152, 0.0722] + 0.5).clip(0, 255).astype(np.uint8)


# ---- the controller -------------------------------------------------------------------------------------------------------
class PatchMatchController:
    """COLMAP's PatchMatchController on a dense workspace: `run()` writes stereo/depth_maps/<image>.<photometric |
    geometric>.bin and stereo/normal_maps/...; `summary` then holds what it did."""

    def __init__(self, options=None, workspace_path="", workspace_format="COLMAP", pmvs_option_name="option-all", config_path=""):
        self.options = _options(options)
        self.workspace_path = os.fspath(workspace_path)
        self.workspace_format = workspace_format
        self.pmvs_option_name = pmvs_option_name
        self.config_path = os.fspath(config_path)
        self.summary = {}
        self._context_factory = _capi.Context  # (the tests put the CPU reference here)

    # what the options and the workspace rule out, before anything is read or written
    def _refuse(self):
        o = self.options
        if str(self.workspace_format).upper() != "COLMAP":
            raise ValueError(f"workspace_format {self.workspace_format!r} is not supported by pycolmap_amd's "
                             "PatchMatchController: only the 'COLMAP' workspace is read (DESIGN.md section 22)")
        if o.write_consistency_graph:
            raise ValueError("write_consistency_graph=True is not supported by pycolmap_amd's PatchMatchController: the "
                             "consistency graphs are not written (DESIGN.md section 22)")
        try:
            gpus = [int(g) for g in str(o.gpu_index).split(",")]
        except ValueError:
            raise ValueError(f"gpu_index {o.gpu_index!r} is not an integer") from None
        if len(gpus) != 1:
            raise ValueError(f"gpu_index {o.gpu_index!r} names {len(gpus)} devices: pycolmap_amd's PatchMatchController "
                             "runs on one (DESIGN.md section 22)")
        o.check()
        return max(gpus[0], 0)

    def _read_workspace(self):
        ws = Path(self.workspace_path)
        for sub in ("sparse", "images", "stereo"):
            if not (ws / sub).is_dir():
                raise ValueError(_check_message(f"Check Failed: ExistsDir({sub}) : Directory {ws / sub} does not exist."))
        rec = _pycolmap.Reconstruction()
        rec.read(str(ws / "sparse"))
        images = dict(rec.images)
        cameras = dict(rec.cameras)
        limit = self.options.max_image_size
        for cid, cam in cameras.items():
            if str(getattr(cam.model, "name", cam.model)) != "PINHOLE":
                raise ValueError(f"camera {cid} of sparse/ is {getattr(cam.model, 'name', cam.model)}, not PINHOLE: "
                                 "PatchMatchController reads the undistorted workspace that undistort_images writes")
            if limit > 0 and max(cam.width, cam.height) > limit:
                raise ValueError(f"max_image_size={limit}: camera {cid} is {cam.width} x {cam.height}. The controller does "
                                 "not rescale; make the workspace at the wanted size with "
                                 f"undistort_images(undistort_options=dict(max_image_size={limit}))")
        return ws, rec, images, cameras

    def run(self) -> None:
        t_all = time.perf_counter()
        o = self.options
        device = self._refuse()
        ws, rec, images, cameras = self._read_workspace()
        by_name = {im.name: iid for iid, im in images.items()}
        cfg_path = self.config_path or str(ws / "stereo" / "patch-match.cfg")
        with open(cfg_path) as f:
            entries = parse_config(f.read(), by_name.keys(), o.allow_missing_files)
        ids = sorted(images)
        index = {iid: k for k, iid in enumerate(ids)}
        # every image's points3D
        points = {pid: np.asarray(p.xyz, np.float64) for pid, p in rec.points3D.items()}
        seen = {iid: sorted({p.point3D_id for p in images[iid].points2D if p.has_point3D() and p.point3D_id in points}) for iid in ids}
        Rm = np.array([np.asarray(images[i].cam_from_world.rotation.matrix(), np.float64) for i in ids]).reshape(-1, 3, 3)
        tv = np.array([np.asarray(images[i].cam_from_world.translation, np.float64) for i in ids]).reshape(-1, 3)
        Km = np.array([list(cameras[images[i].camera_id].params)[:4] for i in ids], np.float64).reshape(-1, 4)

        device_ms = copy_ms = kernel_ms = 0.0
        with self._context_factory(device) as ctx:  # no device: this raises before anything is written
            # ---- the sources of every entry
            auto = [(ref, spec[1]) for ref, spec in entries if spec[0] == "auto"]
            cands = {}
            for ref, n in auto:
                rid = by_name[ref]
                mine = set(seen[rid])
                cands[ref] = auto_candidates(rid, {i: [p for p in seen[i] if p in mine] for i in ids if i != rid}, n)
            chosen = {}
            if any(cands.values()):
                pid_index = {pid: k for k, pid in enumerate(sorted(points))}
                xyz = np.array([points[pid] for pid in sorted(points)]).reshape(-1, 3)
                quat = np.array([list(images[i].cam_from_world.rotation.quat) for i in ids], np.float64).reshape(-1, 4)
                pairs, offs, shared = [], [0], []
                for ref, _ in auto:
                    for i, pts in cands[ref]:
                        pairs.append((index[by_name[ref]], index[i]))
                        shared += [pid_index[p] for p in pts]
                        offs.append(len(shared))
                res = ctx.shared_point_angles(quat, tv, xyz, np.array(pairs, np.uint32), np.array(offs, np.uint64),
                                              np.array(shared, np.uint32), percentile=75.0)
                device_ms += res["device_ms"]
                at = 0
                for ref, _ in auto:
                    k = len(cands[ref])
                    chosen[ref] = auto_select(cands[ref], np.degrees(res["angle"][at:at + k]), o.min_triangulation_angle)
                    at += k
            problems, skipped_empty = [], 0
            for ref, spec in entries:
                rid = by_name[ref]
                if spec[0] == "all":
                    srcs = [i for i in ids if i != rid]
                elif spec[0] == "auto":
                    srcs = chosen.get(ref, [])
                else:
                    srcs = [by_name[s] for s in spec[1]]
                if len(srcs) > _capi.PATCHMATCH_MAX_SOURCES:
                    raise ValueError(f"patch-match.cfg: {ref} has {len(srcs)} source images, more than "
                                     f"{_capi.PATCHMATCH_MAX_SOURCES} (AMC_PATCHMATCH_MAX_SOURCES)")
                if not srcs:  # COLMAP skips a reference image without sources
                    skipped_empty += 1
                    continue
                R, t = Rm[index[rid]], tv[index[rid]]
                depths = [float(R[2] @ points[p] + t[2]) for p in seen[rid]]
                try:
                    rng = depth_range(depths, o.depth_min, o.depth_max)
                except ValueError as e:
                    raise ValueError(f"{ref}: {e}") from None
                problems.append((rid, srcs, rng))

            # ---- the images that the problems name
            used = sorted({i for rid, srcs, _ in problems for i in [rid] + srcs})
            pix = {}
            for i in used:
                a = _grey(read_image(str(ws / "images" / images[i].name)))
                cam = cameras[images[i].camera_id]
                if a.shape != (cam.height, cam.width):
                    raise ValueError(f"{images[i].name}: the image is {a.shape[1]} x {a.shape[0]}, its camera {cam.width} x {cam.height}")
                pix[i] = a

            def out_paths(iid, stage):
                name = images[iid].name
                return (ws / "stereo" / "depth_maps" / f"{name}.{stage}.bin", ws / "stereo" / "normal_maps" / f"{name}.{stage}.bin")

            stats = dict(run=0, skipped=0, bytes=0)

            def stage(name, geom, filt):
                nonlocal device_ms, copy_ms, kernel_ms
                todo = []
                for pbm in problems:
                    dp, npth = out_paths(pbm[0], name)
                    if dp.exists() and npth.exists():  # COLMAP's resume: the maps are there
                        stats["skipped"] += 1
                    else:
                        todo.append(pbm)
                for c in range(0, len(todo), CALL_PROBLEMS):
                    chunk = todo[c:c + CALL_PROBLEMS]
                    # every call gets the whole image table: the random numbers hash the reference image's index in it,
                    # so the maps do not depend on the chunks or on what a resumed run skips
                    local = used
                    li = {iid: k for k, iid in enumerate(local)}
                    in_d = in_n = None
                    if geom:
                        in_d, in_n = [], []
                        for iid in local:
                            dp, npth = out_paths(iid, "photometric")
                            if dp.exists() and npth.exists():
                                in_d.append(read_array(dp))
                                in_n.append(np.ascontiguousarray(np.transpose(read_array(npth), (2, 0, 1))))
                            else:
                                in_d.append(None)
                                in_n.append(None)
                    offs = np.concatenate([[0], np.cumsum([len(s) for _, s, _ in chunk])]).astype(np.uint64)
                    res = ctx.patch_match(
                        [pix[i] for i in local], Km[[index[i] for i in local]], Rm[[index[i] for i in local]],
                        tv[[index[i] for i in local]], np.array([li[r] for r, _, _ in chunk], np.uint32), offs,
                        np.array([li[s] for _, srcs, _ in chunk for s in srcs], np.uint32), np.array([r for _, _, r in chunk]),
                        in_d, in_n, window_radius=o.window_radius, window_step=o.window_step, num_samples=o.num_samples,
                        num_iterations=o.num_iterations, geom_consistency=int(geom), filter=int(filt),
                        filter_min_num_consistent=o.filter_min_num_consistent, sigma_spatial=o.sigma_spatial,
                        sigma_color=o.sigma_color, ncc_sigma=o.ncc_sigma, min_triangulation_angle=o.min_triangulation_angle,
                        incident_angle_sigma=o.incident_angle_sigma, geom_consistency_regularizer=o.geom_consistency_regularizer,
                        geom_consistency_max_cost=o.geom_consistency_max_cost, filter_min_ncc=o.filter_min_ncc,
                        filter_min_triangulation_angle=o.filter_min_triangulation_angle,
                        filter_geom_consistency_max_cost=o.filter_geom_consistency_max_cost)
                    device_ms += res.get("device_ms", 0.0)
                    copy_ms += res.get("copy_ms", 0.0)
                    kernel_ms += res.get("kernel_ms", 0.0)
                    for k, (rid, _, _) in enumerate(chunk):
                        dp, npth = out_paths(rid, name)
                        dp.parent.mkdir(parents=True, exist_ok=True)
                        npth.parent.mkdir(parents=True, exist_ok=True)
                        stats["bytes"] += write_array(dp, res["depth"][k])
                        stats["bytes"] += write_array(npth, np.transpose(res["normal"][k], (1, 2, 0)))
                        stats["run"] += 1

            if o.geom_consistency:
                stage("photometric", False, False)
                stage("geometric", True, o.filter)
            else:
                stage("photometric", False, o.filter)
        self.summary = {"problems_run": stats["run"], "problems_skipped": stats["skipped"], "problems_without_sources": skipped_empty,
                        "bytes_written": stats["bytes"], "device_ms": device_ms, "kernel_ms": kernel_ms, "copy_ms": copy_ms,
                        "host_ms": (time.perf_counter() - t_all) * 1e3 - device_ms}
        _pycolmap._last_stats = dict(self.summary, total_ms=(time.perf_counter() - t_all) * 1e3)
