"""undistort_images: a sparse model and its distorted photographs -> COLMAP's dense workspace (images/, sparse/,
stereo/), with the reference's signature (/root/reference/pycolmap/pipeline/images.h:96-148, 242-261).

The model is read by the host layer (csrc/host/model_io.cc), every image gets its PINHOLE camera (amc_undistort_camera),
the photographs are decoded on a host thread pool (at most 16 threads), warped on the device in batches of bounded bytes
through one amc_undistort_images call each (libamc.so, csrc/undistort.hip) and encoded and written back on the pool, so
that memory is bounded by a few batches and not by the dataset.  Binary PGM / PPM are read and written by the built-in
code; other formats need Pillow.  DESIGN.md section 14 lists the rules and their deviations from COLMAP."""
from __future__ import annotations

import inspect
import os
import shutil
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

from . import _capi, _pycolmap
from ._extraction import MAX_DECODE_THREADS, _read_pnm

BATCH_BYTES = 1 << 28  # source bytes per device call (the call splits further by AMC_UNDISTORT_BATCH_BYTES)
OUTPUT_TYPES = ("COLMAP", "PMVS", "CMP-MVS")
JPEG_QUALITY = 95


def _check_message(text: str) -> str:
    """The reference's exception text (log_exceptions.h): "[file:line] ..." of the raising line."""
    f = inspect.currentframe().f_back
    return f"[{os.path.basename(f.f_code.co_filename)}:{f.f_lineno}] {text}"


# ---- decoding and encoding ------------------------------------------------------------------------------------------
def read_image(path: str) -> np.ndarray:
    """H x W (grey) or H x W x 3 (colour) uint8: colour stays colour and grey stays grey."""
    a = _read_pnm(path)
    if a is None:
        try:
            from PIL import Image
        except ImportError:
            raise ValueError(f"{path}: only binary PGM / PPM can be read without Pillow") from None
        try:
            with Image.open(path) as im:
                im = im.convert("RGB") if im.mode not in ("L", "RGB") else im
                a = np.asarray(im)
        except Exception as e:  # noqa: BLE001 - any decoder failure names the file
            raise ValueError(f"{path}: cannot be decoded ({e})") from None
    return np.ascontiguousarray(a, dtype=np.uint8)


def write_image(path: str, a: np.ndarray) -> None:
    """The image in the format its extension names: PGM / PPM by the built-in writer, the rest through Pillow."""
    ext = Path(path).suffix.lower()
    if ext in (".pgm", ".ppm", ".pnm"):
        if (ext == ".pgm") != (a.ndim == 2) and ext != ".pnm":  # a grey image under .ppm, or colour under .pgm
            a = np.repeat(a[..., None], 3, axis=2) if a.ndim == 2 else \
                np.floor(a.astype(np.float64) @ [0.2126, 0.7152, 0.0722] + 0.5).clip(0, 255).astype(np.uint8)
        head = (b"P5" if a.ndim == 2 else b"P6") + f"\n{a.shape[1]} {a.shape[0]}\n255\n".encode()
        with open(path, "wb") as f:
            f.write(head)
            f.write(np.ascontiguousarray(a).tobytes())
        return
    try:
        from PIL import Image
    except ImportError:
        raise ValueError(f"{path}: only PGM / PPM can be written without Pillow") from None
    kw = {"quality": JPEG_QUALITY} if ext in (".jpg", ".jpeg") else {}
    Image.fromarray(a).save(path, **kw)


def _place(src: str, dst: str, policy) -> None:
    """An image that needs no warp: copied or linked by the policy (COLMAP's FileCopy)."""
    if os.path.lexists(dst):
        os.unlink(dst)
    if policy == _pycolmap.CopyType.copy:
        shutil.copyfile(src, dst)
    elif policy == getattr(_pycolmap.CopyType, "hard-link"):
        os.link(src, dst)
    else:
        os.symlink(os.path.abspath(src), dst)


# ---- the plan (test hook, like _exhaustive_blocks) ----------------------------------------------------------------------
def _options(undistort_options):
    if undistort_options is None:
        return _pycolmap.UndistortCameraOptions()
    if isinstance(undistort_options, dict):
        return _pycolmap.UndistortCameraOptions(undistort_options)
    return undistort_options


def _undistort_plan(input_path, image_list=(), undistort_options=None):
    """Per image of an undistort_images call, without a device: dicts with name, image_id, camera, undistorted_camera
    and copy (True: the image is copied or linked, not warped)."""
    return _pycolmap._undistort_plan(os.fspath(input_path), [str(n) for n in image_list or ()], _options(undistort_options))


def _cam_tuple(c):
    return (int(c.model), int(c.width), int(c.height), list(c.params))


# ---- the pipeline -----------------------------------------------------------------------------------------------------
def undistort_images(output_path, input_path, image_path, image_list=[], output_type="COLMAP",  # noqa: B006
                     copy_policy=_pycolmap.CopyType.copy, num_patch_match_src_images=20,
                     undistort_options=_pycolmap.UndistortCameraOptions()):
    """Undistort the images of the sparse model at `input_path` into a dense workspace at `output_path`."""
    t_all = time.perf_counter()
    output_path, input_path, image_path = os.fspath(output_path), os.fspath(input_path), os.fspath(image_path)
    if not os.path.isdir(input_path):
        raise ValueError(_check_message(f"Check Failed: ExistsDir(input_path) : Directory {input_path} does not exist."))
    if not os.path.isdir(image_path):
        raise ValueError(_check_message(f"Check Failed: ExistsDir(image_path) : Directory {image_path} does not exist."))
    if output_type not in OUTPUT_TYPES:
        raise ValueError(_check_message("Invalid `output_type` - supported values are {'COLMAP', 'PMVS', 'CMP-MVS'}."))
    if output_type != "COLMAP":
        raise ValueError(f"output_type {output_type!r} is not supported by pycolmap_amd's undistort_images: only the "
                         "'COLMAP' workspace is written (DESIGN.md 14.9)")
    copy_policy = _pycolmap.CopyType.copy if copy_policy is None else copy_policy
    copy_policy = _pycolmap.CopyType(copy_policy) if isinstance(copy_policy, str) else copy_policy
    options = _options(undistort_options)
    plan = _undistort_plan(input_path, image_list, options)  # option checks, the model, the warnings

    out = Path(output_path)
    for sub in ("images", "sparse", "stereo/depth_maps", "stereo/normal_maps", "stereo/consistency_graphs"):
        (out / sub).mkdir(parents=True, exist_ok=True)
    for item in plan:  # sub-folders for nested image names
        folder = os.path.dirname(item["name"])
        if folder:
            for sub in ("images", "stereo/depth_maps", "stereo/normal_maps", "stereo/consistency_graphs"):
                (out / sub / folder).mkdir(parents=True, exist_ok=True)

    def decode(item):
        img = read_image(os.path.join(image_path, item["name"]))
        cam = item["camera"]
        if img.shape[1] != cam.width or img.shape[0] != cam.height:
            raise ValueError(f"{item['name']}: the image is {img.shape[1]} x {img.shape[0]}, its camera "
                             f"{cam.width} x {cam.height}")
        return img

    def encode(job):
        item, img = job
        write_image(str(out / "images" / item["name"]), img)

    warp = [it for it in plan if not it["copy"]]
    for it in plan:
        if it["copy"]:
            _place(os.path.join(image_path, it["name"]), str(out / "images" / it["name"]), copy_policy)
    decode_ms = device_ms = kernel_ms = encode_ms = 0.0
    pixels = batches = 0
    if warp:
        with ThreadPoolExecutor(max_workers=max(1, min(MAX_DECODE_THREADS, len(warp)))) as pool, \
                _capi.Context(0) as ctx:
            i, pending = 0, None
            while i < len(warp):  # batches bounded by source bytes: decode, warp, hand to the encoders
                j, nbytes = i, 0
                while j < len(warp) and (j == i or nbytes + warp[j]["camera"].width * warp[j]["camera"].height * 3 <= BATCH_BYTES):
                    nbytes += warp[j]["camera"].width * warp[j]["camera"].height * 3
                    j += 1
                t = time.perf_counter()
                imgs = list(pool.map(decode, warp[i:j]))
                decode_ms += (time.perf_counter() - t) * 1e3
                outs, st = ctx.undistort_images(imgs, [_cam_tuple(it["camera"]) for it in warp[i:j]],
                                                [_cam_tuple(it["undistorted_camera"]) for it in warp[i:j]])
                device_ms += st["device_ms"]
                kernel_ms += st["kernel_ms"]
                batches += st["num_batches"]
                pixels += sum(o.shape[0] * o.shape[1] for o in outs)
                t = time.perf_counter()
                if pending is not None:  # the previous batch's files are written before the next one is queued
                    list(pending)
                pending = pool.map(encode, list(zip(warp[i:j], outs)))
                encode_ms += (time.perf_counter() - t) * 1e3
                i = j
            t = time.perf_counter()
            if pending is not None:
                list(pending)
            encode_ms += (time.perf_counter() - t) * 1e3

    t = time.perf_counter()
    _pycolmap._write_undistorted_model(input_path, str(out / "sparse"), options)
    with open(out / "stereo" / "patch-match.cfg", "w") as f:
        for it in plan:
            f.write(f"{it['name']}\n__auto__, {int(num_patch_match_src_images)}\n")
    with open(out / "stereo" / "fusion.cfg", "w") as f:
        for it in plan:
            f.write(f"{it['name']}\n")
    model_ms = (time.perf_counter() - t) * 1e3
    _pycolmap._last_stats = {"images": len(plan), "warped": len(warp), "copied": len(plan) - len(warp), "pixels": pixels,
                             "num_batches": batches, "decode_ms": decode_ms, "device_ms": device_ms,
                             "kernel_ms": kernel_ms, "encode_ms": encode_ms, "model_ms": model_ms,
                             "total_ms": (time.perf_counter() - t_all) * 1e3}
