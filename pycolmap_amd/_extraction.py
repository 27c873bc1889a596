"""extract_features: images on disk -> SIFT keypoints and descriptors in a COLMAP database, with the reference's
signature (/root/reference/pycolmap/pipeline/extract_features.h:24-58).

Images are listed (recursively, name-sorted) or taken from `image_list`, decoded on a host thread pool (at most 16
threads), downscaled when larger than `max_image_size`, sent to the device in batches of bounded bytes through one
amc_sift_extract call each (libamc.so, csrc/sift.hip), and written with their cameras through the Database binding
inside one transaction.  Binary PGM / PPM are read by the built-in reader; other formats need Pillow.  DESIGN.md
section 10.9 lists the rules and their deviations from COLMAP's ImageReader."""
from __future__ import annotations

import os
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

from . import _capi, _pycolmap

MAX_DECODE_THREADS = 16
BATCH_PIXELS = 1 << 25  # input pixels per device call (the device workspace is sized for the largest image of a call)
IMAGE_EXTENSIONS = {".pgm", ".ppm", ".pnm", ".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".webp"}


# ---- decoding -------------------------------------------------------------------------------------------------------
def _read_pnm(path: str) -> np.ndarray | None:
    """Binary PGM (P5) / PPM (P6), 8 or 16 bits; None when the file is not one of them."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 2 or data[:2] not in (b"P5", b"P6"):
        return None
    fields, pos = [], 2
    while len(fields) < 3:
        while pos < len(data) and data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":
            while pos < len(data) and data[pos:pos + 1] not in (b"\n", b"\r"):
                pos += 1
            continue
        start = pos
        while pos < len(data) and not data[pos:pos + 1].isspace():
            pos += 1
        fields.append(int(data[start:pos]))
    pos += 1  # one whitespace byte ends the header
    w, h, maxval = fields
    ch = 1 if data[:2] == b"P5" else 3
    dt = np.dtype(">u2") if maxval > 255 else np.dtype(np.uint8)
    n = w * h * ch
    a = np.frombuffer(data, dtype=dt, count=n, offset=pos).reshape(h, w, ch) if ch == 3 else \
        np.frombuffer(data, dtype=dt, count=n, offset=pos).reshape(h, w)
    if maxval != 255:
        a = np.floor(a.astype(np.float64) * (255.0 / maxval) + 0.5).astype(np.uint8)
    return a


def _to_grey(a: np.ndarray) -> np.ndarray:
    """RGB -> 8-bit grey by Rec. 709 luma, rounded (FreeImage's conversion, to confirm: DESIGN.md 10.9)."""
    if a.ndim == 2:
        return np.ascontiguousarray(a, dtype=np.uint8)
    rgb = a[..., :3].astype(np.float64)
    return np.floor(0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2] + 0.5).clip(0, 255).astype(np.uint8)


def read_image_grey(path: str) -> np.ndarray:
    """The 8-bit grey image of a file: the built-in PGM / PPM reader, else Pillow when it can be imported."""
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
    return _to_grey(a)


def downscale(img: np.ndarray, max_size: int) -> np.ndarray:
    """COLMAP's size rule (scale = max_size / max(w, h), new sizes truncated); bilinear with pixel centres aligned,
    after a box pre-filter of the integer part of the factor."""
    h, w = img.shape
    scale = max_size / max(w, h)
    nw, nh = max(1, int(w * scale)), max(1, int(h * scale))
    a = img.astype(np.float32)
    k = int((w / nw + h / nh) / 2)
    if k >= 2:  # box pre-filter against aliasing
        c = np.cumsum(np.pad(a, ((1, 0), (1, 0))), 0).cumsum(1)
        r = k // 2
        yy0, xx0 = np.clip(np.arange(h) - r, 0, h), np.clip(np.arange(w) - r, 0, w)
        yy1, xx1 = np.clip(np.arange(h) - r + k, 0, h), np.clip(np.arange(w) - r + k, 0, w)
        a = (c[yy1][:, xx1] - c[yy0][:, xx1] - c[yy1][:, xx0] + c[yy0][:, xx0]) / \
            ((yy1 - yy0)[:, None] * (xx1 - xx0)[None, :])
    ys = np.clip((np.arange(nh) + 0.5) * (h / nh) - 0.5, 0, h - 1)
    xs = np.clip((np.arange(nw) + 0.5) * (w / nw) - 0.5, 0, w - 1)
    y0, x0 = np.floor(ys).astype(int), np.floor(xs).astype(int)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    fy, fx = (ys - y0)[:, None], (xs - x0)[None, :]
    out = (a[y0][:, x0] * (1 - fx) * (1 - fy) + a[y0][:, x1] * fx * (1 - fy) + a[y1][:, x0] * (1 - fx) * fy
           + a[y1][:, x1] * fx * fy)
    return np.floor(out + 0.5).clip(0, 255).astype(np.uint8)


# ---- the file list and the cameras (test hooks, like _exhaustive_blocks) -------------------------------------------------
def _image_list(image_path: str, image_list) -> list[str]:
    """Names relative to image_path with '/' separators: the given list, or every image file below image_path,
    recursively, sorted by name."""
    if image_list:
        names = [str(n).replace(os.sep, "/") for n in image_list]
        for n in names:
            if not (Path(image_path) / n).is_file():
                raise ValueError(f"image_list: {n} does not exist below {image_path}")
        return names
    out = []
    for root, _, files in os.walk(image_path):
        for f in files:
            if Path(f).suffix.lower() in IMAGE_EXTENSIONS:
                out.append(os.path.relpath(os.path.join(root, f), image_path).replace(os.sep, "/"))
    return sorted(out)


def _assign_cameras(names, sizes, camera_mode) -> list[int]:
    """Camera index (0, 1, ...) of every image, in list order (COLMAP's ImageReader, restated in DESIGN.md 10.9):
    SINGLE one camera (every image must have the first one's size), PER_IMAGE one each, PER_FOLDER a new one with each
    new folder, AUTO a new one whenever the size differs from the previous camera's."""
    mode = _pycolmap.CameraMode(camera_mode) if isinstance(camera_mode, str) else camera_mode
    out, cams = [], []  # cams: (folder, size) of each camera
    for name, size in zip(names, sizes):
        folder = name.rsplit("/", 1)[0] if "/" in name else ""
        if not cams:
            new = True
        elif mode == _pycolmap.CameraMode.SINGLE:
            if size != cams[0][1]:
                raise ValueError(f"{name}: camera_mode SINGLE needs images of one size; {size} differs from {cams[0][1]}")
            new = False
        elif mode == _pycolmap.CameraMode.PER_IMAGE:
            new = True
        elif mode == _pycolmap.CameraMode.PER_FOLDER:
            new = folder != cams[-1][0]
        else:
            new = size != cams[-1][1]
        if new:
            cams.append((folder, size))
        out.append(len(cams) - 1)
    return out


def _make_camera(model: str, width: int, height: int, reader_options) -> "_pycolmap.Camera":
    if reader_options.camera_params:
        params = [float(v) for v in reader_options.camera_params.replace(" ", "").split(",") if v]
        return _pycolmap.Camera(model, width, height, params, has_prior_focal_length=False)
    f = reader_options.default_focal_length_factor * max(width, height)
    return _pycolmap.Camera.create(0xFFFFFFFF, model, f, width, height)


def keypoints_to_affine(kp: np.ndarray, sx: float = 1.0, sy: float = 1.0) -> np.ndarray:
    """N x 4 (x, y, scale, orientation) -> COLMAP's N x 6 (x, y, a11, a12, a21, a22) = (x, y, s cos, -s sin, s sin,
    s cos), rescaled to the original image by (sx, sy) as COLMAP's ScaleKeypoints does."""
    x, y, s, t = (kp[:, i].astype(np.float64) for i in range(4))
    c, n = s * np.cos(t), s * np.sin(t)
    return np.stack([x * sx, y * sy, c * sx, -n * sx, n * sy, c * sy], axis=1).astype(np.float32)


# ---- the pipeline -----------------------------------------------------------------------------------------------------
def extract_features(database_path, image_path, image_list=None, camera_mode=None, camera_model="SIMPLE_RADIAL",
                     reader_options=None, sift_options=None, device=None):
    """Extract SIFT features of the images below `image_path` into a new database at `database_path`."""
    t_all = time.perf_counter()
    database_path, image_path = os.fspath(database_path), os.fspath(image_path)
    camera_mode = _pycolmap.CameraMode.AUTO if camera_mode is None else camera_mode
    camera_mode = _pycolmap.CameraMode(camera_mode) if isinstance(camera_mode, str) else camera_mode
    reader_options = _pycolmap.ImageReaderOptions(reader_options) if isinstance(reader_options, dict) else \
        (reader_options or _pycolmap.ImageReaderOptions())
    sift_options = _pycolmap.SiftExtractionOptions(sift_options) if isinstance(sift_options, dict) else \
        (sift_options or _pycolmap.SiftExtractionOptions())
    _pycolmap.Sift(sift_options, _pycolmap.Device.auto if device is None else device)  # option and device checks
    if os.path.exists(database_path):
        raise ValueError(f"{database_path} already exists.")
    if not database_path.endswith(".db"):
        raise ValueError(f"{database_path} does not have the extension .db")
    if not os.path.isdir(image_path):
        raise ValueError(f"{image_path} is not a directory")
    for name in ("mask_path", "camera_mask_path"):
        if getattr(reader_options, name):
            raise ValueError(f"ImageReaderOptions.{name} is not supported by pycolmap_amd's extract_features")
    if reader_options.existing_camera_id != -1:
        raise ValueError("ImageReaderOptions.existing_camera_id is not supported by pycolmap_amd's extract_features")
    try:
        _pycolmap.Camera.create(0, camera_model, 1.0, 2, 2)
    except Exception as e:  # noqa: BLE001
        raise ValueError(f"Invalid camera model: {camera_model} ({e})") from None

    names = _image_list(image_path, image_list)
    max_size = int(sift_options.max_image_size)

    def decode(name):
        img = read_image_grey(str(Path(image_path) / name))
        h, w = img.shape
        small = downscale(img, max_size) if max(w, h) > max_size else img
        return (w, h), small

    t = time.perf_counter()
    with ThreadPoolExecutor(max_workers=max(1, min(MAX_DECODE_THREADS, len(names)))) as pool:
        decoded = list(pool.map(decode, names))
    decode_ms = (time.perf_counter() - t) * 1e3
    cam_of = _assign_cameras(names, [d[0] for d in decoded], camera_mode)

    opts = dict(first_octave=sift_options.first_octave, num_octaves=sift_options.num_octaves,
                octave_resolution=sift_options.octave_resolution, peak_threshold=sift_options.peak_threshold,
                edge_threshold=sift_options.edge_threshold, max_num_orientations=sift_options.max_num_orientations,
                upright=bool(sift_options.upright), normalization=int(sift_options.normalization),
                max_num_features=sift_options.max_num_features, max_image_size=max_size)
    gpu = sift_options.gpu_index.split(",")[0]
    features, device_ms = [None] * len(names), 0.0
    t = time.perf_counter()
    with _capi.Context(max(0, int(gpu))) as ctx:
        i = 0
        while i < len(names):  # batches bounded by input pixels
            j, px = i, 0
            while j < len(names) and (j == i or px + decoded[j][1].size <= BATCH_PIXELS):
                px += decoded[j][1].size
                j += 1
            out, st = ctx.sift_extract([decoded[k][1] for k in range(i, j)], **opts)
            device_ms += st["device_ms"]
            features[i:j] = out
            i = j
    extract_ms = (time.perf_counter() - t) * 1e3

    t = time.perf_counter()
    db = _pycolmap.Database(database_path)
    nfeat = 0
    try:
        with _pycolmap.DatabaseTransaction(db):
            cam_ids = {}
            for k, name in enumerate(names):
                (w, h), small = decoded[k]
                if cam_of[k] not in cam_ids:
                    cam_ids[cam_of[k]] = db.write_camera(_make_camera(camera_model, w, h, reader_options))
                image_id = db.write_image(_pycolmap.Image(name=name, camera_id=cam_ids[cam_of[k]]))
                kp, desc = features[k]
                sx, sy = w / small.shape[1], h / small.shape[0]
                if sx != 1.0 or sy != 1.0:  # back to the original pixels (COLMAP's ScaleKeypoints): x + 0.5 scales too
                    kp6 = keypoints_to_affine(kp, sx, sy)
                else:
                    kp6 = keypoints_to_affine(kp)
                db.write_keypoints(image_id, kp6)
                db.write_descriptors(image_id, desc)
                nfeat += len(kp)
    finally:
        db.close()
    sqlite_ms = (time.perf_counter() - t) * 1e3
    _pycolmap._last_stats = {"images": len(names), "features": nfeat, "decode_ms": decode_ms,
                             "extract_call_ms": extract_ms, "device_ms": device_ms, "sqlite_ms": sqlite_ms,
                             "total_ms": (time.perf_counter() - t_all) * 1e3}
