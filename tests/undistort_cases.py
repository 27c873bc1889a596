"""Shared inputs of the undistortion tests: the eleven cameras, seeded tiny images, the warp cases, and an independent
struct.pack writer / parser of COLMAP 3.9's sparse model files (it shares no code with csrc/host/model_io.cc)."""
from __future__ import annotations

import hashlib
import struct
from pathlib import Path

import numpy as np

W, H = 67, 45  # not a multiple of 4, 16 or 64

MODEL_IDS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4, "OPENCV_FISHEYE": 5,
             "FULL_OPENCV": 6, "FOV": 7, "SIMPLE_RADIAL_FISHEYE": 8, "RADIAL_FISHEYE": 9, "THIN_PRISM_FISHEYE": 10}
MODEL_NAMES = {v: k for k, v in MODEL_IDS.items()}
NUM_PARAMS = [3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12]

# one camera per model on the W x H sensor, distortion strong enough to bend the borders by several pixels
CAMERAS = {
    "SIMPLE_PINHOLE": [58.0, 33.25, 22.5],
    "PINHOLE": [58.0, 61.0, 33.25, 22.5],
    "SIMPLE_RADIAL": [58.0, 33.25, 22.5, 0.21],
    "RADIAL": [58.0, 33.25, 22.5, -0.18, 0.04],
    "OPENCV": [60.0, 62.0, 33.0, 22.25, -0.2, 0.05, 0.001, -0.002],
    "OPENCV_FISHEYE": [40.0, 41.0, 33.5, 22.0, 0.1, 0.01, -0.002, 0.0005],
    "FULL_OPENCV": [60.0, 61.0, 33.0, 22.0, 0.12, -0.03, 0.001, 0.002, 0.004, 0.02, -0.01, 0.002],
    "FOV": [60.0, 59.0, 33.0, 22.5, 0.8],
    "SIMPLE_RADIAL_FISHEYE": [42.0, 33.5, 22.5, 0.05],
    "RADIAL_FISHEYE": [42.0, 33.5, 22.5, -0.04, 0.006],
    "THIN_PRISM_FISHEYE": [50.0, 51.0, 33.0, 22.0, 0.1, 0.01, 0.001, 0.001, 0.001, 0.0, 0.001, 0.001],
}


def camera(model: str, width: int = W, height: int = H, params=None):
    return (model, width, height, np.array(CAMERAS[model] if params is None else params, dtype=np.float64))


def make_image(height: int, width: int, channels: int, seed: int) -> np.ndarray:
    """A seeded image: a smooth ramp (so that interpolation weights matter) plus noise (so that a wrong neighbour
    shows).  channels 1 -> H x W, 3 -> H x W x 3."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    planes = []
    for c in range(channels):
        ramp = (xx * (3 + c) + yy * (5 - c)) % 200
        planes.append(np.clip(ramp + rng.integers(0, 56, size=(height, width)), 0, 255))
    a = np.stack(planes, axis=-1).astype(np.uint8)
    return a[..., 0].copy() if channels == 1 else a


def warp_cases():
    """[(name, image, source camera, undistort options)]: DESIGN.md 14.6's list.  Every model at the W x H size with
    default options (one or three channels in turn) and with the largest target (max_scale 2, blank_pixels 1); the 2 x 2
    bilinear minimum; a row stride above the row length; a forced pre-pass; a strong fisheye; a ROI."""
    out = []
    for i, model in enumerate(CAMERAS):
        ch = 3 if i % 2 else 1
        out.append((f"{model}-default-{ch}ch", make_image(H, W, ch, 100 + i), camera(model), {}))
        out.append((f"{model}-large-{4 - ch}ch", make_image(H, W, 4 - ch, 200 + i), camera(model),
                    dict(max_scale=2.0, blank_pixels=1.0)))
    out.append(("PINHOLE-2x2", make_image(2, 2, 1, 300), camera("PINHOLE", 2, 2, [2.0, 2.0, 1.0, 1.0]), {}))
    out.append(("SIMPLE_RADIAL-2x2-3ch", make_image(2, 2, 3, 301), camera("SIMPLE_RADIAL", 2, 2, [2.0, 1.0, 1.0, 0.05]),
                dict(blank_pixels=1.0)))
    wide = make_image(H, W + 13, 3, 302)
    out.append(("OPENCV-stride-3ch", wide[:, :W], camera("OPENCV"), {}))
    wide1 = make_image(H, W + 5, 1, 303)
    out.append(("RADIAL-stride-1ch", wide1[:, 3:W + 3], camera("RADIAL"), dict(blank_pixels=0.5)))
    out.append(("OPENCV-max_image_size-3ch", make_image(H, W, 3, 304), camera("OPENCV"), dict(max_image_size=30)))
    out.append(("FOV-max_image_size-1ch", make_image(H, W, 1, 305), camera("FOV"), dict(max_image_size=41)))
    out.append(("OPENCV_FISHEYE-strong-3ch", make_image(H, W, 3, 306),
                camera("OPENCV_FISHEYE", params=[20.0, 21.0, 33.5, 22.0, 0.3, 0.05, -0.01, 0.002]),
                dict(blank_pixels=1.0, max_scale=2.0)))
    out.append(("THIN_PRISM_FISHEYE-strong-1ch", make_image(H, W, 1, 307),
                camera("THIN_PRISM_FISHEYE", params=[18.0, 18.0, 33.0, 22.0, 0.2, 0.02, 0.002, 0.001, 0.003, 0.0, 0.002, 0.001]),
                dict(blank_pixels=1.0, max_scale=2.0)))
    out.append(("RADIAL-roi-3ch", make_image(H, W, 3, 308), camera("RADIAL"),
                dict(roi_min_x=0.25, roi_min_y=0.1, roi_max_x=0.9, roi_max_y=0.75)))
    out.append(("PINHOLE-roi-1ch", make_image(H, W, 1, 309), camera("PINHOLE"), dict(roi_max_x=0.5, roi_min_y=0.5)))
    return out


def digest(a: np.ndarray) -> str:
    return hashlib.sha256(str(a.shape).encode() + np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- COLMAP 3.9 sparse model files, written and parsed here with struct alone -----------------------------------------
def tiny_model():
    """2 cameras (OPENCV, SIMPLE_RADIAL_FISHEYE), 3 images (one in a sub-folder), 12 points3D; points2D with and
    without a point3D.  cameras: {id: (model id, w, h, params)}; images: {id: (qvec wxyz, tvec, camera id, name,
    [(x, y, point3D id or -1)])}; points3D: {id: (xyz, rgb, error, [(image id, point2D idx)])}."""
    rng = np.random.default_rng(7)
    cameras = {1: (MODEL_IDS["OPENCV"], W, H, list(CAMERAS["OPENCV"])),
               3: (MODEL_IDS["SIMPLE_RADIAL_FISHEYE"], 52, 40, [36.0, 26.5, 19.75, 0.04])}
    names = {1: "a.ppm", 2: "sub/b.pgm", 5: "c.ppm"}
    cam_of = {1: 1, 2: 3, 5: 1}
    images, tracks = {}, {pid: [] for pid in range(10, 22)}
    for iid, name in names.items():
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        cw, chh = cameras[cam_of[iid]][1:3]
        pts = []
        for k in range(9):
            pid = -1 if k % 3 == 2 else int(10 + (k * 5 + iid) % 12)
            pts.append((float(rng.uniform(4, cw - 4)), float(rng.uniform(4, chh - 4)), pid))
            if pid >= 0:
                tracks[pid].append((iid, k))
        images[iid] = ([float(v) for v in q], [float(v) for v in rng.normal(size=3)], cam_of[iid], name, pts)
    points3D = {pid: ([float(v) for v in rng.normal(size=3)], [int(v) for v in rng.integers(0, 256, 3)],
                      float(rng.uniform(0, 2)), tracks[pid]) for pid in tracks}
    return cameras, images, points3D


def pinhole_model():
    """tiny_model() with both cameras PINHOLE: undistortion leaves it unchanged."""
    cameras, images, points3D = tiny_model()
    cameras = {1: (1, W, H, [58.0, 61.0, 33.25, 22.5]), 3: (1, 52, 40, [36.0, 37.0, 26.5, 19.75])}
    return cameras, images, points3D


def write_model_bin(path, cameras, images, points3D):
    path = Path(path)
    path.mkdir(parents=True, exist_ok=True)
    b = struct.pack("<Q", len(cameras))
    for cid, (mid, w, h, params) in cameras.items():
        b += struct.pack("<IiQQ", cid, mid, w, h) + struct.pack(f"<{len(params)}d", *params)
    (path / "cameras.bin").write_bytes(b)
    b = struct.pack("<Q", len(images))
    for iid, (q, t, cid, name, pts) in images.items():
        b += struct.pack("<I4d3dI", iid, *q, *t, cid) + name.encode() + b"\0" + struct.pack("<Q", len(pts))
        for x, y, pid in pts:
            b += struct.pack("<ddQ", x, y, pid if pid >= 0 else 0xFFFFFFFFFFFFFFFF)
    (path / "images.bin").write_bytes(b)
    b = struct.pack("<Q", len(points3D))
    for pid, (xyz, rgb, err, track) in points3D.items():
        b += struct.pack("<Q3d3BdQ", pid, *xyz, *rgb, err, len(track))
        for iid, idx in track:
            b += struct.pack("<II", iid, idx)
    (path / "points3D.bin").write_bytes(b)


def write_model_txt(path, cameras, images, points3D):
    path = Path(path)
    path.mkdir(parents=True, exist_ok=True)
    r = repr  # shortest round-trip decimal of a float
    lines = ["# Camera list with one line of data per camera:", f"# Number of cameras: {len(cameras)}"]
    for cid, (mid, w, h, params) in cameras.items():
        lines.append(" ".join([str(cid), MODEL_NAMES[mid], str(w), str(h)] + [r(float(p)) for p in params]))
    (path / "cameras.txt").write_text("\n".join(lines) + "\n")
    lines = ["# Image list with two lines of data per image:", f"# Number of images: {len(images)}"]
    for iid, (q, t, cid, name, pts) in images.items():
        lines.append(" ".join([str(iid)] + [r(v) for v in q] + [r(v) for v in t] + [str(cid), name]))
        lines.append(" ".join(f"{r(x)} {r(y)} {pid}" for x, y, pid in pts))
    (path / "images.txt").write_text("\n".join(lines) + "\n")
    lines = ["# 3D point list with one line of data per point:", f"# Number of points: {len(points3D)}"]
    for pid, (xyz, rgb, err, track) in points3D.items():
        lines.append(" ".join([str(pid)] + [r(v) for v in xyz] + [str(v) for v in rgb] + [r(err)] +
                              [f"{iid} {idx}" for iid, idx in track]))
    (path / "points3D.txt").write_text("\n".join(lines) + "\n")


def parse_model_bin(path):
    """The three .bin files back into tiny_model()'s form (dicts in file order)."""
    path = Path(path)
    d = (path / "cameras.bin").read_bytes()
    (n,), o = struct.unpack_from("<Q", d), 8
    cameras = {}
    for _ in range(n):
        cid, mid, w, h = struct.unpack_from("<IiQQ", d, o)
        o += 24
        k = NUM_PARAMS[mid]
        cameras[cid] = (mid, w, h, list(struct.unpack_from(f"<{k}d", d, o)))
        o += 8 * k
    assert o == len(d)
    d = (path / "images.bin").read_bytes()
    (n,), o = struct.unpack_from("<Q", d), 8
    images = {}
    for _ in range(n):
        v = struct.unpack_from("<I4d3dI", d, o)
        o += 64
        e = d.index(b"\0", o)
        name = d[o:e].decode()
        o = e + 1
        (m,) = struct.unpack_from("<Q", d, o)
        o += 8
        pts = []
        for _ in range(m):
            x, y, pid = struct.unpack_from("<ddQ", d, o)
            o += 24
            pts.append((x, y, -1 if pid == 0xFFFFFFFFFFFFFFFF else pid))
        images[v[0]] = (list(v[1:5]), list(v[5:8]), v[8], name, pts)
    assert o == len(d)
    d = (path / "points3D.bin").read_bytes()
    (n,), o = struct.unpack_from("<Q", d), 8
    points3D = {}
    for _ in range(n):
        v = struct.unpack_from("<Q3d3BdQ", d, o)
        o += 51
        track = [struct.unpack_from("<II", d, o + 8 * k) for k in range(v[8])]
        o += 8 * v[8]
        points3D[v[0]] = (list(v[1:4]), list(v[4:7]), v[7], track)
    assert o == len(d)
    return cameras, images, points3D


def write_pnm(path, a: np.ndarray):
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    head = (b"P5" if a.ndim == 2 else b"P6") + f"\n{a.shape[1]} {a.shape[0]}\n255\n".encode()
    path.write_bytes(head + np.ascontiguousarray(a).tobytes())


def read_pnm(path) -> np.ndarray:
    d = Path(path).read_bytes()
    magic, w, h, _ = d.split(None, 3)[:3] + [None]
    head = d.split(b"\n255\n", 1)[0] + b"\n255\n"
    ch = 1 if magic == b"P5" else 3
    a = np.frombuffer(d, np.uint8, offset=len(head))
    return a.reshape(int(h), int(w)) if ch == 1 else a.reshape(int(h), int(w), 3)
