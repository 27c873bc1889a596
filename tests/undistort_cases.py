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


# ---- the edge list: targets given directly as PINHOLE tuples --------------------------------------------
def pinhole(width: int, height: int, fx: float, fy: float, cx: float, cy: float):
    return (1, int(width), int(height), np.array([fx, fy, cx, cy], dtype=np.float64))


def small_camera(model: str, width: int, height: int):
    """A source camera of any size: focal length = the longer side, principal point a quarter pixel off the centre,
    weak distortion (the point of these cases is the shape, not the model)."""
    f, cx, cy = float(max(width, height)), width / 2 + 0.25, height / 2 - 0.25
    params = {"PINHOLE": [f, f * 1.03125, cx, cy], "SIMPLE_RADIAL": [f, cx, cy, 0.03], "RADIAL": [f, cx, cy, -0.04, 0.01],
              "OPENCV": [f, f * 1.03125, cx, cy, -0.04, 0.01, 0.0005, -0.001]}[model]
    return camera(model, width, height, params)


def focal_count(model: str) -> int:
    return 1 if model in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE") else 2


def focal_and_principal_point(cam):
    p, nf = cam[3], focal_count(cam[0])
    return float(p[0]), float(p[nf - 1]), float(p[nf]), float(p[nf + 1])


def target_into(cam, dw: int, dh: int, frac: float = 0.83):
    """The PINHOLE dw x dh target whose pixel centres span the central `frac` of the bilinear lookup's valid range
    (14.3: xs in [0, W - 1)) of the image the warp reads: the source, or the dw x dh resized one when the pre-pass runs
    (14.4).  Stated for the source's pinhole part; weak distortion moves the pixels by less than the margin."""
    sw, sh = cam[1], cam[2]
    fx, fy, cx, cy = focal_and_principal_point(cam)
    ew, eh = (dw, dh) if dw * dh < sw * sh else (sw, sh)
    one_focal = focal_count(cam[0]) == 1
    out = []
    for e, s, d, f, c in ((ew, sw, dw, fx, cx), (eh, sh, dh, fy, cy)):
        z = frac * (e - 1) / max(d - 1, 1)  # read pixels per target pixel
        # Camera::Rescale: the principal point per axis, two focal lengths per axis, one by the mean of the two factors
        fe, ce = f * ((ew / sw + eh / sh) / 2 if one_focal else e / s), c * e / s
        out.append((fe / z if z > 0 else fe, d / 2 - (e / 2 - ce) / z if z > 0 else d / 2))
    return pinhole(dw, dh, out[0][0], out[1][0], out[0][1], out[1][1])


GROUP_TAILS = [(3, 3), (3, 2), (5, 2), (5, 3), (2, 2), (4, 2)]           # pixel count mod 4 = 1, 2, 2, 3, 0, 0
NARROW = [((1, 9), (2, 4)), ((2, 9), (3, 5)), ((3, 7), (4, 5)), ((5, 5), (4, 6))]  # (target, a source with fewer pixels)
BLACK = [(1, 1), (3, 1), (1, 3), (1, 9)]
# (target, channels): 63 | 64 | 65 and 255 | 256 | 257 groups of four pixels, the "+1" counts with a one-pixel tail
WARP_BOUNDARIES = [((63, 4), 1), ((11, 23), 3), ((64, 4), 1), ((65, 4), 1), ((255, 4), 1), ((256, 4), 1), ((41, 25), 3),
                   ((257, 4), 1)]
WARP_LINES = [(257, 1), (1021, 1)]  # prime pixel counts: one row
# (name, source w x h, target w x h, channels): first-pass samples dw * sh and second-pass samples dw * dh on 255 | 256 | 257
RESIZE_BOUNDARIES = [("first-255", (40, 51), (5, 7), 3), ("first-256", (30, 32), (8, 5), 1), ("first-257", (600, 1), (257, 2), 1),
                     ("second-255", (67, 45), (51, 5), 1), ("second-256", (67, 45), (32, 8), 3), ("second-257", (20, 30), (1, 257), 1)]
# (source w x h, target w x h, channels): the per-axis (in -> out) pairs of WINDOW_PAIRS, each on x and on y
WINDOWS = [((1000, 3), (3, 3), 1), ((3, 1000), (3, 3), 1), ((300, 4), (7, 4), 3), ((4, 300), (4, 7), 1),
           ((257, 3), (1, 3), 1), ((3, 257), (3, 1), 3), ((64, 3), (1, 3), 3), ((3, 64), (3, 1), 1),
           ((64, 5), (16, 5), 1), ((5, 64), (5, 16), 3), ((64, 5), (32, 5), 3), ((5, 64), (5, 32), 1),
           ((64, 5), (63, 5), 1), ((5, 64), (5, 63), 3), ((67, 45), (22, 15), 3), ((45, 67), (15, 22), 1),
           ((7, 300), (100, 2), 1), ((300, 7), (2, 100), 3)]
WINDOW_PAIRS = [(1000, 3), (300, 7), (300, 2), (257, 1), (64, 1), (64, 16), (64, 32), (64, 63), (67, 22), (45, 15), (7, 100)]
HUGE_FOCALS = [1e-160, 1e-150]  # u = k / f: u * u overflows for the first, not for the second
HUGE_TARGETS = [(21, 15), (70, 75)]  # with and without the pre-pass on W x H
POLYNOMIAL = ("SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV")
DYADIC = ("PINHOLE", W, H, np.array([64.0, 64.0, 33.5, 22.5]))  # every coordinate of the (g) cases is exact
# seeds by channel count of the (g) pre-pass images: the first from 7000 for which no visible sample of a clipped window
# (weights in 28ths, rounded in FP64) is an exact tie, so that integer arithmetic pins every byte (int_resize)
PREPASS_SEEDS = {1: 7000, 3: 8197}


def edge_cases():
    """[(name, image, source camera, target camera)]: DESIGN.md 14.6's edge list.  The name's first field is the class
    (a .. k of the list there); "black" in a name says that no target pixel can be inside."""
    out = []
    seed = iter(range(1000, 2000))

    def add(name, img, cam, dst):
        out.append((name, img, cam, dst))

    def img_for(cam, ch):
        return make_image(cam[2], cam[1], ch, next(seed))

    # a. group tails: with a 2 x 3 source (no pre-pass; 2 x 2 for the 2 x 2 target) and through the pre-pass
    for (dw, dh) in GROUP_TAILS:
        for ch in (1, 3):
            sw, sh = (2, 2) if dw * dh < 6 else (2, 3)
            cam = small_camera("PINHOLE" if ch == 1 else "SIMPLE_RADIAL", sw, sh)
            add(f"a-tail-{dw}x{dh}-{ch}ch", img_for(cam, ch), cam, target_into(cam, dw, dh))
            cam = camera("RADIAL" if ch == 1 else "OPENCV")
            add(f"a-tail-{dw}x{dh}-{ch}ch-prepass", img_for(cam, ch), cam, target_into(cam, dw, dh))
    # b. narrow targets: a group spans 4, 2, 2 and 1 to 2 rows; the all-black ones
    for (dw, dh), (sw, sh) in NARROW:
        for ch in (1, 3):
            cam = small_camera("SIMPLE_RADIAL" if ch == 1 else "PINHOLE", sw, sh)
            add(f"b-narrow-{dw}x{dh}-{ch}ch", img_for(cam, ch), cam, target_into(cam, dw, dh))
    for i, (dw, dh) in enumerate(BLACK):
        ch = 3 if i % 2 else 1
        cam = camera("OPENCV")
        add(f"b-black-{dw}x{dh}-{ch}ch", img_for(cam, ch), cam, target_into(cam, dw, dh))
    # c. wave and block boundaries of the warp (no pre-pass: a 12 x 9 source), and the two prime counts as one row:
    # black through the pre-pass of W x H (the resized source is one row), with pixels from a 16 x 9 source
    for (dw, dh), ch in WARP_BOUNDARIES:
        cam = small_camera("RADIAL", 12, 9)
        add(f"c-warp-{dw * dh}-{dw}x{dh}-{ch}ch", img_for(cam, ch), cam, target_into(cam, dw, dh))
    for (dw, dh) in WARP_LINES:
        cam = camera("RADIAL")
        add(f"c-warp-{dw * dh}-{dw}x{dh}-3ch-black", img_for(cam, 3), cam, target_into(cam, dw, dh))
        cam = small_camera("OPENCV", 16, 9)
        add(f"c-warp-{dw * dh}-{dw}x{dh}-3ch-line", img_for(cam, 3), cam, target_into(cam, dw, dh))
    # d. block boundaries of the two resize kernels
    for name, (sw, sh), (dw, dh), ch in RESIZE_BOUNDARIES:
        cam = camera("OPENCV") if (sw, sh) == (W, H) else small_camera("SIMPLE_RADIAL", sw, sh)
        add(f"d-{name}-{sw}x{sh}-to-{dw}x{dh}-{ch}ch" + ("-black" if min(dw, dh) == 1 else ""), img_for(cam, ch), cam,
            target_into(cam, dw, dh))
    # e. windows
    for (sw, sh), (dw, dh), ch in WINDOWS:
        cam = camera("RADIAL") if (sw, sh) == (W, H) else small_camera("PINHOLE" if ch == 1 else "SIMPLE_RADIAL", sw, sh)
        add(f"e-window-{sw}x{sh}-to-{dw}x{dh}-{ch}ch" + ("-black" if min(dw, dh) == 1 else ""), img_for(cam, ch), cam,
            target_into(cam, dw, dh))
    # f. every model through a pre-pass that enlarges x and reduces y
    for i, model in enumerate(CAMERAS):
        cam = camera(model)
        fx, fy, cx, cy = focal_and_principal_point(cam)
        add(f"f-mixed-{model}-{1 + 2 * (i % 2)}ch", img_for(cam, 1 + 2 * (i % 2)), cam,
            pinhole(100, 9, fx * 100 / W, fy * 9 / H, cx * 100 / W, cy * 9 / H))
    # g. dyadic known answers (known_answers() states them in integer arithmetic)
    for ch in (1, 3):
        add(f"g-identity-{ch}ch", img_for(DYADIC, ch), DYADIC, pinhole(W, H, 64.0, 64.0, 33.5, 22.5))
    add("g-halfx-1ch", img_for(DYADIC, 1), DYADIC, pinhole(W, H, 64.0, 64.0, 33.0, 22.5))
    add("g-halfy-3ch", img_for(DYADIC, 3), DYADIC, pinhole(W, H, 64.0, 64.0, 33.5, 22.0))
    add("g-halfxy-1ch", img_for(DYADIC, 1), DYADIC, pinhole(W, H, 64.0, 64.0, 33.0, 22.0))
    add("g-mirror-3ch", img_for(DYADIC, 3), DYADIC, pinhole(W, H, -64.0, 64.0, 32.5, 22.5))
    for ch in (1, 3):
        cam = ("PINHOLE", 64, 48, np.array([64.0, 64.0, 32.5, 24.5]))
        add(f"g-prepass-{ch}ch", make_image(48, 64, ch, PREPASS_SEEDS[ch]), cam, pinhole(16, 12, 16.0, 16.0, 8.125, 6.125))
    # h. coordinates that are not finite, or huge; the principal point on the centre of pixel (10, 7)
    for i, model in enumerate(CAMERAS):
        for f in HUGE_FOCALS:
            for (dw, dh) in HUGE_TARGETS:
                ch = 1 + 2 * ((i + (dw > 21)) % 2)
                cam = camera(model)
                add(f"h-huge-{model}-{f:g}-{dw}x{dh}-{ch}ch", img_for(cam, ch), cam, pinhole(dw, dh, f, f, 10.5, 7.5))
    # i. camera branches: r = 0 of the fisheye family on a pixel centre, FOV's small-omega and small-radius branches
    for i, model in enumerate(("OPENCV_FISHEYE", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE")):
        cam = camera(model)
        add(f"i-centre-{model}-{1 + 2 * (i % 2)}ch", img_for(cam, 1 + 2 * (i % 2)), cam, pinhole(21, 15, 8.0, 8.0, 10.5, 7.5))
    for omega in (1e-3, 0.0):
        cam = camera("FOV", params=[60.0, 59.0, 33.0, 22.5, omega])
        add(f"i-fov-omega-{omega:g}-3ch", img_for(cam, 3), cam, pinhole(70, 50, 62.0, 61.0, 35.5, 25.5))
    cam = camera("FOV")
    add("i-fov-small-radius-1ch", img_for(cam, 1), cam, pinhole(70, 50, 500.0, 500.0, 35.5, 25.5))
    # j. saturation
    for value in (255, 0):
        cam = camera("RADIAL")
        for (dw, dh) in ((130, 90), (30, 20)):
            add(f"j-all-{value}-{dw}x{dh}-3ch", np.full((H, W, 3), value, np.uint8), cam,
                pinhole(dw, dh, 58.0 * dw / W, 58.0 * dh / H, 33.25 * dw / W, 22.5 * dh / H))
    yy, xx = np.mgrid[0:64, 0:64]
    cam = small_camera("PINHOLE", 64, 64)
    add("j-checkerboard-64-to-63-1ch", (((xx + yy) % 2) * 255).astype(np.uint8), cam, target_into(cam, 63, 63))
    # k. input layouts
    cam = camera("OPENCV", W, 23, [60.0, 62.0, 33.0, 11.25, -0.2, 0.05, 0.001, -0.002])
    add("k-rows-subsampled-3ch", make_image(46, W, 3, next(seed))[::2], cam, target_into(cam, 70, 24))
    cam = camera("RADIAL")
    add("k-trailing-1-axis", make_image(H, W, 1, next(seed))[..., None], cam, target_into(cam, 40, 30))
    add("k-fortran-order-3ch", np.asfortranarray(make_image(H, W, 3, next(seed))), cam, target_into(cam, 75, 50))
    add("k-negative-row-stride-1ch", make_image(H, W, 1, next(seed))[::-1], cam, target_into(cam, 75, 50))
    return out


def round_half_up_div(n, d):
    """floor(n / d + 1 / 2) of non-negative integers."""
    return (2 * n + d) // (2 * d)


def int_axis_weights(n_in, n_out):
    """14.4 for a reduction by an even integer factor r = n_in / n_out, in integers: [(left, integer weights, their
    sum)] per output sample.  Centre r u + r / 2, window r u - r / 2 .. r u + r + r / 2 - 1 clipped to the image; the
    tent's weights at these half-integer offsets are the odd numbers 1 .. 2 r - 1 over 2 r^2.  An interior window sums
    to 2 r^2 (a power of two for r = 4: every product and sum is then exact in FP64); the clipped windows at the two
    ends sum to less."""
    r = n_in // n_out
    assert r * n_out == n_in and r >= 2 and r % 2 == 0
    out = []
    for u in range(n_out):
        left, right = max(0, r * u - r // 2), min(r * u + r + r // 2, n_in)
        w = [2 * r - abs(2 * i + 1 - (2 * u + 1) * r) for i in range(left, right)]
        assert all(k > 0 for k in w)
        out.append((left, w, sum(w)))
    return out


def int_resize(img, dw, dh):
    """14.4 in integer arithmetic for integer reduction factors: (the resized image, mask of the samples whose value
    depends on an exact tie of a window whose weight sum is no power of two; there the floating-point sum of the
    rounded weights may fall on either side)."""
    a = img.reshape(img.shape[0], img.shape[1], -1).astype(np.int64)
    doubt = np.zeros(a.shape, bool)
    for axis, n_out in ((1, dw), (0, dh)):
        a, doubt = np.moveaxis(a, axis, 0), np.moveaxis(doubt, axis, 0)
        res, dres = [], []
        for left, w, d in int_axis_weights(a.shape[0], n_out):
            n = sum(k * a[left + j] for j, k in enumerate(w))
            tie = (2 * (n % d) == d) & (d & (d - 1) != 0)
            res.append(round_half_up_div(n, d))
            dres.append(tie | doubt[left:left + len(w)].any(axis=0))
        a, doubt = np.moveaxis(np.stack(res), 0, axis), np.moveaxis(np.stack(dres), 0, axis)
    shape = (dh, dw) + img.shape[2:]
    return a.astype(np.uint8).reshape(shape), doubt.reshape(shape)


def known_answers():
    """{name: (expected image, mask of the pixels it pins)} of the (g) cases, in integer arithmetic from 14.3 and 14.4
    alone.  PINHOLE source fx = fy = 64, principal point on half-integers: s = (x + 0.5 + shift_x, y + 0.5 + shift_y)
    exactly, so x0 = x (+ dx = 1/2 when the target's cx is lower by 1/2) and, bottom-up, y0 = H - 1 - y (or H - 2 - y
    with dy = 1/2: the rows y and y + 1).  A two-pixel mean is n / 2, a four-pixel mean n / 4, rounded half up."""
    by = {c[0]: c for c in edge_cases()}
    out = {}

    def blank(shape):
        return np.zeros(shape, np.int64), np.ones(shape[:2], bool)

    for name, (_, img, _, _) in by.items():
        if not name.startswith("g-"):
            continue
        a = img.astype(np.int64)
        want, pinned = blank(a.shape)
        kind = name.split("-")[1]
        if kind == "identity":    # the input; the top row (y0 + 1 = H) and the last column (x0 + 1 = W) are outside
            want[1:, :-1] = a[1:, :-1]
        elif kind == "halfx":
            want[1:, :-1] = round_half_up_div(a[1:, :-1] + a[1:, 1:], 2)
        elif kind == "halfy":     # rows y and y + 1; the last row has y0 = -1, the top row is inside (y0 + 1 = H - 1)
            want[:-1, :-1] = round_half_up_div(a[:-1, :-1] + a[1:, :-1], 2)
        elif kind == "halfxy":
            want[:-1, :-1] = round_half_up_div(a[:-1, :-1] + a[:-1, 1:] + a[1:, :-1] + a[1:, 1:], 4)
        elif kind == "mirror":    # s.x = 65.5 - x: x0 = 65 - x = W - 2 - x with dx = 0; x = W - 1 has x0 = -1
            want[1:, :-1] = a[1:, -2::-1]
        elif kind == "prepass":   # the identity on the 16 x 12 resized image
            small, doubt = int_resize(img, 16, 12)
            want, pinned = blank(small.shape)
            want[1:, :-1] = small.astype(np.int64)[1:, :-1]
            pinned = ~doubt.reshape(12, 16, -1).any(axis=2)
            pinned[0], pinned[:, -1] = True, True
        out[name] = (want.astype(np.uint8), pinned)
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
