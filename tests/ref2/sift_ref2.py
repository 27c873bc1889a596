"""tests/ref2/sift_ref2.py — a SECOND, deliberately different restatement of the SIFT extractor, in float64 numpy /
scipy, written against DESIGN.md section 10.1 / 10.2, Lowe (IJCV 2004) and VLFeat's published documentation of its
conventions (bin centres, the descriptor's frame), and not against tests/sift_ref/sift_ref.cc or sift.hip.

TEST INFRASTRUCTURE ONLY (nothing under pycolmap_amd/ imports it).  Its job is to give the extractor's CPU reference
an independent pin: the GPU suite holds sift.hip to sift_ref.cc bit for bit, which says nothing about whether either
of them is SIFT.  tests/ref2/sift_compare.py measures the distance between the two restatements,
tests/ref2/sift_deviation_budget.json is the committed result, tests/test_sift_ref2_cpu.py / _gpu.py hold to it.

  what                     sift_ref.cc (and sift.hip)                         here
  -----------------------  -------------------------------------------------  --------------------------------------
  arithmetic               float32, one rounding per operation                float64
  blur                     tap loops, float taps, horizontal then vertical    scipy.ndimage.correlate1d, double taps
  gradients                per sample, at the gather                          numpy.gradient of the whole level, once
  extremum test            26 comparisons per pixel                           maximum / minimum over 26 shifted views
  refinement               3 x 3 elimination with partial pivoting            numpy.linalg.solve (LAPACK dgesv)
  histogram sums           64 lane partial sums + xor butterfly (D3)          numpy.bincount over the whole window
  sin / cos / 2^t          polynomials (10.2)                                 libm
  exp(-x), atan2           258-entry table, VLFeat's rational form (10.2)     the same two restated in float64
                                                                              (approx=True), or libm (approx=False)

The two approximations kept under `approx` are the ones whose error (1.5e-3, 0.008 rad) is large enough to move a
descriptor byte; with them restated the descriptors agree to one byte step, without them the distance is what the
approximations cost.

One rule of the project is behind a named option, as tests/ref2/variants.py does for the verification oracle:
`move_after_last_solve` (deviation S10: the refinement's move after its fifth solve).  The default follows the project,
the other setting follows Lowe; sift_compare.py records what the rule costs.

Coordinates inside the module are octave pixel indices (x to the right, y down); `extract` reports COLMAP's
(x * 2^o + 0.5, y * 2^o + 0.5, sigma * 2^o, angle in (-pi, pi]).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
from scipy.ndimage import correlate1d

TWO_PI = 2.0 * math.pi
FLT_EPSILON = 2.0 ** -23
NOMINAL_INPUT_SIGMA = 0.5
MIN_OCTAVE_SIDE = 8          # deviation S3
L1_ROOT, L2 = 0, 1

DEFAULTS = dict(first_octave=-1, num_octaves=4, octave_resolution=3, peak_threshold=0.02 / 3, edge_threshold=10.0,
                max_num_orientations=2, upright=False, normalization=L1_ROOT, max_num_features=8192)


# ------------------------------------------------------------------------------------------------
# 10.2: the two approximations that can move a byte, in float64
# ------------------------------------------------------------------------------------------------
_EXPN_STEP = 25.0 / 256.0
_EXPN_TABLE = np.exp(-np.arange(258) * _EXPN_STEP)


def expn_table(x):
    """exp(-x), x >= 0, by linear interpolation between the 258 samples exp(-k * 25 / 256); 0 beyond 25."""
    x = np.asarray(x, dtype=np.float64)
    t = np.minimum(x, 25.0) / _EXPN_STEP
    k = np.floor(t).astype(np.int64)
    val = _EXPN_TABLE[k] + (t - k) * (_EXPN_TABLE[k + 1] - _EXPN_TABLE[k])
    return np.where(x > 25.0, 0.0, val)


def atan2_rational(y, x):
    """VLFeat's published approximation: with r = (x - |y|) / (x + |y|) on the right half plane (mirrored on the left),
    angle = pi / 4 (or 3 pi / 4) + (c3 r^2 - c1) r, sign of y; |y| carries FLT_EPSILON so that (0, 0) is defined."""
    y = np.asarray(y, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    ay = np.abs(y) + FLT_EPSILON
    right = x >= 0.0
    r = np.where(right, (x - ay) / (x + ay), (x + ay) / (ay - x))
    a = np.where(right, 0.25 * math.pi, 0.75 * math.pi) + (0.1821 * r * r - 0.9675) * r
    return np.where(y < 0.0, -a, a)


def _expn(x, approx):
    return expn_table(x) if approx else np.exp(-np.asarray(x, dtype=np.float64))


# ------------------------------------------------------------------------------------------------
# scale space
# ------------------------------------------------------------------------------------------------
def sigma0_of(S: int) -> float:
    return 1.6 * 2.0 ** (1.0 / S)


def level_sigma(s, S: int) -> float:
    """absolute blur of level s (-1 .. S + 1) in octave pixels"""
    return sigma0_of(S) * 2.0 ** (s / S)


def gaussian_taps(sigma: float) -> np.ndarray:
    r = int(math.ceil(4.0 * sigma))
    g = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    return g / g.sum()


def gaussian_blur(img: np.ndarray, sigma: float) -> np.ndarray:
    g = gaussian_taps(sigma)
    return correlate1d(correlate1d(img, g, axis=1, mode="nearest"), g, axis=0, mode="nearest")


def octave_base(image01: np.ndarray, o: int) -> np.ndarray:
    """The input (already v / 255) sampled at octave o: o = -1 doubles it (even pixels copy, odd ones the mean of their
    two or four neighbours, the last row / column replicated), o > 0 keeps every 2^o-th pixel."""
    a = np.asarray(image01, dtype=np.float64)
    h, w = a.shape
    if o < 0:
        assert o == -1
        p = np.pad(a, ((0, 1), (0, 1)), mode="edge")
        up = np.empty((2 * h, 2 * w))
        up[0::2, 0::2] = a
        up[0::2, 1::2] = 0.5 * (p[:-1, :-1] + p[:-1, 1:])
        up[1::2, 0::2] = 0.5 * (p[:-1, :-1] + p[1:, :-1])
        up[1::2, 1::2] = 0.25 * (p[:-1, :-1] + p[:-1, 1:] + p[1:, :-1] + p[1:, 1:])
        return up
    return a[::1 << o, ::1 << o][:h >> o, :w >> o].copy()


def octave_levels(first: np.ndarray, S: int, sigma_in: float | None = None) -> np.ndarray:
    """The S + 3 Gaussian levels s = -1 .. S + 1 of one octave as an (S + 3, h, w) array.  `first` is level -1 itself
    (sigma_in None: the next octave's base), or an image of blur sigma_in that is first brought to level -1's sigma."""
    L = np.asarray(first, dtype=np.float64)
    if sigma_in is not None:
        target = level_sigma(-1, S)
        if target > sigma_in:
            L = gaussian_blur(L, math.sqrt(target * target - sigma_in * sigma_in))
    levels = [L]
    for s in range(0, S + 2):       # level s from s - 1: the blurs add in quadrature
        a, b = level_sigma(s, S), level_sigma(s - 1, S)
        levels.append(gaussian_blur(levels[-1], math.sqrt(a * a - b * b)))
    return np.stack(levels)


def scale_space(image: np.ndarray, first_octave: int = -1, num_octaves: int = 4, S: int = 3,
                input_sigma: float = NOMINAL_INPUT_SIGMA, scale: float = 1.0 / 255.0):
    """[(o, levels)] for the octaves that are processed.  `image` is multiplied by `scale` (8-bit input: 1 / 255)."""
    img = np.asarray(image, dtype=np.float64) * scale
    h, w = img.shape
    out = []
    for o in range(first_octave, first_octave + num_octaves):
        ho, wo = (h << -o, w << -o) if o < 0 else (h >> o, w >> o)
        if min(ho, wo) < MIN_OCTAVE_SIDE:
            break
        if not out:
            levels = octave_levels(octave_base(img, o), S, sigma_in=input_sigma * 2.0 ** (-o))
        else:
            levels = octave_levels(out[-1][1][S, ::2, ::2][:ho, :wo], S)   # level s = S - 1: twice level -1's sigma
        out.append((o, levels))
    return out


# ------------------------------------------------------------------------------------------------
# detection and refinement
# ------------------------------------------------------------------------------------------------
@dataclass
class Keypoint:
    x: float          # octave pixels
    y: float
    s: float          # refined level
    sigma: float      # octave pixels
    level: int        # index into the octave's levels of the Gaussian whose gradients describe it (DoG level + 1)


def extrema(dog: np.ndarray, S: int, peak_threshold: float) -> np.ndarray:
    """(n, 3) integer (DoG index, y, x) of the strict 26-neighbour extrema with |v| >= 0.8 tp, over DoG levels
    s = 0 .. S - 1 (indices 1 .. S of the S + 2 DoGs) and pixels 1 .. w - 2, 1 .. h - 2, in (level, y, x) order."""
    n, h, w = dog.shape
    found = []
    for d in range(1, S + 1):
        centre = dog[d, 1:-1, 1:-1]
        views = [dog[d + k, 1 + j:h - 1 + j, 1 + i:w - 1 + i]
                 for k in (-1, 0, 1) for j in (-1, 0, 1) for i in (-1, 0, 1) if (k, j, i) != (0, 0, 0)]
        hi = np.maximum.reduce(views)
        lo = np.minimum.reduce(views)
        hit = ((centre >= 0.8 * peak_threshold) & (centre > hi)) | ((centre <= -0.8 * peak_threshold) & (centre < lo))
        yx = np.argwhere(hit)
        found.append(np.column_stack([np.full(len(yx), d), yx + 1]))
    return np.concatenate(found).astype(np.int64) if found else np.zeros((0, 3), np.int64)


def _taylor(dog, d, y, x):
    """value, gradient and Hessian (x, y, s order) of the DoG at an interior sample, by central differences"""
    c = dog[d - 1:d + 2, y - 1:y + 2, x - 1:x + 2]
    v = c[1, 1, 1]
    g = 0.5 * np.array([c[1, 1, 2] - c[1, 1, 0], c[1, 2, 1] - c[1, 0, 1], c[2, 1, 1] - c[0, 1, 1]])
    dxx = c[1, 1, 2] + c[1, 1, 0] - 2 * v
    dyy = c[1, 2, 1] + c[1, 0, 1] - 2 * v
    dss = c[2, 1, 1] + c[0, 1, 1] - 2 * v
    dxy = 0.25 * (c[1, 2, 2] + c[1, 0, 0] - c[1, 2, 0] - c[1, 0, 2])
    dxs = 0.25 * (c[2, 1, 2] + c[0, 1, 0] - c[0, 1, 2] - c[2, 1, 0])
    dys = 0.25 * (c[2, 2, 1] + c[0, 0, 1] - c[0, 2, 1] - c[2, 0, 1])
    return v, g, np.array([[dxx, dxy, dxs], [dxy, dyy, dys], [dxs, dys, dss]])


def refine(dog: np.ndarray, S: int, d: int, y: int, x: int, peak_threshold: float, edge_threshold: float,
           move_after_last_solve: bool = True):
    """Lowe's sub-pixel fit of one extremum: up to five Newton solves, the sample moving by one pixel in x / y between
    them while the offset exceeds 0.6 (never onto the border), then the contrast, edge and range tests.

    move_after_last_solve (deviation S10): the project moves the sample after the fifth solve as well
    and reports the offset of that solve about the new sample (the default here, so that the comparison measures
    everything else).  False is Lowe's reading (2004, section 4: "the interpolation [is] performed about that point"):
    the fit is reported about the sample it was solved at.  A Keypoint, or None."""
    _, h, w = dog.shape
    for solves_left in range(4, -1, -1):
        _, g, H = _taylor(dog, d, y, x)
        try:
            b = np.linalg.solve(H, -g)
        except np.linalg.LinAlgError:
            b = np.zeros(3)
        if not np.all(np.isfinite(b)):
            b = np.zeros(3)
        mx = (1 if b[0] > 0.6 and x < w - 2 else 0) - (1 if b[0] < -0.6 and x > 1 else 0)
        my = (1 if b[1] > 0.6 and y < h - 2 else 0) - (1 if b[1] < -0.6 and y > 1 else 0)
        if (mx == 0 and my == 0) or (solves_left == 0 and not move_after_last_solve):
            break
        x, y = x + mx, y + my
    value = dog[d, y, x] + 0.5 * float(g @ b)
    tr, det = H[0, 0] + H[1, 1], H[0, 0] * H[1, 1] - H[0, 1] * H[0, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        edge = np.float64(tr * tr) / np.float64(det)
    xr, yr, sr = x + b[0], y + b[1], (d - 1) + b[2]
    ok = (abs(value) > peak_threshold and 0.0 <= edge < (edge_threshold + 1.0) ** 2 / edge_threshold
          and np.all(np.abs(b) < 1.5) and 0.0 <= xr <= w - 1 and 0.0 <= yr <= h - 1 and -1.0 <= sr <= S + 1)
    if not ok:
        return None
    return Keypoint(float(xr), float(yr), float(sr), sigma0_of(S) * 2.0 ** (sr / S), d)


def detect(levels: np.ndarray, S: int, peak_threshold: float, edge_threshold: float,
           move_after_last_solve: bool = True) -> list[Keypoint]:
    """The detected and refined keypoints of one octave, in (DoG level, y, x of the detected pixel) order."""
    dog = np.diff(levels, axis=0)
    kps = (refine(dog, S, int(d), int(y), int(x), peak_threshold, edge_threshold, move_after_last_solve)
           for d, y, x in extrema(dog, S, peak_threshold))
    return [k for k in kps if k is not None]


# ------------------------------------------------------------------------------------------------
# gradients, orientation, descriptor
# ------------------------------------------------------------------------------------------------
def gradient_field(level: np.ndarray, approx: bool = True):
    """(magnitude, angle in [0, 2 pi)) of one Gaussian level: central differences, one-sided on the border."""
    gy, gx = np.gradient(np.asarray(level, dtype=np.float64))
    ang = atan2_rational(gy, gx) if approx else np.arctan2(gy, gx)
    return np.hypot(gx, gy), np.mod(ang, TWO_PI)


def _window(centre: float, radius: int, lo: int, hi: int):
    """integer samples round(centre) - radius .. round(centre) + radius clipped to lo .. hi, and their offsets"""
    c = int(math.floor(centre + 0.5))
    idx = np.arange(max(c - radius, lo), min(c + radius, hi) + 1)
    return idx, idx - centre


def orientation_histogram(field, x: float, y: float, sigma: float, approx: bool = True) -> np.ndarray:
    """The 36-bin histogram (bin i centred at (i + 0.5) * 10 degrees) of gradient angles around (x, y): magnitudes
    weighted by a Gaussian of 1.5 sigma over the disc r^2 < W^2 + 0.6, W = max(floor(4.5 sigma), 1), each sample shared
    linearly between its two nearest bins; then six circular [1 1 1] / 3 smoothings."""
    mod, ang = field
    h, w = mod.shape
    sw = 1.5 * sigma
    W = max(int(math.floor(3.0 * sw)), 1)
    ys, dy = _window(y, W, 0, h - 1)
    xs, dx = _window(x, W, 0, w - 1)
    r2 = dx[None, :] ** 2 + dy[:, None] ** 2
    m, a = mod[np.ix_(ys, xs)], ang[np.ix_(ys, xs)]
    vote = np.where(r2 < W * W + 0.6, m * _expn(r2 / (2.0 * sw * sw), approx), 0.0).ravel()
    pos = (36.0 * a / TWO_PI - 0.5).ravel()
    low = np.floor(pos)
    frac = pos - low
    low = low.astype(np.int64)
    hist = (np.bincount(low % 36, vote * (1.0 - frac), 36) + np.bincount((low + 1) % 36, vote * frac, 36))
    for _ in range(6):
        hist = (np.roll(hist, 1) + hist + np.roll(hist, -1)) / 3.0
    return hist


def orientations(field, x: float, y: float, sigma: float, approx: bool = True) -> list[float]:
    """Up to four angles in [0, 2 pi), in bin order: the histogram's local maxima above 0.8 of its largest bin, each
    placed by the parabola through the bin and its two neighbours."""
    hist = orientation_histogram(field, x, y, sigma, approx)
    before, after = np.roll(hist, 1), np.roll(hist, -1)
    peaks = np.flatnonzero((hist > 0.8 * hist.max()) & (hist > before) & (hist > after))[:4]
    out = []
    for i in peaks:
        shift = -0.5 * (after[i] - before[i]) / (after[i] + before[i] - 2.0 * hist[i])
        out.append(TWO_PI * (i + shift + 0.5) / 36.0)
    return out


def raw_histogram(field, x: float, y: float, sigma: float, theta: float, approx: bool = True) -> np.ndarray:
    """The 128 bins of a feature before any normalisation, index t + 8 * bx + 32 * by (VLFeat's order): 4 x 4 spatial
    cells of 3 sigma pixels in the keypoint's frame (x axis along theta), 8 bins of the gradient angle relative to
    theta, every sample spread trilinearly over the 2 x 2 x 2 nearest bin centres and weighted by its magnitude and a
    Gaussian of two cells.  The window is floor(sqrt(2) * 3 sigma * 5 / 2 + 0.5) around the rounded centre and leaves
    the octave's border pixels out (VLFeat's rule: samples 1 .. w - 2, 1 .. h - 2)."""
    mod, ang = field
    h, w = mod.shape
    cell = 3.0 * sigma
    W = int(math.floor(math.sqrt(2.0) * cell * 2.5 + 0.5))
    ys, dy = _window(y, W, 1, h - 2)
    xs, dx = _window(x, W, 1, w - 2)
    hist = np.zeros(128)
    if len(xs) == 0 or len(ys) == 0:
        return hist
    c, s = math.cos(theta), math.sin(theta)
    u = (c * dx[None, :] + s * dy[:, None]) / cell          # cells along the keypoint's x axis
    v = (-s * dx[None, :] + c * dy[:, None]) / cell
    t = 8.0 * np.mod(ang[np.ix_(ys, xs)] - theta, TWO_PI) / TWO_PI
    mass = (mod[np.ix_(ys, xs)] * _expn((u * u + v * v) / 8.0, approx)).ravel()
    # bin centres: spatial at -1.5, -0.5, 0.5, 1.5 cells (indices 0 .. 3), angular at multiples of 45 degrees
    coords = [u.ravel() + 1.5, v.ravel() + 1.5, t.ravel()]
    low = [np.floor(q) for q in coords]
    frac = [q - l for q, l in zip(coords, low)]
    low = [l.astype(np.int64) for l in low]
    for corner in range(8):
        ku, kv, kt = corner & 1, (corner >> 1) & 1, corner >> 2
        bu, bv, bt = low[0] + ku, low[1] + kv, (low[2] + kt) % 8
        wgt = (mass * (frac[0] if ku else 1.0 - frac[0]) * (frac[1] if kv else 1.0 - frac[1])
               * (frac[2] if kt else 1.0 - frac[2]))
        inside = (bu >= 0) & (bu < 4) & (bv >= 0) & (bv < 4)
        hist += np.bincount((bt + 8 * bu + 32 * bv)[inside], wgt[inside], 128)
    return hist


def lowe_index() -> np.ndarray:
    """where VLFeat's bin t + 8 x + 32 y goes in Lowe's layout: y flipped, orientations reversed"""
    i = np.arange(128)
    t, x, y = i % 8, (i // 8) % 4, i // 32
    return (-t) % 8 + 8 * x + 32 * (3 - y)


def descriptor_bytes(hist: np.ndarray, normalization: int = L1_ROOT) -> np.ndarray:
    """128 byte values (int64) of a raw histogram: unit L2 norm, clamp at 0.2, unit L2 norm, Lowe's layout,
    sqrt(x / |x|_1) or x / |x|_2, min(255, round-half-up(512 x))."""
    d = np.asarray(hist, dtype=np.float64)
    d = d / (np.linalg.norm(d) + FLT_EPSILON)
    d = np.minimum(d, 0.2)
    d = d / (np.linalg.norm(d) + FLT_EPSILON)
    out = np.empty(128)
    out[lowe_index()] = d
    if normalization == L1_ROOT:
        total = np.abs(out).sum()
        out = np.sqrt(out / total) if total > 0 else out
    else:
        total = np.linalg.norm(out)
        out = out / total if total > 0 else out
    return np.minimum(255, np.floor(512.0 * out + 0.5)).astype(np.int64)


# ------------------------------------------------------------------------------------------------
# the extractor
# ------------------------------------------------------------------------------------------------
def extract(image: np.ndarray, approx: bool = True, move_after_last_solve: bool = True, **opts):
    """(N x 4 float64 keypoints (x, y, scale, orientation), N x 128 int64 byte values) of a 2-D 8-bit image, in the
    output order of section 10.1: octave, DoG level, y, x of the detected pixel, orientation.  `approx`: the exp table
    and the rational atan2 of 10.2, or libm; `move_after_last_solve`: the project's rule of deviation S10, or Lowe's."""
    unknown = set(opts) - set(DEFAULTS)
    if unknown:
        raise ValueError(f"unknown option {sorted(unknown)}")
    o_ = dict(DEFAULTS, **opts)
    S = int(o_["octave_resolution"])
    norm = {"L1_ROOT": L1_ROOT, "L2": L2}.get(o_["normalization"], o_["normalization"])
    per_octave = []              # (o, fields by level, [(keypoint, angle)])
    for o, levels in scale_space(image, int(o_["first_octave"]), int(o_["num_octaves"]), S):
        fields = {}
        feats = []
        for k in detect(levels, S, float(o_["peak_threshold"]), float(o_["edge_threshold"]), move_after_last_solve):
            if k.level not in fields:
                fields[k.level] = gradient_field(levels[k.level], approx)
            if o_["upright"]:
                angles = [0.0]
            else:
                angles = orientations(fields[k.level], k.x, k.y, k.sigma, approx)[:int(o_["max_num_orientations"])]
            feats += [(k, a) for a in angles]
        per_octave.append((o, fields, feats))
    limit = int(o_["max_num_features"])
    if limit >= 1:               # whole octaves from the coarsest down; the one that crosses the limit keeps its first
        room = limit
        for i in range(len(per_octave) - 1, -1, -1):
            o, fields, feats = per_octave[i]
            per_octave[i] = (o, fields, feats[:max(room, 0)])
            room -= len(feats)
    kp, desc = [], []
    for o, fields, feats in per_octave:
        unit = 2.0 ** o
        for k, a in feats:
            kp.append([k.x * unit + 0.5, k.y * unit + 0.5, k.sigma * unit, a - TWO_PI if a > math.pi else a])
            desc.append(descriptor_bytes(raw_histogram(fields[k.level], k.x, k.y, k.sigma, a, approx), norm))
    return (np.array(kp, dtype=np.float64).reshape(-1, 4), np.array(desc, dtype=np.int64).reshape(-1, 128))
