"""Deterministic test images for the SIFT extractor: blurred noise (texture), raw noise, Gaussian blobs and a rendered
textured plane with views of it under known homographies."""
from __future__ import annotations

import numpy as np


def _blur(a: np.ndarray, sigma: float) -> np.ndarray:
    r = int(np.ceil(3 * sigma))
    g = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    g /= g.sum()
    a = np.apply_along_axis(lambda v: np.convolve(np.pad(v, r, mode="edge"), g, "valid"), 1, a)
    return np.apply_along_axis(lambda v: np.convolve(np.pad(v, r, mode="edge"), g, "valid"), 0, a)


def textured(seed: int, h: int, w: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    a = _blur(rng.random((h, w)), 2.0) * 0.6 + _blur(rng.random((h, w)), 6.0) * 1.4
    a = (a - a.min()) / max(a.max() - a.min(), 1e-9)
    return np.clip(a * 255.0 + 0.5, 0, 255).astype(np.uint8)


def noise(seed: int, h: int, w: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size=(h, w), dtype=np.uint8)


def blobs(h: int, w: int, spots, background: float = 30.0, amplitude: float = 200.0) -> np.ndarray:
    """Isotropic Gaussian blobs (x, y, sigma) in pixel-index coordinates."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.full((h, w), background)
    for x, y, s in spots:
        a += amplitude * np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2 * s * s))
    return np.clip(a + 0.5, 0, 255).astype(np.uint8)


def plane_texture(seed: int, size: int = 1024) -> np.ndarray:
    """A large float texture in [0, 1]: blurred noise at two scales plus random discs (corners and blobs)."""
    rng = np.random.default_rng(seed)
    a = _blur(rng.random((size, size)), 3.0) * 0.7 + _blur(rng.random((size, size)), 10.0) * 1.3
    yy, xx = np.mgrid[0:size, 0:size]
    for _ in range(160):
        cx, cy, r = rng.uniform(0, size), rng.uniform(0, size), rng.uniform(4, 22)
        a[(xx - cx) ** 2 + (yy - cy) ** 2 < r * r] += rng.uniform(-0.4, 0.4)
    return (a - a.min()) / (a.max() - a.min())


def render(tex: np.ndarray, H: np.ndarray, h: int, w: int) -> np.ndarray:
    """View of the texture: pixel (x, y) of the view shows texture point H^-1 (x, y) (pixel-index coordinates),
    bilinear, 8-bit."""
    Hi = np.linalg.inv(H)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    p = Hi @ np.stack([xx.ravel(), yy.ravel(), np.ones(xx.size)])
    u, v = p[0] / p[2], p[1] / p[2]
    u = np.clip(u, 0, tex.shape[1] - 1.001)
    v = np.clip(v, 0, tex.shape[0] - 1.001)
    u0, v0 = np.floor(u).astype(int), np.floor(v).astype(int)
    fu, fv = u - u0, v - v0
    val = (tex[v0, u0] * (1 - fu) * (1 - fv) + tex[v0, u0 + 1] * fu * (1 - fv) + tex[v0 + 1, u0] * (1 - fu) * fv
           + tex[v0 + 1, u0 + 1] * fu * fv)
    return np.clip(val.reshape(h, w) * 255.0 + 0.5, 0, 255).astype(np.uint8)


def similarity(angle_deg: float, scale: float, tx: float, ty: float, cx: float, cy: float) -> np.ndarray:
    """x' = s R (x - c) + c + t."""
    a = np.deg2rad(angle_deg)
    R = scale * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    H = np.eye(3)
    H[:2, :2] = R
    H[:2, 2] = np.array([cx, cy]) + np.array([tx, ty]) - R @ np.array([cx, cy])
    return H
