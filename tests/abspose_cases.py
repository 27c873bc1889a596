"""Absolute pose test scenes shared by the CPU and GPU suites: localisation queries from pycolmap_amd.synth with the
options each case runs under."""
from __future__ import annotations

import numpy as np

from pycolmap_amd import synth


def scene(seed, num_queries, num_points, **kw):
    return synth.localisation_scene(np.random.default_rng(seed), num_queries, num_points=num_points, **kw)


def concat(*scenes):
    off = [np.zeros(1, np.uint64)]
    base = 0
    for s in scenes:
        off.append(s["offsets"][1:] + np.uint64(base))
        base += int(s["offsets"][-1])
    cat = lambda k: np.concatenate([s[k] for s in scenes])  # noqa: E731
    return dict(offsets=np.concatenate(off), camera_models=cat("camera_models"),
                camera_params=[p for s in scenes for p in s["camera_params"]], points2D=cat("points2D"),
                points3D=cat("points3D"), qvec=cat("qvec"), tvec=cat("tvec"), outlier=cat("outlier"))


def subset(sc, idx):
    """The queries idx (in that order) of a scene."""
    off = sc["offsets"].astype(np.int64)
    rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in idx]) if len(idx) else np.zeros(0, np.int64)
    lens = np.array([off[i + 1] - off[i] for i in idx], np.int64)
    return dict(offsets=np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64),
                camera_models=sc["camera_models"][list(idx)], camera_params=[sc["camera_params"][i] for i in idx],
                points2D=sc["points2D"][rows], points3D=sc["points3D"][rows], qvec=sc["qvec"][list(idx)],
                tvec=sc["tvec"][list(idx)], outlier=sc["outlier"][rows])


def degenerate():
    """Queries that must fail or stay finite: collinear points, duplicated points, all behind the camera, NaN input,
    fewer than three correspondences."""
    base = scene(90, 5, 60, outlier_frac=0.0, noise_px=0.0)
    p3 = base["points3D"].copy()
    p2 = base["points2D"].copy()
    p3[0:60] = np.linspace(0, 1, 60)[:, None] * np.array([1.0, 2.0, 3.0]) + base["points3D"][0]   # collinear
    p3[60:120] = p3[60]                                                                         # duplicates
    p2[60:120] = p2[60]
    p2[180:240:3] = np.nan                                                                      # NaN pixels
    p3[181:240:5] = np.nan                                                                      # NaN points
    sc = dict(base, points2D=p2, points3D=p3)
    behind = scene(91, 1, 50, outlier_frac=0.0, noise_px=0.0, behind_frac=1.0)
    tiny = concat(scene(92, 1, 3, outlier_frac=0.0, noise_px=0.0), scene(93, 1, 2, outlier_frac=0.0, noise_px=0.0))
    empty = dict(offsets=np.zeros(2, np.uint64), camera_models=np.zeros(1, np.int32),
                 camera_params=[np.array([1000.0, 500.0, 500.0])], points2D=np.zeros((0, 2)), points3D=np.zeros((0, 3)),
                 qvec=np.zeros((1, 4)), tvec=np.zeros((1, 3)), outlier=np.zeros(0, bool))
    return concat(sc, behind, tiny, empty)


def cases():
    """name -> (scene, estimation options, refinement options, return_covariance)"""
    c = {
        "clean": (scene(1, 6, 300, outlier_frac=0.0, noise_px=0.0), {}, {}, False),
        "noisy": (scene(2, 6, 300, outlier_frac=0.0, noise_px=1.0), {}, {}, True),
        "outliers30": (scene(3, 6, 300, outlier_frac=0.3), {}, {}, False),
        "outliers60": (scene(4, 6, 300, outlier_frac=0.6), {}, {}, False),
        "outliers80": (scene(5, 4, 400, outlier_frac=0.8), {}, {}, True),
        "sizes": (concat(*[scene(10 + n, 2, n, outlier_frac=0.0, noise_px=0.3) for n in (3, 4, 5)],
                         scene(14, 2, 1000, outlier_frac=0.4)), {}, {}, True),
        "focal": (scene(20, 3, 200, outlier_frac=0.2), dict(estimate_focal_length=1, num_focal_length_samples=10), {},
                  True),
        "trial_caps": (scene(21, 4, 200, outlier_frac=0.5), dict(min_num_trials=10, max_num_trials=50), {}, False),
        "max_error_tight": (scene(22, 4, 200, outlier_frac=0.3, noise_px=1.0), dict(max_error=0.5), {}, False),
        "max_error_loose": (scene(23, 4, 200, outlier_frac=0.3), dict(max_error=400.0), {}, False),
        "refine_opts": (scene(24, 4, 200, outlier_frac=0.3, noise_px=2.0), {},
                        dict(gradient_tolerance=1e-10, max_num_iterations=3, loss_function_scale=4.0), True),
        "degenerate": (degenerate(), {}, {}, True),
    }
    for m in range(11):
        c[f"model{m}"] = (scene(40 + m, 2, 250, outlier_frac=0.3, noise_px=0.5, model=m), {}, {}, m % 2 == 0)
    return c
