"""Rig absolute pose test scenes shared by the CPU and GPU suites: seeded multi-camera rigs seeing
a common point cloud, with the options each case runs under."""
from __future__ import annotations

import numpy as np

from pycolmap_amd import synth

W, H, F = 1600, 1200, 1200.0
FAST = dict(min_num_trials=30, max_num_trials=2000)  # the trial limits lowered where the defaults are not under test


def rig_scene(seed, num_points, models=(0,), outlier_frac=0.0, noise_px=0.0, dup_frac=0.0, baseline=0.4):
    """One query: a rig of len(models) cameras (random cam_from_rig, centres within `baseline`; a single camera sits at
    the rig's origin) at a random rig_from_world; every correspondence is a random point in front of a random camera of
    the rig, projected through that camera's model.  dup_frac: that fraction of the correspondences observe, from another
    camera, a 3D point an earlier correspondence has (bit-equal coordinates).  Returns a dict with the arrays of
    Context.estimate_rig_absolute_poses plus qvec / tvec of the true rig_from_world and outlier (N,)."""
    rng = np.random.default_rng(seed)
    C = len(models)
    prm = [np.asarray(synth._localisation_params(m, F, W, H), dtype=np.float64) for m in models]
    Rr, qr = synth.random_rotation(rng)
    tr = -Rr @ rng.uniform(-5.0, 5.0, size=3)
    rigs, Rc, tc = np.zeros((C, 7)), [], []
    for c in range(C):
        if C == 1:
            R, q, t = np.eye(3), np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
        else:
            R, q = synth.random_rotation(rng)
            t = -R @ rng.uniform(-baseline, baseline, size=3)
        rigs[c, :4], rigs[c, 4:] = q, t
        Rc.append(R)
        tc.append(t)
    n = int(num_points)
    idx = rng.integers(0, C, size=n).astype(np.int32)
    p2, p3 = np.zeros((n, 2)), np.zeros((n, 3))
    for k in range(n):
        c = int(idx[k])
        fx = prm[c][0]
        fy = prm[c][1] if int(models[c]) not in (0, 2, 3, 8, 9) else prm[c][0]
        if k and C > 1 and rng.random() < dup_frac:
            j = int(rng.integers(0, k))          # see point j again, from a camera in front of which it lies
            Y = Rr @ p3[j] + tr
            zs = [(Rc[e] @ Y + tc[e])[2] for e in range(C)]
            c = int(np.argmax(zs))
            idx[k] = c
            p3[k] = p3[j]
            Z = Rc[c] @ Y + tc[c]
            uvn = Z[:2] / Z[2]
        else:
            uvn = np.array([rng.uniform(-0.45 * W / fx, 0.45 * W / fx), rng.uniform(-0.45 * H / fy, 0.45 * H / fy)])
            d = rng.uniform(4.0, 12.0)
            Z = np.array([uvn[0] * d, uvn[1] * d, d])
            Y = Rc[c].T @ (Z - tc[c])
            p3[k] = Rr.T @ (Y - tr)
        p2[k] = synth.img_from_cam(int(models[c]), prm[c], uvn[None, :])[0]
    if noise_px > 0:
        p2 += rng.normal(scale=noise_px, size=p2.shape)
    bad = rng.random(n) < outlier_frac
    p2[bad] = np.stack([rng.uniform(0, W, int(bad.sum())), rng.uniform(0, H, int(bad.sum()))], 1)
    return dict(offsets=np.array([0, n], np.uint64), camera_offsets=np.array([0, C], np.uint64),
                camera_models=np.asarray(models, np.int32), camera_params=prm, cams_from_rig=rigs, camera_idxs=idx,
                points2D=p2, points3D=p3, qvec=qr[None, :], tvec=tr[None, :], outlier=bad)


def concat(*scenes):
    off, coff = [np.zeros(1, np.uint64)], [np.zeros(1, np.uint64)]
    b, cb = 0, 0
    for s in scenes:
        off.append(s["offsets"][1:] + np.uint64(b))
        coff.append(s["camera_offsets"][1:] + np.uint64(cb))
        b += int(s["offsets"][-1])
        cb += int(s["camera_offsets"][-1])
    cat = lambda k: np.concatenate([s[k] for s in scenes])  # noqa: E731
    return dict(offsets=np.concatenate(off), camera_offsets=np.concatenate(coff), camera_models=cat("camera_models"),
                camera_params=[p for s in scenes for p in s["camera_params"]], cams_from_rig=cat("cams_from_rig"),
                camera_idxs=cat("camera_idxs"), points2D=cat("points2D"), points3D=cat("points3D"), qvec=cat("qvec"),
                tvec=cat("tvec"), outlier=cat("outlier"))


def subset(sc, idx):
    """The queries idx (in that order) of a batch."""
    off, coff = sc["offsets"].astype(np.int64), sc["camera_offsets"].astype(np.int64)
    parts = []
    for i in idx:
        r, c = slice(off[i], off[i + 1]), slice(coff[i], coff[i + 1])
        parts.append(dict(offsets=np.array([0, off[i + 1] - off[i]], np.uint64),
                          camera_offsets=np.array([0, coff[i + 1] - coff[i]], np.uint64),
                          camera_models=sc["camera_models"][c], camera_params=sc["camera_params"][c],
                          cams_from_rig=sc["cams_from_rig"][c], camera_idxs=sc["camera_idxs"][r],
                          points2D=sc["points2D"][r], points3D=sc["points3D"][r], qvec=sc["qvec"][i:i + 1],
                          tvec=sc["tvec"][i:i + 1], outlier=sc["outlier"][r]))
    return concat(*parts)


def args(sc):
    return (sc["offsets"], sc["camera_offsets"], sc["camera_models"], sc["camera_params"], sc["cams_from_rig"],
            sc["camera_idxs"], sc["points2D"], sc["points3D"])


ALL_MODELS = tuple(range(11))


def cases():
    """name -> (scene, estimation options, refinement options, return_covariance)"""
    c = {}
    # the lane boundaries, N = 2 (failure) and N = 3
    for n in (2, 3, 63, 64, 65, 129):
        c[f"n{n}"] = (rig_scene(100 + n, n, models=(0, 1), noise_px=0.3), FAST, {}, n % 2 == 1)
    c["central"] = (rig_scene(1, 200, models=(1,), outlier_frac=0.3, noise_px=0.5), FAST, {}, True)
    c["two_cameras"] = (rig_scene(2, 200, models=(0, 4), outlier_frac=0.3, noise_px=0.5), FAST, {}, True)
    c["five_cameras_a"] = (rig_scene(3, 250, models=(0, 1, 2, 3, 4), outlier_frac=0.3, noise_px=0.5), FAST, {}, False)
    c["five_cameras_b"] = (rig_scene(4, 250, models=(5, 6, 7, 8, 9), outlier_frac=0.3, noise_px=0.5), FAST, {}, True)
    c["fisheye_prism"] = (rig_scene(5, 200, models=(10, 2), outlier_frac=0.3, noise_px=0.5), FAST, {}, True)
    c["duplicates"] = (rig_scene(6, 200, models=(0, 1, 2), outlier_frac=0.3, noise_px=0.5, dup_frac=0.4), FAST, {}, True)
    c["outliers30"] = (rig_scene(7, 300, models=(0, 1, 2, 3), outlier_frac=0.3, noise_px=0.5), FAST, {}, False)
    c["outliers60"] = (rig_scene(8, 300, models=(0, 1, 2, 3), outlier_frac=0.6, noise_px=0.5), FAST, {}, False)
    # the abort falls inside the first 64-trial round: an outlier-free query stops at min_num_trials
    c["abort_mid_round"] = (rig_scene(9, 150, models=(0, 1)), dict(min_num_trials=20, max_num_trials=2000), {}, False)
    # more than one round: 60 % outliers need a few hundred trials
    c["several_rounds"] = (rig_scene(10, 150, models=(0, 1), outlier_frac=0.6, noise_px=0.3),
                           dict(min_num_trials=20, max_num_trials=5000), {}, False)
    c["max_trials_below_round"] = (rig_scene(11, 150, models=(0, 1), outlier_frac=0.5, noise_px=0.3),
                                   dict(min_num_trials=10, max_num_trials=37), {}, False)
    # past the first stream table (3 x 2000 + 1024 words): 85 % outliers need thousands of trials
    c["stream_overrun"] = (rig_scene(12, 120, models=(0, 1), outlier_frac=0.85, noise_px=0.3),
                           dict(min_num_trials=20, max_num_trials=100000), {}, False)
    c["defaults"] = (rig_scene(13, 100, models=(0, 2), outlier_frac=0.2, noise_px=0.5), {}, {}, True)
    c["refine_opts"] = (rig_scene(14, 150, models=(0, 1), outlier_frac=0.2, noise_px=2.0), FAST,
                        dict(gradient_tolerance=1e-10, max_num_iterations=3, loss_function_scale=4.0), True)
    return c
