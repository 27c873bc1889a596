"""Seeded triangulation batches shared by the CPU and GPU tests and the frozen fixture (tests/golden/
make_tri_ref_golden.py): name -> (scene, options).  A scene is what pycolmap_amd.synth.triangulation_scene returns:
poses (C, 3, 4), offsets (T + 1,), obs_pose (M,), obs_xy (M, 2)."""
import numpy as np

from pycolmap_amd import synth

F = 1000.0
TIGHT = 4.0 / F  # a 4 px angular threshold at f = 1000 (pycolmap's default max_error, 4.0, is 4 radians here)


def scene(seed, num_tracks, **kw):
    return synth.triangulation_scene(np.random.default_rng(seed), num_tracks, f=F, **kw)


def concat(*scenes):
    """One batch of several scenes' tracks (pose indices shifted)."""
    poses, offs, op, xy = [], [0], [], []
    npose = 0
    for s in scenes:
        poses.append(s["poses"])
        o = s["offsets"].astype(np.int64)
        offs.extend((o[1:] + offs[-1]).tolist())
        op.append(s["obs_pose"].astype(np.int64) + npose)
        xy.append(s["obs_xy"])
        npose += len(s["poses"])
    return dict(poses=np.concatenate(poses), offsets=np.array(offs, np.uint64), obs_pose=np.concatenate(op).astype(np.uint32),
                obs_xy=np.concatenate(xy))


def fixed_length(seed, num_tracks, n, **kw):
    return scene(seed, num_tracks, num_cameras=max(2 * n, 20), max_len=n, mean_len=1e9, **kw)


def degenerate(seed):
    """Coincident centres (every observation from one camera), points at infinity (a direction seen from every
    camera), non-finite observations and poses."""
    rng = np.random.default_rng(seed)
    base = scene(seed, 6, noise_px=0.0, outlier_frac=0.0, max_len=6, mean_len=1e9)
    poses = base["poses"].copy()
    op = base["obs_pose"].copy()
    xy = base["obs_xy"].copy()
    off = base["offsets"]
    op[int(off[0]):int(off[1])] = op[int(off[0])]  # track 0: one camera only
    d = rng.normal(size=3)  # track 1: the direction d at infinity
    for k in range(int(off[1]), int(off[2])):
        q = poses[op[k], :, :3] @ d
        xy[k] = q[:2] / q[2]
    xy[int(off[2]) + 1, 0] = np.nan  # track 2: a NaN observation
    xy[int(off[3]), 1] = np.inf  # track 3: an infinite one
    poses = np.concatenate([poses, poses[:1]])
    poses[-1, 0, 3] = np.nan  # track 4: one observation through a pose with a NaN translation
    op[int(off[4])] = len(poses) - 1
    return dict(poses=poses, offsets=off, obs_pose=op, obs_xy=xy)


def cases():
    return {
        "clean": (scene(1, 400, noise_px=0.0, outlier_frac=0.0), dict(max_error=TIGHT)),
        "noisy": (scene(2, 400, outlier_frac=0.0), dict(max_error=TIGHT)),
        "outliers30": (scene(3, 400, outlier_frac=0.3, mean_len=8.0), dict(max_error=TIGHT)),
        "defaults": (scene(4, 200, outlier_frac=0.1), {}),
        "two_obs": (fixed_length(5, 300, 2, outlier_frac=0.1), dict(max_error=TIGHT)),
        "three_obs": (fixed_length(6, 300, 3, outlier_frac=0.2), dict(max_error=TIGHT)),
        "long": (concat(fixed_length(7, 2, 200, outlier_frac=0.3), fixed_length(8, 1, 333, outlier_frac=0.3),
                        fixed_length(9, 1, 500, outlier_frac=0.3)), dict(max_error=TIGHT)),
        "long_trial_caps": (concat(fixed_length(10, 2, 60, outlier_frac=0.3), fixed_length(11, 1, 250, outlier_frac=0.4)),
                            dict(max_error=TIGHT, min_num_trials=20, max_num_trials=700)),
        "min_tri_angle": (scene(12, 400, outlier_frac=0.1, mean_len=6.0), dict(max_error=TIGHT, min_tri_angle=0.3)),
        "min_tri_angle_small": (scene(13, 300, outlier_frac=0.1), dict(max_error=TIGHT, min_tri_angle=0.02)),
        "tiny_max_error": (scene(14, 300, outlier_frac=0.1), dict(max_error=1e-7)),
        "degenerate": (degenerate(15), dict(max_error=TIGHT)),
    }
