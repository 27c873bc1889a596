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


# ---- the edge cases: what cases() does not reach ------------------------------------------------------
FIELDS = ("success", "qvec", "tvec", "num_inliers", "num_all_inliers", "num_trials", "inlier_mask", "covariance")
OVERRUN = dict(min_num_trials=20, max_num_trials=100000)  # a first sample stream of 3 * 2000 + 1024 words
FIRST_STREAM_WORDS = 3 * 2000 + 1024
LAST_TRIAL_WITH_WORDS = FIRST_STREAM_WORDS // 3 - 1  # 2340: a trial takes three words
NO_CONSENSUS = dict(min_num_trials=20, max_num_trials=5000)  # 15,000 words: the table doubles twice
TIGHT = dict(gradient_tolerance=0.0)


def fixed_inliers(seed, n, k, models=(0, 1)):
    """A query of n correspondences of which exactly k are noise-free and the rest uniform random pixels (the
    reference's inlier count says whether one of those fell within max_error of its point: tests/test_rigpose_cpu.py)."""
    sc = rig_scene(seed, n, models=models)
    rng = np.random.default_rng(seed + 100000)
    bad = np.zeros(n, bool)
    bad[rng.permutation(n)[:n - k]] = True
    p2 = sc["points2D"].copy()
    p2[bad] = np.stack([rng.uniform(0, W, n - k), rng.uniform(0, H, n - k)], 1)
    return dict(sc, points2D=p2, outlier=bad)


def no_consensus(seed, n=36):
    """A query whose pixels are all uniform random: no model gathers more than a handful of inliers, so the RANSAC runs
    to max_num_trials (a query of 12 is too small for that: it stops at 1,757 trials)."""
    return fixed_inliers(seed, n, 0)


def _rotations(q):
    x, y, z, w = np.moveaxis(q, -1, 0)
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=-1).reshape(q.shape[:-1] + (3, 3))


def tiny_rig_queries(seed, num_queries, num_points=4, repeat_every=0):
    """num_queries noise-free queries of num_points correspondences over a SIMPLE_PINHOLE and a PINHOLE camera, built
    without a Python loop (rig_scene has one per correspondence).  repeat_every = r: in every r-th query the second
    correspondence repeats the first (the same camera, pixel and 3D point), so that query has a repeated point."""
    rng = np.random.default_rng(seed)
    Q, n = int(num_queries), int(num_points)
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)  # noqa: E731
    qr = unit(rng.normal(size=(Q, 4)))
    qr *= np.where(qr[:, 3:] < 0, -1.0, 1.0)
    Rr = _rotations(qr)
    tr = -np.einsum("qij,qj->qi", Rr, rng.uniform(-5.0, 5.0, size=(Q, 3)))
    qc = unit(rng.normal(size=(Q, 2, 4)))
    qc *= np.where(qc[..., 3:] < 0, -1.0, 1.0)
    Rc = _rotations(qc)
    tc = -np.einsum("qcij,qcj->qci", Rc, rng.uniform(-0.4, 0.4, size=(Q, 2, 3)))
    idx = rng.integers(0, 2, size=(Q, n))
    fy = np.where(idx == 1, 1.02 * F, F)
    uvn = np.stack([rng.uniform(-0.45 * W / F, 0.45 * W / F, size=(Q, n)), rng.uniform(-0.45, 0.45, size=(Q, n)) * H / fy], -1)
    d = rng.uniform(4.0, 12.0, size=(Q, n, 1))
    Z = np.concatenate([uvn * d, d], axis=2)
    Rk, tk = Rc[np.arange(Q)[:, None], idx], tc[np.arange(Q)[:, None], idx]  # (Q, n, 3, 3), (Q, n, 3)
    Y = np.einsum("qkji,qkj->qki", Rk, Z - tk)
    p3 = np.einsum("qji,qkj->qki", Rr, Y - tr[:, None, :])
    p2 = uvn * np.stack([np.full((Q, n), F), fy], -1) + np.array([W / 2.0, H / 2.0])
    if repeat_every and n > 1:
        idx[::repeat_every, 1], p2[::repeat_every, 1], p3[::repeat_every, 1] = \
            idx[::repeat_every, 0], p2[::repeat_every, 0], p3[::repeat_every, 0]
    rigs = np.concatenate([qc, tc], axis=2).reshape(2 * Q, 7)
    prm = [np.asarray(synth._localisation_params(m, F, W, H), dtype=np.float64) for m in (0, 1)]
    return dict(offsets=(n * np.arange(Q + 1)).astype(np.uint64), camera_offsets=(2 * np.arange(Q + 1)).astype(np.uint64),
                camera_models=np.tile(np.array([0, 1], np.int32), Q), camera_params=prm * Q, cams_from_rig=rigs,
                camera_idxs=idx.reshape(-1).astype(np.int32), points2D=p2.reshape(-1, 2), points3D=p3.reshape(-1, 3),
                qvec=qr, tvec=tr, outlier=np.zeros(Q * n, bool))


def empty_query(num_cameras=2):
    """A query of num_cameras cameras and no correspondence."""
    return rig_scene(1, 0, models=(0, 1)[:num_cameras])


def observe(sc, j, c):
    """The pixel at which camera c of a one-query scene sees the 3D point of correspondence j under the true pose, or
    None where the point is not in front of it."""
    q, t = sc["qvec"][0], sc["tvec"][0]
    g = sc["cams_from_rig"][c]
    Z = _rotations(g[:4]) @ (_rotations(q) @ sc["points3D"][j] + t) + g[4:]
    if Z[2] < 0.5:
        return None
    return synth.img_from_cam(int(sc["camera_models"][c]), sc["camera_params"][c], (Z[:2] / Z[2])[None, :])[0]


def with_rows(sc, rows):
    """The one-query scene with the correspondences `rows` = [(camera, pixel, point)] appended."""
    n = len(sc["camera_idxs"]) + len(rows)
    return dict(sc, offsets=np.array([0, n], np.uint64),
                camera_idxs=np.concatenate([sc["camera_idxs"], np.array([r[0] for r in rows], np.int32)]),
                points2D=np.vstack([sc["points2D"]] + [np.asarray(r[1], np.float64)[None, :] for r in rows]),
                points3D=np.vstack([sc["points3D"]] + [np.asarray(r[2], np.float64)[None, :] for r in rows]),
                outlier=np.concatenate([sc["outlier"], np.zeros(len(rows), bool)]))


def seen_again(seed, n, j=0, models=(0, 1, 0)):
    """A noise-free query of n correspondences without repeats, then one more observation of point j from each of the
    two cameras that did not see it (appended, in camera order): n + 2 correspondences, point j seen three times.  The
    seed is one at which point j lies in front of all three cameras."""
    sc = rig_scene(seed, n, models=models)
    others = [c for c in range(3) if c != int(sc["camera_idxs"][j])]
    px = [observe(sc, j, c) for c in others]
    if any(p is None for p in px):
        raise ValueError(f"seen_again: seed {seed} leaves point {j} behind a camera")
    return with_rows(sc, [(c, p, sc["points3D"][j]) for c, p in zip(others, px)])


def collinear(seed, n):
    """A query whose 3D points lie on one line (the observations stay those of the scene's own points)."""
    sc = rig_scene(seed, n, models=(0, 1))
    return dict(sc, points3D=np.linspace(0, 1, n)[:, None] * np.array([1.0, 2.0, 3.0]) + sc["points3D"][0])


def with_value(sc, key, row, col, value):
    a = sc[key].copy()
    a[row, col] = value
    return dict(sc, **{key: a})


def signed_zero(seed, n):
    """A noise-free query in which correspondences n and n + 1 see the point of correspondence 0 again, the world moved
    along x so that this point's x is zero: written 0.0 in rows 0 and n + 1 and -0.0 in row n."""
    sc = seen_again(seed, n)
    s = sc["points3D"][0, 0]
    p3 = sc["points3D"].copy()
    p3[:, 0] -= s                                            # Y = R (X - s e0) + (t + s R e0)
    t = sc["tvec"] + s * _rotations(sc["qvec"][0])[:, 0]
    assert p3[0, 0] == 0.0 and p3[n, 0] == 0.0 and p3[n + 1, 0] == 0.0
    p3[n, 0] = -0.0
    return dict(sc, points3D=p3, tvec=t)


def huge_focal(seed, n, f):
    """A noise-free query over two SIMPLE_PINHOLE cameras of focal length f, the pixels those of focal length F scaled
    about the principal point."""
    sc = rig_scene(seed, n, models=(0, 0))
    c = np.array([W / 2.0, H / 2.0])
    return dict(sc, points2D=(sc["points2D"] - c) * (f / F) + c, camera_params=[np.array([f, c[0], c[1]])] * 2)


def with_unused_camera(sc):
    """The two-camera one-query scene with a third camera, which no correspondence names, between the two."""
    rng = np.random.default_rng(5)
    _, q = synth.random_rotation(rng)
    extra = np.concatenate([q, rng.uniform(-0.4, 0.4, 3)])
    return dict(sc, camera_offsets=np.array([0, 3], np.uint64), camera_models=np.array([sc["camera_models"][0], 3,
                                                                                        sc["camera_models"][1]], np.int32),
                camera_params=[sc["camera_params"][0], np.asarray(synth._localisation_params(3, F, W, H)),
                               sc["camera_params"][1]],
                cams_from_rig=np.vstack([sc["cams_from_rig"][0], extra, sc["cams_from_rig"][1]]),
                camera_idxs=(2 * sc["camera_idxs"]).astype(np.int32))


# (n, k) -> the reference's num_trials under OVERRUN (dyn_max = ComputeNumTrials(k, n), the abort on the first trial at
# or past it that has a model, num_trials two more); trials 0 .. 2340 have words, the round of 64 is 2304 .. 2367
STREAM_WINDOWS = {
    "stream_before_end": (2100, 136, 31),    # 2322: aborts on trial 2320, inside the last round with words
    "stream_near_end": (2101, 145, 33),      # 2333 or 2334
    "stream_last_trial": (2102, 132, 30),    # 2342: aborts on trial 2340, the last trial with words
    "stream_first_without": (3011, 132, 30),  # 2343: trial 2340 has no model, aborts on 2341, the first without words
    "stream_same_round": (2103, 141, 32),    # 2352 or 2353: past the end, in the round in which the table ends
    "stream_next_round": (2104, 137, 31),    # 2374: past that round
}


def stream_batch():
    """The stream-window queries as one batch with small queries between them: overruns beside queries that need no
    rerun."""
    parts = []
    for i, name in enumerate(sorted(STREAM_WINDOWS)):
        parts += [fixed_inliers(*STREAM_WINDOWS[name]), rig_scene(2200 + i, (0, 2, 3, 40, 64, 65)[i], models=(0, 1))]
    return concat(*parts)


COINCIDENT_SEED = 2403  # rig_scene(seed, 12, dup_frac=0.75) with exactly five distinct points
SEEN_AGAIN_SEED = 2501  # point 0 lies in front of all three cameras


def edge_cases():
    """name -> (scene, estimation options, refinement options, return_covariance).  Every shape is the smallest at
    which the code path exists: at most 200 correspondences a query.  tests/test_rigpose_cpu.py asserts by the
    reference's own results and trace that each case is of the kind its name says."""
    c = {}
    # the end of the sample stream
    for name, a in STREAM_WINDOWS.items():
        c[name] = (fixed_inliers(*a), OVERRUN, {}, False)
    c["stream_batch"] = (stream_batch(), OVERRUN, {}, True)
    c["double_twice"] = (no_consensus(4000), NO_CONSENSUS, {}, False)
    # RANSAC control
    c["trials_equal"] = (rig_scene(2300, 100, models=(0, 1), outlier_frac=0.3, noise_px=0.5),
                         dict(min_num_trials=50, max_num_trials=50), {}, False)
    c["zero_trials"] = (rig_scene(2301, 100, models=(0, 1)), dict(min_num_trials=0, max_num_trials=0), {}, True)
    c["one_trial"] = (rig_scene(2302, 100, models=(0, 1)), dict(min_num_trials=0, max_num_trials=1), {}, True)
    c["confidence0"] = (rig_scene(2303, 100, models=(0, 1), outlier_frac=0.3, noise_px=0.5), dict(FAST, confidence=0.0),
                        {}, False)
    c["confidence1"] = (rig_scene(2304, 100, models=(0, 1), outlier_frac=0.3, noise_px=0.5), dict(FAST, confidence=1.0),
                        {}, True)
    c["ratio_clamp"] = (rig_scene(2305, 150, models=(0, 1), outlier_frac=0.6, noise_px=0.5),
                        dict(FAST, min_inlier_ratio=0.5), {}, False)
    # degenerate geometry
    c["zero_baseline"] = (rig_scene(2310, 100, models=(0, 1, 2), outlier_frac=0.3, noise_px=0.5, baseline=0.0), FAST, {},
                          True)
    c["coincident_samples"] = (rig_scene(COINCIDENT_SEED, 12, models=(0, 1, 2), dup_frac=0.75), FAST, {}, True)
    c["collinear"] = (collinear(2312, 40), FAST, {}, True)
    live = rig_scene(2313, 60, models=(0, 1, 2), outlier_frac=0.2, noise_px=0.5)
    k = int(np.flatnonzero(~live["outlier"])[5])
    c["nan_pixel"] = (with_value(live, "points2D", k, 0, np.nan), FAST, {}, True)
    c["nan_point"] = (with_value(live, "points3D", k, 1, np.nan), FAST, {}, True)
    c["nan_rig"] = (with_value(live, "cams_from_rig", 1, 2, np.nan), FAST, {}, True)
    c["signed_zero"] = (signed_zero(SEEN_AGAIN_SEED, 30), FAST, {}, True)
    thrice = seen_again(SEEN_AGAIN_SEED, 30)  # point 0 in rows 0, 30 and 31
    p3 = thrice["points3D"].copy()
    p3[[0, 30], 2] = np.nan
    c["nan_twins"] = (dict(thrice, points3D=p3), FAST, {}, True)
    # point 0 has three observations (rows 0, 30, 31) and the first is 300 px off: 31 of the 32 correspondences are
    # inliers, and rows 30 and 31 count as one point, so 30 unique inliers
    c["chain3_first_out"] = (with_value(thrice, "points2D", 0, 0, thrice["points2D"][0, 0] + 300.0), FAST, {}, True)
    # the same with the second of the three observations off: row 31's chain passes over an unflagged row 30 to row 0
    c["chain3_middle_out"] = (with_value(thrice, "points2D", 30, 0, thrice["points2D"][30, 0] + 300.0), FAST, {}, True)
    for k in (64, 65):
        c[f"inliers{k}"] = (fixed_inliers(2320 + k, 100, k), FAST, {}, k % 2 == 1)
    c["unused_camera"] = (with_unused_camera(rig_scene(2330, 80, models=(0, 1), outlier_frac=0.2, noise_px=0.5)), FAST, {},
                          True)
    c["empty_between"] = (concat(rig_scene(2331, 50, models=(0, 1), outlier_frac=0.2, noise_px=0.5), empty_query(),
                                 rig_scene(2332, 70, models=(0, 1, 2), outlier_frac=0.2, noise_px=0.5)), FAST, {}, True)
    # refinement through the rig entry: every start is a RANSAC model
    near = rig_scene(2340, 100, models=(0, 1), outlier_frac=0.2, noise_px=1.0)
    exact = rig_scene(2341, 100, models=(0, 1))
    c["refine_iterations0"] = (near, FAST, dict(TIGHT, max_num_iterations=0), True)
    c["refine_gradient_huge"] = (near, FAST, dict(gradient_tolerance=1e10), True)
    c["refine_tight_noisy"] = (near, FAST, TIGHT, True)
    c["refine_tight_exact"] = (exact, FAST, TIGHT, True)
    c["refine_scale_tiny"] = (near, FAST, dict(TIGHT, loss_function_scale=1e-120), True)
    c["refine_scale_huge"] = (near, FAST, dict(TIGHT, loss_function_scale=1e60), True)
    c["refine_three_inliers"] = (fixed_inliers(2342, 12, 3), FAST, {}, True)
    # one observation 1e40 pixels away that a max_error of 1e42 keeps an inlier, under a loss wide enough to stay
    # quadratic there: no step lowers the cost, until the 15th rejection takes the radius below 1e-32
    far = rig_scene(2340, 100, models=(0, 1), noise_px=1.0)
    c["refine_min_radius"] = (with_value(far, "points2D", 0, 0, far["points2D"][0, 0] + 1e40), dict(FAST, max_error=1e42),
                              dict(TIGHT, loss_function_scale=1e60), True)
    # three correspondences of two distinct points: a rotation about the line through the two points moves no
    # projection, so the Hessian has rank five and the covariance's rank test fails after a successful RANSAC
    sc = seen_again(SEEN_AGAIN_SEED, 2)
    c["refine_rank_two_points"] = (dict(
        sc, offsets=np.array([0, 3], np.uint64), camera_idxs=sc["camera_idxs"][:3], points2D=sc["points2D"][:3],
        points3D=sc["points3D"][:3], outlier=sc["outlier"][:3]), FAST, {}, True)
    # a focal length of 1e154: the residuals' squares stay finite while the Jacobian's overflow, so the Hessian is
    # infinite at a finite cost, its scaling 0 * inf * 0 is NaN and every elimination fails: five invalid steps after a
    # successful RANSAC
    c["refine_invalid_steps"] = (huge_focal(2341, 100, 1e154), dict(FAST, max_error=1.2e152), TIGHT, True)
    # a loss scale whose square is subnormal (1 / b is infinite) or zero: the start's cost is not finite, so the
    # refinement fails after a successful RANSAC: success is false, num_inliers and the mask are set
    c["refine_scale_subnormal"] = (near, FAST, dict(loss_function_scale=1e-160), True)
    c["refine_scale_zero"] = (near, FAST, dict(loss_function_scale=0.0), False)
    return c


EDGE_CASES = edge_cases()


def digest(result) -> str:
    """sha256 over the result's FIELDS, each as name, dtype, shape and bytes."""
    import hashlib
    h = hashlib.sha256()
    for k in FIELDS:
        if k in result:
            a = np.ascontiguousarray(result[k])
            h.update(f"{k}:{a.dtype.str}:{a.shape}:".encode())
            h.update(a.tobytes())
    return h.hexdigest()


REUSE_FIRST = 2048  # the most blocks rigpose_ransac_kernel is launched with


def reuse_batch():
    """(scene, options, the indices of the 64 small queries): 2,048 queries of 40 correspondences, every second with a
    repeated point, and among them 64 queries of 0 .. 39 correspondences, which the size order gives to blocks 0 .. 63
    as their second query: in that order a three-camera query with repeated points beside a one-camera query without,
    n = 0, 2 and 3, and the 36-correspondence query without consensus, which under NO_CONSENSUS overruns the sample
    stream twice."""
    small = [empty_query(), rig_scene(2600, 2, models=(0, 1)), rig_scene(2601, 3, models=(0, 1)), no_consensus(4000)]
    for i in range(60):
        n = 4 + (i * 35) // 59  # 4 .. 39, so that neighbours in the size order alternate between the two kinds
        if i % 2:
            small.append(rig_scene(2610 + i, n, models=(1,), outlier_frac=0.2, noise_px=0.5))
        else:
            small.append(rig_scene(2610 + i, n, models=(0, 4, 2), outlier_frac=0.2, noise_px=0.5, dup_frac=0.4))
    big = tiny_rig_queries(2700, REUSE_FIRST, 40, repeat_every=2)
    where = [33 * i + 5 for i in range(64)]  # spread over the batch: the size order, not the position, gives the turn
    parts, b = [], 0
    for i in range(64):
        parts.append(subset(big, range(b, where[i] - i)))
        parts.append(small[i])
        b = where[i] - i
    parts.append(subset(big, range(b, REUSE_FIRST)))
    return concat(*[p for p in parts if len(p["offsets"]) > 1]), NO_CONSENSUS, where


def query_count_batch():
    """(scene, options): 65,537 queries, one more than a device batch holds: a query that overruns the first sample
    stream, 65,535 four-point queries, and that query again as the second batch."""
    over = fixed_inliers(*STREAM_WINDOWS["stream_same_round"])
    return concat(over, tiny_rig_queries(2800, (1 << 16) - 1, 4), over), OVERRUN
