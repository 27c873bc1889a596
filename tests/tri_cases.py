"""Seeded triangulation batches shared by the CPU and GPU tests and the frozen fixture (tests/golden/
make_tri_ref_golden.py): name -> (scene, options).  A scene is what pycolmap_amd.synth.triangulation_scene returns:
poses (C, 3, 4), offsets (T + 1,), obs_pose (M,), obs_xy (M, 2).  EDGE_CASES, of the same form, are the smallest shapes
at the edges, frozen as digests in tests/golden/tri_ref_edges_v1.npz."""
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


def with_lengths(seed, lens, noise_px=0.5, outlier_frac=0.0):
    """One track per entry of `lens` (0 and 1 included), distinct cameras within a track."""
    lens = np.asarray(lens, np.int64)
    n = max(int(lens.max(initial=0)), 2)
    base = fixed_length(seed, max(len(lens), 1), n, noise_px=noise_px, outlier_frac=outlier_frac)
    off = base["offsets"].astype(np.int64)
    keep = np.concatenate([np.arange(off[t], off[t] + lens[t]) for t in range(len(lens))] + [np.zeros(0, np.int64)])
    return dict(poses=base["poses"], offsets=np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64),
                obs_pose=base["obs_pose"][keep], obs_xy=np.ascontiguousarray(base["obs_xy"][keep]))


def reorder(sc, perm):
    """The scene's tracks in the order `perm` (the poses stay)."""
    off = sc["offsets"].astype(np.int64)
    lens = np.diff(off)[perm]
    idx = np.concatenate([np.arange(off[t], off[t + 1]) for t in perm] + [np.zeros(0, np.int64)])
    return dict(poses=sc["poses"], offsets=np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64),
                obs_pose=sc["obs_pose"][idx], obs_xy=np.ascontiguousarray(sc["obs_xy"][idx]))


def edited(sc, obs_pose=None, obs_xy=None, poses=None):
    """A copy of the scene's arrays; the dicts map an observation (a pose) index to its new value."""
    out = dict(poses=sc["poses"].copy(), offsets=sc["offsets"].copy(), obs_pose=sc["obs_pose"].copy(),
               obs_xy=sc["obs_xy"].copy())
    for key, changes in (("obs_pose", obs_pose), ("obs_xy", obs_xy), ("poses", poses)):
        for k, v in (changes or {}).items():
            out[key][k] = v
    return out


def on_poses(sc, obs_pose, noise_px=0.5):
    """The scene's points seen from the poses `obs_pose` names, one per observation, instead of the scene's own."""
    op = np.asarray(obs_pose, np.uint32)
    X = np.repeat(sc["xyz"], np.diff(sc["offsets"].astype(np.int64)), axis=0)
    q = np.einsum("mij,mj->mi", sc["poses"][op, :, :3], X) + sc["poses"][op, :, 3]
    xy = q[:, :2] / q[:, 2:3] + np.random.default_rng(len(op)).normal(scale=noise_px / F, size=(len(op), 2))
    return dict(poses=sc["poses"], offsets=sc["offsets"], obs_pose=op, obs_xy=np.ascontiguousarray(xy))


def repeated(sc, t, k, times):
    """Observation k of track t `times` times in a row instead of once."""
    off = sc["offsets"].astype(np.int64)
    o = int(off[t]) + k
    idx = np.concatenate([np.arange(o), np.full(times, o), np.arange(o + 1, off[-1])])
    lens = np.diff(off)
    lens[t] += times - 1
    return dict(poses=sc["poses"], offsets=np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64),
                obs_pose=sc["obs_pose"][idx], obs_xy=np.ascontiguousarray(sc["obs_xy"][idx]))


def axis_cameras(X, centers, flip=()):
    """One track of the point X seen without noise from cameras at `centers` that look along +z; the cameras listed in
    `flip` are turned half round about their y axis and see the point behind them."""
    poses = np.zeros((len(centers), 3, 4))
    xy = np.zeros((len(centers), 2))
    for i, c in enumerate(centers):
        R = np.diag([-1.0, 1.0, -1.0]) if i in flip else np.eye(3)
        poses[i, :, :3] = R
        poses[i, :, 3] = -R @ np.asarray(c, float)
        q = R @ np.asarray(X, float) + poses[i, :, 3]
        xy[i] = q[:2] / q[2]
    return dict(poses=poses, offsets=np.array([0, len(centers)], np.uint64),
                obs_pose=np.arange(len(centers), dtype=np.uint32), obs_xy=xy)


LEN_BINS = (0, 0, 1, 1, 2, 2, 3, 3, 63, 63, 64, 64, 65, 65, 66, 66, 130, 130)
TRACK_COUNTS = (1, 63, 64, 65, 255, 256, 257, 513)
DBL_TRUE_MIN = 5e-324
# the RANSAC limits, on clean tracks of 10 observations (45 pairs) and of 2 and 3 (1 and 3 pairs)
LIMITS_10 = {
    **{f"min{k}": dict(min_num_trials=k) for k in (42, 43, 44, 45, 46)},
    "min0_max0": dict(min_num_trials=0, max_num_trials=0),
    "min1_max1": dict(min_num_trials=1, max_num_trials=1),
    "min42_max42": dict(min_num_trials=42, max_num_trials=42),
    "min41_max42": dict(min_num_trials=41, max_num_trials=42),
    "confidence0": dict(confidence=0.0),
    "confidence1": dict(confidence=1.0, min_num_trials=0),
    "ratio0.9": dict(min_inlier_ratio=0.9, min_num_trials=0, confidence=0.5),
    "ratio1.0": dict(min_inlier_ratio=1.0, min_num_trials=0, confidence=0.5),
    "multiplier0": dict(dyn_num_trials_multiplier=0.0, min_num_trials=0),
}
LIMITS_SHORT = {
    **{f"min{k}": dict(min_num_trials=k) for k in (0, 1, 2, 3, 4)},
    **{k: LIMITS_10[k] for k in ("min0_max0", "min1_max1", "confidence0", "confidence1", "ratio0.9", "ratio1.0",
                                 "multiplier0")},
    "min2_max2": dict(min_num_trials=2, max_num_trials=2),
}
ONE_SAMPLE = dict(min_num_trials=0, max_num_trials=1)  # the pair (0, 1) alone


def threshold_scene():
    """A three-observation track whose third observation lies 3 px off; under ONE_SAMPLE the model is the first two's,
    and at a max_error of 1 px the third is no inlier of it."""
    sc = fixed_length(620, 1, 3, noise_px=0.01, outlier_frac=0.0)
    return edited(sc, obs_xy={2: sc["obs_xy"][2] + np.array([3.0 / F, 0.0])})


def largest_max_error_below(r):
    """The largest double m with fl(m * m) < r."""
    m = float(np.sqrt(r))
    while m * m >= r:
        m = float(np.nextafter(m, 0.0))
    while float(np.nextafter(m, np.inf)) ** 2 < r:
        m = float(np.nextafter(m, np.inf))
    return m


def _trace(sc, opts):
    """The reference's trace of the scene: floats by name (tests/tri_ref_lib.py)."""
    import tri_ref_lib as ref
    tr = ref.triangulate_trace(sc["poses"], sc["offsets"], sc["obs_pose"], sc["obs_xy"], **opts)[4]
    return {k: [float(v) for v in tr[k]] for k in ("angle", "residuals")}


def edge_cases():
    """name -> (scene, options): the smallest shapes at the edges of the lanes and blocks, of the host's length bins, of
    the RANSAC's stops and of the thresholds, and non-finite and extreme input.
    tests/test_triangulation_cpu.py asserts from the reference's trace that each case is of the kind its name says.  Three
    thresholds are taken from the reference's trace here: an observation's residual and two tracks' deciding angles."""
    tight = dict(max_error=TIGHT)
    c = {}
    # lanes and blocks: one lane per track, 64 a wave, 256 a block
    for n in TRACK_COUNTS:
        c[f"tracks_{n}"] = (fixed_length(500 + n, n, 3, outlier_frac=0.1), tight)
    # bins and order: the counting sort of the lengths, longest first, lengths above 64 in track order
    bins = with_lengths(520, LEN_BINS, outlier_frac=0.1)
    c["len_bins"] = (bins, tight)
    c["len_bins_descending"] = (reorder(bins, np.arange(len(LEN_BINS))[::-1]), tight)
    c["mixed_wave"] = (with_lengths(521, [2 + i % 39 for i in range(70)], outlier_frac=0.1), tight)
    # no work
    c["all_empty"] = (dict(poses=np.zeros((0, 3, 4)), offsets=np.zeros(6, np.uint64), obs_pose=np.zeros(0, np.uint32),
                           obs_xy=np.zeros((0, 2))), tight)
    c["all_single"] = (with_lengths(522, [1] * 5), tight)
    c["empty_around"] = (with_lengths(523, [0, 3, 0]), tight)
    # sharing
    c["two_poses"] = (on_poses(fixed_length(524, 8, 3), [k % 2 for k in range(24)]), tight)
    sc = fixed_length(525, 2, 3)
    c["observation_twice_thrice"] = (repeated(repeated(sc, 1, 1, 3), 0, 1, 2), tight)
    one = on_poses(fixed_length(526, 4, 3), [k // 3 for k in range(12)])
    c["one_pose_angle_0"] = (one, dict(tight, min_tri_angle=0.0))
    c["one_pose_angle_true_min"] = (one, dict(tight, min_tri_angle=DBL_TRUE_MIN))
    # the RANSAC's limits
    # ("clean": no outliers; 0.01 px of noise keeps the cosines of the residuals clear of 1, where acos turns NaN)
    clean10 = fixed_length(530, 4, 10, noise_px=0.01, outlier_frac=0.0)
    for k, o in LIMITS_10.items():
        c[f"limit10_{k}"] = (clean10, dict(tight, **o))
    short = concat(fixed_length(531, 3, 2, noise_px=0.01, outlier_frac=0.0),
                   fixed_length(532, 3, 3, noise_px=0.01, outlier_frac=0.0))
    for k, o in LIMITS_SHORT.items():
        c[f"limit23_{k}"] = (short, dict(tight, **o))
    # support
    sc = fixed_length(540, 1, 3, noise_px=0.01, outlier_frac=0.0)
    c["two_inliers"] = (edited(sc, obs_xy={2: sc["obs_xy"][2] + 0.3}), tight)
    # (seeds found with the trace: three growing local iterations in one round; a local model scored, not better)
    c["local_grows"] = (fixed_length(602, 1, 12, noise_px=2.5, outlier_frac=0.0), tight)
    c["local_not_better"] = (fixed_length(620, 1, 6, noise_px=1.0, outlier_frac=0.0), tight)
    # the same growth under a table row: the stop reads the row at the count the local optimisation reached
    c["local_grows_early_stop"] = (c["local_grows"][0], dict(tight, min_num_trials=0))
    # min_tri_angle is the angle of the pair (0, 1) at its own model: the sample passes, and the local model of all
    # three observations, a little further off, has no pair that does
    sc = fixed_length(607, 1, 3, noise_px=1.0, outlier_frac=0.0)
    first_two = dict(sc, offsets=np.array([0, 2], np.uint64), obs_pose=sc["obs_pose"][:2], obs_xy=sc["obs_xy"][:2])
    c["local_refused"] = (sc, dict(tight, min_tri_angle=_trace(first_two, tight)["angle"][0]))
    # thresholds: the residual of the 3 px observation just above max_error^2 and within it by the last bit ...
    sc = threshold_scene()
    m = largest_max_error_below(_trace(sc, dict(ONE_SAMPLE, max_error=1.0 / F))["residuals"][2])
    c["residual_above_max_error"] = (sc, dict(ONE_SAMPLE, max_error=m))
    c["residual_within_max_error"] = (sc, dict(ONE_SAMPLE, max_error=float(np.nextafter(m, np.inf))))
    # ... and a two-observation track's angle exactly at min_tri_angle and just below
    sc = fixed_length(621, 1, 2, outlier_frac=0.0)
    a = _trace(sc, tight)["angle"][0]
    c["angle_at_min_tri_angle"] = (sc, dict(tight, min_tri_angle=a))
    c["angle_below_min_tri_angle"] = (sc, dict(tight, min_tri_angle=float(np.nextafter(a, np.inf))))
    # depth (an exact depth of DBL_EPSILON cannot be planted: the point is estimated)
    X, centers = [0.2, -0.1, 5.0], [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    c["behind_one_camera"] = (axis_cameras(X, centers, flip=(1,)), tight)
    c["behind_all_cameras"] = (axis_cameras(X, centers, flip=(0, 1, 2)), tight)
    # non-finite and extreme
    plus = axis_cameras([0.0, 0.0, 5.0], [[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    minus = dict(plus, poses=np.where(plus["poses"] == 0.0, -0.0, plus["poses"]),
                 obs_xy=np.where(plus["obs_xy"] == 0.0, -0.0, plus["obs_xy"]))
    c["negative_zero"] = (concat(plus, minus), tight)
    sc = fixed_length(550, 2, 4, outlier_frac=0.0)
    c["pixel_1e200"] = (edited(sc, obs_xy={1: [1e200, sc["obs_xy"][1, 1]], 6: [sc["obs_xy"][6, 0], -1e200]}), tight)
    sc = axis_cameras(X, centers + [[1, 1, 0]])
    c["zero_pose"] = (edited(sc, poses={3: np.zeros((3, 4))}), tight)  # R X + t = 0: 0 / 0 in the residual
    p = sc["poses"][0].copy()
    p[:, 3] = [DBL_TRUE_MIN, 1e-310, -3e-320]
    c["subnormal_translation"] = (edited(sc, poses={0: p}), tight)
    return c


def digest(result) -> str:
    """sha256 over the bits of a (xyz, success, inlier_mask, {num_inliers, num_trials}) result."""
    import hashlib
    xyz, ok, mask, st = result
    h = hashlib.sha256()
    for k, a, dt in (("xyz", xyz, np.float64), ("success", ok, np.uint8), ("inlier_mask", mask, np.uint8),
                     ("num_inliers", st["num_inliers"], np.uint32), ("num_trials", st["num_trials"], np.uint64)):
        a = np.ascontiguousarray(a, dtype=dt)
        h.update(f"{k}:{a.dtype.str}:{a.shape}:".encode())
        h.update(a.tobytes())
    return h.hexdigest()


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


EDGE_CASES = edge_cases()
