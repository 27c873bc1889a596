"""Deterministic bundle-adjustment covariance problems for tests/test_ba_covariance_cpu.py,
tests/test_ba_covariance_gpu.py and tests/golden/make_bacov_ref_golden.py.  Every case is the smallest shape that takes
its path; none is a workload.  The dense passes work on 64 x 64 tiles and a panel is one tile wide, so a tile edge and a
panel edge are the same edge: the three-digit column counts below sit one below, on and one above the first and the
second of them.

A case is a dict: name, problem (the positional arguments of Context.ba_covariance), options, point_const, expect
("ok", "fail": success == 0, "refused": AMC_E_INVALID) and, for "fail", the failing column."""
from __future__ import annotations

import functools

import numpy as np

from ba_cases import NUM_FOCAL, model_params, quat_plus

TILE = 64


def scene(seed, nimg, npts, tracks="all", models=(2,), image_cameras=None, noise=0.5, outliers=0, duplicates=0,
          empty_image=None, spread=1.5):
    """A scene at the truth with noisy pixels.  tracks: "all", or a function j -> the images that see point j.
    spread: the points' half extent at depth 6 (a wide field makes the high-order distortion terms observable)."""
    import ba_ref_lib
    rng = np.random.default_rng(seed)
    icam = [0] * nimg if image_cameras is None else [int(c) for c in image_cameras]
    prm = [model_params(m) * (1.0 + 0.01 * c * (np.arange(len(model_params(m))) < NUM_FOCAL[m]))
           for c, m in enumerate(models)]
    q, t = [], []
    for i in range(nimg):
        q.append(quat_plus([0, 0, 0, 1.0], rng.uniform(-0.12, 0.12, 3) if i else np.zeros(3)))
        t.append(np.array([rng.uniform(-1.2, 1.2), rng.uniform(-0.5, 0.5), 6.0 + rng.uniform(-0.5, 0.5)]) if i
                 else np.array([0.0, 0.0, 6.0]))
    if nimg > 1 and abs(t[1][0]) < 0.5:
        t[1][0] = 0.9
    X = rng.uniform(-spread, spread, (npts, 3)) * np.array([1.0, 1.0, 1.5 / spread])
    oi, op = [], []
    for j in range(npts):
        for i in (range(nimg) if tracks == "all" else tracks(j)):
            if i != empty_image:
                oi.append(i)
                op.append(j)
    order = rng.permutation(len(oi))
    oi, op = np.array(oi, np.uint32)[order], np.array(op, np.uint32)[order]
    if duplicates:
        oi, op = np.concatenate([oi, oi[:duplicates]]), np.concatenate([op, op[:duplicates]])
    xy = np.zeros((oi.size, 2))
    for k in range(oi.size):
        i, j = int(oi[k]), int(op[k])
        xy[k] = ba_ref_lib.observation(models[icam[i]], prm[icam[i]], q[i], t[i], X[j], [0.0, 0.0])[1]
    xy += noise * rng.standard_normal(xy.shape)
    for k in rng.choice(oi.size, outliers, replace=False) if outliers else []:
        xy[k] += rng.uniform(-20, 20, 2)
    return dict(models=list(models), camera_params=prm, image_cameras=np.array(icam, np.uint32), qvec=np.array(q),
                tvec=np.array(t), xyz=X, obs_image=oi, obs_point=op, obs_xy=xy)


def masks(sc, cameras="const", gauge=True, pose_const=None):
    """camera_const (C, 12) and pose_const (I, 6).  cameras: "const", "all" (every parameter of the model variable) or
    "focal_extra" (bundle_adjustment's default groups).  gauge: the first pose and the second pose's x translation are
    constant.  pose_const = {image: columns} adds constant columns."""
    cc = np.ones((len(sc["models"]), 12), np.uint8)
    for c, m in enumerate(sc["models"]):
        n, nf = len(model_params(m)), NUM_FOCAL[m]
        if cameras == "all":
            cc[c, :n] = 0
        elif cameras == "focal_extra":
            cc[c, :nf] = 0
            cc[c, nf + 2:n] = 0
    pc = np.zeros((len(sc["image_cameras"]), 6), np.uint8)
    if gauge:
        pc[0, :] = 1
        if pc.shape[0] > 1:
            pc[1, 3] = 1
    for i, cols in (pose_const or {}).items():
        pc[i, list(cols)] = 1
    return cc, pc


def problem(sc, cc, pc):
    return (sc["models"], sc["camera_params"], cc, sc["image_cameras"], sc["qvec"], sc["tvec"], pc, sc["xyz"],
            sc["obs_image"], sc["obs_point"], sc["obs_xy"])


def num_columns(cc, pc, models):
    return int((pc == 0).sum() + sum((cc[c, :len(model_params(m))] == 0).sum() for c, m in enumerate(models)))


def _case(name, sc, cc, pc, options=None, point_const=None, expect="ok", column=None, note=""):
    return dict(name=name, problem=problem(sc, cc, pc), options=dict(options or {}), point_const=point_const,
                expect=expect, column=column, note=note, m=num_columns(cc, pc, sc["models"]))


def _columns_case(m, seed):
    """Exactly m pose columns: the gauge, then as many trailing coordinates of the last image constant as it takes."""
    nimg = (m + 1 + 5) // 6 + 1
    sc = scene(seed, nimg, 12)
    spare = 6 * (nimg - 1) - 1 - m
    free = [k for k in range(6) if not (nimg == 2 and k == 3)]  # (the gauge already holds image 1's x translation)
    cc, pc = masks(sc, pose_const={nimg - 1: free[len(free) - spare:]} if spare else None)
    assert num_columns(cc, pc, sc["models"]) == m
    return sc, cc, pc


_EDGE_NOTES = {1: "a single column", 5: "one image short of a full pose", 6: "one full pose",
               63: "one below the first tile and panel edge", 64: "on the first edge: one tile, no panel below it",
               65: "one above the first edge: the first panel solve and trailing update, a one-column second tile",
               127: "one below the second edge", 128: "on the second edge: two panel steps",
               129: "one above the second edge", 257: "four full tiles and one column: inverse block rows of 5 tiles",
               599: "ten tiles, the last 23 columns wide: several tiles in both directions"}


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for k, m in enumerate(_EDGE_NOTES):
        sc, cc, pc = _columns_case(m, 100 + k)
        out.append(_case(f"columns_{m}", sc, cc, pc, note=_EDGE_NOTES[m]))
    # every camera model with variable intrinsics (one shared camera, 4 images, 24 points), then all eleven in one
    for model in range(11):
        # (FULL_OPENCV's rational terms are observable only over a wide field with more points)
        sc = scene(200 + model, 6, 60, models=(6,), noise=0.3, spread=6.5) if model == 6 else \
            scene(200 + model, 4, 24, models=(model,), noise=0.3)
        cc, pc = masks(sc, cameras="all")
        out.append(_case(f"model_{model}", sc, cc, pc, note="every parameter of the model variable"))
    sc = scene(220, 23, 40, models=tuple(range(11)), image_cameras=list(range(11)) * 2 + [3], noise=0.3, spread=6.5)
    cc, pc = masks(sc, cameras="focal_extra")
    out.append(_case("eleven_models", sc, cc, pc, note="eleven cameras of different widths with two images each, camera 3 with three"))
    sc = scene(221, 6, 30, models=(4,) * 6, image_cameras=range(6), noise=0.3)
    cc, pc = masks(sc, cameras="focal_extra")
    out.append(_case("camera_per_image", sc, cc, pc))
    sc = scene(222, 6, 30, models=(4,), noise=0.3)
    cc, pc = masks(sc, cameras="focal_extra")
    out.append(_case("camera_shared", sc, cc, pc, note="one camera block joining six images' partials"))
    # tracks of 2, 3, 63, 64 and 65 observations among 65 images
    # (24 points seen by all 65 images keep every pose determined)
    lengths = [65] * 24 + [2, 3, 63, 64]
    sc = scene(230, 65, len(lengths), tracks=lambda j: [(7 * j + i) % 65 for i in range(lengths[j])], models=(2,))
    cc, pc = masks(sc, cameras="focal_extra")
    out.append(_case("track_lengths", sc, cc, pc, note="tracks of 2, 3, 63, 64, 65"))
    # an image with more than 64 observations: the second trip of the per-image sum's lanes
    sc = scene(231, 3, 70, models=(2,))
    cc, pc = masks(sc, cameras="focal_extra")
    out.append(_case("segment_70", sc, cc, pc, note="70 observations per image: lanes 0 .. 5 add two terms"))
    sc = scene(232, 4, 20, duplicates=5)
    cc, pc = masks(sc, cameras="focal_extra")
    out.append(_case("duplicate_observations", sc, cc, pc, note="an image sees a point twice"))
    sc = scene(233, 5, 40)
    cc, pc = masks(sc, cameras="focal_extra")
    out.append(_case("points_mixed_const", sc, cc, pc, point_const=(np.arange(40) % 3 == 0).astype(np.uint8)))
    cc, pc = masks(sc, cameras="focal_extra", gauge=False)
    out.append(_case("points_all_const", sc, cc, pc, point_const=np.ones(40, np.uint8),
                     note="no point block: S = B, no destination block, no gauge needed"))
    sc = scene(234, 5, 40, outliers=6, noise=1.0)
    cc, pc = masks(sc, cameras="focal_extra")
    for loss in ("TRIVIAL", "SOFT_L1", "CAUCHY"):
        out.append(_case(f"loss_{loss.lower()}", sc, cc, pc, options=dict(loss_function_type=loss, loss_function_scale=2.0)))
    for name, damping in (("0", 0.0), ("default", 1e-8), ("1", 1.0)):
        out.append(_case(f"damping_{name}", sc, cc, pc, options=dict(damping=damping)))
    # the constant pose columns a config produces: a whole pose, a subset of the position, every pose
    sc = scene(235, 6, 30)
    cc, pc = masks(sc, cameras="focal_extra", pose_const={3: range(6)})
    out.append(_case("pose_const_whole", sc, cc, pc))
    cc, pc = masks(sc, cameras="focal_extra", pose_const={2: [3], 4: [4, 5], 5: [3, 4, 5]})
    out.append(_case("pose_const_positions", sc, cc, pc))
    cc, pc = masks(sc, cameras="focal_extra", gauge=False, pose_const={i: range(6) for i in range(6)})
    out.append(_case("pose_const_all", sc, cc, pc, note="only camera columns"))
    # an image with a variable pose and no observations: its diagonal entries are exactly 0
    sc = scene(236, 5, 20, empty_image=3)
    cc, pc = masks(sc)
    out.append(_case("empty_image_variable", sc, cc, pc, expect="fail", column=int((pc[:3] == 0).sum()),
                     note="S_qq == 0 at the first column of image 3"))
    cc, pc = masks(sc, pose_const={3: range(6)})
    out.append(_case("empty_image_constant", sc, cc, pc))
    sc = scene(237, 3, 10)
    cc, pc = masks(sc, gauge=False, pose_const={i: range(6) for i in range(3)})
    out.append(_case("no_columns", sc, cc, pc, note="m == 0: empty results, no device use"))
    return out


def refused_cases():
    """Problems the entry point refuses with AMC_E_INVALID before the device is used."""
    out = []
    # 8193 columns: 1365 images without observations (8190) behind 3 observed ones with 3 columns
    sc = scene(300, 3, 6)
    n = 1365
    sc["image_cameras"] = np.concatenate([sc["image_cameras"], np.zeros(n, np.uint32)])
    sc["qvec"] = np.concatenate([sc["qvec"], np.tile([0, 0, 0, 1.0], (n, 1))])
    sc["tvec"] = np.concatenate([sc["tvec"], np.zeros((n, 3))])
    cc, pc = masks(sc, gauge=False, pose_const={0: range(6), 1: range(6), 2: range(3)})
    assert num_columns(cc, pc, sc["models"]) == 8193
    out.append(_case("columns_8193", sc, cc, pc, expect="refused"))
    for kind, index in dict(camera_params=(0, 1), qvec=(1, 2), tvec=(2, 0), xyz=(4, 1), obs_xy=(7, 0)).items():
        sc = scene(301, 3, 10)
        if kind == "camera_params":
            sc[kind][index[0]][index[1]] = np.nan
        else:
            sc[kind][index] = np.nan
        cc, pc = masks(sc, cameras="focal_extra")
        out.append(_case(f"nan_{kind}", sc, cc, pc, expect="refused"))
    return out


def by_name(name):
    return next(c for c in cases() + refused_cases() if c["name"] == name)


def digest(result) -> str:
    """sha256 over a result's flags, column map, matrix and point blocks, bit for bit."""
    import hashlib
    h = hashlib.sha256()
    h.update(f'{int(result["success"])} {result["failed_column"]} {result["num_columns"]}'.encode())
    h.update(np.float64(result["min_pivot_ratio"]).tobytes())
    h.update(np.ascontiguousarray(result["column_owner"], np.uint32).tobytes())
    h.update(np.ascontiguousarray(result["column_coord"], np.uint32).tobytes())
    for k in ("matrix", "point_cov"):
        if result[k] is not None:
            h.update(np.ascontiguousarray(result[k], np.float64).tobytes())
    if result["point_present"] is not None:
        h.update(np.ascontiguousarray(result["point_present"], np.uint8).tobytes())
    return h.hexdigest()
