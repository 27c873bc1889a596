"""Deterministic synthetic point filter problems for tests/test_filter_cpu.py, tests/test_filter_gpu.py
and tests/golden/make_filter_ref_golden.py: seeded scenes whose tracks have given lengths, numbers of gross outliers and
baselines, the flat problem of Context.filter_points3d, and the lists of cases (CASES, EDGE_CASES) the fixture freezes."""
from __future__ import annotations

import functools

import numpy as np

import ba_cases

MODEL_NAMES = ba_cases.MODEL_NAMES
DBL_EPSILON = float(np.finfo(np.float64).eps)
DBL_MAX = float(np.finfo(np.float64).max)
WAVE_CLASS_MIN = 64  # 16.4: a selected track of this many elements or more is the wave kernel's
RESULT_KEYS = ("obs_sq_error", "obs_deleted", "point_verdict", "point_error", "num_filtered")


def scene(seed=0, specs=((3, 0, False),), nimg=6, models=(2,), image_cameras=None, cluster=3, noise=0.5, dup=None):
    """A flat problem.  specs: one (track length, gross outliers, narrow) per point.  The first `cluster` images stand
    within 0.01 of each other (a narrow point is seen by them alone, under far less than a degree), the others are
    spread over a baseline of 2.4 at distance 6 (ba_cases.scene's layout).  Image i has camera image_cameras[i] (default
    i modulo the number of cameras).  The pixels are the reference's own projections plus Gaussian noise; a gross outlier
    is moved by 20 to 40 pixels.  dup = j: point j's second element names its first element's image again."""
    import ba_ref_lib
    rng = np.random.default_rng(seed)
    models = [int(m) for m in models]
    icam = [i % len(models) for i in range(nimg)] if image_cameras is None else [int(c) for c in image_cameras]
    assert len(icam) == nimg and max(icam, default=0) < len(models)
    prm = [ba_cases.model_params(m) * (1.0 + 0.01 * c * (np.arange(len(ba_cases.model_params(m))) < ba_cases.NUM_FOCAL[m]))
           for c, m in enumerate(models)]
    q, t = [], []
    for i in range(nimg):
        q.append(ba_cases.quat_plus([0, 0, 0, 1.0], rng.uniform(-0.12, 0.12, 3)))
        if i < cluster:
            t.append(np.array([0.3, 0.1, 6.0]) + rng.uniform(-0.005, 0.005, 3))
        else:
            t.append(np.array([rng.uniform(-1.2, 1.2), rng.uniform(-0.5, 0.5), 6.0 + rng.uniform(-0.5, 0.5)]))
    for i in range(min(cluster, nimg)):  # the cluster shares a rotation: its centres are as close as its translations
        q[i] = q[0]
    X = rng.uniform(-1.5, 1.5, (len(specs), 3))
    off, oi, xy = [0], [], []
    for j, (L, nout, narrow) in enumerate(specs):
        pool = min(cluster, nimg) if narrow else nimg
        assert L <= pool and nout <= L, (j, L, nout, narrow)
        imgs = rng.choice(pool, L, replace=False)
        if dup == j and L > 1:
            imgs[1] = imgs[0]
        out = set(rng.choice(L, nout, replace=False).tolist()) if nout else set()
        for k, i in enumerate(imgs):
            c = icam[int(i)]
            _, r, _, _, _ = ba_ref_lib.observation(models[c], prm[c], q[int(i)], t[int(i)], X[j], [0.0, 0.0])
            p = np.array(r) + noise * rng.standard_normal(2)
            if k in out:
                a = rng.uniform(0, 2 * np.pi)
                p = p + rng.uniform(20, 40) * np.array([np.cos(a), np.sin(a)])
            oi.append(int(i))
            xy.append(p)
        off.append(len(oi))
    return dict(models=models, camera_params=prm, image_cameras=np.array(icam, np.uint32), qvec=np.array(q).reshape(-1, 4),
                tvec=np.array(t).reshape(-1, 3), xyz=X, track_offsets=np.array(off, np.uint64),
                obs_image=np.array(oi, np.uint32), obs_xy=np.array(xy, np.float64).reshape(-1, 2))


def random_specs(seed, n, lengths=(2, 3, 4, 5), p_out=0.15, p_narrow=0.15, cluster=3):
    """n point specs: lengths cycle through `lengths`; a point is narrow with p_narrow (its length cut to the cluster's
    size), and has one gross outlier with p_out (two with p_out squared)."""
    rng = np.random.default_rng(1000 + seed)
    specs = []
    for j in range(n):
        L = lengths[j % len(lengths)]
        narrow = bool(rng.random() < p_narrow)
        if narrow:
            L = min(L, cluster)
        nout = int(rng.random() < p_out) + int(rng.random() < p_out * p_out)
        specs.append((L, min(nout, L), narrow))
    return specs


def problem(sc):
    """The positional arguments of Context.filter_points3d / filter_ref_lib.filter_points3d for the scene."""
    return (list(sc["models"]), sc["camera_params"], sc["image_cameras"], sc["qvec"], sc["tvec"], sc["xyz"],
            sc["track_offsets"], sc["obs_image"], sc["obs_xy"])


# the lengths 16.7 asks for in one call, with and without outliers, wide and narrow: both classes and their boundary,
# marked == L - 2 and marked == L - 1 in both, and a narrow track on either side of the boundary (the whole pair loop)
_LENGTHS = [(1, 0, False), (2, 0, False), (3, 0, False), (5, 1, False), (63, 3, False), (64, 2, False), (65, 4, False),
            (129, 7, False), (300, 20, False), (2, 0, True), (3, 1, True), (63, 0, True), (64, 0, True), (65, 1, True),
            (70, 2, True), (3, 1, False), (3, 2, False), (5, 3, False), (5, 4, False), (64, 62, False), (64, 63, False),
            (65, 63, False), (65, 64, False), (63, 61, False), (63, 62, False), (2, 1, False), (2, 2, False), (1, 1, False)]
_LENGTHS_SCENE = dict(seed=7, specs=_LENGTHS, nimg=300, models=(2, 1), cluster=70)


def _special(sc, what):
    """NaN / inf in one input value, or the depths at the DBL_EPSILON boundary"""
    sc = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else [np.array(p, copy=True) for p in v] if k == "camera_params" else v)
          for k, v in sc.items()}
    v = {"nan": np.nan, "inf": np.inf}[what.split("_")[0]] if what.split("_")[0] in ("nan", "inf") else None
    where = what.split("_", 1)[1] if v is not None else what
    if where == "pixel":
        sc["obs_xy"][2, 0] = v
        sc["obs_xy"][int(sc["track_offsets"][5]), 1] = v
    elif where == "point":
        sc["xyz"][1, 2] = v
        sc["xyz"][6, 0] = v
    elif where == "pose":
        sc["qvec"][1, 0] = v
        sc["tvec"][4, 2] = v
    elif where == "camera":
        sc["camera_params"][0][0] = v
        sc["camera_params"][1][-1] = v
    elif where == "depth_eps":
        # image 0: the identity at the origin, so a point's depth in it is its z, exactly
        sc["qvec"][0] = [0.0, 0.0, 0.0, 1.0]
        sc["tvec"][0] = [0.0, 0.0, 0.0]
        for j, z in ((0, DBL_EPSILON), (1, np.nextafter(DBL_EPSILON, 0.0)), (2, np.nextafter(DBL_EPSILON, 1.0))):
            sc["xyz"][j] = [1e-17 * (j + 1), -1e-17, z]
            sc["obs_image"][int(sc["track_offsets"][j])] = 0
    else:
        raise KeyError(what)
    return sc


_SPECIAL_SCENE = dict(seed=11, specs=[(4, 0, False)] * 6 + [(3, 0, False)] * 4, nimg=6, models=(2, 4), cluster=0)

# name -> (scene arguments, call arguments).  "special" in the scene arguments names a _special change; "select" in the
# call arguments is "none", "one" (the middle point) or "all_but_one" (all but the middle point).
CASES = {"lengths": (_LENGTHS_SCENE, {})}
for _m in range(11):
    CASES[f"model_{MODEL_NAMES[_m]}"] = (dict(seed=30 + _m, specs=random_specs(_m, 40), nimg=5, models=(_m,)), {})
CASES["mixed_models"] = (dict(seed=50, specs=random_specs(50, 80), nimg=13, models=tuple(range(11))), {})
CASES["mixed_models_reversed"] = (dict(seed=50, specs=random_specs(50, 80), nimg=13, models=tuple(reversed(range(11)))), {})

EDGE_CASES = {}
for _n in (0, 1, 63, 64, 65, 255, 256, 257):
    EDGE_CASES[f"points_{_n}"] = (dict(seed=60 + _n % 7, specs=random_specs(_n, _n), nimg=6, models=(2,)), {})
EDGE_CASES["same_image_twice"] = (dict(seed=70, specs=[(3, 0, False), (2, 0, False), (5, 1, False), (3, 0, True)], nimg=6,
                                       models=(4,), dup=0), {})
EDGE_CASES["same_image_twice_len2"] = (dict(seed=70, specs=[(3, 0, False), (2, 0, False), (5, 1, False)], nimg=6,
                                            models=(4,), dup=1), {})
EDGE_CASES["all_marks"] = (_LENGTHS_SCENE, dict(max_reproj_error=0.0))
EDGE_CASES["no_marks"] = (_LENGTHS_SCENE, dict(max_reproj_error=np.inf))
EDGE_CASES["angle_0"] = (_LENGTHS_SCENE, dict(min_tri_angle=0.0))
EDGE_CASES["angle_180"] = (_LENGTHS_SCENE, dict(min_tri_angle=180.0))
for _s in ("none", "one", "all_but_one"):
    EDGE_CASES[f"select_{_s}"] = (_LENGTHS_SCENE, dict(select=_s))
    EDGE_CASES[f"select_{_s}_small"] = (dict(seed=65, specs=random_specs(65, 65), nimg=6, models=(2,)), dict(select=_s))
for _w in ("nan_pixel", "inf_pixel", "nan_point", "inf_point", "nan_pose", "inf_pose", "nan_camera", "inf_camera",
           "depth_eps"):
    EDGE_CASES[_w] = (dict(_SPECIAL_SCENE, special=_w), {})
ALL_CASES = {**CASES, **EDGE_CASES}


@functools.lru_cache(maxsize=None)
def case_scene(name):
    args = dict(ALL_CASES[name][0])
    special = args.pop("special", None)
    sc = scene(**args)
    return _special(sc, special) if special else sc


def case_call(name):
    """(positional arguments, keyword arguments) of filter_points3d for the case"""
    sc = case_scene(name)
    kw = dict(ALL_CASES[name][1])
    select = kw.pop("select", None)
    npts = len(sc["xyz"])
    if select is not None:
        sel = np.zeros(npts, np.uint8) if select in ("none", "one") else np.ones(npts, np.uint8)
        if select != "none" and npts:
            sel[npts // 2] = 1 if select == "one" else 0
        kw["selected"] = sel
    return problem(sc), kw


@functools.lru_cache(maxsize=None)
def reference(name, errors_only=False):
    """The CPU reference's result for the case, computed once per process; the arrays are read-only."""
    import filter_ref_lib
    args, kw = case_call(name)
    out = filter_ref_lib.filter_points3d(*args, errors_only=errors_only, **kw)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def bits(a):
    """the doubles' bits, every NaN as the one canonical NaN: IEEE 754 pins neither a NaN's sign nor its payload, and
    the host's and the device's arithmetic propagate them differently"""
    a = np.array(a, dtype=np.float64).reshape(-1)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def digest(result) -> str:
    """sha256 over the result's arrays and count, bit for bit (bits())."""
    import hashlib
    h = hashlib.sha256()
    h.update(bits(result["obs_sq_error"]).tobytes())
    h.update(np.ascontiguousarray(result["obs_deleted"], np.uint8).tobytes())
    h.update(np.ascontiguousarray(result["point_verdict"], np.uint8).tobytes())
    h.update(bits(result["point_error"]).tobytes())
    h.update(str(int(result["num_filtered"])).encode())
    return h.hexdigest()


def same_bits(a, b) -> bool:
    """two results agree bit for bit (NaNs by their bits)"""
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("obs_sq_error", "point_error")) and \
        np.array_equal(np.asarray(a["obs_deleted"], bool), np.asarray(b["obs_deleted"], bool)) and \
        np.array_equal(a["point_verdict"], b["point_verdict"]) and int(a["num_filtered"]) == int(b["num_filtered"])


# ---- through Python: a Reconstruction's flat problem, as FlattenForFilter builds it (16.5) ----------------------------
def flatten_reconstruction(r, ids=None):
    """(positional arguments, selected) of filter_points3d for a pycolmap Reconstruction: cameras, images and points in
    the maps' order, the observations in track order; ids = None selects every point."""
    cam_index = {cid: k for k, cid in enumerate(r.cameras)}
    img_index = {iid: k for k, iid in enumerate(r.images)}
    models = [MODEL_NAMES.index(c.model.name if hasattr(c.model, "name") else str(c.model)) for c in r.cameras.values()]
    prm = [np.array(c.params, np.float64) for c in r.cameras.values()]
    icam = [cam_index[im.camera_id] for im in r.images.values()]
    q = [np.array(im.cam_from_world.rotation.quat, np.float64) for im in r.images.values()]
    t = [np.array(im.cam_from_world.translation, np.float64) for im in r.images.values()]
    X, off, oi, xy, sel = [], [0], [], [], []
    for pid, p in r.points3D.items():
        X.append(np.array(p.xyz))
        for e in p.track.elements:
            oi.append(img_index[e.image_id])
            xy.append(np.array(r.images[e.image_id].points2D[e.point2D_idx].xy))
        off.append(len(oi))
        sel.append(1 if ids is None or pid in ids else 0)
    args = (models, prm, np.array(icam, np.uint32), np.array(q).reshape(-1, 4), np.array(t).reshape(-1, 3),
            np.array(X).reshape(-1, 3), np.array(off, np.uint64), np.array(oi, np.uint32), np.array(xy).reshape(-1, 2))
    return args, (None if ids is None else np.array(sel, np.uint8))


def apply_result(r_state, res):
    """ApplyFilterResult restated on model_state(r): the state the model must have after the result is applied"""
    out = []
    o0 = 0
    for j, (pid, elements, err) in enumerate(r_state):
        L = len(elements)
        v = int(res["point_verdict"][j])
        if v == 1:
            out.append((pid, list(elements), err))
        elif v == 0:
            keep = [e for k, e in enumerate(elements) if not res["obs_deleted"][o0 + k]]
            out.append((pid, keep, float(res["point_error"][j])))
        o0 += L
    return out


def model_state(r):
    """[(point id, [(image id, point2D index)], error)] in the points' order"""
    return [(pid, [(e.image_id, e.point2D_idx) for e in p.track.elements], p.error) for pid, p in r.points3D.items()]


def point2d_ids(r):
    return {iid: [p.point3D_id for p in im.points2D] for iid, im in r.images.items()}
