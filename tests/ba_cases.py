"""Deterministic synthetic bundle adjustment problems for tests/test_ba_cpu.py, tests/test_ba_gpu.py and
tests/golden/make_ba_ref_golden.py: seeded scenes with every point in front of every camera, the flat problem of
Context.bundle_adjust, and the lists of cases (CASES, EDGE_CASES) the two fixtures freeze."""
from __future__ import annotations

import numpy as np

MODEL_NAMES = ["SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "OPENCV_FISHEYE", "FULL_OPENCV", "FOV",
               "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE"]
NUM_FOCAL = [1, 2, 1, 1, 2, 2, 2, 2, 1, 1, 2]
_F, _CX, _CY = 800.0, 500.0, 400.0
_EXTRA = {0: [], 1: [], 2: [0.05], 3: [0.05, -0.02], 4: [0.05, -0.02, 0.001, -0.001], 5: [0.02, -0.01, 0.003, -0.001],
          6: [0.05, -0.02, 0.001, -0.001, 0.005, 0.01, -0.005, 0.002], 7: [0.6], 8: [0.02], 9: [0.02, -0.01],
          10: [0.02, -0.01, 0.001, -0.001, 0.002, 0.001, 0.0005, -0.0005]}


def model_params(model: int) -> np.ndarray:
    f = [_F] if NUM_FOCAL[model] == 1 else [_F, _F * 1.01]
    return np.array(f + [_CX, _CY] + _EXTRA[model], np.float64)


def param_groups(model: int):
    """(focal, principal point, extra) parameter indices of the model, COLMAP's *_idxs."""
    nf = NUM_FOCAL[model]
    n = len(model_params(model))
    return list(range(nf)), [nf, nf + 1], list(range(nf + 2, n))


def quat_plus(q, d):
    """EigenQuaternionManifold::Plus for q = (x, y, z, w) with numpy's sin / cos."""
    d = np.asarray(d, np.float64)
    n = np.sqrt(d @ d)
    if n == 0.0:
        return np.array(q, np.float64)
    s = np.sin(n) / n
    a = np.array([s * d[0], s * d[1], s * d[2], np.cos(n)])
    q = np.asarray(q, np.float64)
    return np.array([a[3] * q[0] + a[0] * q[3] + a[1] * q[2] - a[2] * q[1],
                     a[3] * q[1] - a[0] * q[2] + a[1] * q[3] + a[2] * q[0],
                     a[3] * q[2] + a[0] * q[1] - a[1] * q[0] + a[2] * q[3],
                     a[3] * q[3] - a[0] * q[0] - a[1] * q[1] - a[2] * q[2]])


def rotate(q, X):
    """q * X for unit q = (x, y, z, w); X (..., 3)."""
    qv, w = np.asarray(q[:3]), q[3]
    uv = 2.0 * np.cross(qv, X)
    return X + w * uv + np.cross(qv, uv)


def scene(seed=0, nimg=3, npts=40, model=2, cameras="shared", tracks="all", noise=0.0, perturb=1.0, outliers=0,
          models=None, image_cameras=None, drop_image=None, duplicates=0, move_point=None):
    """A scene and its flat problem.  cameras: "shared" (one camera), "per_image", or "mixed" (camera 0 for all images
    but the last, camera 1 for the last alone).  tracks: "all" (every image sees every point) or "mixed" (even points
    are seen by every image, odd ones by two).  The start is the truth perturbed by `perturb` times (0.01 rad, 0.05 in
    translation and points, 2 % in the focal lengths, 10 % of the extra parameters); the first pose and the second
    pose's x translation, which bundle_adjustment keeps constant, start at the truth.  The projections come from the
    reference's own camera model (ba_ref_lib.observation at the truth), plus Gaussian pixel noise.
    For EDGE_CASES: `models` gives each camera its own model (a camera that `image_cameras`, the camera index per image,
    does not name is one without images); `drop_image` leaves that image without observations; `duplicates` appends the
    first so many observations again at pixels shifted by 0.5; `move_point` = (j, xyz) puts point j's start there."""
    import ba_ref_lib
    rng = np.random.default_rng(seed)
    icam = {"shared": [0] * nimg, "per_image": list(range(nimg)), "mixed": [0] * (nimg - 1) + [1]}[cameras] \
        if image_cameras is None else [int(c) for c in image_cameras]
    models = [model] * (max(icam) + 1) if models is None else [int(m) for m in models]
    assert len(icam) == nimg and max(icam) < len(models)
    true_prm = [model_params(m) * (1.0 + 0.01 * c * (np.arange(len(model_params(m))) < NUM_FOCAL[m]))
                for c, m in enumerate(models)]
    q_true, t_true = [], []
    for i in range(nimg):
        q_true.append(quat_plus([0, 0, 0, 1.0], rng.uniform(-0.12, 0.12, 3) if i else np.zeros(3)))
        t_true.append(np.array([rng.uniform(-1.2, 1.2), rng.uniform(-0.5, 0.5), 6.0 + rng.uniform(-0.5, 0.5)]) if i
                      else np.array([0.0, 0.0, 6.0]))
    if nimg > 1 and abs(t_true[1][0]) < 0.5:
        t_true[1][0] = 0.9  # a baseline for the gauge's scale
    X_true = rng.uniform(-1.5, 1.5, (npts, 3))
    oi, op = [], []
    for j in range(npts):
        seen = range(nimg) if tracks == "all" or j % 2 == 0 else sorted({j % nimg, (j + 3) % nimg if nimg > 3 else (j + 1) % nimg})
        for i in seen:
            if i == drop_image:
                continue
            oi.append(i)
            op.append(j)
    # a fixed shuffle: the observations arrive in no particular order
    order = rng.permutation(len(oi))
    oi, op = np.array(oi, np.uint32)[order], np.array(op, np.uint32)[order]
    xy = np.zeros((oi.size, 2))
    for k in range(oi.size):
        i, j = int(oi[k]), int(op[k])
        c = icam[i]
        _, r, _, _, _ = ba_ref_lib.observation(models[c], true_prm[c], q_true[i], t_true[i], X_true[j], [0.0, 0.0])
        xy[k] = r
    xy += noise * rng.standard_normal(xy.shape)
    for k in rng.choice(oi.size, outliers, replace=False) if outliers else []:
        xy[k] += rng.uniform(-40, 40, 2)
    q0, t0 = [np.array(q) for q in q_true], [np.array(t) for t in t_true]
    for i in range(1, nimg):
        q0[i] = quat_plus(q_true[i], perturb * rng.uniform(-0.01, 0.01, 3))
        d = perturb * rng.uniform(-0.05, 0.05, 3)
        if i == 1:
            d[0] = 0.0
        t0[i] = t_true[i] + d
    X0 = X_true + perturb * rng.uniform(-0.05, 0.05, X_true.shape)
    prm0 = []
    for m, p in zip(models, true_prm):
        p = p.copy()
        nf = NUM_FOCAL[m]
        p[:nf] *= 1.0 + 0.02 * perturb
        p[nf + 2:] *= 1.0 + 0.1 * perturb
        prm0.append(p)
    if duplicates:
        oi, op = np.concatenate([oi, oi[:duplicates]]), np.concatenate([op, op[:duplicates]])
        xy = np.concatenate([xy, xy[:duplicates] + 0.5])
    if move_point is not None:
        X0[move_point[0]] = move_point[1]
    return dict(model=model, models=models, image_cameras=np.array(icam, np.uint32), true_params=true_prm,
                true_qvec=np.array(q_true), true_tvec=np.array(t_true), true_xyz=X_true, camera_params=prm0, qvec=np.array(q0), tvec=np.array(t0),
                xyz=X0, obs_image=oi, obs_point=op, obs_xy=xy)


def masks(sc, refine_focal_length=True, refine_principal_point=False, refine_extra_params=True, refine_extrinsics=True,
          pose_const=None):
    """The constant masks bundle_adjustment derives from BundleAdjustmentOptions (15.1): camera_const (C, 12) and
    pose_const (I, 6).  `pose_const` = {image: tangent columns} makes those columns constant as well (the C ABI takes any
    mask)."""
    ncam, nimg = len(sc["camera_params"]), len(sc["image_cameras"])
    cc = np.ones((ncam, 12), np.uint8)
    for c, model in enumerate(sc["models"]):
        focal, pp, extra = param_groups(model)
        for flag, idx in ((refine_focal_length, focal), (refine_principal_point, pp), (refine_extra_params, extra)):
            if flag:
                cc[c, idx] = 0
    pc = np.zeros((nimg, 6), np.uint8)
    pc[0, :] = 1
    if nimg > 1:
        pc[1, 3] = 1
    if not refine_extrinsics:
        pc[:] = 1
    for i, columns in (pose_const or {}).items():
        pc[i, list(columns)] = 1
    return cc, pc


def problem(sc, **flags):
    """The positional arguments of Context.bundle_adjust / ba_ref_lib.bundle_adjust for the scene."""
    cc, pc = masks(sc, **flags)
    return (list(sc["models"]), sc["camera_params"], cc, sc["image_cameras"], sc["qvec"],
            sc["tvec"], pc, sc["xyz"], sc["obs_image"], sc["obs_point"], sc["obs_xy"])


# name -> (scene arguments, refine flags, solver options).  The shapes are the smallest at which the kernels can go
# wrong (15.10): the minimum, the wave-boundary lengths of the per-image sums, more than one 256-lane block of points with
# tracks of length 2 and 9, every camera sharing pattern, every model, every flag, every loss, a rejected step and a PCG
# run that ends at its cap.  They all have at most 9 images and cameras, one model per problem, every image observed, the
# gauge's constant pattern alone and an end at MAX_ITERATIONS: EDGE_CASES below has the rest.
CASES = {"min2": (dict(seed=1, nimg=2, npts=8, model=2, noise=0.3), {}, dict(max_num_iterations=5))}
for _n in (63, 64, 65, 129):
    CASES[f"wave{_n}"] = (dict(seed=10 + _n, nimg=3, npts=_n, model=1, noise=0.3), {}, dict(max_num_iterations=3))
for _c in ("shared", "per_image", "mixed"):
    CASES[f"multi9_{_c}"] = (dict(seed=20, nimg=9, npts=300, model=2, cameras=_c, tracks="mixed", noise=0.3), {},
                            dict(max_num_iterations=4))
for _m in range(11):
    CASES[f"model_{MODEL_NAMES[_m]}"] = (dict(seed=30 + _m, nimg=3, npts=40, model=_m, noise=0.3), {},
                                        dict(max_num_iterations=3))
CASES["flags_intrinsics_const"] = (dict(seed=50, nimg=4, npts=50, model=4, noise=0.3),
                                   dict(refine_focal_length=False, refine_extra_params=False), dict(max_num_iterations=3))
CASES["flags_no_extrinsics"] = (dict(seed=51, nimg=4, npts=50, model=4, noise=0.3), dict(refine_extrinsics=False),
                                dict(max_num_iterations=3))
CASES["flags_principal_point"] = (dict(seed=52, nimg=4, npts=50, model=4, noise=0.3), dict(refine_principal_point=True),
                                  dict(max_num_iterations=3))
for _l in ("SOFT_L1", "CAUCHY"):
    CASES[f"loss_{_l}"] = (dict(seed=60, nimg=4, npts=60, model=2, noise=1.0, outliers=6), {},
                           dict(max_num_iterations=4, loss_function_type=_l, loss_function_scale=2.0))
CASES["rejected_step"] = (dict(seed=1, nimg=2, npts=8, model=2, noise=0.3), {}, dict(max_num_iterations=6))
CASES["pcg_cap"] = (dict(seed=71, nimg=5, npts=60, model=2, cameras="per_image", noise=0.3), {},
                    dict(max_num_iterations=3, max_linear_solver_iterations=3))

RESULT_ARRAYS = ("camera_params", "qvec", "tvec", "xyz")
RESULT_STATS = ("num_variable_parameters", "initial_cost", "final_cost", "num_successful_steps", "num_unsuccessful_steps",
                "num_pcg_iterations", "num_pcg_stops_residual", "num_pcg_stops_cap", "termination")


# the accuracy cases of tests/test_ba_cpu.py (scipy on the same problem): pixel noise, one case per loss, shared intrinsics,
# a camera per image and cameras of different models
ACCURACY_CASES = {"trivial_shared": (dict(seed=80, nimg=4, npts=25, model=2, noise=0.5), "TRIVIAL"),
                  "soft_l1_per_image": (dict(seed=81, nimg=4, npts=25, model=2, cameras="per_image", noise=0.5), "SOFT_L1"),
                  "cauchy_shared": (dict(seed=82, nimg=4, npts=25, model=4, noise=0.5), "CAUCHY"),
                  # three models of different parameter counts (3, 8, 4) in one problem; tests/ba_scipy.py restates them
                  "trivial_mixed_models": (dict(seed=84, nimg=5, npts=25, noise=0.5, models=[0, 4, 2],
                                                image_cameras=[0, 1, 2, 0, 1]), "TRIVIAL")}
NOISE_FREE_CASE = dict(seed=83, nimg=4, npts=25, model=2, noise=0.0)


_M = {n: k for k, n in enumerate(MODEL_NAMES)}
_STOP_SCENE = dict(NOISE_FREE_CASE, noise=0.5)
_MANY260 = dict(seed=103, nimg=260, npts=12, model=2, cameras="per_image", tracks="mixed", noise=0.3)

# name -> (scene arguments with the refine flags under "flags" and the extra constant pose columns under "pose_const",
# solver options).  What CASES leaves out (15.10): the second trip of every single-wave loop (more than 64 images and
# cameras), the second 256-lane block of cameras with fewer than 256 points, cameras of different parameter counts in one
# problem, an image without observations, a camera without images, an (image, point) pair seen twice, constant pose
# columns other than the gauge's, every exit other than MAX_ITERATIONS except MIN_RADIUS, a long run of accepted and
# rejected steps, and a PCG breakdown.
# tests/test_ba_cpu.py asserts by the reference's own result that each case is of the kind its name says.
EDGE_CASES = {
    "many65_per_image": (dict(seed=101, nimg=65, npts=24, model=2, cameras="per_image", tracks="mixed", noise=0.3),
                         dict(max_num_iterations=3)),
    "many70_shared": (dict(seed=102, nimg=70, npts=24, model=2, cameras="shared", tracks="mixed", noise=0.3),
                      dict(max_num_iterations=3)),
    "many260_per_image": (_MANY260, dict(max_num_iterations=3)),
    "many260_cameras_const": (dict(_MANY260, flags=dict(refine_focal_length=False, refine_extra_params=False)),
                              dict(max_num_iterations=3)),
    "mixed_models_small_first": (dict(seed=104, nimg=7, npts=40, noise=0.3, image_cameras=[0, 0, 1, 2, 3, 4, 5],
                                      models=[_M[n] for n in ("SIMPLE_PINHOLE", "FULL_OPENCV", "SIMPLE_RADIAL",
                                                              "THIN_PRISM_FISHEYE", "FOV", "PINHOLE")]),
                                 dict(max_num_iterations=4)),
    "mixed_models_big_first": (dict(seed=105, nimg=4, npts=40, noise=0.3, image_cameras=[0, 0, 1, 2],
                                    models=[_M["FULL_OPENCV"], _M["SIMPLE_PINHOLE"], _M["RADIAL"]]),
                               dict(max_num_iterations=4)),
    "empty_image_middle": (dict(seed=106, nimg=5, npts=40, model=2, cameras="per_image", noise=0.3, drop_image=3),
                           dict(max_num_iterations=3)),
    "empty_image_last": (dict(seed=106, nimg=5, npts=40, model=2, cameras="per_image", noise=0.3, drop_image=4),
                         dict(max_num_iterations=3)),
    "camera_without_images": (dict(seed=107, nimg=4, npts=40, noise=0.3, image_cameras=[0, 2, 0, 2],
                                   models=[_M["SIMPLE_RADIAL"], _M["OPENCV"], _M["PINHOLE"]]),
                              dict(max_num_iterations=3)),
    "duplicate_observations": (dict(seed=108, nimg=4, npts=40, model=2, noise=0.3, duplicates=5),
                               dict(max_num_iterations=3)),
    "pose_const_pattern": (dict(seed=109, nimg=4, npts=40, model=2, noise=0.3, pose_const={2: (0, 4), 3: (0, 1, 2)}),
                           dict(max_num_iterations=3)),
    "stop_function_tolerance": (_STOP_SCENE, dict(max_num_iterations=50, function_tolerance=1e-6)),
    "stop_parameter_tolerance": (_STOP_SCENE, dict(max_num_iterations=50, parameter_tolerance=1e-8)),
    "stop_gradient_tolerance": (_STOP_SCENE, dict(max_num_iterations=50, gradient_tolerance=1e-4)),
    "stop_gradient_at_start": (_STOP_SCENE, dict(max_num_iterations=50, gradient_tolerance=1e9)),
    "long_run": (dict(seed=120, nimg=3, npts=12, model=1, noise=0.3), dict(max_num_iterations=40)),
    # one PCG iteration per solve on a far start: from the 73rd solve on, near convergence at a large radius, the reference's
    # p.Sp is not positive in some solves and PCG stops as a breakdown (kind 3) with x = 0
    "pcg_breakdown": (dict(seed=201, nimg=3, npts=12, model=6, noise=0.3, perturb=6.0),
                      dict(max_num_iterations=80, max_linear_solver_iterations=1)),
    # the same run with one invalid step allowed: at its 82nd step the model cost change is not positive
    "invalid_step_in_loop": (dict(seed=201, nimg=3, npts=12, model=6, noise=0.3, perturb=6.0),
                             dict(max_num_iterations=100, max_linear_solver_iterations=1,
                                  max_num_consecutive_invalid_steps=1)),
    # image 0 is the identity rotation with t = (0, 0, 6): the moved point's depth in it is exactly 0.0
    "infinite_start": (dict(seed=111, nimg=3, npts=12, model=1, noise=0.3, move_point=(0, (0.3, -0.2, -6.0))),
                       dict(max_num_iterations=5)),
}


# tests/test_ba_gpu.py's Reconstruction with two camera models whose last image has no observations
E2E_MIXED_SCENE = dict(seed=113, nimg=5, npts=30, noise=0.3, models=[_M["SIMPLE_RADIAL"], _M["OPENCV"]],
                       image_cameras=[0, 0, 1, 1, 1], drop_image=4)


def case_problem(name):
    args, flags, options = CASES[name]
    return problem(scene(**args), **flags), options


def edge_scene(name):
    args = {k: v for k, v in EDGE_CASES[name][0].items() if k not in ("flags", "pose_const")}
    return scene(**args)


def edge_problem(name):
    args, options = EDGE_CASES[name]
    return problem(edge_scene(name), pose_const=args.get("pose_const"), **args.get("flags", {})), options


def digest(result) -> str:
    """sha256 over the result's arrays and statistics, bit for bit."""
    import hashlib
    h = hashlib.sha256()
    for k in RESULT_ARRAYS:
        h.update(np.ascontiguousarray(result[k], np.float64).tobytes())
    for k in RESULT_STATS:
        v = result[k]
        h.update(np.float64(v).tobytes() if isinstance(v, float) else str(v).encode())
    return h.hexdigest()


def reconstruction(sc):
    """The scene as a pycolmap Reconstruction built through its public methods: camera ids 1 .., image ids 1 .., each
    image's points2D in the order of its observations, one add_point3D per point."""
    import pycolmap_amd as pc
    r = pc.Reconstruction()
    for c, p in enumerate(sc["camera_params"]):
        r.add_camera(pc.Camera(model=MODEL_NAMES[sc["models"][c]], width=1000, height=800, params=list(p), camera_id=c + 1))
    tracks = {}
    for i, c in enumerate(sc["image_cameras"]):
        im = pc.Image(name=f"image{i + 1}.png", camera_id=int(c) + 1, id=i + 1)
        im.cam_from_world = pc.Rigid3d(pc.Rotation3d(np.array(sc["qvec"][i])), np.array(sc["tvec"][i]))
        sel = np.flatnonzero(sc["obs_image"] == i)
        im.points2D = [pc.Point2D(sc["obs_xy"][k]) for k in sel]
        for idx, k in enumerate(sel):
            tracks.setdefault(int(sc["obs_point"][k]), []).append(pc.TrackElement(i + 1, idx))
        r.add_image(im)
    for j in range(len(sc["xyz"])):
        r.add_point3D(sc["xyz"][j], pc.Track(tracks[j]))
    return r
