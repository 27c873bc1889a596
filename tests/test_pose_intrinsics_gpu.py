"""GPU tests of the joint pose and camera refinement (include/amc_absrefine.h, pycolmap_amd/_pose_intrinsics.py;
DESIGN.md section 25): every case of absrefine_cases bit for bit against the CPU reference (tests/absrefine_ref) and the
frozen fixture, the nv = 0 entries against the shipped absolute pose entries, batches in any order and split, refused
input, the Python functions and the mapper's registration with refinement."""
import os
from pathlib import Path

import numpy as np
import pytest

import abspose_cases
import absrefine_cases as cases
import absrefine_ref_lib as ref

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "absrefine_ref_v1.npz"
CASES = cases.CASES
REFINE = sorted(n for n in CASES if CASES[n][0] == "refine")
ESTIMATE = sorted(n for n in CASES if CASES[n][0] == "estimate")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return dict(zip(z["names"].tolist(), z["digests"].tolist()))


@pytest.fixture(scope="module")
def reference():
    """Every case through the CPU reference, once."""
    return {n: cases.run(n, ref.estimate, ref.refine) for n in CASES}


@pytest.mark.parametrize("name", REFINE + ESTIMATE)
def test_case_equals_reference_and_fixture(amc_ctx, reference, golden, name):
    got = cases.run(name, amc_ctx.estimate_poses_and_cameras, amc_ctx.refine_poses_and_cameras)
    assert cases.same(got, reference[name]) == []
    assert cases.digest(got) == golden[name]
    assert got["num_batches"] == 1


def _args(sc):
    return sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"], sc["points3D"]


@pytest.mark.parametrize("name", sorted(n for n in abspose_cases.EDGE_CASES if abspose_cases.EDGE_CASES[n][0] == "refine"))
def test_fixed_camera_equals_the_shipped_refinement(amc_ctx, name):
    """nv = 0: refine_poses_and_cameras with both flags false is refine_absolute_poses, bit for bit."""
    _, sc, _, rf, cov = abspose_cases.EDGE_CASES[name]
    old = amc_ctx.refine_absolute_poses(*_args(sc), sc["start_q"], sc["start_t"], sc["mask"], rf, cov)
    new = amc_ctx.refine_poses_and_cameras(*_args(sc), sc["start_q"], sc["start_t"], sc["mask"], rf, cov)
    assert cases.same(new, old, abspose_cases.FIELDS) == []
    want = np.zeros((len(sc["camera_params"]), 12))
    for i, p in enumerate(sc["camera_params"]):
        want[i, :len(p)] = p
    assert np.array_equal(new["camera_params"], want, equal_nan=True)


@pytest.mark.parametrize("name", ["n65", "focal_model4", "focal_mixed_batch", "focal_all_fail"])
def test_fixed_camera_estimate_equals_the_shipped_sequence(amc_ctx, name):
    """nv = 0: estimate_poses_and_cameras is estimate_absolute_poses without refinement iterations, then
    refine_absolute_poses from its pose over its inliers with the camera scaled by its factor."""
    _, sc, est, rf, cov = abspose_cases.EDGE_CASES[name]
    new = amc_ctx.estimate_poses_and_cameras(*_args(sc), est, rf, cov)
    first = amc_ctx.estimate_absolute_poses(*_args(sc), est, dict(rf, max_num_iterations=0), False)
    scaled = []
    for m, p, f in zip(sc["camera_models"], sc["camera_params"], first["focal_factor"]):
        p = np.array(p, np.float64)
        p[:cases.NUM_FOCAL[int(m)]] *= f if f != 0.0 else 1.0
        scaled.append(p)
    mask = first["inlier_mask"].copy()
    off = sc["offsets"].astype(np.int64)
    for i in np.flatnonzero(~first["success"]):
        mask[off[i]:off[i + 1]] = False
    second = amc_ctx.refine_absolute_poses(sc["offsets"], sc["camera_models"], scaled, sc["points2D"], sc["points3D"],
                                           first["qvec"], first["tvec"], mask, rf, cov)
    ok = first["success"] & second["success"]
    assert np.array_equal(new["success"], ok)
    assert np.array_equal(new["qvec"], second["qvec"], equal_nan=True)
    assert np.array_equal(new["tvec"], second["tvec"], equal_nan=True)
    if cov:
        assert np.array_equal(new["covariance"][ok], second["covariance"][ok])
    for k in ("num_inliers", "num_trials", "focal_factor", "inlier_mask"):
        assert np.array_equal(new[k], first[k]), k


BATCH = [n for n in REFINE if CASES[n][3] == cases.BOTH and CASES[n][4]]  # one option set: they can share a call


def _concat_refine(names):
    scs = [CASES[n][1] for n in names]
    sc = abspose_cases.concat(*scs)
    return dict(sc, start_q=np.concatenate([s["start_q"] for s in scs]),
                start_t=np.concatenate([s["start_t"] for s in scs]), mask=np.concatenate([s["mask"] for s in scs]))


def _refine(ctx, sc):
    return ctx.refine_poses_and_cameras(*_args(sc), sc["start_q"], sc["start_t"], sc["mask"], cases.BOTH, True)


def test_one_call_shuffled_and_split(amc_ctx, reference):
    """The cases that share an option set as one call, in two orders and split by AMC_ABSREFINE_BATCH_QUERIES: every
    query's result is the one it has alone."""
    assert len(BATCH) == 24
    per_query = ("success", "qvec", "tvec", "camera_params", "covariance", "num_inliers")
    for order in (list(range(len(BATCH))), list(np.random.default_rng(5).permutation(len(BATCH)))):
        names = [BATCH[i] for i in order]
        sc = _concat_refine(names)
        nq = len(sc["camera_models"])
        want = {k: np.concatenate([reference[n][k] for n in names]) for k in per_query}
        for limit in (None, 1, 2, 64):
            if limit is None:
                os.environ.pop("AMC_ABSREFINE_BATCH_QUERIES", None)
            else:
                os.environ["AMC_ABSREFINE_BATCH_QUERIES"] = str(limit)
            try:
                got = _refine(amc_ctx, sc)
            finally:
                os.environ.pop("AMC_ABSREFINE_BATCH_QUERIES", None)
            assert cases.same(got, want, per_query) == [], (limit, order[:4])
            # greedy contiguous batches of at most `limit` queries (no query here nears the correspondence bound)
            assert got["num_batches"] == (1 if limit is None else -(-nq // limit))


def test_a_call_without_queries(amc_ctx):
    got = amc_ctx.refine_poses_and_cameras(np.zeros(1, np.uint64), np.zeros(0, np.int32), [], np.zeros((0, 2)),
                                           np.zeros((0, 3)), np.zeros((0, 4)), np.zeros((0, 3)), np.zeros(0, bool),
                                           cases.BOTH, True)
    assert got["success"].shape == (0,) and got["camera_params"].shape == (0, 12) and got["covariance"].shape == (0, 6, 6)
    got = amc_ctx.estimate_poses_and_cameras(np.zeros(1, np.uint64), np.zeros(0, np.int32), [], np.zeros((0, 2)),
                                             np.zeros((0, 3)), abspose_cases.FAST, cases.BOTH)
    assert got["success"].shape == (0,) and got["inlier_mask"].shape == (0,)


def test_refused_input(amc_ctx):
    from pycolmap_amd import _capi
    _, sc, _, rf, _ = CASES["model2_f1e1"]
    a = _args(sc)
    for bad in (dict(gradient_tolerance=-1.0), dict(max_num_iterations=-1), dict(loss_function_scale=-1.0),
                dict(gradient_tolerance=float("nan"))):
        with pytest.raises(_capi.AmcError, match="invalid options") as e:
            amc_ctx.refine_poses_and_cameras(*a, sc["start_q"], sc["start_t"], sc["mask"], dict(rf, **bad))
        assert e.value.code == _capi.AMC_E_INVALID
    with pytest.raises(_capi.AmcError, match="camera model 11"):
        amc_ctx.refine_poses_and_cameras(a[0], np.array([11], np.int32), *a[2:], sc["start_q"], sc["start_t"], sc["mask"], rf)
    with pytest.raises(_capi.AmcError, match=r"offsets\[0\] != 0"):
        amc_ctx.refine_poses_and_cameras(np.array([1, 120], np.uint64), a[1], a[2], a[3][:120], a[4][:120], sc["start_q"],
                                         sc["start_t"], sc["mask"][:120], rf)
    with pytest.raises(_capi.AmcError, match="max_error > 0"):
        amc_ctx.estimate_poses_and_cameras(*a, dict(max_error=0.0), rf)


@pytest.mark.parametrize("model", [0, 4, 7])
def test_python_functions_update_the_camera_in_place(model):
    import pycolmap_amd
    from pycolmap_amd import _pose_intrinsics
    sc = cases.wrong_camera(abspose_cases.start(abspose_cases.scene(1100 + model, 1, 150, outlier_frac=0.2, model=model),
                                                model), focal=1.05)
    cam = pycolmap_amd.Camera(model=int(model), width=1600, height=1200, params=sc["camera_params"][0])
    before = np.array(cam.params)
    opts = dict(cases.BOTH)
    want = ref.refine(*_args(sc), sc["start_q"], sc["start_t"], sc["mask"], opts, True)
    pose = pycolmap_amd.Rigid3d(pycolmap_amd.Rotation3d(sc["start_q"][0]), sc["start_t"][0])
    got = pycolmap_amd.refine_absolute_pose(pose, sc["points2D"], sc["points3D"], sc["mask"], cam, opts,
                                            return_covariance=True)
    assert want["success"][0] and got is not None
    n = len(before)
    assert np.array_equal(np.array(cam.params), want["camera_params"][0, :n]) and not np.array_equal(cam.params, before)
    assert np.array_equal(got["cam_from_world"].rotation.quat, want["qvec"][0])
    assert np.array_equal(got["cam_from_world"].translation, want["tvec"][0])
    assert np.array_equal(got["covariance"], want["covariance"][0])
    assert _pose_intrinsics.last_run_stats()["entry"] == "refine_absolute_pose"
    # None leaves the camera untouched: a start that is not finite
    cam2 = pycolmap_amd.Camera(model=int(model), width=1600, height=1200, params=sc["camera_params"][0])
    bad = pycolmap_amd.Rigid3d(pycolmap_amd.Rotation3d(sc["start_q"][0]), np.array([np.inf, 0.0, 0.0]))
    assert pycolmap_amd.refine_absolute_pose(bad, sc["points2D"], sc["points3D"], sc["mask"], cam2, opts) is None
    assert np.array_equal(np.array(cam2.params), before)
    # estimate and refine
    cam3 = pycolmap_amd.Camera(model=int(model), width=1600, height=1200, params=sc["camera_params"][0])
    est = dict(abspose_cases.FAST)
    want = ref.estimate(*_args(sc), est, opts, False)
    got = pycolmap_amd.estimate_and_refine_absolute_pose(sc["points2D"], sc["points3D"], cam3, dict(ransac=est), opts)
    assert want["success"][0] and got is not None
    assert np.array_equal(np.array(cam3.params), want["camera_params"][0, :n])
    assert got["num_inliers"] == int(want["num_inliers"][0])
    assert np.array_equal(got["inlier_mask"], want["inlier_mask"])
    assert np.array_equal(got["cam_from_world"].translation, want["tvec"][0])
    assert _pose_intrinsics.last_run_stats()["entry"] == "estimate_and_refine_absolute_pose"


def test_register_next_image_and_refine_equals_the_walk_with_the_references():
    """One scene of mapper_cases: the library's registration with refinement leaves what the same call leaves with the
    CPU references in the library's place, for a camera without a registered image (refined) and one with (kept); then
    triangulate_image on the result."""
    import mapper_cases as k
    import pycolmap_amd as pc
    import triangulator_cases as tc
    from pycolmap_amd import _pose_intrinsics
    st = k.mapper_state("direct")
    topts = tc.SCENES["direct"][1]
    by_camera = {}
    for i in sorted(st["candidates"]):
        by_camera.setdefault(st["candidates"][i][0], i)
    for cam_id, image_id in sorted(by_camera.items()):
        r1, _, t1, mp1 = k.mapper(st)
        r2, _, t2, mp2 = k.mapper(st)
        before = k.model_snapshot(r1)["cameras"][cam_id]
        assert pc.register_next_image_and_refine(mp1, k.SCENE_OPTIONS, image_id) is True
        assert _pose_intrinsics._register_next_image_and_refine_with(mp2, k.SCENE_OPTIONS, image_id, ref.estimate) is True
        assert k.model_snapshot(r1) == k.model_snapshot(r2) and mp1.last_registration() == mp2.last_registration()
        assert mp1.num_reg_trials(image_id) == 1 and t1.get_modified_points3D() == t2.get_modified_points3D()
        assert (k.model_snapshot(r1)["cameras"][cam_id] != before) == (cam_id == 1)
        assert t1.triangulate_image(topts, image_id) == t2._triangulate_image_with(topts, image_id, tc.reference_solver)
        assert k.model_snapshot(r1) == k.model_snapshot(r2)
