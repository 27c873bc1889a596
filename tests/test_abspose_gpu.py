"""Absolute pose on the GPU (libamc.so's amc_estimate_absolute_poses / amc_refine_absolute_poses,
pycolmap_amd.absolute_pose_estimation / pose_refinement) against its CPU reference (tests/abspose_ref): success,
pose bits, inlier and trial counts, masks, focal factors and covariance bits identical over clean, noisy and outlier
queries, 3 to 20,000 correspondences, all eleven camera models, focal-length estimation, trial caps, error limits,
degenerate input, refinement alone and batches in any order or split; and the same over abspose_cases.EDGE_CASES: the
lane edges, the RANSAC limits, a sample-stream rerun beside queries that need none, focal-length estimation on every
kind of camera, a tie and a failure of every factor, refinement alone through every exit of its solver, and a split on
the query count."""
from pathlib import Path

import numpy as np
import pytest

import abspose_cases
import abspose_ref_lib as ref

pytestmark = pytest.mark.gpu

FIELDS = ("success", "qvec", "tvec", "num_inliers", "num_trials", "focal_factor", "inlier_mask", "covariance")


def gpu(ctx, sc, est=None, rf=None, cov=False):
    return ctx.estimate_absolute_poses(sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"],
                                       sc["points3D"], est, rf, cov)


def cpu(sc, est=None, rf=None, cov=False):
    return ref.estimate(sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"], sc["points3D"], est,
                        rf, cov)


def assert_same(got, want, what):
    for k in FIELDS:
        if k not in want:
            continue
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.dtype == np.float64:
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), f"{what}: {k} differs"


CASES = abspose_cases.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_exact_to_reference(amc_ctx, name):
    sc, est, rf, cov = CASES[name]
    got = gpu(amc_ctx, sc, est, rf, cov)
    assert_same(got, cpu(sc, est, rf, cov), name)
    assert got["device_ms"] > 0 and got["num_batches"] == 1
    if name in ("clean", "noisy", "outliers30", "outliers60") or name.startswith("model"):
        assert got["success"].all()
    if name == "outliers80":  # every query draws past the first sample stream: the batch is rerun on a longer one
        assert (3 * got["num_trials"] > abspose_cases.FIRST_STREAM_WORDS).all()


def test_large_query_20000(amc_ctx):
    sc = abspose_cases.scene(60, 1, 20000, outlier_frac=0.4)
    got = gpu(amc_ctx, sc, cov=True)
    assert_same(got, cpu(sc, cov=True), "n=20000")
    assert got["success"][0]


def test_refinement_alone(amc_ctx):
    sc = abspose_cases.scene(61, 6, 300, outlier_frac=0.3, noise_px=1.0)
    rng = np.random.default_rng(0)
    q = sc["qvec"] + rng.normal(scale=0.01, size=sc["qvec"].shape)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = sc["tvec"] + rng.normal(scale=0.05, size=sc["tvec"].shape)
    mask = ~sc["outlier"]
    mask[:300] = False  # the first query: an all-false mask
    args = (sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"], sc["points3D"], q, t, mask)
    for rf, cov in (({}, False), (dict(max_num_iterations=2), True)):
        got = amc_ctx.refine_absolute_poses(*args, rf, cov)
        assert_same(got, ref.refine(*args, rf, cov), f"refine {rf}")
        assert got["success"].all()
    assert np.array_equal(got["qvec"][0].view(np.uint64), q[0].view(np.uint64))  # nothing to refine: unchanged


def test_batch_equals_per_query_calls_and_any_order(amc_ctx):
    sc = abspose_cases.concat(abspose_cases.scene(62, 5, 150, outlier_frac=0.3),
                              abspose_cases.scene(63, 4, 400, outlier_frac=0.5, model=4))
    est = dict(estimate_focal_length=1, num_focal_length_samples=4)
    whole = gpu(amc_ctx, sc, est, None, True)
    Q = len(sc["offsets"]) - 1
    for i in range(Q):
        one = gpu(amc_ctx, abspose_cases.subset(sc, [i]), est, None, True)
        for k in ("success", "qvec", "tvec", "num_inliers", "num_trials", "focal_factor", "covariance"):
            assert np.array_equal(np.asarray(one[k]).view(np.uint8), np.asarray(whole[k][i:i + 1]).view(np.uint8)), k
        off = sc["offsets"].astype(np.int64)
        assert np.array_equal(one["inlier_mask"], whole["inlier_mask"][off[i]:off[i + 1]])
    perm = np.random.default_rng(1).permutation(Q)
    shuf = gpu(amc_ctx, abspose_cases.subset(sc, perm), est, None, True)
    for k in ("success", "qvec", "tvec", "num_inliers", "num_trials", "focal_factor", "covariance"):
        assert np.array_equal(np.asarray(shuf[k]).view(np.uint8), np.asarray(whole[k][perm]).view(np.uint8)), k


def test_split_into_device_batches(amc_ctx):
    # 8 x 20,000 correspondences x 31 focal factors exceeds one device batch (2^22 problem-correspondences)
    sc = abspose_cases.scene(64, 8, 20000, outlier_frac=0.3)
    est = dict(estimate_focal_length=1, min_num_trials=20, max_num_trials=40)
    whole = gpu(amc_ctx, sc, est)
    assert whole["num_batches"] >= 2
    for i in (0, 7):
        one = gpu(amc_ctx, abspose_cases.subset(sc, [i]), est)
        assert one["num_batches"] == 1
        for k in ("success", "qvec", "tvec", "num_inliers", "num_trials", "focal_factor"):
            assert np.array_equal(np.asarray(one[k]).view(np.uint8), np.asarray(whole[k][i:i + 1]).view(np.uint8)), k


def test_pycolmap_binding_equals_context(amc_ctx):
    import pycolmap_amd as pycolmap
    sc = abspose_cases.scene(65, 1, 300, outlier_frac=0.3, model=1)
    cam = pycolmap.Camera(model="PINHOLE", width=1600, height=1200, params=sc["camera_params"][0])
    est = pycolmap.AbsolutePoseEstimationOptions()
    r = pycolmap.absolute_pose_estimation(sc["points2D"], sc["points3D"], cam, est, return_covariance=True)
    want = gpu(amc_ctx, sc, cov=True)
    assert r is not None and r["num_inliers"] == want["num_inliers"][0]
    assert np.array_equal(np.asarray(r["cam_from_world"].rotation.quat).view(np.uint64), want["qvec"][0].view(np.uint64))
    assert np.array_equal(np.asarray(r["cam_from_world"].translation).view(np.uint64), want["tvec"][0].view(np.uint64))
    assert np.array_equal(r["inliers"], want["inlier_mask"]) and np.array_equal(r["covariance"], want["covariance"][0])
    # lists of vectors work as arrays do
    r2 = pycolmap.absolute_pose_estimation(list(sc["points2D"]), [list(x) for x in sc["points3D"]], cam)
    assert np.array_equal(np.asarray(r2["cam_from_world"].translation), np.asarray(r["cam_from_world"].translation))
    # pose_refinement through the binding equals Context.refine_absolute_poses
    p = pycolmap.pose_refinement(r["cam_from_world"], sc["points2D"], sc["points3D"], r["inliers"], cam)
    w = amc_ctx.refine_absolute_poses(sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"],
                                      sc["points3D"], want["qvec"], want["tvec"], want["inlier_mask"])
    assert np.array_equal(np.asarray(p["cam_from_world"].translation).view(np.uint64), w["tvec"][0].view(np.uint64))


def test_focal_estimation_scales_camera_in_place(amc_ctx):
    import pycolmap_amd as pycolmap
    sc = abspose_cases.scene(66, 1, 300, outlier_frac=0.2, f=1200.0)
    wrong = np.array(sc["camera_params"][0]) * np.array([0.5, 1.0, 1.0])  # half the true focal length
    cam = pycolmap.Camera(model="SIMPLE_PINHOLE", width=1600, height=1200, params=wrong)
    est = pycolmap.AbsolutePoseEstimationOptions(estimate_focal_length=True)
    r = pycolmap.absolute_pose_estimation(sc["points2D"], sc["points3D"], cam, est)
    want = gpu(amc_ctx, dict(sc, camera_params=[wrong]), dict(estimate_focal_length=1))
    assert r is not None and want["success"][0]
    assert np.asarray(cam.params)[0] == wrong[0] * want["focal_factor"][0]
    assert abs(np.asarray(cam.params)[0] / 1200.0 - 1.0) < 0.2
    assert np.array_equal(np.asarray(cam.params)[1:], wrong[1:])


# ---- the edge cases -----------------------------------------------------------------------------------
EDGES = abspose_cases.EDGE_CASES
MAKER = Path(__file__).resolve().parent / "golden" / "make_abspose_ref_golden.py"  # (it reads the edge fixture)
FAST_BATCH = sorted(n for n in EDGES if EDGES[n][0] == "estimate" and EDGES[n][2] == abspose_cases.FAST)


@pytest.fixture(scope="module")
def golden_edges():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mk", MAKER)
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk.load_edges()


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_case_bit_exact_to_reference_and_fixture(amc_ctx, golden_edges, name):
    got = abspose_cases.edge_run(name, amc_ctx.estimate_absolute_poses, amc_ctx.refine_absolute_poses)
    want = abspose_cases.edge_run(name, ref.estimate, ref.refine)
    assert_same(got, want, name)
    assert abspose_cases.digest(got) == golden_edges[name][0]
    assert got["num_batches"] == 1


def test_edge_cases_as_one_batch_in_any_order(amc_ctx):
    assert len(FAST_BATCH) >= 8
    each = [gpu(amc_ctx, EDGES[n][1], abspose_cases.FAST, None, True) for n in FAST_BATCH]
    for order in (np.arange(len(FAST_BATCH)), np.random.default_rng(2).permutation(len(FAST_BATCH))):
        whole = gpu(amc_ctx, abspose_cases.concat(*[EDGES[FAST_BATCH[i]][1] for i in order]), abspose_cases.FAST, None,
                    True)
        lens = [len(each[i]["inlier_mask"]) for i in order]
        ends = np.cumsum(lens)
        for j, i in enumerate(order):
            part = {k: whole[k][j:j + 1] for k in FIELDS if k != "inlier_mask"}
            part["inlier_mask"] = whole["inlier_mask"][ends[j] - lens[j]:ends[j]]
            assert_same(part, {k: each[i][k] for k in FIELDS}, f"{FAST_BATCH[i]} at {j}")


def test_split_on_query_count(amc_ctx):
    # 2^16 queries fill one device batch: the 65,537th, whose RANSAC outruns the first sample stream, is a batch of its own
    last = abspose_cases.overrun_query()
    sc = abspose_cases.concat(abspose_cases.tiny_queries(7, 1 << 16), last)
    got = gpu(amc_ctx, sc, abspose_cases.OVERRUN)
    assert got["num_batches"] >= 2
    want = cpu(sc, abspose_cases.OVERRUN)
    assert 3 * want["num_trials"][-1] > abspose_cases.FIRST_STREAM_WORDS >= 3 * want["num_trials"][:-1].max()
    assert want["success"].all()
    assert_same(got, want, "65,537 queries")
    one = gpu(amc_ctx, last, abspose_cases.OVERRUN)
    part = {k: got[k][-1:] for k in FIELDS if k in got and k != "inlier_mask"}
    part["inlier_mask"] = got["inlier_mask"][-len(one["inlier_mask"]):]
    assert_same(part, {k: one[k] for k in FIELDS if k in one}, "the last query alone")


def test_no_queries(amc_ctx):
    none = (np.zeros(1, np.uint64), np.zeros(0, np.int32), [], np.zeros((0, 2)), np.zeros((0, 3)))
    for cov in (False, True):
        for got in (amc_ctx.estimate_absolute_poses(*none, None, None, cov),
                    amc_ctx.refine_absolute_poses(*none, np.zeros((0, 4)), np.zeros((0, 3)), np.zeros(0, bool), None, cov)):
            assert got["num_batches"] == 0
            for k in FIELDS:
                if k == "covariance" and not cov:
                    assert k not in got
                else:
                    assert len(got[k]) == 0, k
            assert got["qvec"].shape == (0, 4) and got["tvec"].shape == (0, 3)
            assert not cov or got["covariance"].shape == (0, 6, 6)
