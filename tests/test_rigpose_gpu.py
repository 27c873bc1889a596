"""Rig absolute pose on the GPU (libamc.so's amc_estimate_rig_absolute_poses, pycolmap_amd.rig_absolute_pose_estimation)
against its CPU reference (tests/rigpose_ref) and the frozen fixture: success, pose bits, both inlier counts, trial
counts, masks and covariance bits identical over the lane boundaries, one to five cameras of all eleven models,
duplicated 3D points, outliers, aborts inside and after the first round of trials, a trial limit below a round, a
sample-stream overrun, any round size, and batches in any order or split."""
import os

import numpy as np
import pytest

import rigpose_cases
import rigpose_ref_lib as ref

pytestmark = pytest.mark.gpu

FIELDS = ("success", "qvec", "tvec", "num_inliers", "num_all_inliers", "num_trials", "inlier_mask", "covariance")
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "rigpose_ref_v1.npz")


def gpu(ctx, sc, est=None, rf=None, cov=False):
    return ctx.estimate_rig_absolute_poses(*rigpose_cases.args(sc), est, rf, cov)


def cpu(sc, est=None, rf=None, cov=False):
    return ref.estimate(*rigpose_cases.args(sc), est, rf, cov)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    return a.shape == b.shape and np.array_equal(a, b)


def assert_same(got, want, what):
    for k in FIELDS:
        if k in want:
            assert same(got[k], want[k]), f"{what}: {k} differs"


CASES = rigpose_cases.cases()


@pytest.fixture(scope="module")
def whole(amc_ctx):
    """every case in one batch, run once: (batch scene, GPU result) with the defaults lowered as FAST"""
    names = [n for n in sorted(CASES) if CASES[n][1] == rigpose_cases.FAST and CASES[n][2] == {}]
    sc = rigpose_cases.concat(*[CASES[n][0] for n in names])
    return names, sc, gpu(amc_ctx, sc, rigpose_cases.FAST, None, True)


@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_exact_to_reference_and_fixture(amc_ctx, name):
    sc, est, rf, cov = CASES[name]
    got = gpu(amc_ctx, sc, est, rf, cov)
    assert_same(got, cpu(sc, est, rf, cov), name)
    with np.load(GOLDEN) as g:
        for k in FIELDS:
            if f"{name}/{k}" in g:
                assert same(got[k], g[f"{name}/{k}"]), f"{name}: {k} differs from the fixture"
    assert got["device_ms"] > 0 and got["num_batches"] == 1
    assert got["success"][0] == (name != "n2")
    if name == "duplicates":
        assert got["num_inliers"][0] < got["num_all_inliers"][0] == got["inlier_mask"].sum()
    if name == "abort_mid_round":
        assert got["num_trials"][0] < 64
    if name == "several_rounds":
        assert got["num_trials"][0] > 64
    if name == "stream_overrun":
        assert 3 * got["num_trials"][0] > 3 * 2000 + 1024


def test_result_does_not_depend_on_the_round_size(amc_ctx, monkeypatch):
    sc = rigpose_cases.concat(CASES["several_rounds"][0], CASES["duplicates"][0], CASES["abort_mid_round"][0])
    est = CASES["several_rounds"][1]
    want = gpu(amc_ctx, sc, est, None, True)
    for r in ("1", "7", "33"):
        monkeypatch.setenv("AMC_RIGPOSE_ROUND", r)
        assert_same(gpu(amc_ctx, sc, est, None, True), want, f"round {r}")


def test_batch_equals_per_query_calls_and_any_order(amc_ctx, whole):
    names, sc, res = whole
    off = sc["offsets"].astype(np.int64)
    for i, n in enumerate(names):
        one = gpu(amc_ctx, CASES[n][0], rigpose_cases.FAST, None, True)
        for k in FIELDS[:-2] + ("covariance",):
            assert same(one[k], res[k][i:i + 1]), f"{n}: {k}"
        assert np.array_equal(one["inlier_mask"], res["inlier_mask"][off[i]:off[i + 1]])
    perm = np.random.default_rng(1).permutation(len(names))
    shuf = gpu(amc_ctx, rigpose_cases.subset(sc, perm), rigpose_cases.FAST, None, True)
    for k in FIELDS[:-2] + ("covariance",):
        assert same(shuf[k], res[k][perm]), k


def test_split_into_device_batches(amc_ctx):
    # 2 x 2,100,000 + 3,000 correspondences exceed one device batch (2^22 correspondences)
    small = rigpose_cases.rig_scene(70, 3000, models=(0, 1), outlier_frac=0.3, noise_px=0.5)
    big = {k: (np.tile(v, (700, 1)) if v.ndim == 2 else np.tile(v, 700)) for k, v in small.items()
           if k in ("points2D", "points3D", "camera_idxs")}
    one = dict(small, offsets=np.array([0, 2100000], np.uint64), **big)
    est = dict(min_num_trials=5, max_num_trials=10)
    sc = rigpose_cases.concat(one, small, one)
    got = gpu(amc_ctx, sc, est)
    assert got["num_batches"] >= 2
    alone = gpu(amc_ctx, small, est)
    assert alone["num_batches"] == 1
    for k in FIELDS[:-2]:
        assert same(alone[k], got[k][1:2]), k
    assert same(got["qvec"][0], got["qvec"][2]) and got["success"].all()


def test_pycolmap_binding_equals_context(amc_ctx):
    import pycolmap_amd as pycolmap
    sc = CASES["duplicates"][0]
    names = ("SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL")
    cams = [pycolmap.Camera(model=names[i], width=1600, height=1200, params=sc["camera_params"][i]) for i in range(3)]
    rigs = [pycolmap.Rigid3d(pycolmap.Rotation3d(g[:4]), g[4:]) for g in sc["cams_from_rig"]]
    opt = pycolmap.RANSACOptions()
    r = pycolmap.rig_absolute_pose_estimation(sc["points2D"], sc["points3D"], sc["camera_idxs"], rigs, cams, opt,
                                              return_covariance=True)
    want = gpu(amc_ctx, sc, None, None, True)
    assert r is not None and r["num_inliers"] == want["num_inliers"][0]
    assert same(np.asarray(r["rig_from_world"].rotation.quat), want["qvec"][0])
    assert same(np.asarray(r["rig_from_world"].translation), want["tvec"][0])
    assert np.array_equal(r["inliers"], want["inlier_mask"]) and same(r["covariance"], want["covariance"][0])
    # the reference's shifted keyword names: cameras= is the index slot
    r2 = pycolmap.rig_absolute_pose_estimation(sc["points2D"], sc["points3D"], cameras=list(sc["camera_idxs"]),
                                               camera_idxs=rigs, cams_from_rig=cams)
    assert same(np.asarray(r2["rig_from_world"].translation), want["tvec"][0]) and "covariance" not in r2
    two = CASES["n2"][0]
    assert pycolmap.rig_absolute_pose_estimation(two["points2D"], two["points3D"], two["camera_idxs"], rigs[:2],
                                                 cams[:2]) is None
