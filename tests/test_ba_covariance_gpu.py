"""Bundle-adjustment covariance on the GPU: Context.ba_covariance equals the sequential CPU reference
(tests/bacov_ref) and its frozen fixture bit for bit on every case of tests/bacov_cases.py, min_pivot_ratio by bit pattern;
the refusals come before the device is used; estimate_ba_covariance after BundleAdjuster.solve equals the same walk through
the reference."""
from pathlib import Path

import numpy as np
import pytest

import bacov_cases
import bacov_ref_lib as ref
from pycolmap_amd import _capi

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "bacov_ref_v1.npz"


@pytest.fixture(scope="module")
def ctx():
    with _capi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def bits(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)


def assert_same(got, want, what=""):
    for k in ("success", "failed_column", "num_columns"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert bits(got["min_pivot_ratio"])[0] == bits(want["min_pivot_ratio"])[0], (what, got["min_pivot_ratio"],
                                                                                 want["min_pivot_ratio"])
    for k in ("column_owner", "column_coord"):
        assert np.array_equal(got[k], want[k]), (what, k)
    for k in ("matrix", "point_cov"):
        assert (got[k] is None) == (want[k] is None), (what, k)
        if want[k] is not None:
            g, w = bits(got[k]), bits(want[k])
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, (what, k, bad.size, bad[:5], np.asarray(got[k]).reshape(-1)[bad[:5]],
                                   np.asarray(want[k]).reshape(-1)[bad[:5]])
    assert (got["point_present"] is None) == (want["point_present"] is None), what
    if want["point_present"] is not None:
        assert np.array_equal(got["point_present"], want["point_present"]), what


@pytest.mark.parametrize("name", [c["name"] for c in bacov_cases.cases()])
def test_covariance_equals_reference_and_fixture(name, ctx, golden):
    c = bacov_cases.by_name(name)
    want = ref.ba_covariance(*c["problem"], options=c["options"], point_const=c["point_const"])
    got = ctx.ba_covariance(*c["problem"], options=c["options"], point_const=c["point_const"])
    assert_same(got, want, name)
    assert bacov_cases.digest(got) == str(golden[f"{name}/digest"])
    assert got["num_columns"] == c["m"]
    if c["expect"] == "fail":
        assert not got["success"] and got["failed_column"] == c["column"] and got["matrix"] is None
    else:
        assert got["success"] and got["failed_column"] == -1
    if c["m"] == 0:  # no device use: nothing was timed
        assert got["device_ms"] == 0.0 and got["kernel_ms"] == 0.0 and got["matrix"].shape == (0, 0)
        assert not got["point_present"].any()


def test_want_switches_leave_out_the_arrays_and_nothing_else(ctx):
    c = bacov_cases.by_name("points_mixed_const")
    full = ctx.ba_covariance(*c["problem"], options=c["options"], point_const=c["point_const"])
    no_points = ctx.ba_covariance(*c["problem"], options=dict(c["options"], want_points=0), point_const=c["point_const"])
    no_matrix = ctx.ba_covariance(*c["problem"], options=dict(c["options"], want_matrix=0), point_const=c["point_const"])
    assert no_points["point_cov"] is None and no_points["point_present"] is None
    assert np.array_equal(bits(no_points["matrix"]), bits(full["matrix"]))
    assert no_matrix["matrix"] is None and np.array_equal(bits(no_matrix["point_cov"]), bits(full["point_cov"]))
    # the constant points have no block
    assert np.array_equal(full["point_present"], np.asarray(c["point_const"]) == 0)
    assert not full["point_cov"][~full["point_present"]].any()


def test_two_calls_in_a_row_agree(ctx):
    c = bacov_cases.by_name("columns_129")
    a = ctx.ba_covariance(*c["problem"])
    b = ctx.ba_covariance(*c["problem"])
    assert_same(a, b, "repeat")


@pytest.mark.parametrize("name", [c["name"] for c in bacov_cases.refused_cases()])
def test_refusals_come_before_the_device(name, ctx):
    c = bacov_cases.by_name(name)
    with pytest.raises(_capi.AmcError) as e:
        ctx.ba_covariance(*c["problem"], options=c["options"], point_const=c["point_const"])
    assert e.value.code == _capi.AMC_E_INVALID
    assert ("8193 variable columns" if name == "columns_8193" else "not finite") in str(e.value)
    with pytest.raises(ValueError):
        ref.ba_covariance(*c["problem"], options=c["options"], point_const=c["point_const"])
    # the context stays usable
    ok = bacov_cases.by_name("columns_5")
    assert ctx.ba_covariance(*ok["problem"])["success"]


def test_invalid_options_and_masks_are_refused(ctx):
    c = bacov_cases.by_name("columns_5")
    for bad in (dict(damping=-1.0), dict(damping=float("nan")), dict(loss_function_scale=0.0), dict(loss_function_type=3),
                dict(nonsense=1)):
        with pytest.raises(ValueError, match="ba_covariance"):
            ctx.ba_covariance(*c["problem"], options=bad)
    with pytest.raises(ValueError, match="ba_covariance.*point_const"):
        ctx.ba_covariance(*c["problem"], point_const=np.zeros(3, np.uint8))
    # a variable point with a single observation, as amc_bundle_adjust_masked refuses it
    args = list(c["problem"])
    keep = np.ones(len(args[8]), bool)
    keep[np.flatnonzero(np.asarray(args[9]) == 0)[1:]] = False
    args[8], args[9], args[10] = np.asarray(args[8])[keep], np.asarray(args[9])[keep], np.asarray(args[10])[keep]
    with pytest.raises(_capi.AmcError, match="point 0 has 1 observations"):
        ctx.ba_covariance(*args)


# ---- estimate_ba_covariance after BundleAdjuster.solve -------------------------------------------------------------------------
def _global_gauge_config(pc, rec):
    """the config adjust_global_bundle builds: every image, the first pose and the second's x position constant"""
    cfg = pc.BundleAdjustmentConfig()
    ids = sorted(rec.images)
    for iid in ids:
        cfg.add_image(iid)
    cfg.set_constant_cam_pose(ids[0])
    cfg.set_constant_cam_positions(ids[1], [0])
    return cfg


def _adjuster(pc, kind):
    import ba_cases
    import ba_config_cases as cc
    if kind != "global":
        return cc.adjuster(pc, kind)
    rec = ba_cases.reconstruction(ba_cases.scene(seed=343, nimg=5, npts=30, model=2, cameras="mixed", noise=0.3))
    o = pc.BundleAdjustmentOptions()
    o.solver_options.max_num_iterations = 4
    return rec, pc.BundleAdjuster(o, _global_gauge_config(pc, rec))


def _reference_cov_solver(d):
    import ba_config_cases as cc
    return ref.ba_covariance(*cc.flat_args(d), options=dict(d["options"]), point_const=np.asarray(d["point_const"]).reshape(-1))


@pytest.mark.parametrize("kind", ["local", "global", "structure_only"])
def test_solve_then_estimate_equals_the_walk_through_the_reference(kind):
    """BundleAdjuster.solve then estimate_ba_covariance on the GPU against _solve_with and _estimate_ba_covariance_with on
    the references: a local config, the global gauge and a structure-only config, every block equal"""
    import ba_config_cases as cc
    import ba_config_ref_lib
    import pycolmap
    from pycolmap_amd import _ba_covariance
    rec, adj = _adjuster(pycolmap, kind)
    rec_ref, adj_ref = _adjuster(pycolmap, kind)
    assert adj.solve(rec) is True and adj_ref._solve_with(rec_ref, cc.reference_solver(ba_config_ref_lib)) is True
    assert cc.model_bits(rec) == cc.model_bits(rec_ref)
    before = cc.model_bits(rec)
    got = pycolmap.estimate_ba_covariance(pycolmap.BACovarianceOptions(), rec, adj)
    want = _ba_covariance._estimate_ba_covariance_with(pycolmap.BACovarianceOptions(), rec_ref, adj_ref, _reference_cov_solver)
    assert cc.model_bits(rec) == before
    assert got is not None and want is not None

    def same(a, b, what):
        assert (a is None) == (b is None), what
        if a is not None:
            assert np.array_equal(bits(a), bits(b)), what
    ids = sorted(rec.images)
    for iid in ids:
        same(got.get_cam_from_world_cov(iid), want.get_cam_from_world_cov(iid), ("pose", iid))
        same(got.get_cam_cross_cov(ids[-1], iid), want.get_cam_cross_cov(ids[-1], iid), ("cross", iid))
        same(got.get_cam2_from_cam1_cov(iid, ids[-1]), want.get_cam2_from_cam1_cov(iid, ids[-1]), ("relative", iid))
    for cid in rec.cameras:
        same(got.get_camera_cov(cid), want.get_camera_cov(cid), ("camera", cid))
        assert got.variable_camera_param_idxs(cid) == want.variable_camera_param_idxs(cid)
    for pid in rec.points3D:
        same(got.get_point_cov(pid), want.get_point_cov(pid), ("point", pid))
    for k in ("num_columns", "num_pose_blocks", "num_camera_blocks", "num_point_blocks", "min_pivot_ratio", "params"):
        assert got.summary[k] == want.summary[k], k
    assert pycolmap.last_run_stats()["call"] == "estimate_ba_covariance"
    if kind == "structure_only":  # no image in the config: no column, and with m == 0 the results are empty (24.7)
        assert got.summary["num_columns"] == 0 and got.summary["num_point_blocks"] == 0
    else:
        assert got.summary["num_pose_blocks"] >= 3 and got.summary["num_point_blocks"] >= 1 and got.summary["kernel_ms"] > 0
    if kind == "global":
        assert got.get_cam_from_world_cov(ids[0]) is None  # the gauge's constant pose has no column
        second = got.get_cam_from_world_cov(ids[1])
        assert not second[3].any() and not second[:, 3].any() and (np.diag(second)[[0, 1, 2, 4, 5]] > 0).all()


def test_one_image_config_against_the_pose_refinement_covariance(ctx):
    """get_cam_from_world_cov of a one-image config against the pose refinement's covariance (12.8; the module-level
    pose_refinement does not hand it out, Context.refine_absolute_poses(return_covariance=True) does): the same inliers,
    Cauchy scale and pose, within the bound measured on the CPU (tests/ref2/bacov_deviation_budget.json).  A second image
    outside the config sees the same points, which makes them constant (15.12) and keeps their tracks longer than one."""
    import json
    import abspose_cases
    import pycolmap as pc
    sc = abspose_cases.scene(300, 1, 60, outlier_frac=0.0, noise_px=1.0)
    n = int(sc["offsets"][-1])
    r = ctx.refine_absolute_poses(sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"], sc["points3D"],
                                  sc["qvec"], sc["tvec"], np.ones(n, bool), return_covariance=True)
    assert r["success"][0]
    want = np.asarray(r["covariance"][0]).reshape(6, 6)
    model = int(sc["camera_models"][0])
    import ba_cases
    rec = pc.Reconstruction()
    rec.add_camera(pc.Camera(model=ba_cases.MODEL_NAMES[model], width=1600, height=1200, params=list(sc["camera_params"][0]), camera_id=1))
    tracks = []
    for iid in (1, 2):
        im = pc.Image(name=f"image{iid}.png", camera_id=1, id=iid)
        im.cam_from_world = pc.Rigid3d(pc.Rotation3d(np.array(r["qvec"][0])), np.array(r["tvec"][0]) + (iid - 1) * np.array([0.3, 0.0, 0.0]))
        im.points2D = [pc.Point2D(xy) for xy in sc["points2D"]]
        rec.add_image(im)
    for j in range(n):
        tracks.append(rec.add_point3D(sc["points3D"][j], pc.Track([pc.TrackElement(1, j), pc.TrackElement(2, j)])))
    cfg = pc.BundleAdjustmentConfig()
    cfg.add_image(1)
    o = pc.BundleAdjustmentOptions()
    o.loss_function_type = pc.LossFunctionType.CAUCHY
    o.loss_function_scale = _capi.abspose_options(None, None)[1].loss_function_scale
    o.refine_focal_length = o.refine_extra_params = o.refine_principal_point = False
    cov = pc.estimate_ba_covariance(pc.BACovarianceOptions(), rec, pc.BundleAdjuster(o, cfg))
    got = cov.get_cam_from_world_cov(1)
    assert cov.summary["num_columns"] == 6 and cov.get_cam_from_world_cov(2) is None and cov.summary["num_point_blocks"] == 0
    dev = float(np.abs(got - want).max() / np.abs(want).max())
    bound = json.loads((Path(__file__).resolve().parent / "ref2" / "bacov_deviation_budget.json").read_text())["abspose"]["bound"]
    print(f"one image against 12.8: deviation {dev:.3e}, bound {bound:.3e}")
    assert dev <= bound, (dev, bound)
