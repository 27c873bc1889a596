"""GPU parity of the point filter (include/amc_filter.h, csrc/filter.hip): the library against the CPU
reference (tests/filter_ref) and the frozen fixture, bit for bit, on the smallest shapes at which the kernels can go wrong
(tests/filter_cases.py); the errors-only mode; splitting; order independence; and Reconstruction's methods on top."""
import copy
from pathlib import Path

import numpy as np
import pytest

import ba_cases
import ba_ref_lib
import filter_cases as fc
import filter_ref_lib as ref
from pycolmap_amd import _capi

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "filter_ref_v1.npz"
FLAT_BA = ("camera_models", "camera_params", "camera_const", "image_cameras", "qvec", "tvec", "pose_const", "xyz",
           "obs_image", "obs_point", "obs_xy")


@pytest.fixture(scope="module")
def ctx():
    with _capi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


_bits = fc.bits  # (every NaN as one NaN: neither its sign nor its payload is pinned)


def _assert_same(got, want, what=""):
    assert np.array_equal(_bits(got["obs_sq_error"]), _bits(want["obs_sq_error"])), (what, "obs_sq_error")
    assert np.array_equal(got["obs_deleted"], want["obs_deleted"]), (what, "obs_deleted")
    assert np.array_equal(got["point_verdict"], want["point_verdict"]), (what, "point_verdict")
    assert np.array_equal(_bits(got["point_error"]), _bits(want["point_error"])), (what, "point_error")
    assert got["num_filtered"] == want["num_filtered"], (what, "num_filtered")


@pytest.mark.parametrize("errors_only", [False, True], ids=["filter", "errors_only"])
@pytest.mark.parametrize("name", sorted(fc.ALL_CASES))
def test_filter_equals_reference_and_fixture(name, errors_only, ctx, golden):
    args, kw = fc.case_call(name)
    want = fc.reference(name, errors_only)
    got = ctx.filter_points3d(*args, errors_only=errors_only, **kw)
    _assert_same(got, want, name)
    assert fc.digest(got) == str(golden[f"{name}/{'errors' if errors_only else 'filter'}/digest"])
    assert got["num_batches"] == (1 if len(args[5]) else 0)
    assert got["device_ms"] >= got["kernel_ms"] >= 0 and got["host_ms"] >= got["alloc_ms"] >= 0
    assert got["device_ms"] >= got["copy_ms"] >= 0
    if len(args[5]):
        assert got["kernel_ms"] > 0


@pytest.mark.parametrize("name", ["lengths", "points_257", "select_all_but_one_small"])
@pytest.mark.parametrize("batch", [1, 64, 65])
def test_split_call_equals_unsplit_call(name, batch, ctx, monkeypatch):
    args, kw = fc.case_call(name)
    npts = len(args[5])
    for errors_only in (False, True):
        monkeypatch.delenv("AMC_FILTER_BATCH_POINTS", raising=False)
        whole = ctx.filter_points3d(*args, errors_only=errors_only, **kw)
        monkeypatch.setenv("AMC_FILTER_BATCH_POINTS", str(batch))
        split = ctx.filter_points3d(*args, errors_only=errors_only, **kw)
        assert whole["num_batches"] == 1 and split["num_batches"] == -(-npts // batch)
        _assert_same(split, whole, (name, batch, errors_only))
        _assert_same(split, fc.reference(name, errors_only), (name, batch, errors_only))


def test_call_without_points_succeeds(ctx, monkeypatch):
    args, kw = fc.case_call("points_0")
    for batch in (None, 1):
        if batch:
            monkeypatch.setenv("AMC_FILTER_BATCH_POINTS", str(batch))
        got = ctx.filter_points3d(*args, **kw)
        assert got["num_batches"] == 0 and got["num_filtered"] == 0
        assert got["obs_sq_error"].size == 0 and got["point_verdict"].size == 0
    # no cameras and no images either
    got = ctx.filter_points3d([], [], [], np.zeros((0, 4)), np.zeros((0, 3)), np.zeros((0, 3)), [0], [], np.zeros((0, 2)))
    assert got["num_filtered"] == 0 and got["point_error"].size == 0


def _permuted(args, perm):
    models, prm, icam, q, t, X, off, oi, xy = args
    off = np.asarray(off, np.int64)
    idx = np.concatenate([np.arange(off[j], off[j + 1]) for j in perm]) if len(perm) else np.zeros(0, np.int64)
    noff = np.concatenate([[0], np.cumsum((off[1:] - off[:-1])[perm])])
    return (models, prm, icam, q, t, X[perm], noff, oi[idx], xy[idx]), idx


@pytest.mark.parametrize("name", ["lengths", "points_257", "mixed_models"])
def test_permuting_the_points_permutes_the_result(name, ctx):
    args, kw = fc.case_call(name)
    perm = np.random.default_rng(5).permutation(len(args[5]))
    pargs, idx = _permuted(args, perm)
    want = fc.reference(name)
    got = ctx.filter_points3d(*pargs, **kw)
    assert np.array_equal(_bits(got["obs_sq_error"]), _bits(want["obs_sq_error"][idx]))
    assert np.array_equal(got["obs_deleted"], want["obs_deleted"][idx])
    assert np.array_equal(got["point_verdict"], want["point_verdict"][perm])
    assert np.array_equal(_bits(got["point_error"]), _bits(want["point_error"][perm]))
    assert got["num_filtered"] == want["num_filtered"]


def test_two_calls_in_a_row_give_the_same_bits_and_leave_the_inputs(ctx):
    args, kw = fc.case_call("lengths")
    before = copy.deepcopy(args)
    a = ctx.filter_points3d(*args, **kw)
    b = ctx.filter_points3d(*args, **kw)
    _assert_same(a, b)
    for x, y in zip(args, before):
        assert all(np.array_equal(u, v) for u, v in zip(x, y)) if isinstance(x, list) else np.array_equal(x, y)


def test_invalid_input_is_refused(ctx):
    args, _ = fc.case_call("points_63")
    models, prm, icam, q, t, X, off, oi, xy = args

    def refused(*a, **kw):
        with pytest.raises(_capi.AmcError) as e:
            ctx.filter_points3d(*a, **kw)
        assert e.value.code == _capi.AMC_E_INVALID

    refused(*args, max_reproj_error=-1.0)
    refused(*args, max_reproj_error=np.nan)
    refused(*args, min_tri_angle=-0.5)
    refused(*args, min_tri_angle=np.nan)
    refused([11] + list(models[1:]), prm, icam, q, t, X, off, oi, xy)
    refused(models, prm, np.full_like(icam, len(models)), q, t, X, off, oi, xy)
    bad = oi.copy()
    bad[-1] = len(icam)
    refused(models, prm, icam, q, t, X, off, bad, xy)
    # (offsets that do not start at 0 or that decrease never reach the library through Context: filter_inputs and the
    # C ABI's own check are covered by tests/test_filter_cpu.py and the stand-alone program)
    got = ctx.filter_points3d(*args)  # and the context still works
    _assert_same(got, fc.reference("points_63"))


# ---- through Python ------------------------------------------------------------------------------------------------------
E2E_SCENE = dict(seed=300, nimg=5, npts=30, model=2, noise=0.5, outliers=6)
FILTER_SCENE = dict(E2E_SCENE, tracks="mixed", perturb=0.0, outliers=10)
E2E_BA = dict(max_num_iterations=8, loss_function_type="CAUCHY", loss_function_scale=2.0)


def _check_model_against(rec, before_state, before_p2d, res, returned):
    """the model equals ApplyFilterResult of the reference's result: tracks, points2D ids, errors, the return value"""
    want = fc.apply_result(before_state, res)
    got = fc.model_state(rec)
    assert [(p, e) for p, e, _ in got] == [(p, e) for p, e, _ in want]
    assert np.array_equal(_bits([x for _, _, x in got]), _bits([x for _, _, x in want]))
    assert returned == res["num_filtered"]
    alive = {(i, k): pid for pid, elements, _ in want for i, k in elements}
    for iid, ids in fc.point2d_ids(rec).items():
        for k, pid in enumerate(ids):
            assert pid == alive.get((iid, k), 0xFFFFFFFFFFFFFFFF), (iid, k)
            assert (pid == 0xFFFFFFFFFFFFFFFF) or before_p2d[iid][k] == pid


@pytest.mark.parametrize("how", ["all", "ids", "in_images"])
def test_reconstruction_filters_equal_the_reference(how, ctx):
    import pycolmap
    rec = ba_cases.reconstruction(ba_cases.scene(**FILTER_SCENE))
    points3D = rec.points3D
    objs = dict(points3D)
    state, p2d = fc.model_state(rec), fc.point2d_ids(rec)
    if how == "all":
        ids = None
    elif how == "ids":
        ids = set(list(rec.points3D)[::3]) | {10 ** 9}  # an id that does not exist is skipped
    else:
        ids = {p.point3D_id for p in rec.images[2].points2D} - {0xFFFFFFFFFFFFFFFF}
        assert 0 < len(ids) < rec.num_points3D()
    args, sel = fc.flatten_reconstruction(rec, ids)
    want = ref.filter_points3d(*args, selected=sel, max_reproj_error=3.0, min_tri_angle=1.5)
    _assert_same(ctx.filter_points3d(*args, selected=sel, max_reproj_error=3.0, min_tri_angle=1.5), want)
    assert want["obs_deleted"].sum() > 0 and (how == "all" or (want["point_verdict"] == ref.NOT_SELECTED).sum() > 0)
    if how == "all":
        n = rec.filter_all_points3D(3.0, 1.5)
    elif how == "ids":
        n = rec.filter_points3D(3.0, 1.5, ids)
    else:
        n = rec.filter_points3D_in_images(3.0, 1.5, {2})
    _check_model_against(rec, state, p2d, want, n)
    assert rec.points3D is points3D and all(rec.points3D[k] is objs[k] for k in rec.points3D)
    st = pycolmap.last_run_stats()
    assert st["call"] == "filter_points3D" and st["num_filtered"] == n and st["kernel_ms"] > 0


def test_adjust_filter_adjust(ctx):
    """bundle_adjustment -> filter_all_points3D(4.0, 1.5) -> bundle_adjustment: the filter removes exactly the planted
    outlier observations, and the second adjustment ends below the first; both hold on the references' own numbers"""
    import pycolmap
    import pycolmap_amd as pc
    sc = ba_cases.scene(**E2E_SCENE)
    clean = ba_cases.scene(**dict(E2E_SCENE, outliers=0))
    planted = {(int(sc["obs_image"][k]) + 1, int(sc["obs_point"][k]) + 1)
               for k in np.flatnonzero(np.any(sc["obs_xy"] != clean["obs_xy"], axis=1))}
    assert len(planted) == E2E_SCENE["outliers"]
    rec = ba_cases.reconstruction(sc)
    options = pc.BundleAdjustmentOptions(solver_options=dict(max_num_iterations=E2E_BA["max_num_iterations"]),
                                         loss_function_type="CAUCHY", loss_function_scale=2.0)
    # the references' chain on the flat problem
    flat = pc._pycolmap._bundle_adjustment_problem(rec, options)
    b1 = ba_ref_lib.bundle_adjust(*[flat[k] for k in FLAT_BA], options=E2E_BA)
    op, oi = flat["obs_point"].ravel(), flat["obs_image"].ravel()
    off = np.concatenate([[0], np.cumsum(np.bincount(op, minlength=len(flat["xyz"])))])
    f = ref.filter_points3d(flat["camera_models"].ravel(), b1["camera_params"], flat["image_cameras"].ravel(), b1["qvec"],
                            b1["tvec"], b1["xyz"], off, oi, flat["obs_xy"], max_reproj_error=4.0, min_tri_angle=1.5)
    assert {(int(oi[k]) + 1, int(op[k]) + 1) for k in np.flatnonzero(f["obs_deleted"])} == planted
    assert np.all(f["point_verdict"] == ref.KEPT) and f["num_filtered"] == len(planted)
    keep = ~f["obs_deleted"]
    b2 = ba_ref_lib.bundle_adjust(flat["camera_models"], b1["camera_params"], flat["camera_const"], flat["image_cameras"],
                                  b1["qvec"], b1["tvec"], flat["pose_const"], b1["xyz"], oi[keep], op[keep],
                                  flat["obs_xy"][keep], options=E2E_BA)
    assert b2["final_cost"] < b1["final_cost"]
    # the same through Python
    pc.bundle_adjustment(rec, options)
    first = pycolmap.last_run_stats()
    assert first["final_cost"] == b1["final_cost"]
    before = {(iid, k) for iid, ids in fc.point2d_ids(rec).items() for k, pid in enumerate(ids) if pid != 0xFFFFFFFFFFFFFFFF}
    assert rec.filter_all_points3D(4.0, 1.5) == len(planted)
    after = {(iid, k): pid for iid, ids in fc.point2d_ids(rec).items() for k, pid in enumerate(ids) if pid != 0xFFFFFFFFFFFFFFFF}
    removed = before - set(after)
    ids0 = fc.point2d_ids(ba_cases.reconstruction(sc))
    assert {(iid, ids0[iid][k]) for iid, k in removed} == planted and rec.num_points3D() == E2E_SCENE["npts"]
    assert np.array_equal(_bits([p.error for p in rec.points3D.values()]), _bits(f["point_error"]))
    pc.bundle_adjustment(rec, options)
    second = pycolmap.last_run_stats()
    assert second["final_cost"] == b2["final_cost"] and second["final_cost"] < first["final_cost"]
    assert second["num_observations"] == first["num_observations"] - len(planted)


def test_update_point3D_errors_then_mean_equals_the_reference(ctx):
    rec = ba_cases.reconstruction(ba_cases.scene(**E2E_SCENE))
    assert all(p.error == -1.0 for p in rec.points3D.values()) and rec.compute_mean_reprojection_error() == -1.0
    args, _ = fc.flatten_reconstruction(rec)
    want = ref.filter_points3d(*args, errors_only=True)
    state = [(p, e) for p, e, _ in fc.model_state(rec)]
    assert rec.update_point3D_errors() is None
    assert [(p, e) for p, e, _ in fc.model_state(rec)] == state  # nothing is deleted
    assert np.array_equal(_bits([p.error for p in rec.points3D.values()]), _bits(want["point_error"]))
    total = 0.0
    for e in want["point_error"]:  # ascending ids are the points' order here
        total += float(e)
    assert rec.compute_mean_reprojection_error() == total / len(want["point_error"])
    rec2 = ba_cases.reconstruction(ba_cases.scene(**E2E_SCENE))
    rec2.update_point_3d_errors()
    assert [p.error for p in rec2.points3D.values()] == [p.error for p in rec.points3D.values()]
