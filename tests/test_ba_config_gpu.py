"""Bundle adjustment with constant points on the GPU and BundleAdjuster.solve: Context.bundle_adjust with
a point mask equals the CPU reference (tests/ba_config_ref) and its frozen fixture bit for bit on
tests/ba_config_cases.py's cases, the costs by bit pattern (16.6 F6); the masked entry with NULL and with zeros equals
amc_bundle_adjust on the existing cases; BundleAdjuster.solve equals the reference applied to the model, and the rest of
the model keeps its bits."""
import copy
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import ba_cases
import ba_config_cases as cc
import ba_config_ref_lib as ref
from pycolmap_amd import _capi

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "ba_config_ref_v1.npz"
GOLDEN_BA = Path(__file__).resolve().parent / "golden" / "ba_ref_v1.npz"
GOLDEN_BA_EDGES = Path(__file__).resolve().parent / "golden" / "ba_ref_edges_v1.npz"


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
    for k in ba_cases.RESULT_STATS:
        if k in ("initial_cost", "final_cost"):
            assert bits(got[k])[0] == bits(want[k])[0], (what, k, got[k], want[k])
        else:
            assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ba_cases.RESULT_ARRAYS:
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k)


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_masked_bundle_adjust_equals_reference_and_fixture(name, ctx, golden):
    args, pm, options = cc.case_problem(name)
    want = ref.bundle_adjust(*args, options=options, point_const=pm)
    got = ctx.bundle_adjust(*args, options=options, point_const=pm)
    assert_same(got, want, name)
    assert ba_cases.digest(got) == str(golden[f"{name}/digest"])
    # a constant point's xyz comes back bit for bit
    assert np.array_equal(bits(got["xyz"][pm != 0]), bits(np.asarray(args[7])[pm != 0]))
    assert got["num_variable_parameters"] == want["num_variable_parameters"]
    if name == "everything_const":
        assert got["termination"] == "NOTHING_TO_REFINE" and got["num_variable_parameters"] == 0


def test_refused_masks_and_the_context_stays_usable(ctx):
    """a variable point with one observation and a constant point without observations are AMC_E_INVALID; a constant
    point with one observation is not"""
    args, pm, options = cc.case_problem("all_points_const")
    oi, op = np.asarray(args[8]), np.asarray(args[9])
    first = np.flatnonzero(op == 0)

    def without(drop):
        keep = np.ones(oi.size, bool)
        keep[drop] = False
        a = list(args)
        a[8], a[9], a[10] = oi[keep], op[keep], np.asarray(args[10])[keep]
        return tuple(a)
    one = np.zeros(len(pm), np.uint8)
    with pytest.raises(_capi.AmcError, match="point 0 has 1 observations"):
        ctx.bundle_adjust(*without(first[1:]), options=options, point_const=one)
    one[0] = 1
    with pytest.raises(_capi.AmcError, match="point 0 has 0 observations"):
        ctx.bundle_adjust(*without(first), options=options, point_const=one)
    got = ctx.bundle_adjust(*without(first[1:]), options=options, point_const=one)
    want = ref.bundle_adjust(*without(first[1:]), options=options, point_const=one)
    assert_same(got, want, "a constant point with one observation")
    with pytest.raises(ValueError, match="point_const"):
        ctx.bundle_adjust(*args, options=options, point_const=one[:-1])


def _masked_raw(ctx, args, options, mask):
    """amc_bundle_adjust_masked called directly: mask None is the NULL pointer"""
    models, prm, cmask, icam, q, t, pc, X, oi, op, xy = _capi.ba_inputs(*args)
    o = _capi.ba_options(options)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    pb = _capi.BaProblem(models.size, ptr(models), ptr(prm), ptr(cmask), icam.size, ptr(icam), ptr(q), ptr(t), ptr(pc),
                         X.shape[0], ptr(X), oi.size, ptr(oi), ptr(op), ptr(xy))
    res = _capi.BaResult()
    rc = ctx._lib.amc_bundle_adjust_masked(ctx._h, C.byref(pb), None if mask is None else ptr(mask), C.byref(o), C.byref(res))
    assert rc == 0
    out = {k: getattr(res, k) for k, _ in _capi.BaResult._fields_}
    out["termination"] = _capi.BA_TERMINATIONS[res.termination]
    out.update(camera_params=prm, qvec=q, tvec=t, xyz=X)
    return out


@pytest.mark.parametrize("name", sorted(ba_cases.CASES) + sorted(ba_cases.EDGE_CASES))
def test_masked_entry_with_null_and_with_zeros_equals_bundle_adjust(name, ctx):
    edge = name in ba_cases.EDGE_CASES
    args, options = ba_cases.edge_problem(name) if edge else ba_cases.case_problem(name)
    frozen = np.load(GOLDEN_BA_EDGES if edge else GOLDEN_BA)
    plain = ctx.bundle_adjust(*args, options=options)
    assert ba_cases.digest(plain) == str(frozen[f"{name}/digest"])
    assert_same(_masked_raw(ctx, args, options, None), plain, "NULL")
    assert_same(_masked_raw(ctx, args, options, np.zeros(len(args[7]), np.uint8)), plain, "zeros")


@pytest.mark.parametrize("name", ["points257_second", "two_models_one_const"])
def test_permuted_points_with_the_mask_permuted(name, ctx):
    """15.7: no sum runs over the points' index except the sums over a vector of the step's scalars, which see the same
    terms in another order; so the reference itself is the yardstick for the permuted problem, and a constant point stays
    where it was in either order"""
    args, pm, options = cc.case_problem(name)
    pargs, ppm, order = cc.permuted(args, pm)
    got = ctx.bundle_adjust(*pargs, options=options, point_const=ppm)
    assert_same(got, ref.bundle_adjust(*pargs, options=options, point_const=ppm), name)
    assert np.array_equal(bits(got["xyz"][ppm != 0]), bits(np.asarray(args[7])[order][ppm != 0]))


def test_two_calls_in_a_row_and_inputs_untouched(ctx):
    args, pm, options = cc.case_problem("points257_second")
    before = [np.array(a, copy=True) for a in args] + [pm.copy()]
    a = ctx.bundle_adjust(*args, options=options, point_const=pm)
    b = ctx.bundle_adjust(*args, options=options, point_const=pm)
    assert_same(a, b)
    for x, y in zip(before, list(args) + [pm]):
        assert np.array_equal(x, np.asarray(y))


# ---- through Python ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.SCENES))
def test_solve_equals_reference_applied_to_the_model(name, ctx, golden):
    import pycolmap_amd as pc
    r, adj = cc.adjuster(pc, name)
    r_ref = copy.deepcopy(r)
    start = cc.model_bits(r)
    d = adj._problem(r)
    flat = ctx.bundle_adjust(*cc.flat_args(d), options=cc.SCENES[name][2], point_const=np.asarray(d["point_const"]).reshape(-1))
    assert ba_cases.digest(flat) == str(golden[f"scene/{name}/digest"])
    assert adj.solve(r) is True
    st = adj.summary
    assert st == pc.last_run_stats() and st["call"] == "BundleAdjuster.solve"
    assert st["device_ms"] >= st["kernel_ms"] > 0
    adj_ref = pc.BundleAdjuster(adj.options, adj.config)
    assert adj_ref._solve_with(r_ref, cc.reference_solver(ref)) is True
    got, want = cc.model_bits(r), cc.model_bits(r_ref)
    assert got == want
    for k in ("num_images", "num_points", "num_observations", "num_variable_parameters", "num_constant_points",
              "num_skipped_points", "num_successful_steps", "num_unsuccessful_steps", "num_pcg_iterations", "termination"):
        assert st[k] == adj_ref.summary[k], k
    for k in ("initial_cost", "final_cost"):
        assert bits(st[k])[0] == bits(adj_ref.summary[k])[0] == bits(flat[k])[0], k
    # the rest of the model keeps its bits
    cams, imgs, pts = list(r.cameras), list(r.images), list(r.points3D)
    in_problem = {("camera", cams[int(k)]) for k in np.asarray(d["camera_at"]).reshape(-1)}
    in_problem |= {("image", imgs[int(k)]) for k in np.asarray(d["image_at"]).reshape(-1)}
    in_problem |= {("point", pts[int(k)]) for k in np.asarray(d["point_at"]).reshape(-1)}
    changed = {k for k in start if start[k] != got[k]}
    assert changed and changed <= in_problem
    const_pts = {("point", pts[int(k)]) for k, c in zip(np.asarray(d["point_at"]).reshape(-1), np.asarray(d["point_const"]).reshape(-1)) if c}
    assert not (changed & const_pts)


def test_chain_triangulate_local_solve_filter():
    """triangulate_image for every image, a local solve around the last images with the rest of the map held fixed,
    filter_points3D of the points the solve moved: the planted points remain and sit at their true places"""
    import pycolmap_amd as pc
    import triangulator_cases as tc
    sc = tc.scene(seed=33, nimg=12, npts=25, models=(2,), noise=0.3, wrong=3, views=(5, 12))
    r, g = tc.reconstruction(sc)
    t = pc.IncrementalTriangulator(g, r)
    for iid in sc["images"]:
        t.triangulate_image({}, iid)
    cfg = pc.BundleAdjustmentConfig()
    local = list(sc["images"])[-3:]
    for iid in local:
        cfg.add_image(iid)
    cfg.set_constant_cam_pose(local[0])
    # every track is longer than the three local images, so a point is variable only when it is listed: the points of the
    # last image, whose other views then enter as constant poses
    for p2 in r.images[local[-1]].points2D:
        if p2.has_point3D():
            cfg.add_variable_point(p2.point3D_id)
    assert cfg.num_variable_points() > 0
    o = pc.BundleAdjustmentOptions()
    o.refine_focal_length = o.refine_extra_params = False
    o.solver_options.max_num_iterations = 5
    before = cc.model_bits(r)
    adj = pc.BundleAdjuster(o, cfg)
    assert adj.solve(r) is True
    st = adj.summary
    assert st["final_cost"] < st["initial_cost"] and st["num_constant_points"] > 0
    after = cc.model_bits(r)
    moved = {k[1] for k in before if k[0] == "point" and before[k] != after[k]}
    assert moved and {k for k in before if k[0] == "image" and before[k] != after[k]} <= {("image", i) for i in local[1:]}
    r.filter_points3D(4.0, 1.5, moved)
    planted = {j: set(tr) for j, tr in sc["planted"].items()}
    checked = 0
    for pid in moved & set(r.points3D):
        p = r.points3D[pid]
        track = {(e.image_id, e.point2D_idx) for e in p.track.elements}
        owners = [j for j, tr in planted.items() if track <= tr]
        if len(owners) == 1:
            np.testing.assert_allclose(np.array(p.xyz), sc["xyz"][owners[0]], atol=0.05)
            checked += 1
    assert checked > 0
