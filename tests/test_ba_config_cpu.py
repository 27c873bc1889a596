"""BundleAdjustmentConfig, BundleAdjuster and bundle adjustment with constant points without a GPU: the
surface and its ValueErrors, num_residuals against a brute-force count, the masked CPU reference (tests/ba_config_ref)
against tests/ba_ref with an all-zero mask, against its frozen fixture, against hand-built answers and against scipy with
point masks; the set-up against an independent Python restatement; solve with the reference in the library's place; the
host half under ASan + UBSan in a stand-alone program."""
import copy
import json
import pickle
from pathlib import Path

import numpy as np
import pytest

import ba_cases
import ba_config_cases as cc
import ba_config_ref_lib as ref
import ba_ref_lib
import pycolmap_amd as pc
from pycolmap_amd import _capi

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "ba_config_ref_v1.npz"
BUDGET = ROOT / "tests" / "ref2" / "ba_config_deviation_budget.json"


def bits(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)


# ---- the surface ------------------------------------------------------------------------------------------------------------
def test_names_and_the_exported_symbol():
    import pycolmap
    assert pycolmap.BundleAdjustmentConfig is pc.BundleAdjustmentConfig and pycolmap.BundleAdjuster is pc.BundleAdjuster
    assert "amc_bundle_adjust_masked" in _capi.EXPORTED_SYMBOLS
    assert hasattr(_capi.load(), "amc_bundle_adjust_masked")
    header = (ROOT / "include" / "amc_ba.h").read_text()
    assert "int amc_bundle_adjust_masked(amc_ctx* ctx, amc_ba_problem* problem, const uint8_t* point_const," in header
    assert "#define AMC_ABI_VERSION 5" in (ROOT / "include" / "amc.h").read_text()
    for absent in ("triangulate_points", "incremental_mapping", "Sim3d"):
        with pytest.raises(AttributeError):
            getattr(pycolmap, absent)


def test_config_counts_sets_and_copies():
    c = pc.BundleAdjustmentConfig()
    assert (c.num_images(), c.num_points(), c.num_constant_cam_intrinsics(), c.num_constant_cam_poses(),
            c.num_constant_cam_positions(), c.num_variable_points(), c.num_constant_points()) == (0,) * 7
    for i in (5, 2, 9):
        c.add_image(i)
    c.add_image(5)
    assert c.num_images() == 3 and c.has_image(2) and not c.has_image(3) and c.image_ids == {2, 5, 9}
    c.remove_image(9)
    assert c.image_ids == {2, 5}
    c.set_constant_cam_intrinsics(7)
    assert c.is_constant_cam_intrinsics(7) and not c.is_constant_cam_intrinsics(8) and c.num_constant_cam_intrinsics() == 1
    c.set_variable_cam_intrinsics(7)
    assert not c.is_constant_cam_intrinsics(7)
    c.set_constant_cam_pose(2)
    assert c.has_constant_cam_pose(2) and c.num_constant_cam_poses() == 1
    c.set_variable_cam_pose(2)
    assert not c.has_constant_cam_pose(2)
    c.set_constant_cam_positions(5, [2, 0])
    assert c.has_constant_cam_positions(5) and c.constant_cam_positions(5) == [2, 0] and c.num_constant_cam_positions() == 1
    c.remove_constant_cam_positions(5)
    assert not c.has_constant_cam_positions(5)
    c.set_constant_cam_positions(5, [1])
    c.add_variable_point(11)
    c.add_constant_point(12)
    assert c.has_point(11) and c.has_point(12) and not c.has_point(13)
    assert c.has_variable_point(11) and not c.has_variable_point(12) and c.has_constant_point(12)
    assert (c.num_points(), c.num_variable_points(), c.num_constant_points()) == (2, 1, 1)
    assert c.variable_point3D_ids == {11} and c.constant_point3D_ids == {12}
    for d in (copy.copy(c), copy.deepcopy(c), pickle.loads(pickle.dumps(c))):
        assert repr(d) == repr(c) and d.image_ids == c.image_ids and d.constant_cam_positions(5) == [1]
        assert d.variable_point3D_ids == {11} and d.constant_point3D_ids == {12}
        d.add_image(77)
        assert not c.has_image(77)
    assert repr(c) == ("BundleAdjustmentConfig(num_images=2, num_constant_cam_intrinsics=0, num_constant_cam_poses=0, "
                       "num_constant_cam_positions=1, num_variable_points=1, num_constant_points=1)")
    c.remove_variable_point(11)
    c.remove_constant_point(12)
    assert c.num_points() == 0
    c.add_constant_point(11)  # after the removal the other list takes it


@pytest.mark.parametrize("call, expr", [
    (lambda c: c.set_constant_cam_pose(4), "HasImage(image_id)"),
    (lambda c: c.set_constant_cam_positions(4, [0]), "HasImage(image_id)"),
    (lambda c: c.set_constant_cam_pose(2), "!HasConstantCamPositions(image_id)"),
    (lambda c: c.set_constant_cam_positions(1, [0]), "!HasConstantCamPose(image_id)"),
    (lambda c: c.set_constant_cam_positions(3, []), "idxs.size() > 0"),
    (lambda c: c.set_constant_cam_positions(3, [0, 1, 2, 0]), "idxs.size() <= 3"),
    (lambda c: c.set_constant_cam_positions(3, [1, 1]), "!VectorContainsDuplicateValues(idxs)"),
    (lambda c: c.set_constant_cam_positions(3, [3]), "idx >= 0 && idx < 3"),
    (lambda c: c.set_constant_cam_positions(3, [-1]), "idx >= 0 && idx < 3"),
    (lambda c: c.constant_cam_positions(3), "HasConstantCamPositions(image_id)"),
    (lambda c: c.add_constant_point(8), "!HasVariablePoint(point3D_id)"),
    (lambda c: c.add_variable_point(9), "!HasConstantPoint(point3D_id)"),
])
def test_config_checks_are_value_errors_in_the_check_format(call, expr):
    c = pc.BundleAdjustmentConfig()
    for i in (1, 2, 3):
        c.add_image(i)
    c.set_constant_cam_pose(1)
    c.set_constant_cam_positions(2, [0])
    c.add_variable_point(8)
    c.add_constant_point(9)
    before = repr(c)
    with pytest.raises(ValueError) as e:
        call(c)
    msg = str(e.value)
    assert msg.startswith("[ba_config_host.h:") and msg.endswith("] Check Failed: " + expr), msg
    assert repr(c) == before


def _brute_force_residuals(r, images, points):
    n = sum(1 for iid in images for p in r.images[iid].points2D if p.has_point3D())
    n += sum(1 for pid in points for e in r.points3D[pid].track.elements if e.image_id not in images)
    return 2 * n


@pytest.mark.parametrize("name", sorted(cc.SCENES))
def test_num_residuals_against_a_brute_force_count(name):
    r, adj = cc.adjuster(pc, name)
    cfg = adj.config
    want = _brute_force_residuals(r, cfg.image_ids, cfg.variable_point3D_ids | cfg.constant_point3D_ids)
    assert cfg.num_residuals(r) == want > 0
    cfg.add_image(999)
    with pytest.raises(ValueError):
        cfg.num_residuals(r)


def test_adjuster_reads_back_and_refuses_unknown_ids():
    r, adj = cc.adjuster(pc, "local")
    assert adj.options.solver_options.max_num_iterations == 4 and adj.config.image_ids == {2, 3, 4} and adj.summary == {}
    start = cc.model_bits(r)
    for make in (lambda c: c.add_image(99), lambda c: c.add_variable_point(999), lambda c: c.add_constant_point(998)):
        cfg = cc.local_config(pc)
        make(cfg)
        with pytest.raises(ValueError, match="the reconstruction has no"):
            pc.BundleAdjuster(adj.options, cfg)._solve_with(r, cc.reference_solver(ref))
    assert cc.model_bits(r) == start
    # no residual: False, nothing touched, no solver call
    empty = pc.BundleAdjuster(adj.options, pc.BundleAdjustmentConfig())
    assert empty._solve_with(r, lambda d: pytest.fail("the solver was called")) is False
    assert empty.solve(r) is False and cc.model_bits(r) == start
    # the caller's config is not modified by a solve (COLMAP adds the pulled-in cameras to it)
    cfg = cc.local_config(pc)
    a = pc.BundleAdjuster(adj.options, cfg)
    assert a._solve_with(r, cc.reference_solver(ref)) is True
    assert repr(cfg) == repr(cc.local_config(pc)) == repr(a.config) and not a.config.is_constant_cam_intrinsics(2)


def test_solve_without_a_gpu_raises_and_leaves_the_model():
    if _capi.device_count() > 0:
        pytest.skip("a GPU is visible; this test covers the CPU-only container")
    r, adj = cc.adjuster(pc, "local")
    start = cc.model_bits(r)
    with pytest.raises(_capi.AmcError):
        adj.solve(r)
    assert cc.model_bits(r) == start and adj.summary == {}


# ---- the masked reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ba_cases.CASES) + sorted(ba_cases.EDGE_CASES))
def test_zero_mask_equals_the_unmasked_reference(name):
    args, options = ba_cases.edge_problem(name) if name in ba_cases.EDGE_CASES else ba_cases.case_problem(name)
    want = ba_ref_lib.bundle_adjust(*args, options=options)
    for mask in ([None] if name == "min2" else []) + [np.zeros(len(args[7]), np.uint8)]:
        got = ref.bundle_adjust(*args, options=options, point_const=mask)
        for k in ba_cases.RESULT_STATS:
            assert bits(got[k])[0] == bits(want[k])[0] if isinstance(want[k], float) else got[k] == want[k], k
        for k in ba_cases.RESULT_ARRAYS:
            assert np.array_equal(bits(got[k]), bits(want[k])), k


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_reference_equals_fixture(name, golden):
    assert sorted(cc.CASES) == [str(n) for n in golden["names"]]
    args, pm, options = cc.case_problem(name)
    r = ref.bundle_adjust(*args, options=options, point_const=pm)
    assert ba_cases.digest(r) == str(golden[f"{name}/digest"])
    stats = np.array([ref.TERMINATIONS.index(r[k]) if k == "termination" else r[k] for k in ba_cases.RESULT_STATS], np.float64)
    assert np.array_equal(bits(stats), bits(golden[f"{name}/stats"]))
    # 15.12: constant points come back bit for bit and have no column
    assert np.array_equal(bits(r["xyz"][pm != 0]), bits(np.asarray(args[7])[pm != 0]))
    nvar = int((np.asarray(args[2]) == 0).sum() + (np.asarray(args[6]) == 0).sum() + 3 * (pm == 0).sum())
    for c, m in enumerate(args[0]):  # slots past the model's parameter count are constant
        nvar -= int((np.asarray(args[2])[c, len(ba_cases.model_params(m)):] == 0).sum())
    assert r["num_variable_parameters"] == nvar
    if r["termination"] != "NOTHING_TO_REFINE":
        assert r["final_cost"] < r["initial_cost"]


def test_cases_are_of_the_kind_their_names_say():
    def run(name):
        args, pm, options = cc.case_problem(name)
        return ref.bundle_adjust(*args, options=options, point_const=pm)
    r = run("rejected_step")
    assert r["num_unsuccessful_steps"] >= 1 and r["num_successful_steps"] >= 1
    r = run("pcg_breakdown")  # a solve that ends neither by the residual rule nor at the cap ended as a breakdown
    solves = r["num_successful_steps"] + r["num_unsuccessful_steps"]
    assert r["num_pcg_stops_residual"] + r["num_pcg_stops_cap"] < solves
    r = run("everything_const")
    assert r["termination"] == "NOTHING_TO_REFINE" and r["num_variable_parameters"] == 0
    assert run("points0_all")["termination"] == "NOTHING_TO_REFINE"
    assert run("all_points_const")["num_variable_parameters"] == 6 * 4 - 7 + 2
    # the three position subsets leave one, two and three translation columns out
    assert [run(f"positions_{s}")["num_variable_parameters"] for s in ("0", "12", "012")] == [78, 77, 76]


def test_reference_refuses_what_the_library_refuses():
    args, pm, options = cc.case_problem("all_points_const")
    oi, op, xy = (np.asarray(a) for a in args[8:])
    first = np.flatnonzero(op == 0)

    def without(drop):
        keep = np.ones(oi.size, bool)
        keep[drop] = False
        return args[:8] + (oi[keep], op[keep], xy[keep])
    one = np.zeros(len(pm), np.uint8)
    with pytest.raises(ValueError):  # a variable point with one observation
        ref.bundle_adjust(*without(first[1:]), options=options, point_const=one)
    one[0] = 1
    with pytest.raises(ValueError):  # a constant point without observations
        ref.bundle_adjust(*without(first), options=options, point_const=one)
    assert ref.bundle_adjust(*without(first[1:]), options=options, point_const=one)["num_successful_steps"] >= 1


def test_a_constant_points_residual_moves_the_pose_and_not_the_point():
    """hand-built: two images, every point constant; one point is moved off its place, so its residual is the only
    large one: its xyz comes back bit for bit while the variable pose moves, and the cost counts its residuals"""
    sc = ba_cases.scene(seed=350, nimg=2, npts=10, model=0, noise=0.0, perturb=0.0)
    args = list(ba_cases.problem(sc, refine_focal_length=False, refine_extra_params=False))
    assert np.array_equal(sc["xyz"], sc["true_xyz"])
    pm = np.ones(10, np.uint8)
    still = ref.bundle_adjust(*args, options=dict(max_num_iterations=3), point_const=pm)
    assert still["initial_cost"] < 1e-20 and np.abs(still["tvec"] - sc["tvec"]).max() < 1e-9
    X = np.array(sc["xyz"])
    X[4] += [0.05, -0.03, 0.02]
    args[7] = X
    r = ref.bundle_adjust(*args, options=dict(max_num_iterations=5), point_const=pm)
    assert np.array_equal(bits(r["xyz"]), bits(X))
    assert r["initial_cost"] > 1.0 and r["final_cost"] < r["initial_cost"]
    assert np.abs(r["tvec"][1] - sc["tvec"][1]).max() > 1e-4 and np.array_equal(bits(r["tvec"][0]), bits(sc["tvec"][0]))
    assert r["num_variable_parameters"] == 5


def test_noise_free_constant_points_return_the_true_pose():
    """hand-built: noise-free constant points at the truth and perturbed variable poses: resection of every pose"""
    sc = ba_cases.scene(seed=351, nimg=3, npts=20, model=0, noise=0.0, perturb=1.0)
    args = list(ba_cases.problem(sc, refine_focal_length=False, refine_extra_params=False))
    args[7] = sc["true_xyz"]
    args[1] = sc["true_params"]
    r = ref.bundle_adjust(*args, options=dict(max_num_iterations=30), point_const=np.ones(20, np.uint8))
    assert np.abs(sc["qvec"] - sc["true_qvec"]).max() > 1e-3
    assert np.abs(r["qvec"] - sc["true_qvec"]).max() < 1e-9 and np.abs(r["tvec"] - sc["true_tvec"]).max() < 1e-8
    assert r["final_cost"] < 1e-12 and np.array_equal(bits(r["xyz"]), bits(sc["true_xyz"]))


# ---- the set-up against an independent restatement ----------------------------------------------------------------------------
def _setup_restated(r, images, const_poses, const_positions, const_cameras, var_points, const_points, flags):
    """DESIGN.md 15.12's four steps on the Python objects: a dict keyed by ids"""
    nfocal = {m: n for m, n in zip(ba_cases.MODEL_NAMES, ba_cases.NUM_FOCAL)}
    residuals, count, skipped, cameras, pulled, order = [], {}, set(), set(), set(), []
    for iid, im in r.images.items():
        if iid not in images:
            continue
        n = 0
        for p2 in im.points2D:
            if not p2.has_point3D():
                continue
            if len(r.points3D[p2.point3D_id].track.elements) < 2:
                skipped.add(p2.point3D_id)
                continue
            residuals.append((iid, p2.point3D_id, tuple(p2.xy)))
            count[p2.point3D_id] = count.get(p2.point3D_id, 0) + 1
            n += 1
        if n:
            order.append(iid)
            cameras.add(im.camera_id)
    for listed in (var_points, const_points):
        for pid, p in r.points3D.items():
            if pid not in listed:
                continue
            if len(p.track.elements) < 2:
                skipped.add(pid)
                continue
            if count.get(pid, 0) == len(p.track.elements):
                continue
            for e in p.track.elements:
                if e.image_id in images:
                    continue
                residuals.append((e.image_id, pid, tuple(r.images[e.image_id].points2D[e.point2D_idx].xy)))
                count[pid] = count.get(pid, 0) + 1
                if e.image_id not in order:
                    order.append(e.image_id)
                cid = r.images[e.image_id].camera_id
                if cid not in cameras:
                    cameras.add(cid)
                    pulled.add(cid)
    pose_const = {}
    for iid in order:
        if iid not in images or not flags["refine_extrinsics"] or iid in const_poses:
            pose_const[iid] = [1] * 6
        else:
            pose_const[iid] = [0, 0, 0] + [int(k in const_positions.get(iid, [])) for k in range(3)]
    camera_const = {}
    none = not (flags["refine_focal_length"] or flags["refine_principal_point"] or flags["refine_extra_params"])
    for cid, cam in r.cameras.items():
        if cid not in cameras:
            continue
        nf, n = nfocal[cam.model.name if hasattr(cam.model, "name") else str(cam.model)], len(cam.params)
        row = [1] * 12
        if not (none or cid in pulled or cid in const_cameras):
            for k in range(n):
                group = "refine_focal_length" if k < nf else "refine_principal_point" if k < nf + 2 else "refine_extra_params"
                row[k] = 0 if flags[group] else 1
        camera_const[cid] = row
    point_const = {pid: int(len(r.points3D[pid].track.elements) > count[pid] or pid in const_points)
                   for pid in r.points3D if count.get(pid)}
    return dict(images=order, cameras=[c for c in r.cameras if c in cameras], pose_const=pose_const,
                camera_const=camera_const, point_const=point_const, residuals=residuals, skipped=len(skipped))


def _random_setup(seed):
    rng = np.random.default_rng(seed)
    sc = cc.local_scene() if seed % 2 else cc.pose_only_scene()
    r = ba_cases.reconstruction(sc)
    cfg = pc.BundleAdjustmentConfig()
    const_poses, const_positions = set(), {}
    for iid in r.images:
        if rng.random() < 0.5:
            cfg.add_image(iid)
            k = rng.integers(4)
            if k == 0:
                cfg.set_constant_cam_pose(iid)
                const_poses.add(iid)
            elif k == 1:
                idxs = [int(v) for v in rng.permutation(3)[:rng.integers(1, 4)]]
                cfg.set_constant_cam_positions(iid, idxs)
                const_positions[iid] = idxs
    const_cameras = {cid for cid in r.cameras if rng.random() < 0.3}
    for cid in const_cameras:
        cfg.set_constant_cam_intrinsics(cid)
    var_points, const_points = set(), set()
    for pid in r.points3D:
        k = rng.integers(5)
        if k == 0:
            cfg.add_variable_point(pid)
            var_points.add(pid)
        elif k == 1:
            cfg.add_constant_point(pid)
            const_points.add(pid)
    flags = dict(refine_focal_length=bool(rng.integers(2)), refine_principal_point=bool(rng.integers(2)),
                 refine_extra_params=bool(rng.integers(2)), refine_extrinsics=bool(rng.integers(4)))
    o = pc.BundleAdjustmentOptions()
    for k, v in flags.items():
        setattr(o, k, v)
    return r, pc.BundleAdjuster(o, cfg), (set(cfg.image_ids), const_poses, const_positions, const_cameras, var_points,
                                          const_points, flags)


def _check_setup(r, adj, described):
    d = adj._problem(r)
    want = _setup_restated(r, *described)
    cams, imgs, pts = list(r.cameras), list(r.images), list(r.points3D)
    got_images = [imgs[int(k)] for k in np.asarray(d["image_at"]).reshape(-1)]
    got_cameras = [cams[int(k)] for k in np.asarray(d["camera_at"]).reshape(-1)]
    got_points = [pts[int(k)] for k in np.asarray(d["point_at"]).reshape(-1)]
    assert got_images == want["images"] and got_cameras == want["cameras"]
    assert got_points == [p for p in r.points3D if p in want["point_const"]]
    assert [int(v) for v in np.asarray(d["point_const"]).reshape(-1)] == [want["point_const"][p] for p in got_points]
    assert np.asarray(d["pose_const"]).tolist() == [want["pose_const"][i] for i in got_images]
    assert np.asarray(d["camera_const"]).tolist() == [want["camera_const"][c] for c in got_cameras]
    got_res = [(got_images[int(i)], got_points[int(j)], (float(x), float(y))) for i, j, (x, y) in
               zip(np.asarray(d["obs_image"]).reshape(-1), np.asarray(d["obs_point"]).reshape(-1), np.asarray(d["obs_xy"]))]
    assert got_res == want["residuals"]
    assert d["num_skipped_points"] == want["skipped"]
    for k, iid in enumerate(got_images):
        im = r.images[iid]
        assert cams[int(np.asarray(d["camera_at"]).reshape(-1)[int(np.asarray(d["image_cameras"]).reshape(-1)[k])])] == im.camera_id
        assert np.array_equal(np.asarray(d["tvec"])[k], np.asarray(im.cam_from_world.translation))
    for k, pid in enumerate(got_points):
        assert np.array_equal(np.asarray(d["xyz"])[k], np.asarray(r.points3D[pid].xyz))
    return d, want


def test_setup_of_the_named_scenes():
    r, adj = cc.adjuster(pc, "local")
    flags = dict(refine_focal_length=True, refine_principal_point=False, refine_extra_params=True, refine_extrinsics=True)
    d, want = _check_setup(r, adj, ({2, 3, 4}, set(), {3: [0]}, set(), {6}, {3, 10}, flags))
    # the kinds local_scene() plants
    assert want["images"] == [2, 3, 4, 6, 1, 5] and want["cameras"] == [1, 2]
    assert want["camera_const"][2] == [1] * 12 and want["camera_const"][1][:4] == [0, 1, 1, 0]
    pcst = want["point_const"]
    assert pcst[1] == 0 and pcst[2] == 1 and pcst[3] == 1 and pcst[6] == 0 and pcst[10] == 1 and pcst[4] == 1 and 24 not in pcst
    assert sum(1 for res in want["residuals"] if res[1] == 4) == 1 and want["skipped"] == 1
    assert want["pose_const"][3] == [0, 0, 0, 1, 0, 0] and want["pose_const"][6] == [1] * 6
    r, adj = cc.adjuster(pc, "structure_only")
    d, want = _check_setup(r, adj, (set(), set(), {}, set(), set(range(1, 21, 2)), set(), flags))
    assert all(v == [1] * 6 for v in want["pose_const"].values()) and set(want["point_const"].values()) == {0}


@pytest.mark.parametrize("seed", range(12))
def test_setup_against_the_restatement_on_seeded_configs(seed):
    _check_setup(*_random_setup(seed))


# ---- solve with the reference in the library's place ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.SCENES))
def test_solve_with_the_reference(name, golden):
    r, adj = cc.adjuster(pc, name)
    start = cc.model_bits(r)
    d = adj._problem(r)
    pm = np.asarray(d["point_const"]).reshape(-1)
    assert np.array_equal(pm, golden[f"scene/{name}/point_const"])
    want = ref.bundle_adjust(*cc.flat_args(d), options=cc.SCENES[name][2], point_const=pm)
    assert ba_cases.digest(want) == str(golden[f"scene/{name}/digest"])
    assert adj._solve_with(r, cc.reference_solver(ref)) is True
    got = cc.model_bits(r)
    cams, imgs, pts = list(r.cameras), list(r.images), list(r.points3D)
    expect = dict(start)
    for k, c in enumerate(np.asarray(d["camera_at"]).reshape(-1)):
        n = len(r.cameras[cams[int(c)]].params)
        expect["camera", cams[int(c)]] = want["camera_params"][k, :n].tobytes()
    for k, i in enumerate(np.asarray(d["image_at"]).reshape(-1)):
        q = want["qvec"][k]
        stored = np.asarray(r.images[imgs[int(i)]].cam_from_world.rotation.quat, np.float64)
        assert sorted(np.abs(stored)) == sorted(np.abs(q))  # the same four numbers, whatever the attribute's order
        expect["image", imgs[int(i)]] = stored.tobytes() + want["tvec"][k].tobytes()
    for k, j in enumerate(np.asarray(d["point_at"]).reshape(-1)):
        expect["point", pts[int(j)]] = want["xyz"][k].tobytes()
    assert got == expect
    changed = {k for k in start if start[k] != got[k]}
    const_pts = {("point", pts[int(j)]) for j, c in zip(np.asarray(d["point_at"]).reshape(-1), pm) if c}
    assert changed and not (changed & const_pts)
    st = adj.summary
    assert st == pc.last_run_stats()
    # the keys last_run_stats() has after bundle_adjustment, plus num_constant_points
    for k in ("call", "num_images", "num_points", "num_observations", "num_variable_parameters", "num_filtered_observations",
              "num_skipped_points", "initial_cost", "final_cost", "num_successful_steps", "num_unsuccessful_steps",
              "num_pcg_iterations", "termination", "device_ms", "kernel_ms", "host_ms", "num_constant_points"):
        assert k in st, k
    assert st["num_constant_points"] == int(pm.sum()) and st["final_cost"] == want["final_cost"]
    assert st["num_variable_parameters"] == want["num_variable_parameters"]


# ---- accuracy against an independent solver -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def budget():
    """tests/test_ba_cpu.py's rule on its accuracy scenes with every second point constant: both scipy costs, the
    reference's cost and the bound per case, written to tests/ref2/ba_config_deviation_budget.json (a record: the test
    asserts on the figures computed here)"""
    import ba_config_scipy
    out = {}
    for name, (scene_args, loss) in ba_cases.ACCURACY_CASES.items():
        sc = ba_cases.scene(**scene_args)
        args = ba_cases.problem(sc)
        pm = cc.mask("second", len(sc["xyz"]))
        P = ba_config_scipy.MaskedProblem(*args, loss=loss, loss_scale=2.0, point_const=pm)
        c10, _ = P.solve(1e-10)
        c14, (_, _, _, X) = P.solve(1e-14)
        assert np.array_equal(X[pm != 0], np.asarray(sc["xyz"])[pm != 0])
        r = ref.bundle_adjust(*args, options=dict(loss_function_type=loss, loss_function_scale=2.0, max_num_iterations=100),
                              point_const=pm)
        margin = 10.0 * abs(c10 - c14) / c14
        out[name] = dict(scipy_cost_tol_1e_10=c10, scipy_cost_tol_1e_14=c14, reference_cost=r["final_cost"],
                         relative_margin=margin, bound=c14 * (1.0 + margin), termination=r["termination"])
    try:
        BUDGET.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    except OSError:
        pass  # a read-only checkout: the figures are asserted on all the same
    return out


@pytest.mark.parametrize("name", sorted(ba_cases.ACCURACY_CASES))
def test_converged_cost_with_a_mask_is_not_above_scipys(name, budget):
    """the existing rule: the reference's final cost is at most scipy's cost at tolerance 1e-14 times one plus ten times
    the relative gap between scipy's costs at 1e-10 and 1e-14"""
    b = budget[name]
    assert b["reference_cost"] <= b["bound"], b


# ---- the host half under sanitizers -----------------------------------------------------------------------------------------------
def _sanitized_program(tmp_path, name, sources):
    """Builds tests/shim/<name>.cc (+ sources) with ASan + UBSan, the way tests/test_ba_cpu.py builds its programs.  Whether
    the sanitizer runtime is installed is probed with a trivial program first, so that a failure of the real build is a
    failure and not a skip."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    flags = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined"]
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("sanitizer runtime not installed")
    exe = tmp_path / name
    b = subprocess.run(flags + [str(ROOT / "tests" / "shim" / (name + ".cc"))] + [str(ROOT / s) for s in sources] +
                       ["-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    return exe


def _run_sanitized(exe, *args):
    import os
    import subprocess
    return subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))


def test_config_setup_and_masked_plan_under_asan(tmp_path):
    """csrc/host/ba_config_host.h (the config's checks, the set-up, the write-back) and csrc/ba_plan.h's checks with a point
    mask in a stand-alone program under ASan + UBSan (tests/shim/ba_config_host_fuzz.cc): 300 seeded models and configs,
    valid and corrupted (ids the model does not hold, broken cross references, masks that leave a variable point one
    observation or a constant point none)"""
    exe = _sanitized_program(tmp_path, "ba_config_host_fuzz", ["pycolmap_amd/csrc/host/model_io.cc",
                                                               "pycolmap_amd/csrc/host/reconstruction.cc"])
    r = _run_sanitized(exe)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[1]) > 2000
