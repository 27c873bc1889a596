"""The joint pose and camera refinement without a GPU: the surface, the header against _capi, the
CPU reference (tests/absrefine_ref) against its fixture, against the section-12 reference where the camera is constant,
against central differences and scipy within measured budgets, two answers worked out by hand, the mapper's
registration with the references in the library's place, and the host plan in a stand-alone program under ASan + UBSan."""
import ctypes
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import abspose_cases
import abspose_ref_lib
import absrefine_cases as cases
import absrefine_ref_lib as ref
import pycolmap
import pycolmap_amd as pc
from pycolmap_amd import _capi, _pose_intrinsics

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "absrefine_ref_v1.npz"
BUDGET = ROOT / "tests" / "ref2" / "absrefine_deviation_budget.json"
sys.path.insert(0, str(ROOT / "tests" / "ref2"))
NAMES = ("refine_absolute_pose", "estimate_and_refine_absolute_pose", "register_next_image_and_refine")


# ---- the surface ---------------------------------------------------------------------------------------------------------
def test_names_on_both_packages_and_the_alias_message():
    for name in NAMES:
        assert getattr(pycolmap, name) is getattr(pc, name) is getattr(_pose_intrinsics, name) and name in pycolmap._PUBLIC
        assert getattr(pc, name).__doc__ and "section 25" in getattr(pc, name).__doc__
    assert "refine_absolute_pose" in pycolmap.__doc__ and "DESIGN.md section 25" in pycolmap.__doc__
    with pytest.raises(AttributeError, match=r"refine_absolute_pose, estimate_and_refine_absolute_pose, and "
                                             r"register_next_image_and_refine with the mapper as first argument; DESIGN.md section 25"):
        pycolmap.incremental_mapping
    # the compiled module's surface is pinned elsewhere (tests/test_host_surface_cpu.py): these are Python names only
    assert not any(hasattr(pc._pycolmap, n) for n in NAMES)


def test_the_old_entries_keep_refusing_the_flags():
    cam = pc.Camera(model=0, width=100, height=100, params=[100.0, 50.0, 50.0])
    pose = pc.Rigid3d()
    for flag in ("refine_focal_length", "refine_extra_params"):
        with pytest.raises(ValueError, match=f"{flag}=True is not supported"):
            pc.pose_refinement(pose, np.zeros((3, 2)), np.zeros((3, 3)), np.ones(3, bool), cam,
                               pc.AbsolutePoseRefinementOptions({flag: True}))


def test_option_protocol_and_shape_checks():
    cam = pc.Camera(model=2, width=100, height=100, params=[100.0, 50.0, 50.0, 0.1])
    pose = pc.Rigid3d()
    with pytest.raises(ValueError, match=r"Check Failed: points2D.size\(\) == points3D.size\(\) \(3 vs. 2\)"):
        pc.refine_absolute_pose(pose, np.zeros((3, 2)), np.zeros((2, 3)), np.ones(3, bool), cam)
    with pytest.raises(ValueError, match=r"Check Failed: inlier_mask.size\(\) == points2D.size\(\) \(2 vs. 3\)"):
        pc.refine_absolute_pose(pose, np.zeros((3, 2)), np.zeros((3, 3)), np.ones(2, bool), cam)
    with pytest.raises(ValueError, match=r"Check Failed: points2D.size\(\) == points3D.size\(\) \(3 vs. 4\)"):
        pc.estimate_and_refine_absolute_pose(np.zeros((3, 2)), np.zeros((4, 3)), cam)
    with pytest.raises(ValueError, match="points2D must be an N x 2 array"):
        pc.refine_absolute_pose(pose, np.zeros((3, 3)), np.zeros((3, 3)), np.ones(3, bool), cam)
    with pytest.raises(TypeError, match="refinement_options"):
        pc.refine_absolute_pose(pose, np.zeros((3, 2)), np.zeros((3, 3)), np.ones(3, bool), cam, 5)
    with pytest.raises(TypeError, match="a Camera is needed"):
        pc.refine_absolute_pose(pose, np.zeros((3, 2)), np.zeros((3, 3)), np.ones(3, bool), None)
    # the classes and dicts give the same C options
    o = pc.AbsolutePoseRefinementOptions(dict(refine_focal_length=True, max_num_iterations=7))
    assert _pose_intrinsics._refinement(o) == _pose_intrinsics._refinement(dict(refine_focal_length=True, max_num_iterations=7))
    assert _pose_intrinsics._refinement(o)["refine_focal_length"] == 1 and _pose_intrinsics._refinement(None)["refine_extra_params"] == 0
    e = _pose_intrinsics._estimation(dict(estimate_focal_length=True, ransac=dict(max_error=3.0)))
    assert e["estimate_focal_length"] == 1 and e["max_error"] == 3.0 and e["max_num_trials"] == 100000
    assert e == _pose_intrinsics._estimation(pc.AbsolutePoseEstimationOptions(dict(estimate_focal_length=True, ransac=dict(max_error=3.0))))


def test_without_a_gpu_the_functions_raise_and_change_nothing():
    if _capi.device_count() > 0:
        pytest.skip("a GPU is visible; this test covers the CPU-only container")
    import mapper_cases as k
    sc = cases.CASES["model2_f1e1"][1]
    cam = pc.Camera(model=2, width=1600, height=1200, params=sc["camera_params"][0])
    before = np.array(cam.params)
    pose = pc.Rigid3d(pc.Rotation3d(sc["start_q"][0]), sc["start_t"][0])
    with pytest.raises(_capi.AmcError):
        pc.refine_absolute_pose(pose, sc["points2D"], sc["points3D"], sc["mask"], cam, cases.BOTH)
    with pytest.raises(_capi.AmcError):
        pc.estimate_and_refine_absolute_pose(sc["points2D"], sc["points3D"], cam, None, cases.BOTH)
    assert np.array_equal(np.array(cam.params), before)
    st = k.mapper_state("direct")
    r, _, _, mp = k.mapper(st)
    snap = k.model_snapshot(r)
    first = sorted(st["candidates"])[0]
    with pytest.raises(_capi.AmcError):
        pc.register_next_image_and_refine(mp, k.SCENE_OPTIONS, first)
    assert k.model_snapshot(r) == snap and mp.num_reg_trials(first) == 0 and mp.last_registration() == {}


def test_header_symbols_and_structs():
    lib = _capi.load()
    text = (ROOT / "include" / "amc_absrefine.h").read_text()
    for name in ("amc_refine_poses_and_cameras", "amc_estimate_poses_and_cameras", "amc_absrefine_result_free"):
        assert hasattr(lib, name) and name in _capi.EXPORTED_SYMBOLS and name in text
    assert lib.amc_abi_version() == 5 and "AMC_ABI_VERSION 5" in (ROOT / "include" / "amc.h").read_text()
    assert ctypes.sizeof(_capi.AbsRefineResult) == 2 * 8 + 9 * 8 + 2 * 8 + 8 + 8
    body = text[text.index("typedef struct amc_absrefine_result"):text.index("} amc_absrefine_result;")]
    assert re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [f for f, _ in _capi.AbsRefineResult._fields_]
    assert "absrefine.hip" in (ROOT / "pycolmap_amd" / "build.py").read_text()
    source = (ROOT / "pycolmap_amd" / "csrc" / "absrefine.hip").read_text() + (ROOT / "pycolmap_amd" / "csrc" / "absrefine_core.h").read_text()
    assert "atomic" not in source.replace("No atomics", "")
    assert "AMC_ABSREFINE_BATCH_QUERIES" in source and "AMC_ABSREFINE_BATCH_QUERIES" in (ROOT / "README.md").read_text()
    assert "amc_absrefine.h" in (ROOT / "INTEGRATION.md").read_text()


# ---- the reference ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference():
    out = {}
    for n in cases.CASES:
        if cases.CASES[n][0] == "refine":
            out[n] = cases.run(n, None, ref.refine, trace=True)
        else:
            out[n] = (cases.run(n, ref.estimate, None), None)
    return out


def test_reference_equals_the_fixture(reference):
    z = np.load(GOLDEN)
    names = z["names"].tolist()
    assert names == list(cases.CASES) and GOLDEN.stat().st_size < 64 * 1024
    for i, n in enumerate(names):
        r, tr = reference[n]
        assert cases.digest(r) == z["digests"][i], n
        if tr is not None:
            assert [int(tr[k][0]) for k in ref.TRACE_FIELDS] == z["traces"][i].tolist(), n


def test_the_cases_are_what_their_names_say(reference):
    for n, want in cases.EXPECTED_EXITS.items():
        assert ref.EXITS[int(reference[n][1]["exit"][0])] == want, n
    for it in (0, 1, 2):
        assert int(reference[f"exit_max_iterations{it}"][1]["iterations"][0]) == it
    assert not reference["exit_invalid_steps"][0]["success"][0] and int(reference["exit_invalid_steps"][1]["invalid"][0]) == 5
    # fewer residuals than columns: the solve runs on its damping and succeeds; the rank rule fails the query
    for k in (3, 7):
        assert reference[f"few{k}"][0]["success"][0] and int(reference[f"few{k}"][1]["accepted"][0]) > 0
        assert not reference[f"few{k}_cov"][0]["success"][0] and int(reference[f"few{k}_cov"][1]["rank_failed"][0]) == 1
        assert np.array_equal(reference[f"few{k}"][0]["qvec"], reference[f"few{k}_cov"][0]["qvec"])
    # NaN / inf: the query fails with its camera as given, its neighbour is what it is alone
    for n in ("nan_pixel", "inf_point", "nan_pose", "inf_param", "nan_focal"):
        r, tr = reference[n]
        assert r["success"].tolist() == [False, True] and ref.EXITS[int(tr["exit"][0])] == "NOT_FINITE_START", n
        sc = cases.CASES[n][1]
        assert np.array_equal(r["camera_params"][0, :5], sc["camera_params"][0], equal_nan=True)
        assert np.array_equal(r["camera_params"][1], reference["nan_pixel"][0]["camera_params"][1])
    # a far focal length and a distortion from zero both arrive at the truth
    for n in ("focal_half", "focal_double"):
        r, sc = reference[n][0], cases.CASES[n][1]
        assert r["success"][0] and abs(r["camera_params"][0, 0] / sc["true_params"][0][0] - 1.0) < 1e-6, n
    r, sc = reference["distortion_zero"][0], cases.CASES["distortion_zero"][1]
    assert np.array_equal(reference["distortion_truth"][0]["success"], [True]) and r["success"][0]
    assert np.abs(r["camera_params"][0, 4:8] - sc["true_params"][0][4:8]).max() < 5e-3  # (0.3 px of noise on 150 points)
    # flags that name no parameter leave the camera as it was: SIMPLE_PINHOLE and PINHOLE have no extra parameters
    for m in (0, 1):
        a, b = reference[f"model{m}_f0e0"][0], reference[f"model{m}_f0e1"][0]
        assert cases.same(a, b) == []
    # estimation
    r = reference["estimate_all_factors_fail"][0]
    assert not r["success"].any() and (r["focal_factor"] == 0).all() and not r["inlier_mask"].any()
    r = reference["estimate_empty_and_two_points"][0]
    assert r["success"].tolist() == [True, False, False, True]
    r, f = reference["estimate_focal_model0"][0], reference["estimate_focal_fixed_camera"][0]
    sc = cases.CASES["estimate_focal_model0"][1]
    assert r["success"][0] and f["success"][0] and r["focal_factor"][0] == f["focal_factor"][0] != 1.0
    assert f["camera_params"][0, 0] == sc["camera_params"][0][0] * f["focal_factor"][0]  # scaled, not refined
    assert abs(r["camera_params"][0, 0] / sc["true_params"][0][0] - 1.0) < 0.01 < abs(f["camera_params"][0, 0] / sc["true_params"][0][0] - 1.0)


@pytest.mark.parametrize("name", sorted(n for n in abspose_cases.EDGE_CASES if abspose_cases.EDGE_CASES[n][0] == "refine"))
def test_constant_camera_equals_section_12_bit_for_bit(name):
    """nv = 0: pose, success, covariance and trace of the K-column solver are those of the six-column one."""
    _, sc, _, rf, cov = abspose_cases.EDGE_CASES[name]
    args = (sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"], sc["points3D"], sc["start_q"],
            sc["start_t"], sc["mask"], rf, cov)
    old, told = abspose_ref_lib.refine(*args, trace=True)
    new, tnew = ref.refine(*args, trace=True)
    assert cases.same(new, old, abspose_cases.FIELDS) == []
    for k in ref.TRACE_FIELDS:
        assert np.array_equal(told[k], tnew[k]), k


@pytest.mark.parametrize("model", range(11))
def test_constant_camera_equals_section_12_for_every_model_and_mask(model):
    sc = abspose_cases.scene(1300 + model, 1, 130, outlier_frac=0.1, noise_px=1.0, model=model)
    for count in (1, 5, 6, 63, 64, 65, 129, 130):
        s = abspose_cases.start(sc, model, count=count)
        args = (s["offsets"], s["camera_models"], s["camera_params"], s["points2D"], s["points3D"], s["start_q"], s["start_t"],
                s["mask"])
        for flags in ({}, dict(refine_extra_params=1) if model < 2 else {}):
            old, told = abspose_ref_lib.refine(*args, {}, True, trace=True)
            new, tnew = ref.refine(*args, flags, True, trace=True)
            assert cases.same(new, old, abspose_cases.FIELDS) == [], (count, flags)
            assert all(np.array_equal(told[k], tnew[k]) for k in ref.TRACE_FIELDS)


# ---- derivatives and the solver against independent restatements, within measured budgets -----------------------------------
def test_derivatives_against_central_differences():
    import absrefine_ref2 as r2
    budget = json.loads(BUDGET.read_text())["derivatives"]
    assert budget["margin"] == 2.0 * budget["measured_max"] and 0 < budget["margin"] < 1e-6
    got = r2.measure_derivatives()
    assert set(got) == set(budget["measured"]) and len(got) == 13  # eleven models, FOV on each of its three branches
    for k, v in got.items():
        print(k, v)
        assert v <= budget["margin"], (k, v)


def test_solver_against_scipy_and_the_truth():
    import absrefine_ref2 as r2
    budget = json.loads(BUDGET.read_text())
    for k in ("cost_excess", "focal_rel", "extra_abs", "pose_abs"):
        assert budget[k]["margin"] == 2.0 * budget[k]["measured_max"] > 0, k
    excess, focal, extra, pose = r2.measure_solver()  # asserts that the reference succeeded and that scipy converged
    for got, k in ((excess, "cost_excess"), (focal, "focal_rel"), (extra, "extra_abs"), (pose, "pose_abs")):
        for name, v in got.items():
            print(k, name, v)
            assert v <= budget[k]["margin"], (k, name, v)


# ---- two answers by hand ---------------------------------------------------------------------------------------------------
def test_one_gauss_newton_step_on_the_focal_column_is_exact():
    """SIMPLE_PINHOLE looking down the axis at points of depth 5, only the focal length wrong: the pixel is
    f X / 5 + c, so the focal column of the Jacobian is u = X / 5, the residual is (f - f*) u, and one Gauss-Newton step
    on that column alone is -sum(u r) / sum(u u) = f* - f whatever the points are."""
    f_true, f = 800.0, 1000.0
    X = np.array([[1.0, 0.5, 5.0], [-2.0, 1.0, 5.0], [0.25, -1.5, 5.0], [1.5, 2.0, 5.0]])
    q, t = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
    num = den = 0.0
    for x in X:
        obs = f_true * x[:2] / 5.0 + np.array([500.0, 400.0])
        xy, J, idx = ref.project(0, [f, 500.0, 400.0], q, t, x, True, True)
        assert idx == [0] and J.shape == (2, 8)
        assert np.array_equal(J[:, 7], x[:2] / 5.0)           # the focal column is the normalised point, exactly
        r = xy - obs
        num += float(J[:, 7] @ r)
        den += float(J[:, 7] @ J[:, 7])
    assert abs(-num / den - (f_true - f)) <= 1e-12 * abs(f_true - f)  # a dozen roundings of 1e-16 each


def test_no_inliers_is_success_with_nothing_changed():
    sc = cases.CASES["mask0of65"][1]
    r, tr = cases.run("mask0of65_cov", None, ref.refine, trace=True)
    assert r["success"][0] and ref.EXITS[int(tr["exit"][0])] == "NOTHING_TO_REFINE" and int(tr["iterations"][0]) == 0
    assert np.array_equal(r["qvec"], sc["start_q"]) and np.array_equal(r["tvec"], sc["start_t"])
    assert np.array_equal(r["camera_params"][0, :8], sc["camera_params"][0]) and not r["covariance"].any()


# ---- the mapper --------------------------------------------------------------------------------------------------------------
def _hand_solver(seen, fail_refinement=False):
    """the literal sequence: the section-12 reference's RANSAC per focal factor, the camera scaled by the chosen factor,
    then the joint refinement from the RANSAC's own pose over its inliers"""
    def solver(d):
        seen.append(d)
        n = len(d["points2D"])
        model, prm = int(d["camera_model"]), np.asarray(d["camera_params"], np.float64).reshape(-1)
        est = {k: (int(v) if isinstance(v, bool) else v) for k, v in d["estimation"].items()}
        first = abspose_ref_lib.estimate([0, n], [model], [prm], d["points2D"], d["points3D"], est, dict(max_num_iterations=0))
        out = dict(success=False, qvec=first["qvec"][0], tvec=first["tvec"][0], num_inliers=int(first["num_inliers"][0]),
                   focal_factor=float(first["focal_factor"][0]), inlier_mask=first["inlier_mask"].astype(np.uint8),
                   camera_params=prm.copy())
        if not first["success"][0] or fail_refinement:
            return out
        scaled = prm.copy()
        scaled[:cases.NUM_FOCAL[model]] *= first["focal_factor"][0]
        flags = {k: int(bool(v)) for k, v in d["refinement"].items()}
        second = ref.refine([0, n], [model], [scaled], d["points2D"], d["points3D"], first["qvec"], first["tvec"],
                            first["inlier_mask"], flags)
        return dict(out, success=bool(second["success"][0]), qvec=second["qvec"][0], tvec=second["tvec"][0],
                    camera_params=second["camera_params"][0])
    return solver


def test_register_next_image_and_refine_against_the_sequence_by_hand():
    import mapper_cases as k
    st = k.mapper_state("direct")  # camera 2 has the model's images, camera 1 none
    by_camera = {}
    for i in sorted(st["candidates"]):
        by_camera.setdefault(st["candidates"][i][0], i)
    changed = {}
    for cam_id, image_id in sorted(by_camera.items()):
        r1, _, _, mp1 = k.mapper(st)
        r2, _, _, mp2 = k.mapper(st)
        before = k.model_snapshot(r1)["cameras"][cam_id]
        seen = []
        ok1 = _pose_intrinsics._register_next_image_and_refine_with(mp1, k.SCENE_OPTIONS, image_id, ref.estimate)
        ok2 = mp2._register_next_image_with(k.SCENE_OPTIONS, image_id, _hand_solver(seen))
        assert ok1 is True and ok2 is True
        assert k.model_snapshot(r1) == k.model_snapshot(r2) and mp1.last_registration() == mp2.last_registration()
        assert mp1.num_reg_trials(image_id) == mp2.num_reg_trials(image_id) == 1 and image_id in r1.images
        last = mp1.last_registration()
        flags = seen[0]["refinement"]
        assert flags == dict(refine_focal_length=last["would_refine_focal_length"], refine_extra_params=last["would_refine_extra_params"])
        changed[cam_id] = k.model_snapshot(r1)["cameras"][cam_id] != before
        assert changed[cam_id] == (flags["refine_focal_length"] or flags["refine_extra_params"])
    assert changed == {1: True, 2: False}  # exactly the camera without a registered image is refined


def test_a_failed_refinement_changes_only_the_trial_count():
    import mapper_cases as k
    st = k.mapper_state("direct")
    r, _, t, mp = k.mapper(st)
    image_id = sorted(i for i, c in st["candidates"].items() if c[0] == 1)[0]
    snap = k.model_snapshot(r)
    assert mp._register_next_image_with(k.SCENE_OPTIONS, image_id, _hand_solver([], fail_refinement=True)) is False
    assert k.model_snapshot(r) == snap and mp.num_reg_trials(image_id) == 1 and image_id in mp.candidates
    assert t.get_modified_points3D() == set() and mp.last_registration()["success"] is False

    def failing(*a):  # the same through the public function's solver
        out = ref.estimate(*a)
        out["success"][:] = False
        return out
    assert _pose_intrinsics._register_next_image_and_refine_with(mp, k.SCENE_OPTIONS, image_id, failing) is False
    assert k.model_snapshot(r) == snap and mp.num_reg_trials(image_id) == 2


def test_a_solver_without_camera_params_behaves_as_before():
    import mapper_cases as k
    st = k.mapper_state("direct")
    r, _, _, mp = k.mapper(st)
    image_id = sorted(i for i, c in st["candidates"].items() if c[0] == 1)[0]
    before = k.model_snapshot(r)["cameras"]
    seen = []

    def solver(d):
        seen.append(sorted(d))
        return k.pose_solver(d)
    assert mp._register_next_image_with(k.SCENE_OPTIONS, image_id, solver) is True
    assert "refinement" in seen[0] and k.model_snapshot(r)["cameras"] == before
    with pytest.raises(ValueError, match="camera_params are not 12 values"):
        r2, _, _, mp2 = k.mapper(st)
        mp2._register_next_image_with(k.SCENE_OPTIONS, image_id, lambda d: dict(k.pose_solver(d), camera_params=np.zeros(3)))


# ---- the host plan ---------------------------------------------------------------------------------------------------------------
def test_host_plan_under_asan(tmp_path):
    """The host half (pycolmap_amd/csrc/absrefine_plan.h: the checks, the batches, the launch classes) in a stand-alone
    program under ASan + UBSan (tests/shim/absrefine_plan_fuzz.cc): 400 seeded calls with their corruptions."""
    from test_ba_cpu import _run_sanitized, _sanitized_program
    r = _run_sanitized(_sanitized_program(tmp_path, "absrefine_plan_fuzz", []))
    assert r.returncode == 0 and r.stdout.startswith("ok 400 "), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    batches, launches = (int(v) for v in r.stdout.split()[2:4])
    assert batches > 1000 and launches > batches
