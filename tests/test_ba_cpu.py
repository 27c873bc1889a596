"""Bundle adjustment without a GPU: the C header and the ctypes view, the pycolmap surface
(option classes, Reconstruction, the controller's flat problem), the host code under sanitizers, and the CPU reference
(tests/ba_ref) against central differences of its own residual, a numpy restatement of its summation order, its frozen
fixtures (the cases and the edge cases of tests/ba_cases.py, with a check that the edge cases are of the kinds their names
say), and scipy's least_squares on the same parametrisation."""
import json
from pathlib import Path

import numpy as np
import pytest

import ba_cases
import ba_ref_lib as ref
from pycolmap_amd import _capi

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "ba_ref_v1.npz"
GOLDEN_EDGES = ROOT / "tests" / "golden" / "ba_ref_edges_v1.npz"
BUDGET = ROOT / "tests" / "ref2" / "ba_deviation_budget.json"


# ---- the surface ------------------------------------------------------------------------------------------------------
def test_header_symbols_and_option_defaults():
    new = {"amc_ba_opts_default", "amc_bundle_adjust"}
    assert new <= set(_capi.EXPORTED_SYMBOLS)
    lib = _capi.load()
    assert all(hasattr(lib, n) for n in new) and lib.amc_abi_version() == 5
    assert hasattr(_capi.Context, "bundle_adjust")
    want = dict(loss_function_type=0, max_num_iterations=100, max_linear_solver_iterations=200,
                max_num_consecutive_invalid_steps=10, loss_function_scale=1.0, function_tolerance=0.0,
                gradient_tolerance=0.0, parameter_tolerance=0.0)
    o = _capi.ba_options()
    assert {k: getattr(o, k) for k in want} == want
    c = _capi.BaOpts()
    lib.amc_ba_opts_default(c)
    assert {k: getattr(c, k) for k in want} == want  # the C defaults are the Python ones
    assert [_capi.ba_options(dict(loss_function_type=n)).loss_function_type for n in ("TRIVIAL", "soft_l1", "CAUCHY")] == [0, 1, 2]
    with pytest.raises(ValueError):
        _capi.ba_options(dict(loss_function_type="HUBER"))
    with pytest.raises(ValueError):
        _capi.ba_options(dict(no_such_option=1))
    text = (ROOT / "include" / "amc_ba.h").read_text()
    for field, _ in _capi.BaOpts._fields_ + _capi.BaProblem._fields_ + _capi.BaResult._fields_:
        assert field in text, field


def test_inputs_are_checked_before_the_library_is_called():
    args, _ = ba_cases.case_problem("min2")
    bad = list(args)
    bad[4] = np.zeros((3, 4))  # three rotations for two images
    with pytest.raises(ValueError):
        _capi.ba_inputs(*bad)
    bad = list(args)
    bad[8] = np.asarray(args[8], np.int64) - 5
    with pytest.raises(ValueError):
        _capi.ba_inputs(*bad)
    with pytest.raises(ValueError):  # the reference rejects what the library rejects: a point seen once
        ref.bundle_adjust(*args[:8], args[8][:1], args[9][:1], args[10][:1])


def _sanitized_program(tmp_path, name, sources):
    """Builds tests/shim/<name>.cc (+ sources) with ASan + UBSan.  Whether the sanitizer runtime is installed is probed
    with a trivial program first, so that a failure of the real build is a failure and not a skip."""
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


def test_host_checks_and_orders_under_asan(tmp_path):
    """The host half (pycolmap_amd/csrc/ba_plan.h: the checks of 15.2, the three CSR orders) in a stand-alone program
    under ASan + UBSan (tests/shim/ba_plan_fuzz.cc): 200 seeded problems and nine corruptions of each (indices out of
    range in every index array, an unknown model, values that are not finite, a point seen once, a NULL array) on heap
    arrays of the exact sizes; every corruption is refused without a read through it, every valid plan has 15.2's orders."""
    r = _run_sanitized(_sanitized_program(tmp_path, "ba_plan_fuzz", []))
    assert r.returncode == 0 and r.stdout.startswith("ok 2000"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])


def test_reconstruction_and_flattening_under_asan(tmp_path):
    """The host code behind Reconstruction and bundle_adjustment (model_io.cc, reconstruction.cc, ba_host.h) in a
    stand-alone program under ASan + UBSan (tests/shim/ba_host_fuzz.cc): a model written, read, filtered (a length-2 track
    deleted), flattened and written back; each of its three files truncated at every length and with every word
    damaged; ids out of range in every cross reference."""
    exe = _sanitized_program(tmp_path, "ba_host_fuzz", ["pycolmap_amd/csrc/host/model_io.cc",
                                                        "pycolmap_amd/csrc/host/reconstruction.cc"])
    work = tmp_path / "model"
    work.mkdir()
    r = _run_sanitized(exe, str(work))
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[1]) > 1000


# ---- the pycolmap surface ----------------------------------------------------------------------------
BA_DEFAULTS = dict(loss_function_scale=1.0, refine_focal_length=True, refine_principal_point=False,
                   refine_extra_params=True, refine_extrinsics=True, print_summary=True,
                   min_num_residuals_for_multi_threading=50000)
CERES_DEFAULTS = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0, max_num_iterations=100,
                      max_linear_solver_iterations=200, max_num_consecutive_invalid_steps=10,
                      max_consecutive_nonmonotonic_steps=10, minimizer_progress_to_stdout=False)


def test_option_classes_defaults_and_dataclass_protocol():
    import pycolmap_amd as pc
    o = pc.BundleAdjustmentOptions()
    assert {k: getattr(o, k) for k in BA_DEFAULTS} == BA_DEFAULTS
    assert o.loss_function_type == pc.LossFunctionType.TRIVIAL
    assert {k: getattr(o.solver_options, k) for k in CERES_DEFAULTS} == CERES_DEFAULTS
    assert hasattr(o.solver_options, "num_threads")
    d = o.todict()
    assert d["solver_options"]["max_linear_solver_iterations"] == 200 and d["refine_extra_params"] is True
    assert isinstance(o.todict(recursive=False)["solver_options"], pc.CeresSolverOptions)
    k = pc.BundleAdjustmentOptions(refine_principal_point=True, loss_function_type="CAUCHY",
                                   solver_options=dict(max_num_iterations=7))
    assert k.refine_principal_point and k.loss_function_type == pc.LossFunctionType.CAUCHY
    assert k.solver_options.max_num_iterations == 7 and k.solver_options.max_linear_solver_iterations == 200
    f = pc.BundleAdjustmentOptions({"loss_function_scale": 2.5, "refine_extrinsics": False})
    assert f.loss_function_scale == 2.5 and not f.refine_extrinsics and f.refine_focal_length
    f.mergedict({"loss_function_type": "SOFT_L1", "solver_options": {"function_tolerance": 1e-6}})
    assert f.loss_function_type == pc.LossFunctionType.SOFT_L1 and f.solver_options.function_tolerance == 1e-6
    text = o.summary()
    assert text.startswith("BundleAdjustmentOptions:") and "solver_options: CeresSolverOptions:" in text
    assert "max_linear_solver_iterations = 200" in text and repr(o) == text
    assert "refine_focal_length: bool = True" in o.summary(write_type=True)
    assert pc.CeresSolverOptions(max_num_iterations=3).todict()["max_num_iterations"] == 3
    import copy
    c = copy.deepcopy(k)
    c.solver_options.max_num_iterations = 9
    assert k.solver_options.max_num_iterations == 7


def test_loss_function_type_from_strings():
    import pycolmap_amd as pc
    assert [pc.LossFunctionType(n) for n in ("TRIVIAL", "SOFT_L1", "CAUCHY")] == \
        [pc.LossFunctionType.TRIVIAL, pc.LossFunctionType.SOFT_L1, pc.LossFunctionType.CAUCHY]
    assert [int(v) for v in (pc.LossFunctionType.TRIVIAL, pc.LossFunctionType.SOFT_L1, pc.LossFunctionType.CAUCHY)] == [0, 1, 2]
    with pytest.raises(ValueError):
        pc.LossFunctionType("HUBER")
    o = pc.BundleAdjustmentOptions()
    o.loss_function_type = "CAUCHY"
    assert o.loss_function_type == pc.LossFunctionType.CAUCHY


HAND_MODEL = {
    "cameras.txt": "# Camera list with one line of data per camera:\n"
                   "2 SIMPLE_RADIAL 1000 800 800.5 500 400 0.0625\n1 PINHOLE 640 480 600 601.25 320 240\n",
    "images.txt": "# Image list with two lines of data per image:\n"
                  "5 1 0 0 0 0.5 0.25 6 2 five.png\n10.5 20.25 40 30 40 -1 50.5 60 41\n"
                  "3 0.5 0.5 0.5 0.5 -1.5 0 7.125 1 three.png\n11 21 40 31 41 41\n"
                  "9 1 0 0 0 1 2 3 2 nine.png\n12 22 40\n",
    "points3D.txt": "# 3D point list with one line of data per point:\n"
                    "41 0.5 -0.25 2 10 20 30 0.75 5 2 3 1\n40 1 2 3 255 0 128 1.5 5 0 3 0 9 0\n",
}


def _write_hand_model(folder):
    folder.mkdir()
    for name, text in HAND_MODEL.items():
        (folder / name).write_text(text)
    return folder


def _check_hand_model(r):
    assert (r.num_cameras(), r.num_images(), r.num_reg_images(), r.num_points3D()) == (2, 3, 3, 2)
    assert list(r.cameras) == [2, 1] and list(r.images) == [5, 3, 9] and list(r.points3D) == [41, 40]  # file order
    assert r.reg_image_ids() == [5, 3, 9]
    c = r.cameras[2]
    assert (c.model.name, c.width, c.height, list(c.params)) == ("SIMPLE_RADIAL", 1000, 800, [800.5, 500.0, 400.0, 0.0625])
    assert list(r.cameras[1].params) == [600.0, 601.25, 320.0, 240.0]
    im = r.images[3]
    assert (im.name, im.camera_id, im.image_id) == ("three.png", 1, 3)
    assert list(im.cam_from_world.rotation.quat) == [0.5, 0.5, 0.5, 0.5] and list(im.cam_from_world.translation) == [-1.5, 0.0, 7.125]
    assert list(r.images[5].cam_from_world.rotation.quat) == [0.0, 0.0, 0.0, 1.0]
    p2 = r.images[5].points2D
    assert [(list(p.xy), p.has_point3D()) for p in p2] == [([10.5, 20.25], True), ([30.0, 40.0], False), ([50.5, 60.0], True)]
    assert [p.point3D_id for p in p2][::2] == [40, 41] and r.images[5].num_points3D() == 2
    pt = r.points3D[40]
    assert (list(pt.xyz), list(pt.color), pt.error) == ([1.0, 2.0, 3.0], [255, 0, 128], 1.5)
    assert [(e.image_id, e.point2D_idx) for e in pt.track.elements] == [(5, 0), (3, 0), (9, 0)] and pt.track.length() == 3
    assert [(e.image_id, e.point2D_idx) for e in r.points3D[41].track.elements] == [(5, 2), (3, 1)]
    assert r.compute_num_observations() == 5 and r.compute_mean_track_length() == 2.5
    assert repr(r) == "Reconstruction(num_reg_images=3, num_cameras=2, num_points3D=2, num_observations=5)"
    assert "num_points3D = 2" in r.summary() and "mean_track_length = 2.5" in r.summary()
    assert repr(r.images[9]) == 'Image(image_id=9, camera_id=2, name="nine.png", triangulated=1/1)'


def test_reconstruction_round_trips_through_txt_and_bin(tmp_path):
    import pycolmap_amd as pc
    txt = _write_hand_model(tmp_path / "txt")
    r = pc.Reconstruction()
    r.read_text(str(txt))
    _check_hand_model(r)
    _check_hand_model(pc.Reconstruction(str(txt)))
    out = tmp_path / "bin"
    out.mkdir()
    r.write(str(out))
    assert sorted(p.name for p in out.iterdir()) == ["cameras.bin", "images.bin", "points3D.bin"]
    b = pc.Reconstruction()
    b.read_binary(str(out))
    _check_hand_model(b)
    again = tmp_path / "bin2"
    again.mkdir()
    b.write_binary(str(again))
    for name in ("cameras.bin", "images.bin", "points3D.bin"):
        assert (out / name).read_bytes() == (again / name).read_bytes()
    c = pc.Reconstruction()
    c.read(str(out))
    _check_hand_model(c)
    with pytest.raises(ValueError):
        pc.Reconstruction(str(tmp_path / "nothing_here"))
    (out / "images.bin").write_bytes((out / "images.bin").read_bytes()[:-9])
    with pytest.raises(ValueError):
        pc.Reconstruction(str(out))
    assert repr(pc.Image()) == 'Image(image_id=Invalid, camera_id=Invalid, name="", triangulated=0/0)'  # as before


def test_maps_have_reference_semantics(tmp_path):
    import copy
    import pycolmap_amd as pc
    r = pc.Reconstruction(str(_write_hand_model(tmp_path / "txt")))
    assert r.cameras is r.cameras and r.images[5] is r.images[5] and r.points3D[40] is r.points3D[40]
    r.cameras[1].params = [1.0, 2.0, 3.0, 4.0]
    r.images[3].cam_from_world.translation = [9.0, 8.0, 7.0]
    r.points3D[41].xyz = [4.0, 5.0, 6.0]
    out = tmp_path / "bin"
    out.mkdir()
    r.write(str(out))  # the operations see the edits
    b = pc.Reconstruction(str(out))
    assert list(b.cameras[1].params) == [1.0, 2.0, 3.0, 4.0] and list(b.images[3].cam_from_world.translation) == [9.0, 8.0, 7.0]
    assert list(b.points3D[41].xyz) == [4.0, 5.0, 6.0]
    for c in (copy.copy(r), copy.deepcopy(r)):
        c.cameras[1].params = [0.0, 0.0, 0.0, 0.0]
        assert list(r.cameras[1].params) == [1.0, 2.0, 3.0, 4.0]
    cam = pc.Camera(model="SIMPLE_PINHOLE", width=10, height=10, params=[5.0, 5.0, 5.0], camera_id=4)
    r.add_camera(cam)
    assert r.cameras[4] is cam and r.num_cameras() == 3
    with pytest.raises(ValueError):
        r.add_camera(cam)
    im = pc.Image(name="new.png", camera_id=4, id=12)
    im.points2D = [pc.Point2D([1.0, 2.0]), pc.Point2D([3.0, 4.0], 40)]
    r.add_image(im)
    with pytest.raises(ValueError):  # point 40's track does not name image 12 back
        r.compute_num_observations()
    im.points2D = [pc.Point2D([1.0, 2.0]), pc.Point2D([3.0, 4.0])]
    pid = r.add_point3D([0.0, 0.0, 1.0], pc.Track([pc.TrackElement(12, 0), pc.TrackElement(5, 1)]), [1, 2, 3])
    assert pid == 42 and r.images[12].points2D[0].point3D_id == 42 and r.images[5].points2D[1].point3D_id == 42
    assert list(r.points3D[42].color) == [1, 2, 3] and r.compute_num_observations() == 7
    with pytest.raises(ValueError):
        r.add_point3D([0.0, 0.0, 1.0], pc.Track([pc.TrackElement(12, 0)]))  # that point2D is taken
    with pytest.raises(ValueError):
        r.add_point3D([0.0, 0.0, 1.0], pc.Track([pc.TrackElement(77, 0)]))


def test_filter_observations_with_negative_depth(tmp_path):
    """image 9 is turned to look away: its one observation (of point 40, track length 3) goes and the point stays with
    two; then image 3 as well: point 40 (length 2) and point 41 (length 2) are deleted whole"""
    import pycolmap_amd as pc
    r = pc.Reconstruction(str(_write_hand_model(tmp_path / "txt")))
    assert r.filter_observations_with_negative_depth() == 0 and r.num_points3D() == 2
    points = r.points3D
    r.images[9].cam_from_world.translation = [0.0, 0.0, -50.0]
    assert r.filter_observations_with_negative_depth() == 1
    assert [(e.image_id, e.point2D_idx) for e in r.points3D[40].track.elements] == [(5, 0), (3, 0)]
    assert not r.images[9].points2D[0].has_point3D() and r.compute_num_observations() == 4
    r.images[3].cam_from_world.translation = [0.0, 0.0, -50.0]
    assert r.filter_observations_with_negative_depth() == 2
    assert r.num_points3D() == 0 and r.points3D is points and len(points) == 0
    assert all(not p.has_point3D() for i in (5, 3, 9) for p in r.images[i].points2D)


def test_names_resolve_through_import_pycolmap():
    import pycolmap
    import pycolmap_amd as pc
    for name in ("bundle_adjustment", "BundleAdjustmentOptions", "CeresSolverOptions", "LossFunctionType", "Reconstruction",
                 "Point3D", "Point2D", "Track", "TrackElement"):
        assert getattr(pycolmap, name) is getattr(pc, name), name
    assert "bundle_adjustment" in pycolmap.__doc__
    for name in ("patch_match_stereo", "incremental_mapping", "Sim3d", "triangulate_points"):
        with pytest.raises(AttributeError, match="outside pycolmap_amd's scope.*undistortion.*bundle adjustment"):
            getattr(pycolmap, name)
    for name in ("transform", "crop", "write_text", "export_PLY", "normalize"):
        assert not hasattr(pc.Reconstruction, name), name


def test_fewer_than_two_views_is_an_error_message_and_no_change(tmp_path, capfd):
    import pycolmap_amd as pc
    r = pc.Reconstruction()
    r.add_camera(pc.Camera(model="SIMPLE_PINHOLE", width=10, height=10, params=[5.0, 5.0, 5.0], camera_id=1))
    r.add_image(pc.Image(name="only.png", camera_id=1, id=1))
    assert pc.bundle_adjustment(r) is None
    assert pc.bundle_adjustment(pc.Reconstruction(), pc.BundleAdjustmentOptions()) is None
    err = capfd.readouterr().err
    assert err.count("Need at least two views.") == 2 and err.startswith("E")
    assert list(r.cameras[1].params) == [5.0, 5.0, 5.0] and r.num_images() == 1


def test_flat_problem_follows_the_controller_rules(tmp_path):
    """15.1 on the hand-written model: the first image's pose and the second's x translation constant, the groups of each
    camera model by the refine_* flags, the observations point by point"""
    import pycolmap_amd as pc
    r = pc.Reconstruction(str(_write_hand_model(tmp_path / "txt")))
    p = pc._pycolmap._bundle_adjustment_problem(r)
    assert p["camera_models"].ravel().tolist() == [2, 1] and p["image_cameras"].ravel().tolist() == [0, 1, 0]
    assert p["pose_const"].tolist() == [[1] * 6, [0, 0, 0, 1, 0, 0], [0] * 6]
    assert p["camera_const"].tolist() == [[0, 1, 1, 0] + [1] * 8, [0, 0, 1, 1] + [1] * 8]
    assert p["qvec"].tolist()[1] == [0.5, 0.5, 0.5, 0.5] and p["tvec"].tolist()[0] == [0.5, 0.25, 6.0]
    assert p["xyz"].tolist() == [[0.5, -0.25, 2.0], [1.0, 2.0, 3.0]]
    assert p["obs_point"].ravel().tolist() == [0, 0, 1, 1, 1] and p["obs_image"].ravel().tolist() == [0, 1, 0, 1, 2]
    assert p["obs_xy"].tolist() == [[50.5, 60.0], [31.0, 41.0], [10.5, 20.25], [11.0, 21.0], [12.0, 22.0]]
    q = pc._pycolmap._bundle_adjustment_problem(r, pc.BundleAdjustmentOptions(
        refine_focal_length=False, refine_principal_point=True, refine_extra_params=False, refine_extrinsics=False))
    assert q["pose_const"].all() and q["camera_const"].tolist() == [[1, 0, 0, 1] + [1] * 8, [1, 1, 0, 0] + [1] * 8]


# ---- Jacobians --------------------------------------------------------------------------------------------------------
def _central(f, x):
    num = []
    for i in range(x.size):
        h = 1e-6 * max(1.0, abs(x[i]))
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        num.append((f(xp) - f(xm)) / (xp[i] - xm[i]))
    return np.array(num).T


@pytest.mark.parametrize("model", range(11))
def test_jacobian_blocks_match_central_differences(model):
    """every model, every parameter group (focal, principal point, extra), the pose tangent and the point"""
    rng = np.random.default_rng(100 + model)
    prm = ba_cases.model_params(model)
    worst = 0.0
    for _ in range(4):
        q = ba_cases.quat_plus([0, 0, 0, 1.0], rng.uniform(-0.3, 0.3, 3))
        t = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 5.0])
        X = rng.uniform(-1.0, 1.0, 3)
        xy = np.array([500.0, 400.0]) + rng.uniform(-30, 30, 2)
        _, r, Jp, Jc, Jx = ref.observation(model, prm, q, t, X, xy)
        res = lambda q_, t_, X_, p_: ref.observation(model, p_, q_, t_, X_, xy)[1]  # noqa: E731
        num_p = _central(lambda d: res(ba_cases.quat_plus(q, d[:3]), t + d[3:], X, prm), np.zeros(6))
        num_x = _central(lambda x: res(q, t, x, prm), X)
        num_c = _central(lambda p: res(q, t, X, p), prm)
        assert np.all(Jc[:, prm.size:] == 0.0)
        for J, num in ((Jp, num_p), (Jx, num_x), (Jc[:, :prm.size], num_c)):
            worst = max(worst, np.abs(J - num).max() / max(1.0, np.abs(J).max()))
    # the step and the bound of tests/test_rigpose_cpu.py's central differences
    assert worst < 1e-6, worst


@pytest.mark.parametrize("loss", [1, 2])
def test_loss_corrector_scales_residual_and_jacobian(loss):
    prm = ba_cases.model_params(4)
    q, t, X, xy = ba_cases.quat_plus([0, 0, 0, 1.0], [0.1, -0.2, 0.05]), [0.1, 0.2, 5.0], [0.4, -0.3, 0.7], [560.0, 370.0]
    _, r0, Jp0, Jc0, Jx0 = ref.observation(4, prm, q, t, X, xy)
    cost, r, Jp, Jc, Jx = ref.observation(4, prm, q, t, X, xy, loss, 2.0)
    s, b = float(r0 @ r0), 4.0
    rho, rho1 = (2 * b * (np.sqrt(1 + s / b) - 1), 1 / np.sqrt(1 + s / b)) if loss == 1 else (b * np.log1p(s / b), 1 / (1 + s / b))
    assert cost == pytest.approx(0.5 * rho, rel=1e-14)
    w = np.sqrt(rho1)
    for got, plain in ((r, r0), (Jp, Jp0), (Jc, Jc0), (Jx, Jx0)):
        assert np.allclose(got, w * plain, rtol=1e-14, atol=0)
    assert ref.observation(4, prm, q, t, X, xy, loss, 2.0, jac=False)[0] == cost


# ---- reductions -------------------------------------------------------------------------------------------------------
def _sum64_numpy(v):
    """15.7 restated: 64 chains over the strided entries from 0.0, then the xor butterfly 32 .. 1"""
    p = np.zeros(64)
    for k, x in enumerate(v):
        p[k & 63] = p[k & 63] + x
    m = 32
    while m >= 1:
        p = np.array([p[i] + p[i ^ m] for i in range(64)])
        m >>= 1
    return p[0]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_fixed_order_sum_equals_its_numpy_restatement(n):
    v = np.random.default_rng(n).standard_normal(n) * 10.0 ** np.random.default_rng(n + 1).integers(-8, 8, n)
    assert ref.sum64(v) == _sum64_numpy(v)
    assert ref.sum64(v) == pytest.approx(np.sum(v), rel=1e-9, abs=1e-9 * np.abs(v).max())


def test_block_inverse():
    rng = np.random.default_rng(5)
    for n in (6, 12):
        A = rng.standard_normal((n + 3, n))
        A = A.T @ A + np.eye(n)
        got = ref.spd_inverse(A)
        assert np.abs(got @ A - np.eye(n)).max() <= 100 * np.linalg.cond(A) * np.finfo(np.float64).eps
    assert np.array_equal(ref.spd_inverse(-np.eye(6)), np.eye(6))  # a pivot that is not positive: the identity


# ---- the solver against its fixture -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def solved():
    """the reference on every case, once"""
    return {name: ref.bundle_adjust(*ba_cases.case_problem(name)[0], options=ba_cases.case_problem(name)[1])
            for name in ba_cases.CASES}


def test_fixture_lists_the_cases(golden):
    assert sorted(golden["names"]) == sorted(ba_cases.CASES)
    assert GOLDEN.stat().st_size < 100_000


@pytest.mark.parametrize("name", sorted(ba_cases.CASES))
def test_reference_equals_its_fixture_bit_for_bit(name, golden, solved):
    r = solved[name]
    stats = np.array([ref.TERMINATIONS.index(r[k]) if k == "termination" else r[k] for k in ba_cases.RESULT_STATS])
    assert np.array_equal(stats.view(np.uint64), golden[f"{name}/stats"].view(np.uint64))
    assert np.array_equal(r["qvec"].view(np.uint64), golden[f"{name}/qvec"].view(np.uint64))
    assert np.array_equal(r["tvec"].view(np.uint64), golden[f"{name}/tvec"].view(np.uint64))
    assert ba_cases.digest(r) == str(golden[f"{name}/digest"])


def test_case_list_has_a_rejected_step_a_capped_and_a_converged_pcg(solved):
    assert solved["rejected_step"]["num_unsuccessful_steps"] >= 1 and solved["rejected_step"]["num_successful_steps"] >= 1
    assert solved["pcg_cap"]["num_pcg_stops_cap"] >= 1
    assert ba_cases.CASES["pcg_cap"][2]["max_linear_solver_iterations"] == 3
    assert solved["pcg_cap"]["num_pcg_iterations"] == 3 * solved["pcg_cap"]["num_pcg_stops_cap"]
    assert solved["multi9_mixed"]["num_pcg_stops_residual"] >= 1 and solved["multi9_mixed"]["num_pcg_stops_cap"] == 0


def test_constant_parameters_do_not_move_and_costs_decrease(solved):
    for name, r in solved.items():
        args, _ = ba_cases.case_problem(name)
        cc, pc = np.asarray(args[2]), np.asarray(args[6])
        assert r["final_cost"] < r["initial_cost"], name
        start = _capi.ba_inputs(*args)
        assert np.array_equal(r["camera_params"][cc != 0], start[1][cc != 0]), name
        for i in range(pc.shape[0]):
            if pc[i, :3].all():
                assert np.array_equal(r["qvec"][i], start[4][i]), name
            assert np.array_equal(r["tvec"][i][pc[i, 3:] != 0], start[5][i][pc[i, 3:] != 0]), name
        nvar = int((pc == 0).sum()) + 3 * start[7].shape[0] + sum(
            int((cc[c, :len(p)] == 0).sum()) for c, p in enumerate(args[1]))
        assert r["num_variable_parameters"] == nvar, name


def test_observation_order_changes_nothing_but_the_sums_order():
    """the sort is stable by image: a permutation that keeps each image's observations in their order is bit-neutral"""
    args, options = ba_cases.case_problem("wave65")
    order = np.argsort(np.asarray(args[8]), kind="stable")
    a = ref.bundle_adjust(*args, options=options)
    b = ref.bundle_adjust(*args[:8], args[8][order], args[9][order], args[10][order], options=options)
    assert ba_cases.digest(a) == ba_cases.digest(b)


# ---- the edge cases: shapes and exits that CASES leaves out (15.10) -----------------------------------------------------
@pytest.fixture(scope="module")
def golden_edges():
    return np.load(GOLDEN_EDGES)


@pytest.fixture(scope="module")
def solved_edges():
    """the reference on every edge case, once"""
    return {name: ref.bundle_adjust(*ba_cases.edge_problem(name)[0], options=ba_cases.edge_problem(name)[1])
            for name in ba_cases.EDGE_CASES}


def test_edge_fixture_lists_the_edge_cases(golden_edges):
    assert sorted(golden_edges["names"]) == sorted(ba_cases.EDGE_CASES)
    assert GOLDEN_EDGES.stat().st_size < 20_000


@pytest.mark.parametrize("name", sorted(ba_cases.EDGE_CASES))
def test_reference_equals_its_edge_fixture_bit_for_bit(name, golden_edges, solved_edges):
    r = solved_edges[name]
    stats = np.array([ref.TERMINATIONS.index(r[k]) if k == "termination" else r[k] for k in ba_cases.RESULT_STATS],
                     np.float64)
    assert np.array_equal(stats.view(np.uint64), golden_edges[f"{name}/stats"].view(np.uint64))
    assert ba_cases.digest(r) == str(golden_edges[f"{name}/digest"])


def test_edge_cases_cover_the_exits_and_the_paths(solved_edges):
    """by the reference's own result and the problems' own shapes, so that the list cannot decay"""
    r = solved_edges
    steps = lambda n: r[n]["num_successful_steps"] + r[n]["num_unsuccessful_steps"]  # noqa: E731
    assert r["stop_function_tolerance"]["termination"] == "FUNCTION_TOLERANCE" and steps("stop_function_tolerance") >= 1
    assert r["stop_parameter_tolerance"]["termination"] == "PARAMETER_TOLERANCE"
    assert r["stop_parameter_tolerance"]["num_successful_steps"] >= 1
    assert r["stop_gradient_tolerance"]["termination"] == "GRADIENT_TOLERANCE" and steps("stop_gradient_tolerance") >= 1
    assert r["stop_gradient_at_start"]["termination"] == "GRADIENT_TOLERANCE" and steps("stop_gradient_at_start") == 0
    assert r["stop_gradient_at_start"]["final_cost"] == r["stop_gradient_at_start"]["initial_cost"]
    assert r["stop_gradient_at_start"]["num_pcg_iterations"] == 0
    inf = r["infinite_start"]
    assert inf["termination"] == "INVALID_STEPS" and steps("infinite_start") == 0
    assert inf["initial_cost"] == np.inf and inf["final_cost"] == np.inf  # +inf, not NaN: it compares by value as well
    start = _capi.ba_inputs(*ba_cases.edge_problem("infinite_start")[0])
    for k, i in (("camera_params", 1), ("qvec", 4), ("tvec", 5), ("xyz", 7)):
        assert np.array_equal(inf[k], start[i]), k
    assert r["long_run"]["num_successful_steps"] >= 10 and r["long_run"]["num_unsuccessful_steps"] >= 5
    assert ba_cases.EDGE_CASES["long_run"][1] == dict(max_num_iterations=40)
    # every solve of pcg_breakdown is one iteration; one that ends by neither the residual rule nor the cap is a breakdown
    b = r["pcg_breakdown"]
    assert b["num_pcg_iterations"] == steps("pcg_breakdown") == 80
    assert b["num_pcg_stops_residual"] + b["num_pcg_stops_cap"] < steps("pcg_breakdown")
    v = r["invalid_step_in_loop"]
    assert v["termination"] == "INVALID_STEPS" and v["num_successful_steps"] >= 1 and np.isfinite(v["final_cost"])
    assert steps("invalid_step_in_loop") < ba_cases.EDGE_CASES["invalid_step_in_loop"][1]["max_num_iterations"]
    shape = {n: ba_cases.edge_problem(n)[0] for n in ba_cases.EDGE_CASES}
    nimg, ncam, npts = (lambda n: len(shape[n][3])), (lambda n: len(shape[n][0])), (lambda n: len(shape[n][7]))  # noqa: E731
    assert nimg("many65_per_image") > 64 and ncam("many65_per_image") > 64
    assert nimg("many70_shared") > 64 and ncam("many70_shared") == 1
    for n in ("many260_per_image", "many260_cameras_const"):
        assert nimg(n) > 256 and ncam(n) > 256 and npts(n) < 256
    assert np.asarray(shape["many260_cameras_const"][2]).all() and not np.asarray(shape["many260_per_image"][2]).all()
    # both orders of a narrow and the widest camera, and 3-, 4-, 5- and 12-parameter cameras side by side
    counts = lambda n: [len(p) for p in shape[n][1]]  # noqa: E731
    small, big = counts("mixed_models_small_first"), counts("mixed_models_big_first")
    assert small[0] == 3 and max(small) == 12 and {3, 4, 5, 12} <= set(small) and small.index(12) > 0
    assert big[0] == 12 and min(big) == 3
    assert np.bincount(shape["mixed_models_small_first"][3]).tolist() == [2, 1, 1, 1, 1, 1]
    for n, i in (("empty_image_middle", 3), ("empty_image_last", 4)):
        assert nimg(n) == 5 and i not in set(np.asarray(shape[n][8]).tolist()) and not np.asarray(shape[n][6])[i].any()
    used = set(np.asarray(shape["camera_without_images"][3]).tolist())
    assert used == {0, 2} and ncam("camera_without_images") == 3 and len(set(shape["camera_without_images"][0])) >= 2
    pairs = list(zip(np.asarray(shape["duplicate_observations"][8]).tolist(), np.asarray(shape["duplicate_observations"][9]).tolist()))
    assert len(pairs) - len(set(pairs)) == 5
    assert np.asarray(shape["pose_const_pattern"][6]).tolist() == [[1] * 6, [0, 0, 0, 1, 0, 0], [1, 0, 0, 0, 1, 0], [1, 1, 1, 0, 0, 0]]


def test_edge_cases_coarse_properties(solved_edges):
    for name, r in solved_edges.items():
        if name not in ("infinite_start", "stop_gradient_at_start"):
            assert r["final_cost"] < r["initial_cost"], name
    for name, i in (("empty_image_middle", 3), ("empty_image_last", 4)):
        start = _capi.ba_inputs(*ba_cases.edge_problem(name)[0])
        r = solved_edges[name]
        assert np.array_equal(r["qvec"][i].view(np.uint64), start[4][i].view(np.uint64)), name
        assert np.array_equal(r["tvec"][i].view(np.uint64), start[5][i].view(np.uint64)), name
        assert not np.array_equal(r["tvec"][2], start[5][2])  # an observed image did move
    start = _capi.ba_inputs(*ba_cases.edge_problem("camera_without_images")[0])
    r = solved_edges["camera_without_images"]
    assert np.array_equal(r["camera_params"][1].view(np.uint64), start[1][1].view(np.uint64))
    assert not np.array_equal(r["camera_params"][0], start[1][0]) and not np.array_equal(r["camera_params"][2], start[1][2])
    # pose_const_pattern: constant translation columns are equal and a rotation with all three columns constant is
    # bit-equal.  A single constant rotation column is a zero entry of each step's tangent d in q_new = Plus(q, d), not
    # of the composition of several steps (two rotations about y and z compose to one with an x part), so it is read
    # off one step: Plus is the product (sin|d|/|d| d, cos|d|) * q, hence the vector part of q_new * q^-1 is parallel
    # to d.  Bound: two quaternion products of entries below 1 in magnitude, four terms each, and one division:
    # 16 units of double precision.
    args, _ = ba_cases.edge_problem("pose_const_pattern")
    start = _capi.ba_inputs(*args)
    pc = np.asarray(args[6])
    for r in (solved_edges["pose_const_pattern"], ref.bundle_adjust(*args, options=dict(max_num_iterations=1))):
        for i in range(pc.shape[0]):
            assert np.array_equal(r["tvec"][i][pc[i, 3:] != 0], start[5][i][pc[i, 3:] != 0]), i
            assert not np.array_equal(r["tvec"][i][pc[i, 3:] == 0], start[5][i][pc[i, 3:] == 0]) or pc[i, 3:].all(), i
            if pc[i, :3].all():
                assert np.array_equal(r["qvec"][i].view(np.uint64), start[4][i].view(np.uint64)), i
    assert r["num_successful_steps"] == 1

    def step_tangent(q0, q1):
        """the vector part of q1 * q0^-1, (x, y, z, w) quaternions"""
        inv = np.array([-q0[0], -q0[1], -q0[2], q0[3]]) / (q0 @ q0)
        return np.array([q1[3] * inv[0] + q1[0] * inv[3] + q1[1] * inv[2] - q1[2] * inv[1],
                         q1[3] * inv[1] - q1[0] * inv[2] + q1[1] * inv[3] + q1[2] * inv[0],
                         q1[3] * inv[2] + q1[0] * inv[1] - q1[1] * inv[0] + q1[2] * inv[3]])

    d = step_tangent(start[4][2], r["qvec"][2])  # image 2: rotation column 0 constant, 1 and 2 variable
    assert min(abs(d[1]), abs(d[2])) > 1e-6 and abs(d[0]) <= 16 * np.finfo(np.float64).eps, d
    d = step_tangent(start[4][1], r["qvec"][1])  # image 1, for contrast: all three rotation columns variable
    assert np.abs(d).min() > 1e-6, d


# ---- accuracy against an independent solver ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def budget():
    """Both scipy costs, the reference's cost and the bound per case, written to tests/ref2/ba_deviation_budget.json (the
    file is a record: the tests below assert on the figures computed here, not on the file's contents)."""
    import ba_scipy
    out = {}
    for name, (scene_args, loss) in ba_cases.ACCURACY_CASES.items():
        sc = ba_cases.scene(**scene_args)
        args = ba_cases.problem(sc)
        P = ba_scipy.Problem(*args, loss=loss, loss_scale=2.0)
        c10, _ = P.solve(1e-10)
        c14, _ = P.solve(1e-14)
        r = ref.bundle_adjust(*args, options=dict(loss_function_type=loss, loss_function_scale=2.0, max_num_iterations=100))
        margin = 10.0 * abs(c10 - c14) / c14
        out[name] = dict(scipy_cost_tol_1e_10=c10, scipy_cost_tol_1e_14=c14, reference_cost=r["final_cost"],
                         relative_margin=margin, bound=c14 * (1.0 + margin), termination=r["termination"])
    sc = ba_cases.scene(**ba_cases.NOISE_FREE_CASE)
    args = ba_cases.problem(sc)
    _, (q, t, prm, X) = ba_scipy.Problem(*args).solve(1e-14)
    r = ref.bundle_adjust(*args, options=dict(max_num_iterations=100))

    def errors(q_, t_, prm_, X_):
        return dict(qvec=float(np.abs(np.asarray(q_) - sc["true_qvec"]).max()),
                    tvec=float(np.abs(np.asarray(t_) - sc["true_tvec"]).max()),
                    xyz=float(np.abs(np.asarray(X_) - sc["true_xyz"]).max()),
                    focal=float(abs(prm_[0][0] - sc["true_params"][0][0])))
    out["noise_free"] = dict(scipy_error=errors(q, t, prm, X),
                             reference_error=errors(r["qvec"], r["tvec"], r["camera_params"], r["xyz"]))
    try:
        BUDGET.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    except OSError:
        pass  # a read-only checkout: the figures are asserted on all the same
    return out


@pytest.mark.parametrize("name", sorted(ba_cases.ACCURACY_CASES))
def test_converged_cost_is_not_above_scipys(name, budget):
    """the margin comes from the yardstick alone: ten times the relative difference of scipy's costs at ftol = xtol =
    1e-10 and 1e-14 (two minimisers stop at different points of a flat valley)"""
    b = budget[name]
    assert b["reference_cost"] <= b["bound"], b


def test_noise_free_scene_returns_to_the_truth(budget):
    """the gauge is fully fixed (first pose, the second's x translation): bound = ten times scipy's own error"""
    b = budget["noise_free"]
    for k in ("qvec", "tvec", "xyz", "focal"):
        assert b["reference_error"][k] <= 10.0 * b["scipy_error"][k], (k, b)
