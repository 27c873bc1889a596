"""The initial pair, the global adjustment and the image filter without a GPU: the surface on both
packages, the header against _capi, the flat input checks, the CPU reference of the two-view triangulation against its frozen
fixture, against an independent numpy restatement and against answers by hand, the normalisation on scenes whose result is
exact, register_initial_image_pair and adjust_global_bundle with callables in the library's place, filter_images, and the host
halves in a stand-alone program under ASan + UBSan."""
import ctypes
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import initpair_cases as k
import mapper_cases as mk
import pycolmap
import pycolmap_amd as pc
from pycolmap_amd import _capi
from pycolmap_amd import _pycolmap as P

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "initpair_ref_v1.npz"
BUDGET = ROOT / "tests" / "ref2" / "initpair_deviation_budget.json"
NEW = ("register_initial_image_pair", "adjust_global_bundle", "filter_images")
NO_POINT = mk.NO_POINT


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_names_on_both_packages_and_the_pinned_absences():
    for name in NEW:
        assert getattr(pycolmap, name) is getattr(pc, name) and name in pycolmap._PUBLIC
        assert "DESIGN.md section 21" in getattr(pc, name).__doc__
        assert "DESIGN.md section 21" in getattr(P, "_" + name + "_with", getattr(pc, name)).__doc__
        assert not hasattr(pc.IncrementalMapper, name)
    assert "register_initial_image_pair" in pycolmap.__doc__ and "DESIGN.md section 21" in pycolmap.__doc__
    for name in ("adjust_local_bundle", "adjust_global_bundle", "find_initial_image_pair", "register_initial_image_pair", "filter_images"):
        assert not hasattr(pc.IncrementalMapper, name)
    for name in ("find_initial_image_pair", "incremental_mapping", "triangulate_points", "adjust_local_bundle"):
        with pytest.raises(AttributeError, match="IncrementalMapper.find_next_images, register_next_image, find_local_bundle") as e:
            getattr(pycolmap, name)
        for pinned in ("outside pycolmap_amd's scope", "undistortion", "bundle adjustment", "track completion and merging", "register_initial_image_pair"):
            assert pinned in str(e.value)
    for name in ("normalize", "transform", "crop", "filter_images", "register_image", "add_observation", "merge_points3D", "write_text", "export_PLY"):
        assert not hasattr(pc.Reconstruction, name)
    for name in ("last_initial_pair", "reg_image_ids", "filtered_images"):
        assert hasattr(pc.IncrementalMapper, name)
    assert pc.IncrementalMapper.last_initial_pair.__doc__ and "DESIGN.md section 21" in pc.IncrementalMapper.reg_image_ids.__doc__


def test_header_symbols_and_structs():
    lib = _capi.load()
    text = (ROOT / "include" / "amc_initpair.h").read_text()
    for name in ("amc_pair_tri_opts_default", "amc_triangulate_pairs", "amc_pair_tri_result_free"):
        assert hasattr(lib, name) and name in _capi.EXPORTED_SYMBOLS and name in text
    assert lib.amc_abi_version() == 5
    o = _capi.PairTriOpts()
    lib.amc_pair_tri_opts_default(ctypes.byref(o))
    assert o.min_tri_angle == _capi.INITPAIR_DEFAULT_MIN_TRI_ANGLE == k.DEFAULT_ANGLE == np.radians(16.0) and o.reserved == 0.0
    assert ctypes.sizeof(_capi.PairTriOpts) == 16 and ctypes.sizeof(_capi.PairTriProblem) == 12 * 8 and ctypes.sizeof(_capi.PairTriResult) == 6 * 8 + 8 + 5 * 8
    for s in (_capi.PairTriOpts, _capi.PairTriProblem, _capi.PairTriResult):
        for field, _ in s._fields_:
            assert field in text, field
    assert "AMC_INITPAIR_MAX_CORRS ((uint64_t)1 << 26)" in text and _capi.INITPAIR_MAX_CORRS == 1 << 26
    assert "initpair.hip" in (ROOT / "pycolmap_amd" / "build.py").read_text()
    source = (ROOT / "pycolmap_amd" / "csrc" / "initpair.hip").read_text()
    assert "atomic" not in source.replace("no atomics", "").replace("No atomics", "")
    assert "AMC_INITPAIR_BATCH_CORRS" in source and "AMC_INITPAIR_BATCH_CORRS" in text and "AMC_INITPAIR_BATCH_CORRS" in (ROOT / "README.md").read_text()
    res = _capi.PairTriResult()  # NULL arguments are refused before a device is looked for
    assert lib.amc_triangulate_pairs(None, None, None, ctypes.byref(res)) == _capi.AMC_E_INVALID
    lib.amc_pair_tri_result_free(ctypes.byref(res))
    lib.amc_pair_tri_result_free(None)


def test_flat_input_is_checked_before_the_library():
    a = list(k.call("random")[0])
    for i, value in ((1, a[1][:-1]), (3, a[3][:-1]), (4, a[4][:-1]), (6, a[6][:-1]), (7, a[7][:-1]), (8, a[8][:-1]), (5, -np.ones((len(a[5]), 2))),
                     (2, -np.ones(len(a[2]))), (1, [np.zeros(13)] * len(a[1])), (6, -np.asarray(a[6], np.int64))):
        bad = list(a)
        bad[i] = value
        with pytest.raises(ValueError, match="triangulate_pairs"):
            _capi.pair_tri_inputs(*bad)
    got = _capi.pair_tri_inputs(*a)
    assert got[1].shape == (3, 12) and got[5].dtype == np.uint32 and got[6].dtype == np.uint64 and got[7].flags.c_contiguous
    assert not np.shares_memory(got[7], a[7])  # copies: the caller's arrays are not touched


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def test_reference_reproduces_the_fixture():
    golden = np.load(GOLDEN)
    assert sorted(golden["cases"].tolist()) == sorted(k.CASES)
    whole = 0
    for name in sorted(k.CASES):
        res = k.reference(name)
        assert k.digest(res) == str(golden[f"{name}/digest"]), name
        if f"{name}/xyz" in golden:
            whole += 1
            assert np.array_equal(res["accepted"], golden[f"{name}/accepted"]) and np.array_equal(k.bits(res["xyz"]), k.bits(golden[f"{name}/xyz"]))
            assert np.array_equal(k.bits(res["tri_angle"]), k.bits(golden[f"{name}/tri_angle"]))
    assert whole == len(k.CASES)
    nan = k.reference("nonfinite")["tri_angle"]
    assert np.isnan(nan).sum() >= 6 and set(k.bits(nan[np.isnan(nan)]).tolist()) == {0x7ff8000000000000}  # the one quiet NaN


def test_the_shapes_the_issue_names_are_in_the_case_list():
    for n in (0, 1, 63, 64, 65, 257):
        assert len(k.call(f"corrs_{n}")[0][7]) == n and len(k.call(f"corrs_{n}")[0][5]) == 1
    for n in (0, 1, 64, 65):
        assert len(k.call(f"pairs_{n}")[0][5]) == n
    for m, model in enumerate(__import__("ba_cases").MODEL_NAMES):
        assert k.call(f"model_{model}")[0][0] == [m]
    a = k.call("mixed_models")[0]
    assert any(a[0][a[2][p[0]]] != a[0][a[2][p[1]]] for p in a[5])  # two different models in one pair
    assert k.call("angle_zero")[1]["min_tri_angle"] == 0.0 and k.call("angle_pi")[1]["min_tri_angle"] == k.PI
    assert k.reference("angle_zero")["accepted"].all() and not k.reference("angle_pi")["accepted"].any()
    a = k.call("nonfinite")[0]
    assert not np.isfinite(a[7]).all() and not np.isfinite(a[8]).all() and not np.isfinite(a[3]).all() and not np.isfinite(a[4]).all()


def test_reference_against_the_numpy_restatement_and_the_budget():
    budget = json.loads(BUDGET.read_text())
    measured = k.measure_deviation()
    total = left_out = 0
    for f in ("xyz", "tri_angle"):
        assert budget[f]["margin"] == 2.0 * budget[f]["measured_max_abs_difference"] > 0
        assert measured[f] <= budget[f]["margin"], (f, measured[f])
    m_angle, m_depth = budget["tri_angle"]["margin"], budget["xyz"]["margin"] * 16.0  # a depth is a sum of products of the point with a pose of norm <= 8
    for name in k.RESTATEMENT_CASES:
        a, kw = k.call(name)
        got, want = k.np_triangulate_pairs(*a, **kw), k.reference(name)
        clear = (np.abs(got["tri_angle"] - kw["min_tri_angle"]) > m_angle) & (np.abs(got["depths"] - np.finfo(float).eps) > m_depth).all(axis=1)
        assert np.array_equal(got["accepted"][clear], want["accepted"][clear]), name
        total += len(clear)
        left_out += int((~clear).sum())
    assert total >= 500 and left_out <= 0.01 * total


def test_answers_by_hand():
    r = k.reference("symmetric")  # centres (-1, 0, 0) and (1, 0, 0), rays through (0, 0, 1): a right angle
    assert r["xyz"].tolist() == [[0.0, 0.0, 1.0]] and r["tri_angle"].tolist() == [np.pi / 2] and r["accepted"].tolist() == [True]
    assert r["depths"].tolist() == [[1.0, 1.0]]
    r = k.reference("depths")  # in front of both, behind camera 1 only, behind camera 2 only, behind both
    assert r["xyz"].tolist() == [[0.0, 0.0, 2.0]] * 4 and r["depths"].tolist() == [[2.0, 2.0], [-2.0, 2.0], [2.0, -2.0], [-2.0, -2.0]]
    assert r["accepted"].tolist() == [True, False, False, False] and len(set(r["tri_angle"].tolist())) == 1
    assert abs(r["tri_angle"][0] - 2 * np.arctan(0.5)) < 1e-15 and r["tri_angle"][0] > k.DEFAULT_ANGLE
    r = k.reference("parallel")  # the point is at infinity: no finite point, no angle, never accepted, not even at 0
    assert not np.isfinite(r["xyz"]).all(axis=1).any() and np.isnan(r["tri_angle"]).all() and not r["accepted"].any()
    a, _ = k.call("parallel")
    assert not k.ref.triangulate_pairs(*a, min_tri_angle=0.0)["accepted"].any()
    r = k.reference("coincident")  # no baseline: the angle is 0 wherever there is a point
    assert not r["accepted"].any() and r["tri_angle"][1:].tolist() == [0.0, 0.0]
    a, _ = k.call("coincident")
    assert k.ref.triangulate_pairs(*a, min_tri_angle=0.0)["accepted"].tolist() == [False, False, True]  # depths nan, 0 and 5


# ---- the normalisation -------------------------------------------------------------------------------------------------------------
QUARTER_X = [np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)]  # a quarter turn about x: a centre on the x axis stays where it is


def _axis_model(centres_x, points, quarter=()):
    """images 1, 2, .. with centres on the x axis (identity rotation, or a quarter turn about x for the ids in `quarter`),
    one point2D each; points {id: xyz} seen by images 1 and 2 ... it takes two images to hold a point"""
    r = pc.Reconstruction()
    r.add_camera(pc.Camera(model="SIMPLE_PINHOLE", width=100, height=100, params=[50.0, 50.0, 50.0], camera_id=1))
    for i, cx in enumerate(centres_x, 1):
        im = pc.Image(name=f"{i}.png", camera_id=1, id=i)
        im.cam_from_world = pc.Rigid3d(pc.Rotation3d(np.array(QUARTER_X if i in quarter else [0.0, 0.0, 0.0, 1.0])), np.array([-cx, 0.0, 0.0]))
        im.points2D = [pc.Point2D([1.0, 2.0]) for _ in points]
        r.add_image(im)
    for n, xyz in enumerate(points):
        r.add_point3D(np.array(xyz), pc.Track([pc.TrackElement(1, n), pc.TrackElement(2, n)]))
    return r


def _poses(r):
    return {i: (np.asarray(im.cam_from_world.rotation.quat).tolist(), np.asarray(im.cam_from_world.translation).tolist()) for i, im in r.images.items()}


def test_normalisation_of_three_centres_is_exact():
    """centres 0, 4 and 20 on the x axis: the whole range counts, extent 20, scale 1/2, centroid 8"""
    pts = [[8.0, 0.0, 0.0], [0.0, 2.0, -6.0], [20.0, -0.5, 1.0]]
    r = _axis_model([0.0, 4.0, 20.0], pts, quarter=(2,))
    applied, scale, centroid = P._normalize_model(r, [3, 1, 2])
    assert applied and scale == 0.5 and list(centroid) == [8.0, 0.0, 0.0]
    want_t = {1: [4.0, 0.0, 0.0], 2: [2.0, 0.0, 0.0], 3: [-6.0, 0.0, 0.0]}  # t' = -(centre - 8) / 2
    for i, (q, t) in _poses(r).items():
        assert t == want_t[i] and q == (QUARTER_X if i == 2 else [0.0, 0.0, 0.0, 1.0])
    assert [np.asarray(p.xyz).tolist() for _, p in sorted(r.points3D.items())] == [[0.0, 0.0, 0.0], [-4.0, 1.0, -3.0], [6.0, -0.25, 0.5]]
    poses, points, s, c = k.ref.normalize(_poses(_axis_model([0.0, 4.0, 20.0], pts, quarter=(2,))), {n + 1: x for n, x in enumerate(pts)}, [3, 1, 2])
    assert s == 0.5 and {i: (list(q), list(t)) for i, (q, t) in poses.items()} == _poses(r)


def test_normalisation_takes_the_percentiles_of_eleven_centres():
    """sorted centres -100, 0, 1, .., 8, 1000: ranks trunc(0.1 * 10) = 1 and trunc(0.9 * 10) = 9 bound 0 .. 8; extent 8, scale 5/4,
    centroid 4"""
    xs = [3.0, 1000.0, 0.0, 8.0, 1.0, -100.0, 5.0, 2.0, 7.0, 4.0, 6.0]
    r = _axis_model(xs, [[4.0, 4.0, 0.0]], quarter=(1, 5))
    applied, scale, centroid = P._normalize_model(r, list(range(11, 0, -1)))
    assert applied and scale == 1.25 and list(centroid) == [4.0, 0.0, 0.0]
    assert {i: t for i, (_, t) in _poses(r).items()} == {i: [-(x - 4.0) * 1.25, 0.0, 0.0] for i, x in enumerate(xs, 1)}
    assert np.asarray(r.points3D[1].xyz).tolist() == [0.0, 5.0, 0.0]
    # another extent and other percentiles: the whole range 1100, extent 11 -> scale 1/100; centroid (sum of xs) / 11 = 936 / 11
    r = _axis_model(xs, [[4.0, 4.0, 0.0]])
    applied, scale, centroid = P._normalize_model(r, list(range(1, 12)), 11.0, 0.0, 1.0)
    assert applied and scale == 0.01 and centroid[0] == sum(sorted(xs)) / 11.0


def test_normalisation_below_two_images_and_without_extent():
    r = _axis_model([3.0, 5.0], [[1.0, 2.0, 3.0]])
    before = mk.model_snapshot(r)
    for ids in ([], [2]):
        assert P._normalize_model(r, ids)[0] is False and mk.model_snapshot(r) == before  # a no-op
    r = _axis_model([3.0, 3.0], [[1.0, 2.0, 3.0]])  # one centre twice: no extent, scale 1, the centroid still moves to the origin
    applied, scale, centroid = P._normalize_model(r, [1, 2])
    assert applied and scale == 1.0 and list(centroid) == [3.0, 0.0, 0.0]
    assert [t for _, t in _poses(r).values()] == [[0.0, 0.0, 0.0]] * 2 and np.asarray(r.points3D[1].xyz).tolist() == [-2.0, 2.0, 3.0]
    for bad in (lambda: P._normalize_model(r, [1, 2], 0.0), lambda: P._normalize_model(r, [1, 2], 10.0, 0.9, 0.1), lambda: P._normalize_model(r, [1, 7])):
        with pytest.raises(ValueError):
            bad()


# ---- register_initial_image_pair ---------------------------------------------------------------------------------------------------
def _fresh(name="direct"):
    st = k.empty_state(name)
    r, g, t, mp = mk.mapper(st)
    return st, r, g, t, mp, k.best_pair(g, st["candidates"])


def _nothing_but(mp, r, t, st, before, trials):
    return (mk.model_snapshot(r) == before and mp.candidates == sorted(st["candidates"]) and mp.num_total_reg_images() == 0 and mp.reg_image_ids == [] and
            t.get_modified_points3D() == set() and {i: mp.num_reg_trials(i) for i in st["candidates"]} == {i: trials.get(i, 0) for i in st["candidates"]})


def test_every_reason_for_false_changes_nothing_but_the_trial_counts():
    st, r, g, t, mp, (id1, id2) = _fresh()
    before = mk.model_snapshot(r)
    o = k.START_OPTIONS  # at least 8 inliers, an angle above 4 degrees, |t_z| below 0.95
    seen = []

    def never(d):
        seen.append(d)
        raise AssertionError("the pair solver runs only after a success")
    reasons = (("too few inliers", dict(num_inliers=7)), ("forward motion", dict(tz=0.95)), ("forward motion", dict(tz=-0.96)),
               ("angle", dict(tri_angle=float(np.radians(4.0)))), ("angle", dict(tri_angle=float("nan"))), ("a failed pose step", dict(pose_ok=False)))
    for n, (why, kw) in enumerate(reasons, 1):
        assert P._register_initial_image_pair_with(mp, o, id1, id2, k.forced_two_view_solver(**kw), never) is False, why
        assert _nothing_but(mp, r, t, st, before, {id1: n, id2: n}), why
        last = mp.last_initial_pair()
        assert last["success"] is False and (last["image_id1"], last["image_id2"]) == (id1, id2) and last["num_points3D"] == 0
        assert last["num_correspondences"] == g.num_correspondences_between_images(id1, id2) and last["config"] == 2
    assert not seen
    # each threshold from its other side succeeds
    ok = k.forced_two_view_solver(num_inliers=8, tz=0.9499, tri_angle=float(np.nextafter(np.radians(4.0), 1.0)))
    assert P._register_initial_image_pair_with(mp, o, id1, id2, ok, k.pair_solver) is True


def test_value_errors_change_nothing():
    st, r, g, t, mp, (id1, id2) = _fresh()
    before = mk.model_snapshot(r)
    solver = k.forced_two_view_solver()
    for a, b in ((id1, id1), (id1, 4242), (4242, id2)):
        with pytest.raises(ValueError, match="IsCandidate"):
            P._register_initial_image_pair_with(mp, k.START_OPTIONS, a, b, solver, k.pair_solver)
    with pytest.raises(ValueError, match="init_min_num_inliers > 0"):
        P._register_initial_image_pair_with(mp, dict(init_min_num_inliers=0), id1, id2, solver, k.pair_solver)
    with pytest.raises(ValueError, match="shape"):
        P._register_initial_image_pair_with(mp, k.START_OPTIONS, id1, id2, lambda *a: dict(pose_ok=True, config=2, inlier_matches=np.zeros((3, 2)), qvec=[0, 0, 1],
                                                                                         tvec=[0, 0, 0], tri_angle=0.5), k.pair_solver)
    assert _nothing_but(mp, r, t, st, before, {}) and mp.last_initial_pair() == {}
    # an image that is in the model already
    assert P._register_initial_image_pair_with(mp, k.START_OPTIONS, id1, id2, solver, k.pair_solver) is True
    snap = mk.model_snapshot(r)
    other = [i for i in mp.candidates][0]
    for a, b in ((id1, other), (other, id2), (id1, id2)):
        with pytest.raises(ValueError, match="IsCandidate"):
            P._register_initial_image_pair_with(mp, k.START_OPTIONS, a, b, solver, k.pair_solver)
    assert mk.model_snapshot(r) == snap and mp.num_reg_trials(other) == 0 and mp.num_total_reg_images() == 2


def test_without_a_gpu_the_public_functions_raise_and_change_nothing():
    if _capi.device_count() > 0:
        pytest.skip("a GPU is visible; this test covers the CPU-only container")
    st, r, g, t, mp, (id1, id2) = _fresh()
    before = mk.model_snapshot(r)
    with pytest.raises(_capi.AmcError):
        pc.register_initial_image_pair(mp, k.START_OPTIONS, id1, id2)
    assert _nothing_but(mp, r, t, st, before, {}) and mp.last_initial_pair() == {}
    st4 = mk.mapper_state("direct", 4)
    r4, _, _, mp4 = mk.mapper(st4)
    before = mk.model_snapshot(r4)
    with pytest.raises(_capi.AmcError):
        pc.adjust_global_bundle(mp4, k.START_OPTIONS, pc.BundleAdjustmentOptions())
    assert mk.model_snapshot(r4) == before


def test_a_successful_pair_goes_into_the_model_as_section_21_says():
    st, r, g, t, mp, (id1, id2) = _fresh()
    q2 = [0.0, np.sin(0.1), 0.0, np.cos(0.1)]
    seen = []

    def two_view(*a):
        seen.append(a)
        return k.forced_two_view_solver(qvec=q2, tx=-2.0, tz=0.25, num_inliers=10)(*a)
    assert P._register_initial_image_pair_with(mp, k.START_OPTIONS, id1, id2, two_view, k.pair_solver) is True
    cam1, pts1, cam2, pts2, matches, options = seen[0]
    corr = g.find_correspondences_between_images(id1, id2)
    assert np.array_equal(matches, corr) and np.array_equal(pts1, st["candidates"][id1][1]) and np.array_equal(pts2, st["candidates"][id2][1])
    assert options.ransac.min_num_trials == 30 and options.ransac.max_error == 4.0 and options.min_num_inliers == 15  # TwoViewGeometryOptions otherwise
    assert cam1.camera_id == st["candidates"][id1][0] and cam2.camera_id == st["candidates"][id2][0]
    # every correspondence of the graph, in its order, through the reference by hand
    cams = st["cameras"]
    c1, c2 = cams[st["candidates"][id1][0]], cams[st["candidates"][id2][0]]
    want = k.ref.triangulate_pairs([c1[0], c2[0]], [c1[3], c2[3]], [0, 1], [[0, 0, 0, 1], q2], [[0, 0, 0], [-2.0, 0.0, 0.25]], [[0, 1]], [0, len(corr)],
                                   st["candidates"][id1][1][corr[:, 0]], st["candidates"][id2][1][corr[:, 1]], min_tri_angle=np.radians(4.0))
    kept = np.flatnonzero(want["accepted"])
    assert 0 < len(kept) and sorted(r.points3D) == list(range(1, len(kept) + 1))
    for pid, n in zip(sorted(r.points3D), kept):
        p = r.points3D[pid]
        assert np.array_equal(k.bits(p.xyz), k.bits(want["xyz"][n])) and [(e.image_id, e.point2D_idx) for e in p.track.elements] == [(id1, corr[n, 0]), (id2, corr[n, 1])]
        assert r.images[id1].points2D[corr[n, 0]].point3D_id == pid and r.images[id2].points2D[corr[n, 1]].point3D_id == pid and p.error == -1.0
    assert sum(p.has_point3D() for i in (id1, id2) for p in r.images[i].points2D) == 2 * len(kept)
    assert list(r.images[id1].cam_from_world.rotation.quat) == [0, 0, 0, 1] and list(r.images[id1].cam_from_world.translation) == [0, 0, 0]
    assert list(r.images[id2].cam_from_world.rotation.quat) == q2 and list(r.images[id2].cam_from_world.translation) == [-2.0, 0.0, 0.25]
    assert t.get_modified_points3D() == set()  # as in COLMAP the points do not enter the modified set
    assert mp.candidates == sorted(set(st["candidates"]) - {id1, id2}) and mp.num_total_reg_images() == 2 and mp.reg_image_ids == [id1, id2]
    assert mp.num_reg_trials(id1) == mp.num_reg_trials(id2) == 1
    assert mp.last_initial_pair() == dict(image_id1=id1, image_id2=id2, success=True, num_correspondences=len(corr), num_inliers=10, tri_angle=0.5,
                                          translation_z=0.25, config=2, num_points3D=len(kept))
    assert pc.last_run_stats()["call"] == "register_initial_image_pair" and pc.last_run_stats()["num_device_calls"] == 0
    # the other order: image 2 first
    st, r, g, t, mp, _ = _fresh()
    assert P._register_initial_image_pair_with(mp, k.START_OPTIONS, id2, id1, two_view, k.pair_solver) is True
    assert mp.reg_image_ids == [id2, id1] and list(r.images[id2].cam_from_world.rotation.quat) == [0, 0, 0, 1]
    assert sorted(map(tuple, seen[1][4])) == sorted(map(tuple, corr[:, ::-1]))  # the graph's order from the other side


def test_the_walk_with_the_oracle_and_the_references_starts_two_scenes():
    started = {}
    for name in mk.scene_names():
        st, r, g, t, mp, (id1, id2) = _fresh(name)
        started[name] = P._register_initial_image_pair_with(mp, k.START_OPTIONS, id1, id2, k.oracle_two_view_solver, k.pair_solver)
        last = mp.last_initial_pair()
        assert last["success"] == started[name] and (last["num_points3D"] > 0) == started[name] and mp.num_total_reg_images() == (2 if started[name] else 0)
    assert started["direct"] and started["transitive_2"]


# ---- adjust_global_bundle ------------------------------------------------------------------------------------------------------------
def _by_hand(r, reg, constant_poses, x_position, ba):
    """the same steps through the public calls, with the reference solver and the reference normalisation"""
    import ba_config_cases as bc
    import ba_config_ref_lib
    r.filter_observations_with_negative_depth()
    config = pc.BundleAdjustmentConfig()
    for i in reg:
        config.add_image(i)
    for i in constant_poses:
        config.set_constant_cam_pose(i)
    if x_position is not None:
        config.set_constant_cam_positions(x_position, [0])
    assert pc.BundleAdjuster(ba, config)._solve_with(r, bc.reference_solver(ba_config_ref_lib)) is True
    poses, points, scale, _ = k.ref.normalize(_poses(r), {p: np.asarray(pt.xyz).tolist() for p, pt in r.points3D.items()}, reg)
    return poses, points, scale


@pytest.mark.parametrize("fix_existing", [False, True])
def test_adjust_global_bundle_equals_the_steps_by_hand(fix_existing):
    import ba_config_cases as bc
    import ba_config_ref_lib
    st = mk.mapper_state("direct", 4)
    ba = pc.BundleAdjustmentOptions(refine_focal_length=False, refine_extra_params=False)
    o = dict(k.START_OPTIONS, fix_existing_images=fix_existing)
    models = []
    for _ in range(2):
        r, g, t, mp = mk.mapper(st)
        new = mp._find_next_images_with(o, mk.vis_solver)[0]
        assert mp._register_next_image_with(o, new, mk.pose_solver) is True
        behind = sorted(r.points3D)[0]  # a point behind its cameras: the negative-depth filter has to take it first
        r.points3D[behind].xyz = np.array([0.0, 0.0, 500.0])
        models.append((r, mp, new, behind))
    (r, mp, new, behind), (r2, mp2, _, _) = models
    existing = sorted(st["images"])
    assert mp.reg_image_ids == existing + [new]
    seen = []
    solver = bc.reference_solver(ba_config_ref_lib)

    def spy(d):
        seen.append({f: np.array(d[f]) for f in ("pose_const", "image_at", "point_const")})
        return solver(d)
    assert P._adjust_global_bundle_with(mp, o, ba, spy) is True
    stats = dict(pc.last_run_stats())
    assert behind not in r.points3D and stats["call"] == "adjust_global_bundle"
    # the config it built, as the flat problem shows it: six constant pose columns for a constant pose, the x column alone for the position
    order = list(r.images)  # image_at: the flat problem's images as positions in the model, which keeps the dict's order
    by_id = {order[int(i)]: row.tolist() for i, row in zip(seen[0]["image_at"].reshape(-1), seen[0]["pose_const"].reshape(-1, 6))}
    assert sorted(by_id) == sorted(existing + [new])
    if fix_existing:
        assert all(by_id[i] == [1] * 6 for i in existing) and by_id[new] == [0] * 6
    else:
        assert by_id[existing[0]] == [1] * 6 and by_id[existing[1]] == [0, 0, 0, 1, 0, 0] and all(by_id[i] == [0] * 6 for i in existing[2:] + [new])
    poses, points, scale = _by_hand(r2, existing + [new], existing if fix_existing else existing[:1], None if fix_existing else existing[1], ba)
    assert scale == stats["normalize_scale"] and 0 < scale != 1.0
    assert {i: (k.bits(q).tolist(), k.bits(t).tolist()) for i, (q, t) in _poses(r).items()} == {i: (k.bits(q).tolist(), k.bits(t).tolist()) for i, (q, t) in poses.items()}
    assert {p: k.bits(pt.xyz).tolist() for p, pt in r.points3D.items()} == {p: k.bits(x).tolist() for p, x in points.items()}


def test_adjust_global_bundle_needs_two_images():
    st, r, g, t, mp, _ = _fresh()
    with pytest.raises(ValueError, match="reg_image_ids.size\\(\\) >= 2"):
        P._adjust_global_bundle_with(mp, k.START_OPTIONS, pc.BundleAdjustmentOptions(), lambda d: None)


# ---- filter_images -----------------------------------------------------------------------------------------------------------------
GOOD, BOGUS = (1, 1000, 800, (800.0, 810.0, 500.0, 400.0), True), (1, 1000, 800, (5.0, 810.0, 500.0, 400.0), True)


def _chain_state(nimg):
    """images 1 .. nimg on a line, three points2D each.  Image nimg - 1 sees no point; image nimg has the bogus camera.  Point j
    (1 .. nimg - 3) is seen by images j and j + 1 at their points2D 0 and 1; one point more is seen by images 1, 2 and nimg, another
    by images 3 and nimg.  Candidate 99 is fresh.  Matches tie point2D 0 of 99, nimg - 1 and nimg to point2D 0 of image 1."""
    blind, bogus = nimg - 1, nimg
    images = {i: [2 if i == bogus else 1, np.array([0.0, 0.0, 0.0, 1.0]), np.array([-0.5 * i, 0.0, 0.0]), np.array([[100.0 + i, 50.0], [200.0, 60.0 + i], [300.0, 70.0]]),
                  np.full(3, NO_POINT, np.uint64)] for i in range(1, nimg + 1)}
    points = {j: (np.array([0.5 * j, 0.1, 8.0]), [(j, 0), (j + 1, 1)]) for j in range(1, nimg - 2)}
    points[nimg - 2] = (np.array([1.0, 1.0, 9.0]), [(1, 2), (2, 2), (bogus, 2)])
    points[nimg - 1] = (np.array([2.0, 1.0, 9.0]), [(3, 2), (bogus, 1)])
    for pid, (_, track) in points.items():
        for i, p in track:
            images[i][4][p] = pid
    sizes = {i: 3 for i in list(images) + [99]}
    matches = [(c, 1, np.array([[0, 0]], np.uint32)) for c in (99, blind, bogus)]
    return dict(cameras={1: GOOD, 2: BOGUS}, images={i: tuple(v) for i, v in images.items()}, points=points,
                candidates={99: (1, np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]))}, graph_images=sizes, matches=matches)


def test_filter_images_does_nothing_below_twenty_images():
    st = _chain_state(19)
    r, g, t, mp = mk.mapper(st)
    before = mk.model_snapshot(r)
    assert pc.filter_images(mp, {}) == 0 and mk.model_snapshot(r) == before and mp.filtered_images == [] and mp.candidates == [99]
    assert mp.reg_image_ids == list(range(1, 20))


def test_filter_images_removes_the_blind_and_the_bogus_image():
    st = _chain_state(20)
    r, g, t, mp = mk.mapper(st)
    points_before = {p: [(e.image_id, e.point2D_idx) for e in pt.track.elements] for p, pt in r.points3D.items()}
    assert pc.filter_images(mp, {}) == 2
    assert sorted(r.images) == list(range(1, 19)) == mp.reg_image_ids and mp.filtered_images == [19, 20] and mp.candidates == [19, 20, 99]
    assert mp.num_total_reg_images() == 20  # COLMAP's counter never goes down
    # the observations of image 20 are gone: the three-element track loses one, the two-element track goes entirely
    assert [(e.image_id, e.point2D_idx) for e in r.points3D[18].track.elements] == [(1, 2), (2, 2)] and 19 not in r.points3D
    assert r.images[3].points2D[2].point3D_id == NO_POINT and r.images[1].points2D[2].point3D_id == 18
    assert {p: v for p, v in points_before.items() if p < 18} == {p: [(e.image_id, e.point2D_idx) for e in pt.track.elements] for p, pt in r.points3D.items() if p < 18}
    # candidates again, none of their points2D carrying a point: they can be added to a fresh mapper as they are
    ranked = mp._find_next_images_with(dict(abs_pose_min_num_inliers=1), mk.vis_solver)
    assert ranked == [99, 19, 20]  # the filtered ones in the second group at zero trials, the fresh one first although its id is the largest
    assert mp.num_reg_trials(19) == mp.num_reg_trials(20) == 0
    assert pc.filter_images(mp, {}) == 0  # eighteen images are left
    with pytest.raises(ValueError, match="init_min_num_inliers > 0"):
        pc.filter_images(mp, dict(init_min_num_inliers=0))
    # without the bogus thresholds only the blind image goes
    r, g, t, mp = mk.mapper(_chain_state(20))
    assert pc.filter_images(mp, dict(min_focal_length_ratio=0.0)) == 1 and mp.filtered_images == [19] and 19 in r.points3D


def test_reg_image_ids_follow_the_model():
    st = mk.mapper_state("direct", 3)
    r, g, t, mp = mk.mapper(st)
    existing = sorted(st["images"])
    assert mp.reg_image_ids == existing
    new = mp._find_next_images_with(k.START_OPTIONS, mk.vis_solver)[0]
    assert mp._register_next_image_with(k.START_OPTIONS, new, mk.pose_solver) is True
    assert mp.reg_image_ids == existing + [new]
    import copy
    twin = copy.deepcopy(mp)
    assert twin.reg_image_ids == existing + [new] and twin.filtered_images == [] and twin.last_initial_pair() == {}
    with pytest.raises(AttributeError):
        mp.reg_image_ids = []


# ---- the host halves under sanitizers ----------------------------------------------------------------------------------------------
def test_host_halves_under_asan(tmp_path):
    """The host halves (csrc/host/initial_pair_host.h) in a stand-alone program under ASan + UBSan (tests/shim/initial_pair_host_fuzz.cc)."""
    import os
    import shutil
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    flags = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined"]
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("sanitizer runtime not installed")
    exe = tmp_path / "initial_pair_host_fuzz"
    b = subprocess.run(flags + [str(ROOT / "tests" / "shim" / "initial_pair_host_fuzz.cc"), str(ROOT / "pycolmap_amd" / "csrc" / "host" / "model_io.cc"),
                                str(ROOT / "pycolmap_amd" / "csrc" / "host" / "reconstruction.cc"), "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[1]) >= 2000
    # the existing shim of the mapper's host halves still compiles against the header this change added to
    b = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", str(ROOT / "tests" / "shim" / "mapper_host_fuzz.cc")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
