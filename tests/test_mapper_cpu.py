"""IncrementalMapper without a GPU: the surface, the header, the reference against an independent
Python / numpy restatement, answers worked out by hand, the host halves with the references in the library's place
against the literal sequential loop, the fixture, and the host halves in a stand-alone program under ASan + UBSan."""
import copy
import ctypes
import json
import pickle
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mapper_cases as k
import mapper_ref_lib as ref
import pycolmap
import pycolmap_amd as pc
from pycolmap_amd import _capi

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "mapper_ref_v1.npz"
BUDGET = ROOT / "tests" / "ref2" / "mapper_deviation_budget.json"
NO_POINT = k.NO_POINT
DEG = np.pi / 180.0


# ---- small worlds by hand ----------------------------------------------------------------------------------------------------
PINHOLE = (0, 640, 480, [500.0, 320.0, 240.0], True)  # SIMPLE_PINHOLE with a focal length prior


def hand_state(images, points, candidates, matches, cameras=None):
    """images {id: (camera, centre, number of points2D)}: identity rotation, points2D at (10 k + id, 7 k); points {id: (xyz,
    track)}; candidates {id: (camera, xy)}; matches [(id1, id2, [(p, q)])]"""
    ims = {}
    for i, (cam, centre, n) in images.items():
        ims[i] = [cam, np.array([0.0, 0.0, 0.0, 1.0]), -np.asarray(centre, np.float64), np.array([[10.0 * p + i, 7.0 * p] for p in range(n)]).reshape(-1, 2),
                  np.full(n, NO_POINT, np.uint64)]
    for pid, (_, track) in points.items():
        for i, p in track:
            ims[i][4][p] = pid
    sizes = {i: len(v[3]) for i, v in ims.items()}
    sizes.update({i: len(np.asarray(c[1]).reshape(-1, 2)) for i, c in candidates.items()})
    return dict(cameras=cameras or {1: PINHOLE}, images={i: tuple(v) for i, v in ims.items()},
                points={p: (np.asarray(x, np.float64), list(t)) for p, (x, t) in points.items()},
                candidates={i: (c[0], np.asarray(c[1], np.float64).reshape(-1, 2)) for i, c in candidates.items()}, graph_images=sizes,
                matches=[(a, b, np.array(m, np.uint32).reshape(-1, 2)) for a, b, m in matches])


def failing_pose(seen=None):
    def solver(d):
        if seen is not None:
            seen.append(d)
        n = len(d["points2D"])
        return dict(success=False, qvec=[0, 0, 0, 1], tvec=[0, 0, 0], num_inliers=0, focal_factor=0.0, inlier_mask=np.zeros(n, np.uint8))
    return solver


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_names_on_both_packages():
    for name in ("IncrementalMapper", "IncrementalMapperOptions", "ImageSelectionMethod"):
        assert getattr(pycolmap, name) is getattr(pc, name) and name in pycolmap._PUBLIC
    assert "IncrementalMapper" in pycolmap.__doc__ and "DESIGN.md section 20" in pycolmap.__doc__
    for name in ("incremental_mapping", "triangulate_points", "find_initial_image_pair"):
        with pytest.raises(AttributeError, match="IncrementalMapper.find_next_images, register_next_image, find_local_bundle"):
            getattr(pycolmap, name)
    for name in ("find_next_images", "register_next_image", "find_local_bundle", "add_candidate", "candidates", "num_reg_trials", "num_total_reg_images",
                 "last_registration"):
        assert hasattr(pc.IncrementalMapper, name), name
        if name != "candidates":
            assert getattr(pc.IncrementalMapper, name).__doc__
    for name in ("adjust_local_bundle", "adjust_global_bundle", "find_initial_image_pair", "register_initial_image_pair", "filter_images"):
        assert not hasattr(pc.IncrementalMapper, name), name
    for name in ("register_image", "filter_images", "add_observation", "transform"):  # R1 stays
        assert not hasattr(pc.Reconstruction, name), name
    assert "DESIGN.md section 20" in pc.IncrementalMapper.find_next_images.__doc__


def test_selection_method_enum():
    M = pc.ImageSelectionMethod
    assert [m.name for m in (M.MAX_VISIBLE_POINTS_NUM, M.MAX_VISIBLE_POINTS_RATIO, M.MIN_UNCERTAINTY)] == list(ref.METHODS)
    assert [int(M(n)) for n in ref.METHODS] == [0, 1, 2] and M("MIN_UNCERTAINTY") == M.MIN_UNCERTAINTY
    with pytest.raises(ValueError, match="Invalid string value nearest for enum ImageSelectionMethod"):
        M("nearest")
    assert pc.IncrementalMapperOptions(image_selection_method="MAX_VISIBLE_POINTS_RATIO").image_selection_method == M.MAX_VISIBLE_POINTS_RATIO


def test_options_defaults_and_protocol():
    O = pc.IncrementalMapperOptions
    o = O()
    want = dict(zip(ref.OPTION_FIELDS, ref.OPTION_DEFAULTS))
    want["image_selection_method"] = pc.ImageSelectionMethod.MIN_UNCERTAINTY
    assert len(ref.OPTION_FIELDS) == 21 and o.todict() == want  # the twenty options and the selection method the reference binds
    for f, v in want.items():
        assert type(getattr(o, f)) is type(v), f
    assert O(dict(max_reg_trials=5)).max_reg_trials == 5 and O(local_ba_num_images=3, init_max_error=2.5).todict() == dict(want, local_ba_num_images=3, init_max_error=2.5)
    o.mergedict(dict(abs_pose_max_error=3.0, fix_existing_images=True))
    assert (o.abs_pose_max_error, o.fix_existing_images) == (3.0, True)
    with pytest.raises(ValueError, match="unknown option 'ba_local_num_images'"):
        O(ba_local_num_images=2)
    s = o.summary()
    assert s.startswith("IncrementalMapperOptions:") and "    abs_pose_max_error = 3.0" in s and "image_selection_method = ImageSelectionMethod.MIN_UNCERTAINTY" in s
    assert "abs_pose_max_error: float = 3.0" in o.summary(True) and repr(o) == s
    for other in (pickle.loads(pickle.dumps(o)), copy.copy(o), copy.deepcopy(o)):
        assert other is not o and other.todict() == o.todict()
    assert "(int, default: 30)" in O.abs_pose_min_num_inliers.__doc__


def test_option_checks():
    st = k.mapper_state("direct")
    _, _, _, mp = k.mapper(st)
    some = sorted(st["candidates"])[0]
    model_image = sorted(st["images"])[0]
    for bad, what in ((dict(abs_pose_min_num_inliers=0), "abs_pose_min_num_inliers > 0"), (dict(abs_pose_max_error=0.0), r"abs_pose_max_error > 0\.0"),
                      (dict(abs_pose_min_inlier_ratio=1.5), r"abs_pose_min_inlier_ratio <= 1\.0"), (dict(local_ba_num_images=1), "local_ba_num_images >= 2"),
                      (dict(local_ba_min_tri_angle=float("nan")), r"local_ba_min_tri_angle >= 0\.0"), (dict(max_reg_trials=0), "max_reg_trials >= 1"),
                      (dict(min_focal_length_ratio=2.0, max_focal_length_ratio=1.0), "max_focal_length_ratio >= min_focal_length_ratio"),
                      (dict(init_min_num_inliers=0), "init_min_num_inliers > 0")):
        for call in (lambda o: mp._find_next_images_with(o, k.vis_solver), lambda o: mp._register_next_image_with(o, some, k.pose_solver),
                     lambda o: mp._find_local_bundle_with(o, model_image, k.angle_solver)):
            with pytest.raises(ValueError, match="Check Failed: " + what):
                call(bad)
    assert mp.num_reg_trials(some) == 0


def test_mapper_object_and_candidates():
    st = k.mapper_state("direct")
    r, g, t, mp = k.mapper(st)
    ids = sorted(st["candidates"])
    assert mp.candidates == ids and mp.num_total_reg_images() == 2 and mp.num_reg_trials(ids[0]) == 0 and mp.last_registration() == {}
    assert mp.triangulator is t and mp.reconstruction is r and mp.correspondence_graph is g
    assert repr(mp) == f"IncrementalMapper(num_reg_images=2, num_candidates={len(ids)}, num_total_reg_images=2)"
    with pytest.raises(TypeError):
        pc.IncrementalMapper(r)

    def image(iid, n, cam=1, carry=None):
        im = pc.Image(name="x", camera_id=cam, id=iid)
        im.points2D = [pc.Point2D([1.0, 2.0]) for _ in range(n)]
        if carry is not None:
            pts = im.points2D
            pts[0].point3D_id = carry
            im.points2D = pts
        return im
    n0 = len(st["candidates"][ids[0]][1])
    model_id = sorted(st["images"])[0]
    for bad, what in ((image(ids[0], n0), "is a candidate already"), (image(model_id, len(st["images"][model_id][3])), "is in the reconstruction"),
                      (image(4242, 3), "Check Failed: ExistsImage"), (pc.Image(name="x", camera_id=1), "has no image_id")):
        with pytest.raises(ValueError, match=what):
            mp.add_candidate(bad)
    # a fresh mapper: a camera the reconstruction lacks, a point count the graph does not give, a point2D that carries a point
    mp2 = pc.IncrementalMapper(t)
    for bad, what in ((image(ids[0], n0, cam=99), "no camera 99"), (image(ids[0], n0 + 1), "the graph gives it"), (image(ids[0], n0, carry=1), "carries a point3D")):
        with pytest.raises(ValueError, match=what):
            mp2.add_candidate(bad)
    assert mp2.candidates == []
    # the candidate is a copy: the caller's image can change afterwards
    im = image(ids[0], n0)
    mp2.add_candidate(im)
    im.points2D = []
    assert mp2.candidates == [ids[0]] and mp2._find_next_images_with(k.SCENE_OPTIONS, k.vis_solver) in ([ids[0]], [])
    with pytest.raises(ValueError, match="IsCandidate"):
        mp2._register_next_image_with({}, ids[1], k.pose_solver)  # no candidate of this mapper
    with pytest.raises(ValueError, match="IsCandidate"):
        mp._register_next_image_with({}, model_id, k.pose_solver)
    with pytest.raises(ValueError, match="has no image 4242"):
        mp._find_local_bundle_with({}, 4242, k.angle_solver)
    assert mp2.num_reg_trials(ids[1]) == 0 and mp.num_reg_trials(model_id) == 0


def test_copy_shares_and_deepcopy_separates():
    st = k.mapper_state("direct")
    r, g, t, mp = k.mapper(st)
    first = mp._find_next_images_with(k.SCENE_OPTIONS, k.vis_solver)[0]
    deep, shallow = copy.deepcopy(mp), copy.copy(mp)
    assert shallow.triangulator is t and deep.triangulator is not t and deep.reconstruction is not r
    assert mp._register_next_image_with(k.SCENE_OPTIONS, first, k.pose_solver)
    assert first in r.images and first not in deep.reconstruction.images and first not in mp.candidates
    assert first in deep.candidates and first in shallow.candidates and deep.num_reg_trials(first) == 0 == shallow.num_reg_trials(first)
    assert deep.num_total_reg_images() == 2 and mp.num_total_reg_images() == 3 and deep.last_registration() == {}
    # the deep copy goes its own way and arrives at the same model
    assert deep._register_next_image_with(k.SCENE_OPTIONS, first, k.pose_solver)
    assert k.model_snapshot(deep.reconstruction) == k.model_snapshot(r) and deep.last_registration() == mp.last_registration()
    # the shallow copy shares the reconstruction, where the image is by now: it is no candidate there any more
    with pytest.raises(ValueError, match="IsCandidate"):
        shallow._register_next_image_with(k.SCENE_OPTIONS, first, k.pose_solver)
    assert first not in shallow._find_next_images_with(k.SCENE_OPTIONS, k.vis_solver)


def test_header_symbols_and_structs():
    lib = _capi.load()
    text = (ROOT / "include" / "amc_mapper.h").read_text()
    for name in ("amc_image_visibility", "amc_visibility_result_free", "amc_pair_angle_opts_default", "amc_shared_point_angles", "amc_pair_angle_result_free"):
        assert hasattr(lib, name) and name in _capi.EXPORTED_SYMBOLS and name in text
    assert lib.amc_abi_version() == 5
    o = _capi.PairAngleOpts()
    lib.amc_pair_angle_opts_default(ctypes.byref(o))
    assert o.percentile == 75.0
    assert ctypes.sizeof(_capi.VisibilityProblem) == 11 * 8 and ctypes.sizeof(_capi.VisibilityResult) == 5 * 8 + 8 + 5 * 8
    assert ctypes.sizeof(_capi.PairAngleOpts) == 8 and ctypes.sizeof(_capi.PairAngleProblem) == 9 * 8 and ctypes.sizeof(_capi.PairAngleResult) == 2 * 8 + 8 + 5 * 8
    for s in (_capi.VisibilityProblem, _capi.VisibilityResult, _capi.PairAngleOpts, _capi.PairAngleProblem, _capi.PairAngleResult):
        for field, _ in s._fields_:
            assert field in text, field
    assert "AMC_MAPPER_MAX_PAIR_POINTS ((uint64_t)1 << 20)" in text and _capi.MAPPER_MAX_PAIR_POINTS == 1 << 20
    assert "AMC_MAPPER_MAX_SCORE 17895696ull" in text and _capi.MAPPER_MAX_SCORE == ref.MAX_SCORE == sum(16 ** l for l in range(1, 7))
    assert "AMC_MAPPER_NO_POINT3D UINT64_MAX" in text and _capi.MAPPER_NO_POINT3D == ref.NO_POINT
    assert "mapper.hip" in (ROOT / "pycolmap_amd" / "build.py").read_text()
    source = (ROOT / "pycolmap_amd" / "csrc" / "mapper.hip").read_text()
    assert "atomic" not in source.replace("no atomics", "").replace("No atomics", "")
    for hook in ("AMC_MAPPER_BATCH_IMAGES", "AMC_MAPPER_BATCH_PAIRS"):
        assert hook in source and hook in (ROOT / "README.md").read_text()


def test_flat_input_is_checked_before_the_library():
    a = list(k.vis_call("sizes"))
    for i, value in ((0, a[0][:-1]), (2, a[2][:-1]), (5, a[5][:-1]), (6, a[6][:-1]), (7, a[7][:-1]), (7, -np.ones(len(a[7])))):
        bad = list(a)
        bad[i] = value
        with pytest.raises(ValueError, match="image_visibility"):
            _capi.visibility_inputs(*bad)
    b = list(k.angle_call("sizes")[0])
    for i, value in ((0, b[0][:-1]), (4, b[4][:-1]), (5, b[5][:-1]), (3, -np.ones((len(b[3]), 2)))):
        bad = list(b)
        bad[i] = value
        with pytest.raises(ValueError, match="shared_point_angles"):
            _capi.pair_angle_inputs(*bad)


def test_without_a_gpu_the_methods_raise_and_change_nothing():
    if _capi.device_count() > 0:
        pytest.skip("a GPU is visible; this test covers the CPU-only container")
    st = k.mapper_state("direct")
    r, _, t, mp = k.mapper(st)
    before = k.model_snapshot(r)
    first = mp._find_next_images_with(k.SCENE_OPTIONS, k.vis_solver)[0]
    for call in (lambda: mp.find_next_images(k.SCENE_OPTIONS), lambda: mp.register_next_image(k.SCENE_OPTIONS, first),
                 lambda: mp.find_local_bundle(k.SCENE_OPTIONS, sorted(st["images"])[0])):
        with pytest.raises(_capi.AmcError):
            call()
    assert k.model_snapshot(r) == before and mp.num_reg_trials(first) == 0 and mp.candidates == sorted(st["candidates"])
    assert t.get_modified_points3D() == set() and mp.last_registration() == {} and mp.num_total_reg_images() == 2


# ---- the reference against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(k.VIS_CASES))
def test_visibility_reference_equals_restatement(name):
    assert k.vis_same(k.vis_reference(name), k.np_visibility(*k.vis_call(name))), name


def test_angle_reference_against_restatement_and_the_budget():
    budget = json.loads(BUDGET.read_text())["angle"]
    worst = k.measure_angle_difference()  # asserts that the NaNs coincide
    assert worst <= budget["measured_max_abs_difference_rad"] and budget["margin_rad"] == 2.0 * budget["measured_max_abs_difference_rad"]
    assert 0 < budget["margin_rad"] < 1e-12  # a few hundred ulps of pi / 2: two summation orders, no more


def test_percentile_rank_and_total_order():
    for n, want in ((1, 0), (2, 1), (3, 2), (4, 2), (5, 3), (6, 4), (7, 5), (63, 47), (64, 47), (65, 48), (257, 192), (1 << 20, 786431)):
        assert k.rank_of(n) == want == int(round(0.75 * (n - 1) + 1e-9)), n  # (n - 1 = 2, 6, 62: the half rounds away from zero)
        v = np.arange(n, dtype=np.float64)[::-1].copy() if n <= 257 else None
        if v is not None:
            assert ref.percentile(v) == float(want)
    nan, inf = float("nan"), float("inf")
    assert ref.percentile([nan, 1.0, -inf, inf, 0.0, -0.0], 0) == -inf and ref.percentile([nan, 1.0, -inf, inf], 75) == inf
    assert np.isnan(ref.percentile([nan, 1.0, inf], 100)) and np.isnan(ref.percentile([nan, nan, 1.0, 2.0], 75))
    assert np.signbit(ref.percentile([0.0, -0.0, 0.0], 0)) and not np.signbit(ref.percentile([0.0, -0.0, 0.0], 50))  # -0 before +0
    assert ref.percentile([3.0, 1.0, 2.0], 50) == 2.0 and ref.percentile([5.0], 75) == 5.0


@pytest.mark.parametrize("name", k.scene_names())
def test_find_next_images_reference_equals_restatement(name):
    for nm in (2, 6):
        st = k.mapper_state(name, nm)
        rs = k.ref_scene(st)
        for method in ref.METHODS:
            o = dict(k.SCENE_OPTIONS, image_selection_method=method)
            assert rs.find_next_images(**o) == k.np_find_next_images(st, **o), (name, nm, method)


def test_find_local_bundle_reference_equals_restatement_outside_the_margin():
    margin = json.loads(BUDGET.read_text())["angle"]["margin_rad"]
    counted = left_out = 0
    for name in k.scene_names():
        st = k.mapper_state(name, 6)
        rs = k.ref_scene(st)
        for iid in st["images"]:
            for angle in (6.0, 20.0, 45.0):
                o = dict(k.SCENE_OPTIONS, local_ba_min_tri_angle=angle, local_ba_num_images=3)
                want, distance = k.np_find_local_bundle(st, iid, **o)
                if distance <= margin:
                    left_out += 1
                    continue
                counted += 1
                assert rs.find_local_bundle(iid, **o) == want, (name, iid, angle)
    assert counted >= 80 and left_out <= 0.1 * (counted + left_out)


# ---- answers by hand ---------------------------------------------------------------------------------------------------------------
def test_pyramid_with_a_point_on_every_levels_cell_edge():
    # 640 pixels across: a finest cell is 10 wide; x = 320, 160, ... 10 sit on the first edge of levels 0 .. 5 and belong to
    # the cell that begins there; 9.999 is still cell 0
    xs = [0.0, 320.0, 160.0, 80.0, 40.0, 20.0, 10.0, 9.999]
    assert [ref.cell(x, 640) for x in xs] == [0, 32, 16, 8, 4, 2, 1, 0]
    assert [ref.cell(x, 640) for x in (639.999, 640.0, 641.0, 1e300, float("inf"))] == [63] * 5
    assert [ref.cell(x, 640) for x in (-0.0, -1.0, -1e300, float("-inf"), float("nan"), 5e-324)] == [0] * 6
    assert [ref.cell(1.0, w) for w in (0, 1, 64, 65)] == [63, 63, 1, 0] and ref.cell(0.0, 0) == 0  # 0 / 0 is NaN: cell 0
    args = k._vis_problem([1], np.array([7], np.uint64), [(640, 480, [[x, 0.0] for x in xs], [[(0, 0)]] * len(xs))])
    # distinct cells per level, finest first: {0,1,2,4,8,16,32}, {0,1,2,4,8,16}, {0,1,2,4,8}, {0,1,2,4}, {0,1,2}, {0,1}
    want = 7 * 4096 + 6 * 1024 + 5 * 256 + 4 * 64 + 3 * 16 + 2 * 4
    for res in (ref.image_visibility(*args), k.np_visibility(*args)):
        assert res["score"].tolist() == [want] == [36408] and res["num_visible_points3D"].tolist() == [8] and res["max_score"] == 17895696
    full = k.vis_reference("every_cell")
    assert full["score"].tolist() == [17895696, 17895696] and k.vis_reference("one_cell")["score"].tolist() == [4096 + 1024 + 256 + 64 + 16 + 4]
    assert k.vis_reference("corr_counts")["num_observations"].tolist() == [4] and k.vis_reference("corr_counts")["num_visible_points3D"].tolist() == [2]


def ranking_world():
    """two model images and the candidates 10 .. 13; the statistics come from the solver of each test"""
    xy = [[1.0, 1.0], [2.0, 2.0]]
    return hand_state({1: (1, [0, 0, 0], 2), 2: (1, [1, 0, 0], 2)}, {1: ([0, 0, 5], [(1, 0), (2, 0)])}, {i: (1, xy) for i in (10, 11, 12, 13)},
                      [(10, 1, [(0, 0)]), (11, 1, [(1, 0)]), (12, 2, [(0, 0)]), (13, 2, [(1, 1)])])


def stats_solver(nobs, nvis, score):
    return lambda d: dict(num_observations=np.array(nobs, np.uint32), num_visible_points3D=np.array(nvis, np.uint32), score=np.array(score, np.uint64))


def test_ranking_under_the_three_methods_with_ties_and_tried_candidates():
    _, _, _, mp = k.mapper(ranking_world())
    solver = stats_solver([10, 5, 16, 2], [5, 5, 8, 2], [100, 100, 50, 999])  # candidates 10, 11, 12, 13
    o = dict(abs_pose_min_num_inliers=3)  # 13 sees 2 points: dropped whatever its score

    def ranked(method, **more):
        return mp._find_next_images_with(dict(o, image_selection_method=method, **more), solver)
    assert ranked("MAX_VISIBLE_POINTS_NUM") == [12, 10, 11]    # 8, then 5 and 5: the smaller id first
    assert ranked("MAX_VISIBLE_POINTS_RATIO") == [11, 10, 12]  # 1.0, then 0.5 and 0.5
    assert ranked("MIN_UNCERTAINTY") == [10, 11, 12]           # 100 and 100, then 50
    assert ranked("MIN_UNCERTAINTY", abs_pose_min_num_inliers=2) == [13, 10, 11, 12] and ranked("MIN_UNCERTAINTY", abs_pose_min_num_inliers=9) == []
    # ranks are floats: 2^24 and 2^24 + 1 are one float, so the smaller id wins although its score is smaller
    big = stats_solver([9] * 4, [9] * 4, [1 << 24, (1 << 24) + 1, (1 << 24) + 2, 3])
    assert mp._find_next_images_with(dict(o, image_selection_method="MIN_UNCERTAINTY"), big) == [12, 10, 11, 13]
    # a candidate that was tried goes behind those that were not, whatever its rank; at max_reg_trials it leaves
    assert not mp._register_next_image_with(dict(abs_pose_min_num_inliers=1), 12, failing_pose())
    assert mp.num_reg_trials(12) == 1 and ranked("MAX_VISIBLE_POINTS_NUM") == [10, 11, 12] and ranked("MAX_VISIBLE_POINTS_NUM", max_reg_trials=1) == [10, 11]
    assert not mp._register_next_image_with(dict(abs_pose_min_num_inliers=1), 10, failing_pose())
    assert ranked("MAX_VISIBLE_POINTS_NUM") == [11, 12, 10] and ranked("MIN_UNCERTAINTY") == [11, 10, 12]
    with pytest.raises(ValueError, match="shape"):
        mp._find_next_images_with(o, stats_solver([1], [1], [1]))


def pairs_world(candidate_camera=1):
    """images 1, 2 (camera 1) and 3 (camera 2, bogus); P1 seen by (1, 0) and (2, 0), P2 by (1, 1) and (3, 0), P3 by (2, 1) and
    (2, 2).  Candidate 9: p0 -> (1, 0), (2, 0): P1 twice, one pair; p1 -> (1, 1), (2, 1): P2 and P3, two pairs; p2 -> (3, 0): P2
    through the bogus camera, visible but no pair; p3 -> (1, 2), which carries nothing; p4 unmatched."""
    cameras = {1: PINHOLE, 2: (0, 640, 480, [5.0, 320.0, 240.0], True), 3: (0, 640, 480, [400.0, 320.0, 240.0], False)}
    xy = [[100.0, 50.0], [200.0, 60.0], [300.0, 70.0], [400.0, 80.0], [500.0, 90.0]]
    return hand_state({1: (1, [0, 0, 0], 3), 2: (1, [1, 0, 0], 3), 3: (2, [2, 0, 0], 1)},
                      {1: ([0.1, 0.2, 5.0], [(1, 0), (2, 0)]), 2: ([0.3, -0.2, 6.0], [(1, 1), (3, 0)]), 3: ([-0.4, 0.1, 7.0], [(2, 1), (2, 2)])},
                      {9: (candidate_camera, xy)}, [(9, 1, [(0, 0), (1, 1), (3, 2)]), (9, 2, [(0, 0), (1, 1)]), (9, 3, [(2, 0)])], cameras)


def test_pairs_two_points_for_one_point2D_duplicates_and_the_bogus_camera():
    st = pairs_world()
    r, _, t, mp = k.mapper(st)
    seen = []
    assert not mp._register_next_image_with(dict(abs_pose_min_num_inliers=3), 9, failing_pose(seen))
    d = seen[0]
    assert d["points2D"].tolist() == [[100.0, 50.0], [200.0, 60.0], [200.0, 60.0]]
    assert d["points3D"].tolist() == [[0.1, 0.2, 5.0], [0.3, -0.2, 6.0], [-0.4, 0.1, 7.0]]
    assert d["camera_model"] == 0 and d["camera_params"].reshape(-1)[:3].tolist() == [500.0, 320.0, 240.0]
    assert d["estimation"] == dict(estimate_focal_length=False, num_focal_length_samples=30, min_focal_length_ratio=0.1, max_focal_length_ratio=10.0,
                                   max_error=12.0, min_inlier_ratio=0.25, confidence=0.99999, dyn_num_trials_multiplier=3.0, min_num_trials=100,
                                   max_num_trials=10000)
    last = mp.last_registration()
    assert (last["num_visible_points3D"], last["num_pairs"], last["success"], last["image_id"]) == (3, 3, False, 9)
    # fewer pairs than wanted: False without a call, and the trial still counts
    assert not mp._register_next_image_with(dict(abs_pose_min_num_inliers=4), 9, failing_pose(seen)) and len(seen) == 1 and mp.num_reg_trials(9) == 2
    # with a looser bogus threshold camera 2 is fine, and (p2, P2) is a fourth pair
    assert not mp._register_next_image_with(dict(abs_pose_min_num_inliers=3, min_focal_length_ratio=0.001), 9, failing_pose(seen))
    assert mp.last_registration()["num_pairs"] == 4 and mp.last_registration()["num_visible_points3D"] == 3  # four pairs from three points2D
    assert len(seen) == 2 and seen[1]["points2D"].tolist()[3] == [300.0, 70.0] and seen[1]["points3D"].tolist()[3] == [0.3, -0.2, 6.0]
    assert 9 not in r.images and mp.candidates == [9] and t.get_modified_points3D() == set() and mp.num_reg_trials(9) == 3
    rs = k.ref_scene(st)
    # finest cells (10, 6), (20, 8), (30, 9): three cells on the four finest levels, (0, 0) and (1, 0) on the 4 x 4 level, one on the 2 x 2
    assert rs.candidate_statistics(9) == (4, 3, 3 * (4096 + 1024 + 256 + 64) + 2 * 16 + 1 * 4)
    assert not rs.register_next_image(9, abs_pose_min_num_inliers=4) and rs.last_registration()["num_pairs"] == 3

    # a success: the inliers without a point join their points, in pair order; p1 takes P2 and leaves P3 alone
    def accept(d):
        return dict(success=True, qvec=[0.0, 0.0, 0.0, 1.0], tvec=[0.5, 0.25, 0.0], num_inliers=3, focal_factor=1.0, inlier_mask=[1, 1, 1])
    assert mp._register_next_image_with(dict(abs_pose_min_num_inliers=3, max_reg_trials=9), 9, accept)
    assert [p.point3D_id for p in r.images[9].points2D] == [1, 2, NO_POINT, NO_POINT, NO_POINT]
    assert r.images[9].cam_from_world.translation.tolist() == [0.5, 0.25, 0.0] and r.images[9].camera_id == 1 and r.images[9].name == "image9.png"
    assert [(e.image_id, e.point2D_idx) for e in r.points3D[1].track.elements] == [(1, 0), (2, 0), (9, 0)]
    assert [(e.image_id, e.point2D_idx) for e in r.points3D[2].track.elements] == [(1, 1), (3, 0), (9, 1)] and r.points3D[3].track.length() == 2
    assert t.get_modified_points3D() == {1, 2} and mp.candidates == [] and mp.num_total_reg_images() == 4 and mp.num_reg_trials(9) == 4
    assert mp.last_registration()["success"] and mp.last_registration()["num_inliers"] == 3
    assert pc.last_run_stats()["call"] == "register_next_image" and pc.last_run_stats()["num_device_calls"] == 0
    # an inlier count below the threshold is a failure although the solver succeeded
    _, _, _, mp2 = k.mapper(st)
    assert not mp2._register_next_image_with(dict(abs_pose_min_num_inliers=3), 9, lambda d: dict(accept(d), num_inliers=2))
    with pytest.raises(ValueError, match="shape"):
        mp2._register_next_image_with(dict(abs_pose_min_num_inliers=3), 9, lambda d: dict(accept(d), inlier_mask=[1, 1]))


@pytest.mark.parametrize("camera, options, want", [
    (1, {}, (False, False, False)),                                       # used by model images and sane: everything fixed
    (3, {}, (True, True, True)),                                          # used by none, no prior: estimate and refine
    (3, dict(abs_pose_refine_focal_length=False), (False, False, True)),
    (3, dict(abs_pose_refine_extra_params=False), (True, True, False)),
    (2, {}, (False, True, True)),                                         # in use but bogus: refine; it has a prior, so no estimate
    (2, dict(min_focal_length_ratio=0.001), (False, False, False)),       # not bogus under these thresholds
])
def test_the_num_reg_images_per_camera_rule(camera, options, want):
    st = pairs_world(candidate_camera=camera)
    r, _, _, mp = k.mapper(st)
    seen = []
    o = dict(abs_pose_min_num_inliers=1, **options)
    assert not mp._register_next_image_with(o, 9, failing_pose(seen))
    last = mp.last_registration()
    assert (last["estimate_focal_length"], last["would_refine_focal_length"], last["would_refine_extra_params"]) == want
    assert seen[0]["estimation"]["estimate_focal_length"] == want[0]
    rs = k.ref_scene(st)
    rs.register_next_image(9, **o)
    ref_last = rs.last_registration()
    assert (ref_last["estimate_focal_length"], ref_last["would_refine_focal_length"], ref_last["would_refine_extra_params"]) == want
    # the estimated focal length reaches the camera only with a registration (J6)
    before = list(r.cameras[camera].params)
    assert not mp._register_next_image_with(o, 9, lambda d: dict(failing_pose()(d), focal_factor=1.5, num_inliers=3))
    assert list(r.cameras[camera].params) == before
    n = len(seen[0]["points2D"])
    assert mp._register_next_image_with(dict(o, max_reg_trials=9), 9, lambda d: dict(success=True, qvec=[0, 0, 0, 1.0], tvec=[0, 0, 0.0], num_inliers=n,
                                                                                      focal_factor=1.5, inlier_mask=np.ones(n, np.uint8)))
    assert list(r.cameras[camera].params) == ([1.5 * before[0]] + before[1:] if want[0] else before)


def bundle_world(rows):
    """image 1 at the origin sees ten points around (0, 0, 10); image i of rows = [(shared, angle in degrees)] sits at
    (10 tan(angle), 0, 0) and sees the first `shared` of them, ids 2, 3, .. in the given order"""
    X = [[0.02 * (p % 3 - 1), 0.02 * (p % 2), 10.0 + 0.01 * p] for p in range(10)]
    images = {1: (1, [0, 0, 0], 10)}
    tracks = {p + 1: [(1, p)] for p in range(10)}
    for n, (shared, angle) in enumerate(rows):
        images[n + 2] = (1, [10.0 * np.tan(angle * DEG), 0, 0], 10)
        for p in range(shared):
            tracks[p + 1].append((n + 2, p))
    return hand_state(images, {pid: (X[pid - 1], tr) for pid, tr in tracks.items()}, {}, [])


def bundles(st, image_id, **o):
    """the bundle by the reference, the restatement and the host half with the reference in the library's place"""
    _, _, _, mp = k.mapper(st)
    want = k.ref_scene(st).find_local_bundle(image_id, **o)
    restated, distance = k.np_find_local_bundle(st, image_id, **o)
    assert distance > 1e-3 * DEG  # hand-built: nowhere near a threshold
    assert want == restated == mp._find_local_bundle_with(o, image_id, k.angle_solver)
    return want


def test_bundle_where_every_threshold_row_selects_one_image():
    # rows of (6, 4, 3, 2.4, 2, 1.5, 1.2, 1) degrees and (6, 6, 5, 4, 3, 2, 1, 1) shared points: image k + 2 passes row k first
    rows = [(10, 7.0), (9, 5.0), (5, 3.5), (4, 2.5), (3, 2.2), (2, 1.7), (1, 1.3), (1, 1.1), (1, 0.1)]
    st = bundle_world(rows)
    assert bundles(st, 1, local_ba_num_images=9) == [2, 3, 4, 5, 6, 7, 8, 9]
    for want in range(1, 8):
        assert bundles(st, 1, local_ba_num_images=want + 1) == list(range(2, 2 + want))
    assert bundles(st, 1, local_ba_num_images=10) == list(range(2, 11)) == bundles(st, 1, local_ba_num_images=50)  # all of them: no angles
    # twice the angle threshold: image 2 passes row 2 (8 degrees) ... and the order follows the rows, not the overlap
    assert bundles(st, 1, local_ba_num_images=4, local_ba_min_tri_angle=10.5)[:1] == [2]
    # an angle that only a late row admits comes behind images with less overlap
    late = bundle_world([(10, 1.1), (9, 7.0), (8, 5.0), (1, 0.1)])
    assert bundles(late, 1, local_ba_num_images=4) == [3, 4, 2]


def test_bundle_that_needs_the_fill_up():
    st = bundle_world([(3, 0.01), (7, 0.02), (7, 0.03), (5, 0.01)])  # no baseline to speak of: no row admits anybody
    assert bundles(st, 1, local_ba_num_images=3) == [3, 4]      # the most overlapping, the smaller id first
    assert bundles(st, 1, local_ba_num_images=4) == [3, 4, 5]
    half = bundle_world([(10, 0.01), (9, 7.0), (8, 0.02), (1, 0.01)])
    assert bundles(half, 1, local_ba_num_images=4) == [3, 2, 4]  # image 3 by its angle, then the fill-up in overlap order
    _, _, _, mp = k.mapper(st)
    assert mp._find_local_bundle_with(dict(local_ba_num_images=3), 1, k.angle_solver) == [3, 4]
    s = pc.last_run_stats()
    assert s["call"] == "find_local_bundle" and s["num_overlapping_images"] == 4 and s["num_pairs"] == 4 and s["num_device_calls"] == 0


def test_bundle_counts_a_point_seen_twice_twice():
    # image 2 sees P1 (far away: about 1 degree between the two rays) through three points2D and P2 (next to the baseline:
    # about 37 degrees) through one; image 3 sees P1, P2 and P3 once each
    X = {1: [0.0, 0.0, 10.0], 2: [0.1, 0.0, 0.3], 3: [0.0, 0.5, 10.0]}
    images = {1: (1, [0, 0, 0], 3), 2: (1, [0.2, 0, 0], 4), 3: (1, [4.0, 0, 0], 3), 4: (1, [0.0, 0.1, 0], 1)}
    points = {1: (X[1], [(1, 0), (2, 0), (2, 1), (2, 2), (3, 0), (4, 0)]), 2: (X[2], [(1, 1), (2, 3), (3, 1)]), 3: (X[3], [(1, 2), (3, 2)])}
    st = hand_state(images, points, {}, [])
    rs = k.ref_scene(st)
    bundle, overlap = rs.find_local_bundle(1, overlap=True, local_ba_num_images=2, local_ba_min_tri_angle=6.0)
    assert [(i, n) for i, n, _ in overlap] == [(2, 4), (3, 3), (4, 1)]  # image 2's four observations count four times
    c = {i: -np.asarray(st["images"][i][2]) for i in st["images"]}
    a21, a22 = k.np_angles(c[1], c[2], [X[1], X[2]])
    # the multiset [a21, a21, a21, a22] has rank round(2.25) = 2: a21, about 1.1 degrees; without the repeats [a21, a22] would give a22
    assert abs(overlap[0][2] - a21) < 1e-12 and a21 < 2 * DEG < 6 * DEG < a22 and k.rank_of(4) == 2 and k.rank_of(2) == 1
    assert bundle == [3] == bundles(st, 1, local_ba_num_images=2, local_ba_min_tri_angle=6.0)  # image 2 fails the first rows, image 3 passes
    assert bundles(st, 1, local_ba_num_images=2, local_ba_min_tri_angle=1.0) == [2]


# ---- the host halves against the sequential loop, and the fixture -----------------------------------------------------------------------
@pytest.mark.parametrize("name", k.scene_names())
def test_host_halves_equal_the_sequential_reference_on_the_scenes(name):
    golden = np.load(GOLDEN)
    st = k.mapper_state(name)
    rs = k.ref_scene(st)
    r, _, t, mp = k.mapper(st)
    o = k.SCENE_OPTIONS
    log = []
    while True:
        ranked = mp._find_next_images_with(o, k.vis_solver)
        assert ranked == rs.find_next_images(**o) and pc.last_run_stats()["call"] == "find_next_images"
        if not ranked:
            break
        ok = mp._register_next_image_with(o, ranked[0], k.pose_solver)
        assert ok == rs.register_next_image(ranked[0], **o)
        last, want = mp.last_registration(), rs.last_registration()
        assert {f: last[f] for f in ref.LAST_FIELDS} == want and last["image_id"] == ranked[0]
        bundle = None
        if ok:
            bundle = mp._find_local_bundle_with(o, ranked[0], k.angle_solver)
            assert bundle == rs.find_local_bundle(ranked[0], **o) and ranked[0] not in bundle and set(bundle) <= set(r.images)
        log.append((ranked, ranked[0], ok, bundle))
        assert k.model_snapshot(r) == k.ref_snapshot(rs, st)
        assert t.get_modified_points3D() == rs.modified() and mp.candidates == rs.candidates() and mp.num_total_reg_images() == rs.num_total_reg_images()
        assert all(mp.num_reg_trials(i) == rs.num_reg_trials(i) for i in st["candidates"])
    trials = {i: mp.num_reg_trials(i) for i in sorted(st["candidates"])}
    assert k.loop_digest(log, trials, k.model_snapshot(r)) == str(golden[f"scene/{name}/digest"])
    steps, registered = golden[f"scene/{name}/steps"].tolist()
    assert (len(log), sum(1 for e in log if e[2])) == (steps, registered) and (registered >= 1 or name == "two_view_off")  # (too few points there)
    assert max(trials.values()) <= 3 and (steps == registered or max(trials.values()) == 3)  # a failure is tried max_reg_trials times


def test_focal_length_estimation_without_a_prior_equals_the_reference():
    st = k.mapper_state("all_models", has_prior_focal_length=False)
    rs = k.ref_scene(st)
    r, _, _, mp = k.mapper(st)
    o = k.SCENE_OPTIONS
    first = rs.find_next_images(**o)[0]
    assert mp._register_next_image_with(o, first, k.pose_solver) == rs.register_next_image(first, **o)
    last = mp.last_registration()
    assert last["estimate_focal_length"] and {f: last[f] for f in ref.LAST_FIELDS} == rs.last_registration()
    assert k.model_snapshot(r) == k.ref_snapshot(rs, st)


def test_reference_reproduces_the_fixture():
    golden = np.load(GOLDEN)
    assert golden["vis_cases"].tolist() == sorted(k.VIS_CASES) and golden["angle_cases"].tolist() == sorted(k.ANGLE_CASES)
    assert golden["scenes"].tolist() == k.scene_names() and len(k.scene_names()) == 5
    for name in sorted(k.VIS_CASES):
        res = k.vis_reference(name)
        assert k.vis_digest(res) == str(golden[f"vis/{name}/digest"]), name
        if f"vis/{name}/score" in golden:
            assert all(np.array_equal(res[f], golden[f"vis/{name}/{f}"]) for f in ("num_observations", "num_visible_points3D", "score"))
    for name in sorted(k.ANGLE_CASES):
        if name == "bound":
            continue  # a million angles: the GPU test compares this one with the fixture's digest and the live reference
        res = k.angle_reference(name)
        assert k.angle_digest(res) == str(golden[f"angle/{name}/digest"]), name
        assert np.array_equal(k.bits(res["angle"]), k.bits(golden[f"angle/{name}/angle"]))
    assert GOLDEN.stat().st_size < 1 << 20


def test_the_shapes_the_issue_names_are_in_the_case_lists():
    a = k.vis_call("sizes")
    assert np.diff(a[4].astype(np.int64)).tolist() == [0, 1, 63, 64, 65, 257]
    assert [len(k.vis_call(f"cands_{n}")[2]) for n in (0, 1, 64, 65)] == [0, 1, 64, 65]
    assert sorted(set(np.diff(k.vis_call("corr_counts")[6].astype(np.int64)).tolist())) == [0, 1, 65]
    b, _ = k.angle_call("sizes")
    assert np.diff(b[4].astype(np.int64)).tolist() == list(k.PAIR_SIZES) == [1, 2, 3, 5, 63, 64, 65, 257]
    assert int(np.diff(k.angle_call("bound")[0][4].astype(np.int64)).max()) == _capi.MAPPER_MAX_PAIR_POINTS
    assert [len(k.angle_call(f"pairs_{n}")[0][3]) for n in (0, 1, 64, 65)] == [0, 1, 64, 65]
    nonfinite = k.angle_reference("nonfinite")["angle"]
    assert np.isnan(nonfinite).any() and (~np.isnan(nonfinite)).any()
    assert k.angle_reference("coincident")["angle"][0] == 0.0


def test_host_halves_under_asan(tmp_path):
    """The host halves (csrc/host/mapper_host.h) in a stand-alone program under ASan + UBSan (tests/shim/mapper_host_fuzz.cc)."""
    import os
    import shutil
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    flags = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined"]
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("sanitizer runtime not installed")
    exe = tmp_path / "mapper_host_fuzz"
    b = subprocess.run(flags + [str(ROOT / "tests" / "shim" / "mapper_host_fuzz.cc"), str(ROOT / "pycolmap_amd" / "csrc" / "host" / "model_io.cc"),
                                str(ROOT / "pycolmap_amd" / "csrc" / "host" / "reconstruction.cc"), "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[1]) >= 1000
