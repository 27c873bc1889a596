"""Track completion and track merging without a GPU: the surface, the header, the option checks, the
host half with the CPU reference in the library's place against the sequential reference applied to the model, the
reference against an independent Python restatement and against answers worked out by hand, the frozen fixture, and the
host half under ASan + UBSan."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ba_cases
import pycolmap
import pycolmap_amd as pc
import tracks_cases as k
import tracks_ref_lib as ref
import triangulator_cases as tc
from pycolmap_amd import _capi
from pycolmap_amd import _pycolmap as P

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "tracks_ref_v1.npz"
NO_POINT = k.NO_POINT
FUNCTIONS = ("complete_tracks", "complete_all_tracks", "merge_tracks", "merge_all_tracks")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def complete_with(t, opts, ids=None):
    return P._complete_tracks_with(t, opts, ids, k.complete_solver)


def merge_with(t, opts, ids=None):
    return P._merge_tracks_with(t, opts, ids, k.merge_solver)


def both_ways(st, op, ids=None, modified=(), **opts):
    """the operation by the sequential reference and by the host half with the flat reference in the library's place:
    they must agree.  Returns (count, points, point2D ids, modified ids, the Reconstruction)."""
    rs = k.ref_scene(st, modified=modified)
    want = rs.complete(ids, **opts) if op == "complete" else rs.merge(ids, **opts)
    r, _, t = k.reconstruction(st)
    for pid in modified:
        t.add_modified_point3D(pid)
    got = (complete_with if op == "complete" else merge_with)(t, opts, ids)
    assert got == want
    assert k.same_points(k.recon_points(r), rs.points())
    assert k.same_point2D_ids(k.recon_point2D_ids(r), rs.point2D_ids())
    assert t.get_modified_points3D() == {p for p in rs.modified() if p in rs.points()}
    return got, rs.points(), rs.point2D_ids(), t.get_modified_points3D(), r


# ---- the surface --------------------------------------------------------------------------------------------------------------
def test_functions_exist_on_both_packages_and_nowhere_else():
    for name in FUNCTIONS:
        assert callable(getattr(pc, name)) and getattr(pycolmap, name) is getattr(pc, name)
        assert name in pycolmap._PUBLIC and not hasattr(pc.IncrementalTriangulator, name)
        assert "DESIGN.md section 18" in getattr(pc, name).__doc__
    for name in ("add_observation", "merge_points3D"):
        assert not hasattr(pc.Reconstruction, name)
    with pytest.raises(AttributeError, match="track completion and merging"):
        pycolmap.complete_image
    assert "complete_tracks" in pycolmap.__doc__


def test_header_symbols_and_structs():
    lib = _capi.load()
    text = (ROOT / "include" / "amc_tracks.h").read_text()
    for name in ("amc_complete_opts_default", "amc_complete_tracks", "amc_complete_result_free", "amc_merge_opts_default",
                 "amc_merge_tracks", "amc_merge_result_free"):
        assert hasattr(lib, name) and name in _capi.EXPORTED_SYMBOLS and name in text
    assert lib.amc_abi_version() == 5
    co, mo = _capi.CompleteOpts(), _capi.MergeOpts()
    lib.amc_complete_opts_default(ctypes.byref(co))
    lib.amc_merge_opts_default(ctypes.byref(mo))
    assert co.complete_max_reproj_error == 4.0 and mo.merge_max_reproj_error == 4.0
    assert ctypes.sizeof(_capi.CompleteProblem) == 12 * 8 and ctypes.sizeof(_capi.CompleteResult) == 5 * 8 + 8 + 5 * 8
    assert ctypes.sizeof(_capi.MergeProblem) == 17 * 8 and ctypes.sizeof(_capi.MergeResult) == 6 * 8 + 5 * 8 + 8 + 5 * 8
    for s in (_capi.CompleteOpts, _capi.CompleteProblem, _capi.CompleteResult, _capi.MergeOpts, _capi.MergeProblem, _capi.MergeResult):
        for field, _ in s._fields_:
            assert field in text, field
    assert "AMC_MERGE_MAX_COMPONENT_OBS 4096" in text


def test_option_checks_and_bad_arguments():
    st = k.world(4, [[0.1, 0.2, 0.3]], {0: [1, 2, 3, 4]}, [([0.1, 0.2, 0.3], [(0, 1), (0, 2)])])
    r, g, t = k.reconstruction(st)
    before = k.recon_points(r)
    for bad, what in ((dict(complete_max_reproj_error=0.0), "complete_max_reproj_error > 0"), (dict(merge_max_reproj_error=-1.0), "merge_max_reproj_error > 0"),
                      (dict(complete_max_transitivity=-1), "complete_max_transitivity >= 0"), (dict(min_angle=float("nan")), "min_angle > 0")):
        for call in (lambda o: complete_with(t, o), lambda o: merge_with(t, o, [1]), lambda o: pc.complete_all_tracks(t, o), lambda o: pc.merge_tracks(t, o, [1])):
            with pytest.raises(ValueError, match=what):
                call(bad)
    with pytest.raises(TypeError):
        pc.complete_tracks(t, {}, 3)  # not an iterable
    with pytest.raises(TypeError, match="non-negative ints"):
        pc.merge_tracks(t, {}, [1, -2])
    with pytest.raises(TypeError):
        pc.merge_tracks(r, {}, [1])  # not a triangulator
    with pytest.raises(ValueError, match="shape"):
        P._complete_tracks_with(t, {}, None, lambda d: dict(cand_pass=[1, 1, 1]))
    assert k.same_points(k.recon_points(r), before) and t.get_modified_points3D() == set()
    # ids are a set: a generator, numpy integers, ids that do not exist, an id twice
    assert complete_with(t, {}, (i for i in [np.uint64(1), 1, 77])) == 2
    assert pc.last_run_stats()["call"] == "complete_tracks" and pc.last_run_stats()["num_device_calls"] == 0
    assert complete_with(t, {}, []) == 0 and merge_with(t, {}, [5, 6]) == 0


def test_without_a_gpu_the_functions_raise_and_leave_the_model():
    if _capi.device_count() > 0:
        pytest.skip("a GPU is visible; this test covers the CPU-only container")
    st, opts = k.scene_state("direct")
    r, _, t = k.reconstruction(st)
    before, ids = k.recon_points(r), k.recon_point2D_ids(r)
    for call in (lambda: pc.complete_all_tracks(t, opts), lambda: pc.complete_tracks(t, opts, [1, 2, 3]),
                 lambda: pc.merge_all_tracks(t, opts), lambda: pc.merge_tracks(t, opts, list(before))):
        with pytest.raises(_capi.AmcError):
            call()
    assert k.same_points(k.recon_points(r), before) and k.same_point2D_ids(k.recon_point2D_ids(r), ids)
    assert t.get_modified_points3D() == set()


# ---- whole scenes ----------------------------------------------------------------------------------------------------------------
def test_reference_reproduces_fixture(golden):
    assert sorted(golden["cases"].tolist()) == sorted(k.ALL_CASES) and sorted(golden["scenes"].tolist()) == sorted(k.SCENES)
    for name in sorted(k.ALL_CASES):
        res = k.reference(name)
        assert k.digest(name, res) == str(golden[f"{name}/digest"]), name
        for key in (k.COMPLETE_KEYS if name.startswith("c/") else k.MERGE_KEYS):
            if f"{name}/{key}" in golden:
                a, b = np.asarray(res[key]), golden[f"{name}/{key}"]
                assert np.array_equal(k.bits(a), k.bits(b)) if a.dtype == np.float64 else np.array_equal(a, b), (name, key)
    # what the flat cases are for: both verdicts, non-finite errors, depth below epsilon, merges and refusals
    r = k.reference("c/nonfinite")
    assert np.isnan(r["cand_sq_error"]).any() and r["cand_pass"][np.isnan(r["cand_sq_error"])].all()  # H2
    assert (r["cand_sq_error"] == k.DBL_MAX).any()
    r = k.reference("c/threshold")
    assert r["cand_sq_error"][0] == 25.0 and r["cand_pass"].tolist() == [True, False, True, False]
    assert k.reference("m/chain_5")["root_return"].tolist() == [18, 0, 0, 0, 0, 0] and k.reference("m/chain_5")["num_merges"] == 5
    assert k.reference("m/far_apart")["num_merges"] == 0 and k.reference("m/obs_4096")["num_merges"] > 0
    assert len(k.case_call("m/obs_4096")[0][10]) == 4096 + 4


@pytest.mark.parametrize("ids", ["all", "subset"])
@pytest.mark.parametrize("op", ["complete", "merge", "both"])
@pytest.mark.parametrize("name", sorted(k.SCENES))
def test_host_half_with_reference_in_the_librarys_place(name, op, ids, golden):
    st, opts = k.scene_state(name)
    counts, points, p2, modified, _ = k.scene_reference(name, op, ids)
    assert k.state_digest(sum(counts), points) == str(golden[f"scene/{name}/{op}/{ids}/digest"])
    assert counts == golden[f"scene/{name}/{op}/{ids}/counts"].tolist() and all(c > 0 for c in counts)
    r, _, t = k.reconstruction(st)
    survivors = dict(r.points3D)
    listed = None if ids == "all" else k.subset_ids(st)
    got = []
    if op in ("complete", "both"):
        got.append(complete_with(t, opts, listed))
        s = pc.last_run_stats()
        assert s["num_completed_observations"] == got[-1] and s["num_candidates_tested"] >= got[-1] and s["num_items"] > 0
        assert s["num_candidates_visited"] >= got[-1]
    if op in ("merge", "both"):
        got.append(merge_with(t, opts, listed))
        s = pc.last_run_stats()
        assert s["num_merges"] > 0 and s["num_components"] > 0 and 4 <= s["largest_component"] <= k.MAX_COMPONENT_OBS
    assert got == counts
    assert k.same_points(k.recon_points(r), points)
    assert k.same_point2D_ids(k.recon_point2D_ids(r), p2)
    assert t.get_modified_points3D() == modified
    # surviving objects stay the same objects; merged points are new ones
    assert all(r.points3D[pid] is obj for pid, obj in survivors.items() if pid in r.points3D)
    assert all(pid in survivors or r.points3D[pid].error == -1.0 for pid in r.points3D)


@pytest.mark.parametrize("name", sorted(k.SCENES))
def test_reference_equals_python_restatement(name):
    st, opts = k.scene_state(name)
    counts, points, p2, modified, margin = k.scene_reference(name, "both", "all")
    assert margin > 1e-9, "17.7's condition: no deciding error within 1e-9 relative of its threshold"
    py = k.PyTracks(st, **opts)
    assert [py.complete(), py.merge()] == counts
    got = py.state_points()
    assert list(got) == list(points)
    for pid in points:
        np.testing.assert_allclose(got[pid][0], points[pid][0], rtol=0, atol=1e-12)
        assert got[pid][1] == points[pid][1] and got[pid][2:] == points[pid][2:], pid
    assert py.modified == modified
    assert k.same_point2D_ids({i: im[4] for i, im in py.images.items()}, p2)
    counts_s, points_s, _, _, margin_s = k.scene_reference(name, "both", "subset")
    assert margin_s > 1e-9
    py = k.PyTracks(st, **opts)
    listed = k.subset_ids(st)
    assert [py.complete(listed), py.merge(listed)] == counts_s and list(py.state_points()) == list(points_s)


# ---- completion by hand ------------------------------------------------------------------------------------------------------------
X0 = [0.1, 0.2, 0.3]


def test_a_planted_observation_left_out_of_a_track_comes_back():
    st = k.world(5, [X0], {0: [1, 2, 3, 4]}, [(X0, [(0, 1), (0, 2), (0, 3)])])
    n, points, p2, modified, r = both_ways(st, "complete")
    k4 = st["index"][(0, 4)]
    assert n == 1 and points[1][3][-1] == (4, k4) and p2[4][k4] == 1 and modified == {1}
    assert np.array_equal(points[1][0], np.array(X0))  # the position never changes
    # the observation is reached from three track elements and tested once
    s = pc.last_run_stats()
    assert (s["num_items"], s["num_candidates_tested"], s["num_candidates_visited"], s["num_completed_observations"]) == (1, 1, 1, 1)
    # ... and when it fails it is visited from each of them, but still one candidate
    st = k.world(5, [X0], {0: [1, 2, 3, 4]}, [(X0, [(0, 1), (0, 2), (0, 3)])], offsets={(0, 4): (30.0, 0.0)})
    assert both_ways(st, "complete")[0] == 0
    s = pc.last_run_stats()
    assert (s["num_candidates_tested"], s["num_candidates_visited"]) == (1, 3)


@pytest.mark.parametrize("transitivity, added", [(0, []), (1, [3]), (2, [3, 4]), (5, [3, 4, 5, 6, 7])])
def test_transitivity_and_the_last_level_accepts_but_does_not_queue(transitivity, added):
    chain = [(i, i + 1) for i in range(1, 8)]  # 1-2-3-..-8
    st = k.world(8, [X0], {0: list(range(1, 9))}, [(X0, [(0, 1), (0, 2)])], edges={0: chain})
    n, points, _, _, _ = both_ways(st, "complete", complete_max_transitivity=transitivity)
    assert n == len(added) and [i for i, _ in points[1][3]] == [1, 2] + added


def test_two_points_compete_for_one_observation_the_lower_id_wins():
    st = k.world(5, [X0], {0: [1, 2, 3, 4, 5]}, [(X0, [(0, 1), (0, 2)]), (X0, [(0, 4), (0, 5)])])
    n, points, p2, modified, _ = both_ways(st, "complete")
    assert n == 1 and [i for i, _ in points[1][3]] == [1, 2, 3] and len(points[2][3]) == 2 and modified == {1}
    n, points, _, modified, _ = both_ways(st, "complete", ids=[2])
    assert n == 1 and [i for i, _ in points[2][3]] == [4, 5, 3] and modified == {2}
    n, points, _, _, _ = both_ways(st, "complete", ids=[2, 1, 2])  # a set, in ascending order: 1 first
    assert n == 1 and len(points[1][3]) == 3


def test_a_later_walk_is_cut_where_an_earlier_point_claimed_the_bridge():
    # point 1: 1 -> 2 -> 4, reaching 4 on its last level; point 2: {5, 6} -> 4 -> 3
    st = k.world(6, [X0], {0: [1, 2, 3, 4, 5, 6]}, [(X0, [(0, 1)]), (X0, [(0, 5), (0, 6)])],
                 edges={0: [(1, 2), (2, 4), (4, 5), (3, 4), (5, 6)]})
    n, points, p2, _, _ = both_ways(st, "complete", complete_max_transitivity=2)
    assert n == 2 and [i for i, _ in points[1][3]] == [1, 2, 4] and [i for i, _ in points[2][3]] == [5, 6]
    assert p2[3][st["index"][(0, 3)]] == NO_POINT  # behind the bridge: nobody reached it
    s = pc.last_run_stats()
    # the closures on the model before the call: {2, 4} for point 1, {4, 2, 3} for point 2, whose walk read nothing
    assert s["num_candidates_tested"] == 5 and s["num_candidates_visited"] == 2
    n, points, _, _, _ = both_ways(st, "complete", ids=[2], complete_max_transitivity=2)
    assert n == 3 and [i for i, _ in points[2][3]] == [5, 6, 4, 2, 3]  # alone it crosses the bridge: 4, then 4's list 2, 3


def test_bogus_camera_nan_pixel_and_images_outside_the_reconstruction():
    st = k.world(5, [X0], {0: [1, 2, 3, 4, 5]}, [(X0, [(0, 1), (0, 2)])], bogus_images=(4,), nan_pixels=((0, 5),))
    n, points, _, _, _ = both_ways(st, "complete")
    assert n == 2 and [i for i, _ in points[1][3]] == [1, 2, 3, 5]  # 4 is bogus; 5's NaN error is not above the bound (H2)
    n, _, _, _, _ = both_ways(st, "complete", max_focal_length_ratio=0.5)  # now every camera is bogus
    assert n == 0
    # an image of the graph that the reconstruction does not hold is passed over
    st = k.world(4, [X0], {0: [1, 2, 3, 4]}, [(X0, [(0, 1), (0, 2)])])
    r, _, t = k.reconstruction(st)
    st3 = dict(st, images={i: im for i, im in st["images"].items() if i != 3})
    r3, _ = tc.reconstruction(st3)
    r3.add_point3D(np.array(X0), pc.Track([pc.TrackElement(i, kk) for i, kk in st["points"][1][3]]), [1, 2, 3])
    g = t.correspondence_graph
    t3 = pc.IncrementalTriangulator(g, r3)
    assert complete_with(t3, {}) == 1 and [e.image_id for e in r3.points3D[1].track.elements] == [1, 2, 4]


def _axis_state(pixels, X):
    """three images with the identity pose; a point at X with a track in images 1 and 2 at the principal point; image 3
    holds `pixels`, each matched to the track's element in image 1"""
    prm = ba_cases.model_params(0)
    c = np.array([prm[1], prm[2]])
    q, t = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
    pix = np.array(pixels, np.float64).reshape(-1, 2)
    n = len(pix)
    images = {1: (1, q, t, np.tile(c, (n, 1)), np.full(n, NO_POINT, np.uint64)), 2: (1, q, t, c.reshape(1, 2), np.array([1], np.uint64)),
              3: (1, q, t, pix, np.full(n, NO_POINT, np.uint64))}
    images[1][4][0] = 1
    matches = [(1, 2, np.array([[0, 0]], np.uint32)), (1, 3, np.array([[0, 0]], np.uint32))]
    # the other pixels of image 3 hang on further points2D of image 2?  no: one correspondence per image pair and point2D,
    # so they hang on image 1's other points2D, which are matched to the track's element in image 2
    for j in range(1, n):
        matches.append((1, 3, np.array([[j, j]], np.uint32)))
        matches.append((2, 1, np.array([[0, j]], np.uint32)))
    return dict(cameras={1: (0, tc.WIDTH, tc.HEIGHT, prm)}, images=images, points={1: (np.array(X, np.float64), (9, 9, 9), 0.0, [(1, 0), (2, 0)])},
                graph_images={1: n, 2: 1, 3: n}, matches=matches), c


def test_an_error_exactly_at_the_threshold_is_kept_and_one_double_above_is_dropped():
    prm = ba_cases.model_params(0)
    cx, cy = prm[1], prm[2]
    st, _ = _axis_state([[cx + 3.0, cy + 4.0]], [0.0, 0.0, 5.0])
    assert both_ways(st, "complete", complete_max_reproj_error=5.0)[0] == 1  # 25 is not above 25
    assert both_ways(st, "complete", complete_max_reproj_error=float(np.nextafter(5.0, 0.0)))[0] == 0
    st, _ = _axis_state([[cx + 3.0, float(np.nextafter(cy + 4.0, np.inf))]], [0.0, 0.0, 5.0])
    assert both_ways(st, "complete", complete_max_reproj_error=5.0)[0] == 0
    # a point behind the cameras: DBL_MAX, whatever the pixel
    st, _ = _axis_state([[cx, cy]], [0.0, 0.0, -5.0])
    assert both_ways(st, "complete", complete_max_reproj_error=1e150)[0] == 0
    st, _ = _axis_state([[cx, cy]], [0.0, 0.0, 5.0])
    assert both_ways(st, "complete")[0] == 1


# ---- merging by hand -----------------------------------------------------------------------------------------------------------------
def _near(d):
    return [X0[0] + d, X0[1] - d, X0[2] + 0.5 * d]


def test_two_duplicates_merge_with_the_weighted_mean_track_order_and_colour():
    a, b = _near(1e-3), _near(-2e-3)
    st = k.world(7, [X0], {0: list(range(1, 8))}, [(a, [(0, 1), (0, 2)]), (b, [(0, i) for i in range(3, 8)])])
    n, points, p2, modified, r = both_ways(st, "merge", modified=(1,))
    assert n == 7 and list(points) == [3] and modified == {3}
    want = [(2.0 * a[c] + 5.0 * b[c]) / 7.0 for c in range(3)]
    assert np.array_equal(k.bits(points[3][0]), k.bits(want))
    c1, c2 = k.colour(1), k.colour(2)
    assert points[3][1] == tuple(int((2.0 * c1[c] + 5.0 * c2[c]) / 7.0) for c in range(3)) and points[3][2] == -1.0
    assert [i for i, _ in points[3][3]] == [1, 2, 3, 4, 5, 6, 7]  # current's elements, then the other's
    assert all((ids == 3).all() for ids in p2.values())
    assert list(r.points3D[3].color) == list(points[3][1])
    # from the other side the order turns round and the id is the same
    n, points, _, _, _ = both_ways(st, "merge", ids=[2])
    assert n == 7 and [i for i, _ in points[3][3]] == [3, 4, 5, 6, 7, 1, 2]
    assert np.array_equal(k.bits(points[3][0]), k.bits([(5.0 * b[c] + 2.0 * a[c]) / 7.0 for c in range(3)]))


def test_one_outlying_observation_blocks_the_merge_and_the_pair_is_tried_once():
    a, b = _near(1e-3), _near(-2e-3)
    st = k.world(7, [X0], {0: list(range(1, 8))}, [(a, [(0, 1), (0, 2)]), (b, [(0, i) for i in range(3, 8)])], offsets={(0, 6): (30.0, 0.0)})
    tried = []

    def solver(d):
        out = k.merge_solver(d)
        tried.append(out["num_pairs_tried"])
        return out
    r, _, t = k.reconstruction(st)
    before = k.recon_points(r)
    assert P._merge_tracks_with(t, {}, None, solver) == 0 and k.same_points(k.recon_points(r), before)
    assert tried == [1]  # ten correspondences join the two points; root 2 meets the pair again: COLMAP's cache
    rs = k.ref_scene(st)
    assert rs.merge() == 0 and rs.pairs_tried() == 1
    assert both_ways(st, "merge", merge_max_reproj_error=40.0)[0] == 7


def test_a_chain_returns_the_deepest_merge_and_merged_roots_return_zero():
    pts = [(_near(1e-3), [(0, 1), (0, 2)]), (_near(-1e-3), [(0, 3), (0, 4)]), (_near(2e-3), [(0, 5), (0, 6)])]
    st = k.world(6, [X0], {0: list(range(1, 7))}, pts)
    n, points, _, modified, _ = both_ways(st, "merge", ids=[1])  # the unlisted neighbours 2 and 3 take part
    assert n == 6 and list(points) == [5] and modified == {5}  # 1 + 2 -> 4, 4 + 3 -> 5
    assert [i for i, _ in points[5][3]] == [1, 2, 3, 4, 5, 6]
    m4 = [(2.0 * pts[0][0][c] + 2.0 * pts[1][0][c]) / 4.0 for c in range(3)]
    assert np.array_equal(k.bits(points[5][0]), k.bits([(4.0 * m4[c] + 2.0 * pts[2][0][c]) / 6.0 for c in range(3)]))
    n, points, _, _, _ = both_ways(st, "merge")  # roots 2 and 3 are gone when their turn comes
    assert n == 6 and list(points) == [5]
    n, points, _, _, _ = both_ways(st, "merge", ids=[3, 2])  # 2 + 1 -> 4, 4 + 3 -> 5; then root 3 is gone
    assert n == 6 and [i for i, _ in points[5][3]] == [3, 4, 1, 2, 5, 6]


def test_new_ids_follow_the_roots_ids_across_components_and_the_modified_set():
    Y0 = [-0.4, 0.3, -0.2]
    # component A: points 1 and 3 (four observations); component B: points 2 and 4 (seven: first in the flat problem);
    # point 5 stands alone
    tracks = [(_near(1e-3), [(0, 1), (0, 2)]), (Y0, [(1, 1), (1, 2), (1, 3)]), (_near(-1e-3), [(0, 3), (0, 4)]),
              (Y0, [(1, 4), (1, 5), (1, 6), (1, 7)]), ([0.5, 0.5, 0.5], [(2, 1), (2, 2)])]
    st = k.world(7, [X0, Y0, [0.5, 0.5, 0.5]], {0: [1, 2, 3, 4], 1: [1, 2, 3, 4, 5, 6, 7], 2: [1, 2]}, tracks)
    n, points, _, modified, r = both_ways(st, "merge", modified=(3, 5, 2))
    assert n == 4 + 7 and list(points) == [5, 6, 7]
    assert [i for i, _ in points[6][3]] == [1, 2, 3, 4] and [i for i, _ in points[7][3]] == [1, 2, 3, 4, 5, 6, 7]  # 6 = 1 + 3, 7 = 2 + 4
    assert modified == {5, 6, 7}
    s = pc.last_run_stats()
    assert (s["num_components"], s["largest_component"], s["num_merges"]) == (2, 7, 2)
    assert list(r.points3D) == [5, 6, 7]  # the survivor keeps its place, the new points follow in the order they were made
    n, points, _, _, _ = both_ways(st, "merge", ids=[4, 3])  # root 3 before root 4
    assert n == 11 and [i for i, _ in points[6][3]] == [3, 4, 1, 2] and [i for i, _ in points[7][3]] == [4, 5, 6, 7, 1, 2, 3]


def _big_component(nobs):
    """point 1 with one observation in image 1, point 2 with nobs - 1 in image 2, one correspondence between them"""
    prm = ba_cases.model_params(0)
    q, t = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
    n = nobs - 1
    xy = np.tile([prm[1], prm[2]], (n, 1))
    images = {1: (1, q, t, xy[:1], np.array([1], np.uint64)), 2: (1, q, t, xy, np.full(n, 2, np.uint64))}
    points = {1: (np.array([0.0, 0.0, 5.0]), (1, 1, 1), 0.0, [(1, 0)]), 2: (np.array([0.0, 0.0, 6.0]), (2, 2, 2), 0.0, [(2, j) for j in range(n)])}
    return dict(cameras={1: (0, tc.WIDTH, tc.HEIGHT, prm)}, images=images, points=points, graph_images={1: 1, 2: n},
                matches=[(1, 2, np.array([[0, 0]], np.uint32))])


def test_a_component_of_4096_observations_is_merged_and_one_of_4097_is_refused():
    r, _, t = k.reconstruction(_big_component(k.MAX_COMPONENT_OBS))
    assert merge_with(t, {}, [1]) == k.MAX_COMPONENT_OBS and list(r.points3D) == [3]
    assert pc.last_run_stats()["largest_component"] == k.MAX_COMPONENT_OBS
    r, _, t = k.reconstruction(_big_component(k.MAX_COMPONENT_OBS + 1))
    t.add_modified_point3D(2)
    for call in (lambda: merge_with(t, {}, [1]), lambda: pc.merge_all_tracks(t, {}), lambda: pc.merge_tracks(t, {}, [2])):
        with pytest.raises(ValueError, match="component of 4097 observations, more than 4096"):
            call()
    assert list(r.points3D) == [1, 2] and r.points3D[2].track.length() == k.MAX_COMPONENT_OBS and t.get_modified_points3D() == {2}
    assert merge_with(t, {}, [77]) == 0  # the bound is for the components the listed points lie in


def test_graph_without_the_tracks_images_raises_and_leaves_the_model():
    st = k.world(4, [X0], {0: [1, 2, 3, 4]}, [(_near(1e-3), [(0, 1), (0, 2)]), (_near(-1e-3), [(0, 3)])])
    r, _, t = k.reconstruction(st)
    before = k.recon_points(r)
    t2 = pc.IncrementalTriangulator(pc.CorrespondenceGraph(), r)
    for call in (lambda: complete_with(t2, {}), lambda: merge_with(t2, {}), lambda: pc.complete_tracks(t2, {}, [1]), lambda: pc.merge_tracks(t2, {}, [2])):
        with pytest.raises(ValueError, match=r"\[correspondence_graph.h:\d+\] Check Failed: ExistsImage"):
            call()
    assert k.same_points(k.recon_points(r), before)
    for rs_call in (lambda s: s.complete(), lambda s: s.merge()):
        with pytest.raises(ValueError):
            rs_call(ref.Scene(st["cameras"], st["images"], st["points"], {}, []))
    with pytest.raises(ValueError, match="shape"):
        P._merge_tracks_with(t, {}, None, lambda d: dict(root_return=[0, 0], root_merge_offsets=[0, 1, 1], merge_current=[], merge_other=[], merge_xyz=[]))
    with pytest.raises(ValueError, match="does not fit"):
        P._merge_tracks_with(t, {}, None, lambda d: dict(root_return=[0, 0], root_merge_offsets=[0, 1, 1], merge_current=[0], merge_other=[0], merge_xyz=[[0, 0, 0]]))
    assert k.same_points(k.recon_points(r), before) and t.get_modified_points3D() == set()


def test_host_half_under_asan(tmp_path):
    """The host half (csrc/host/track_ops_host.h, csrc/tracks_plan.h) in a stand-alone program under ASan + UBSan
    (tests/shim/track_ops_host_fuzz.cc)."""
    import os
    import shutil
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    flags = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined"]
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("sanitizer runtime not installed")
    exe = tmp_path / "track_ops_host_fuzz"
    b = subprocess.run(flags + [str(ROOT / "tests" / "shim" / "track_ops_host_fuzz.cc"),
                                str(ROOT / "pycolmap_amd" / "csrc" / "host" / "model_io.cc"),
                                str(ROOT / "pycolmap_amd" / "csrc" / "host" / "reconstruction.cc"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[1]) >= 1000
