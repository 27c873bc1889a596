"""GPU parity of retriangulate (include/amc_retri.h, csrc/retri.hip): the library against the CPU
reference (tests/retri_ref) and the frozen fixture, bit for bit, on the smallest shapes at which the kernels can go wrong
(tests/retri_cases.py); every correspondence against Context.triangulate_observations on its equivalent two-candidate
item; independence of the launch bound and of the pairs' layout; refused input; and retriangulate on top, alone and in the
mapper's chain."""
from pathlib import Path

import numpy as np
import pytest

import retri_cases as k
import retri_ref_lib as ref
import tracks_cases as trc
from pycolmap_amd import _capi

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "retri_ref_v1.npz"


@pytest.fixture(scope="module")
def ctx():
    with _capi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _call(ctx, name, args=None, **more):
    a, kw = k.case_call(name)
    return ctx.retriangulate_pairs(*(a if args is None else args), **{**kw, **more})


def _num_launches(args, bound=None):
    """the rounds in order, each cut greedily on pair boundaries at `bound` correspondences"""
    poff, roff = [int(v) for v in args[10]], [int(v) for v in args[12]]
    n = 0
    for r in range(len(roff) - 1):
        i = roff[r]
        while i < roff[r + 1]:
            j = i + 1
            while bound is None and j < roff[r + 1] or bound is not None and j < roff[r + 1] and poff[j + 1] - poff[i] <= bound:
                j += 1
            n, i = n + 1, j
    return n


@pytest.mark.parametrize("name", sorted(k.ALL_CASES))
def test_library_equals_reference_and_fixture(name, ctx, golden):
    got = _call(ctx, name)
    want = k.reference(name)
    assert k.same(got, want), name  # NaNs as 16.6 F6
    assert k.digest(got) == str(golden[f"{name}/digest"])
    assert (got["num_pairs_run"], got["num_continued"], got["num_created"]) == (want["num_pairs_run"], want["num_continued"], want["num_created"])
    a, _ = k.case_call(name)
    assert got["num_launches"] == _num_launches(a)
    device_call = len(a[9]) > 0
    assert got["device_ms"] >= got["kernel_ms"] >= 0 and got["device_ms"] >= got["copy_ms"] >= 0 and got["host_ms"] >= got["alloc_ms"] >= 0
    assert (got["kernel_ms"] > 0) == device_call


@pytest.mark.parametrize("name, tri, ran", [("filled_pair_skipped", [0, 0, 6], [True, True, False]), ("filled_pair_runs", [0, 0, 1], [True, True, True])])
def test_the_ratio_is_taken_on_the_state_the_earlier_rounds_left(name, tri, ran, ctx):
    a, _ = k.case_call(name)
    got = _call(ctx, name)
    assert k.initial_num_tri(a) == [0, 0, 0]  # on the uploaded state the last pair has no common point at all
    assert got["pair_num_tri"].tolist() == tri and got["pair_ran"].tolist() == ran


@pytest.mark.parametrize("name", sorted(k.ALL_CASES))
def test_every_correspondence_equals_the_existing_kernel_on_its_item(name, ctx):
    a, kw = k.case_call(name)
    got = _call(ctx, name)
    targs, tkw, want = k.equivalent_items(a, kw, got)
    if not want:
        assert not got["corr_action"].any()
        return
    k.check_equivalent(want, ctx.triangulate_observations(*targs, **tkw))


@pytest.mark.parametrize("name, bound", [("sizes", 64), ("sizes", 1), ("mixed", 26), ("pairs_257", 1), ("all_models", 8)])
def test_result_does_not_depend_on_the_launch_bound(name, bound, ctx, monkeypatch):
    a, _ = k.case_call(name)
    monkeypatch.setenv("AMC_RETRI_BATCH_CORRS", str(bound))
    split = _call(ctx, name)
    sizes = np.diff(np.asarray(a[10], np.int64))
    assert sizes.max() > bound  # a pair larger than the bound: a launch of its own
    assert split["num_launches"] == _num_launches(a, bound) > _num_launches(a)  # the bound cuts a round
    assert k.same(split, k.reference(name)), (name, bound)


@pytest.mark.parametrize("name", ["mixed", "sizes", "all_models", "pairs_257"])
def test_pairs_permuted_inside_their_rounds_give_the_permuted_result(name, ctx):
    a, kw = k.case_call(name)
    want = k.reference(name)
    pa, pkw, order, corr_map = k.permuted(a, kw, seed=5)
    assert order != sorted(order)
    got = ctx.retriangulate_pairs(*pa, **pkw)
    assert np.array_equal(got["pair_ran"], want["pair_ran"][order]) and np.array_equal(got["pair_num_tri"], want["pair_num_tri"][order])
    assert np.array_equal(got["corr_action"], want["corr_action"][corr_map])
    # created positions in the permuted correspondence order
    where = np.full(len(want["corr_action"]), -1)
    where[want["corr_action"] == ref.CREATED] = np.arange(want["num_created"])
    rows = [where[c] for c in corr_map if where[c] >= 0]
    assert np.array_equal(k.bits(got["created_xyz"]), k.bits(want["created_xyz"][rows]))


def test_calls_without_work_and_calls_in_a_row(ctx):
    got = _call(ctx, "rounds_0")
    assert got["num_launches"] == 0 and got["device_ms"] == 0 and got["corr_action"].size == 0
    got = _call(ctx, "pairs_0")  # empty rounds around one with a pair
    assert got["num_launches"] == 1
    for name in ("sizes", "mixed", "rounds_65", "rounds_1", "sizes", "mixed"):  # larger calls between equal ones
        assert k.same(_call(ctx, name), k.reference(name)), name


def test_refused_flat_input(ctx):
    a, kw = k.case_call("mixed")

    def call(i=None, value=None, **opts):
        p = list(a)
        if i is not None:
            p[i] = value
        return ctx.retriangulate_pairs(*p, **{**kw, **opts})
    n_obs, n_pts, n_img = len(a[5]), len(a[8]), len(a[2])
    obs = np.array(a[11]).copy()
    obs[0, 0] = n_obs
    twice = np.array(a[11]).copy()
    twice[1] = twice[0]
    wrong_image = np.array(a[11]).copy()
    wrong_image[0] = wrong_image[0][::-1]
    point = np.array(a[7]).copy()
    point[3] = n_pts
    one_round = np.array([0, len(a[9])], np.uint64)  # all pairs in one round: they share images
    pimg = np.array(a[9]).copy()
    pimg[0] = [n_img, 0]
    spare_points = np.zeros((2 * len(a[11]) + 1, 3))  # more points than the correspondences can use
    for bad in (lambda: call(0, [11, 1]), lambda: call(8, spare_points), lambda: call(11, obs), lambda: call(11, twice), lambda: call(11, wrong_image),
                lambda: call(7, point), lambda: call(12, one_round), lambda: call(9, pimg), lambda: call(2, np.full(n_img, 7, np.uint32)),
                lambda: call(5, np.full(n_obs, n_img, np.uint32)), lambda: call(12, np.array([0, 1], np.uint64)),
                lambda: call(create_max_angle_error=0.0), lambda: call(re_max_angle_error=-1.0), lambda: call(min_angle=float("nan")),
                lambda: call(re_min_ratio=-0.5), lambda: call(re_min_ratio=float("nan"))):
        with pytest.raises(_capi.AmcError) as e:
            bad()
        assert e.value.code == _capi.AMC_E_INVALID and "amc_retriangulate_pairs" in str(e.value)
    with pytest.raises(_capi.AmcError, match="twice"):
        call(11, twice)
    with pytest.raises(_capi.AmcError, match="two pairs with image"):
        call(12, one_round)
    assert k.same(call(), k.reference("mixed"))  # the context is as good as before


# ---- through Python ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", k.SCENES)
def test_retriangulate_equals_sequential_reference_called_twice(name, golden):
    import pycolmap_amd as pc
    from pycolmap_amd import _pycolmap as P
    st, opts = k.scene_state(name)
    calls, _ = k.scene_reference(name)
    r, _, t = trc.reconstruction(st)
    survivors = dict(r.points3D)
    for count, points, p2, modified, trials in calls:
        assert pc.retriangulate(t, opts) == count
        s = pc.last_run_stats()
        assert s["call"] == "retriangulate" and s["num_device_calls"] == (1 if s["num_pairs"] else 0)
        assert s["num_continued_observations"] + 2 * s["num_created_points"] == count and s["num_pairs_run"] <= s["num_pairs"]
        assert s["num_pairs"] == 0 or s["device_ms"] >= s["kernel_ms"] > 0
        assert k.same_model(r, points, p2)
        assert t.get_modified_points3D() == modified and P._retriangulate_trials(t) == trials
    assert calls[0][0] > 0 and all(r.points3D[pid] is obj for pid, obj in survivors.items())
    assert k.state_digest(calls[1][0], calls[1][1], calls[1][4]) == str(golden[f"scene/{name}/digest"])


def test_chain_triangulate_adjust_retriangulate_complete_merge_filter_equals_the_reference_chain():
    """triangulate every image, take every third element off the longer tracks and delete every fourth point (as drift
    and a filter would have), BundleAdjuster on all of it with the poses fixed, retriangulate, complete and merge the
    modified points, filter_all_points3D: the library's chain against the same chain with the references in the
    library's place"""
    import ba_config_cases as bc
    import ba_config_ref_lib
    import pycolmap_amd as pc
    import triangulator_cases as tc
    from pycolmap_amd import _pycolmap as P
    sc = tc.scene(seed=33, nimg=12, npts=25, models=(2,), noise=0.3, wrong=3, views=(5, 12), drop=0.4)
    out = []
    for use_library in (True, False):
        r, g = tc.reconstruction(sc)
        t = pc.IncrementalTriangulator(g, r)
        for iid in sc["images"]:
            if use_library:
                t.triangulate_image({}, iid)
            else:
                t._triangulate_image_with({}, iid, tc.reference_solver)
        for n, (pid, p) in enumerate(sorted(r.points3D.items())):
            if n % 4 == 3:
                r.delete_point3D(pid)
            elif p.track.length() >= 4:
                for e in list(p.track.elements)[2::3]:
                    r.delete_observation(e.image_id, e.point2D_idx)
        config = pc.BundleAdjustmentConfig()
        for iid in sc["images"]:
            config.add_image(iid)
            config.set_constant_cam_pose(iid)
        adjuster = pc.BundleAdjuster(pc.BundleAdjustmentOptions(refine_focal_length=False, refine_extra_params=False), config)
        if use_library:
            adjuster.solve(r)
        else:
            adjuster._solve_with(r, bc.reference_solver(ba_config_ref_lib))
        opts = dict(re_min_ratio=0.6)
        counts = [pc.retriangulate(t, opts) if use_library else P._retriangulate_with(t, opts, k.reference_solver)]
        modified = t.get_modified_points3D()
        if use_library:
            counts += [pc.complete_tracks(t, {}, modified), pc.merge_tracks(t, {}, modified)]
        else:
            counts += [P._complete_tracks_with(t, {}, modified, trc.complete_solver), P._merge_tracks_with(t, {}, modified, trc.merge_solver)]
        after = trc.recon_points(r)
        counts.append(r.filter_all_points3D(4.0, 1.5))  # (the filter has no hook: the library's in both chains)
        out.append((counts, after, trc.recon_points(r), trc.recon_point2D_ids(r), t.get_modified_points3D(), P._retriangulate_trials(t)))
    lib, want = out
    assert lib[0] == want[0] and lib[0][0] > 0
    assert trc.same_points(lib[1], want[1]) and trc.same_points(lib[2], want[2]) and trc.same_point2D_ids(lib[3], want[3])
    assert lib[4] == want[4] and lib[5] == want[5] and len(lib[5]) > 0


def test_model_untouched_after_a_refused_call():
    import pycolmap_amd as pc
    from pycolmap_amd import _pycolmap as P
    st, opts = k.scene_state("direct")
    r, g, t = trc.reconstruction(st)
    before, ids = trc.recon_points(r), trc.recon_point2D_ids(r)
    t.add_modified_point3D(1)
    with pytest.raises(ValueError, match="re_max_angle_error > 0"):
        pc.retriangulate(t, dict(re_max_angle_error=0.0))
    # a graph that names points2D the reconstruction does not hold
    g2 = pc.CorrespondenceGraph()
    for iid, n in st["graph_images"].items():
        g2.add_image(iid, n + 50)
    g2.add_correspondences(1, 2, np.array([[0, 0], [len(st["images"][1][3]) + 7, 1]], np.uint32))
    g2.finalize()
    t2 = pc.IncrementalTriangulator(g2, r)
    with pytest.raises(ValueError, match="which the reconstruction does not hold"):
        pc.retriangulate(t2, opts)
    assert trc.same_points(trc.recon_points(r), before) and trc.same_point2D_ids(trc.recon_point2D_ids(r), ids)
    assert t.get_modified_points3D() == {1} and P._retriangulate_trials(t) == {} and P._retriangulate_trials(t2) == {}
    assert pc.retriangulate(t, opts) == k.scene_reference("direct")[0][0][0]
