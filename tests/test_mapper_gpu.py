"""GPU parity of the mapper's device calls (include/amc_mapper.h, csrc/mapper.hip): the library against
the CPU reference (tests/mapper_ref) and the frozen fixture, bit for bit, on the smallest shapes at which the kernels can go
wrong (tests/mapper_cases.py); independence of the batch bounds and of the items' order; refused input; and the three
methods on top, in the mapper's loop on the five scenes against the same loop with the references in the library's
place."""
from pathlib import Path

import numpy as np
import pytest

import mapper_cases as k
from pycolmap_amd import _capi

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "mapper_ref_v1.npz"


@pytest.fixture(scope="module")
def ctx():
    with _capi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _times_ok(got, device_call):
    assert got["device_ms"] >= got["kernel_ms"] >= 0 and got["device_ms"] >= got["copy_ms"] >= 0 and got["host_ms"] >= got["alloc_ms"] >= 0
    assert (got["kernel_ms"] > 0) == device_call and (got["device_ms"] > 0) == device_call


# ---- image_visibility ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(k.VIS_CASES))
def test_visibility_equals_reference_and_fixture(name, ctx, golden):
    a = k.vis_call(name)
    got = ctx.image_visibility(*a)
    assert k.vis_same(got, k.vis_reference(name)), name
    assert k.vis_digest(got) == str(golden[f"vis/{name}/digest"]) and got["max_score"] == _capi.MAPPER_MAX_SCORE
    ncand = len(a[2])
    assert got["num_batches"] == (1 if ncand else 0)
    _times_ok(got, ncand > 0)  # a call without candidates touches no device


@pytest.mark.parametrize("name, bound", [("sizes", 1), ("sizes", 4), ("cands_65", 64), ("cands_65", 3), ("random", 7), ("edges", 5)])
def test_visibility_does_not_depend_on_the_batch_bound(name, bound, ctx, monkeypatch):
    a = k.vis_call(name)
    monkeypatch.setenv("AMC_MAPPER_BATCH_IMAGES", str(bound))
    got = ctx.image_visibility(*a)
    ncand = len(a[2])
    assert got["num_batches"] == -(-ncand // bound) > 1  # consecutive candidates, `bound` per launch
    assert k.vis_same(got, k.vis_reference(name)), (name, bound)


@pytest.mark.parametrize("name", ["sizes", "cands_65", "random", "edges"])
def test_visibility_of_permuted_candidates_is_the_permuted_result(name, ctx):
    want = k.vis_reference(name)
    pa, order = k.vis_permuted(k.vis_call(name), seed=7)
    assert order.tolist() != sorted(order.tolist())
    got = ctx.image_visibility(*pa)
    for f in ("num_observations", "num_visible_points3D", "score"):
        assert np.array_equal(got[f], want[f][order]), f


def test_visibility_refuses_bad_input(ctx):
    a = list(k.vis_call("sizes"))

    def call(i, value):
        p = list(a)
        p[i] = value
        return ctx.image_visibility(*p)
    ipoff, cpoff, coff, ci, cp = a[0], a[4], a[6], a[7], a[8]
    swapped = ipoff.copy()
    swapped[1], swapped[2] = ipoff[2], ipoff[1]
    first = coff.copy()
    first[0] = 1
    down = coff.copy()
    down[3] = coff[-1] + 5
    bad_image = ci.copy()
    bad_image[0] = len(ipoff) - 1
    bad_point = cp.copy()
    bad_point[0] = int(ipoff[ci[0] + 1] - ipoff[ci[0]])
    cdown = cpoff.copy()
    cdown[2] = cpoff[3] + 1
    for bad in (lambda: call(0, swapped), lambda: call(6, first), lambda: call(6, down), lambda: call(7, bad_image), lambda: call(8, bad_point),
                lambda: call(4, cdown)):
        with pytest.raises(_capi.AmcError) as e:
            bad()
        assert e.value.code == _capi.AMC_E_INVALID and "amc_image_visibility" in str(e.value)
    with pytest.raises(_capi.AmcError, match="names point2D"):
        call(8, bad_point)
    assert k.vis_same(ctx.image_visibility(*a), k.vis_reference("sizes"))  # the context is as good as before


# ---- shared_point_angles ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(k.ANGLE_CASES))
def test_angles_equal_reference_and_fixture(name, ctx, golden):
    a, kw = k.angle_call(name)
    got = ctx.shared_point_angles(*a, **kw)
    assert k.angle_same(got, k.angle_reference(name)), name  # NaN is the one quiet NaN on both sides
    assert k.angle_digest(got) == str(golden[f"angle/{name}/digest"])
    npairs = len(a[3])
    assert got["num_batches"] == (1 if npairs else 0)
    _times_ok(got, npairs > 0)  # a call without pairs touches no device


@pytest.mark.parametrize("name, bound", [("sizes", 1), ("sizes", 3), ("pairs_65", 64), ("pairs_65", 4), ("nonfinite", 2), ("random", 9)])
def test_angles_do_not_depend_on_the_batch_bound(name, bound, ctx, monkeypatch):
    a, kw = k.angle_call(name)
    monkeypatch.setenv("AMC_MAPPER_BATCH_PAIRS", str(bound))
    got = ctx.shared_point_angles(*a, **kw)
    assert got["num_batches"] == -(-len(a[3]) // bound) > 1  # consecutive pairs, `bound` per launch
    assert k.angle_same(got, k.angle_reference(name)), (name, bound)


@pytest.mark.parametrize("name", ["sizes", "pairs_65", "nonfinite", "random"])
def test_angles_of_permuted_pairs_are_the_permuted_result(name, ctx):
    a, kw = k.angle_call(name)
    want = k.angle_reference(name)
    pa, order = k.angle_permuted(a, seed=3)
    assert order.tolist() != sorted(order.tolist())
    got = ctx.shared_point_angles(*pa, **kw)
    assert np.array_equal(k.bits(got["angle"]), k.bits(want["angle"][order]))


def test_the_rank_rounds_half_away_from_zero_on_the_device(ctx):
    """pairs of 3, 7 and 63 points: 0.75 (n - 1) = 1.5, 4.5 and 46.5 take the elements of rank 2, 5 and 47"""
    q, t = [[0, 0, 0, 1.0], [0, 0, 0, 1.0]], [[0, 0, 0.0], [-1.0, 0, 0]]
    X = [[0.5, 0.0, 1.0 + p] for p in range(63)]  # the angle falls with the distance: the order is known
    pairs = [(0, 1, list(range(n))[::-1]) for n in (3, 7, 63)]
    a = k._ang_problem(q, t, X, pairs)
    got = ctx.shared_point_angles(*a)
    every = k.ref.shared_point_angles(*a, all_angles=True)
    asc = np.sort(every["angles"][:3]), np.sort(every["angles"][3:10]), np.sort(every["angles"][10:])
    assert [k.rank_of(n) for n in (3, 7, 63)] == [2, 5, 47]
    assert got["angle"].tolist() == [asc[0][2], asc[1][5], asc[2][47]] == every["angle"].tolist()


def test_angles_refuse_bad_input(ctx):
    a, _ = k.angle_call("sizes")
    a = list(a)

    def call(i=None, value=None, **kw):
        p = list(a)
        if i is not None:
            p[i] = value
        return ctx.shared_point_angles(*p, **kw)
    poff, pi, sp = a[4], a[3], a[5]
    empty = poff.copy()
    empty[2] = empty[1]  # a pair without shared points
    first = poff.copy()
    first[0] = 1
    bad_image = pi.copy()
    bad_image[1, 1] = len(a[0])
    bad_point = sp.copy()
    bad_point[-1] = len(a[2])
    for bad in (lambda: call(4, empty), lambda: call(4, first), lambda: call(3, bad_image), lambda: call(5, bad_point), lambda: call(percentile=100.5),
                lambda: call(percentile=-1.0), lambda: call(percentile=float("nan"))):
        with pytest.raises(_capi.AmcError) as e:
            bad()
        assert e.value.code == _capi.AMC_E_INVALID and "amc_shared_point_angles" in str(e.value)
    # one point more than the header's bound
    n = _capi.MAPPER_MAX_PAIR_POINTS + 1
    with pytest.raises(_capi.AmcError, match="AMC_MAPPER_MAX_PAIR_POINTS") as e:
        ctx.shared_point_angles(a[0], a[1], a[2], [[0, 1]], [0, n], np.zeros(n, np.uint32))
    assert e.value.code == _capi.AMC_E_INVALID
    assert k.angle_same(call(), k.angle_reference("sizes"))  # the context is as good as before


def test_calls_in_a_row_on_one_context(ctx):
    for name in ("random", "sizes", "cands_0", "every_cell", "random"):
        assert k.vis_same(ctx.image_visibility(*k.vis_call(name)), k.vis_reference(name)), name
    for name in ("random", "pairs_0", "sizes", "nonfinite", "random"):
        a, kw = k.angle_call(name)
        assert k.angle_same(ctx.shared_point_angles(*a, **kw), k.angle_reference(name)), name


# ---- through Python ------------------------------------------------------------------------------------------------------------
def _loop(name, use_library):
    """find_next_images, register_next_image, triangulate_image, find_local_bundle, BundleAdjuster on the bundle, complete and
    merge the modified points, filter, until no candidate is worth trying: what every step returned and left behind"""
    import ba_config_cases as bc
    import ba_config_ref_lib
    import pycolmap_amd as pc
    import tracks_cases as trc
    import triangulator_cases as tc
    from pycolmap_amd import _pycolmap as P
    st = k.mapper_state(name)
    r, _, t, mp = k.mapper(st)
    o = k.SCENE_OPTIONS
    topts = tc.SCENES[name][1]
    steps, device_calls = [], 0
    while True:
        ranked = mp.find_next_images(o) if use_library else mp._find_next_images_with(o, k.vis_solver)
        device_calls += pc.last_run_stats()["num_device_calls"]
        if not ranked:
            break
        iid = ranked[0]
        ok = mp.register_next_image(o, iid) if use_library else mp._register_next_image_with(o, iid, k.pose_solver)
        device_calls += pc.last_run_stats()["num_device_calls"]
        step = [ranked, iid, ok, mp.last_registration()]
        if ok:
            step.append(t.triangulate_image(topts, iid) if use_library else t._triangulate_image_with(topts, iid, tc.reference_solver))
            bundle = mp.find_local_bundle(o, iid) if use_library else mp._find_local_bundle_with(o, iid, k.angle_solver)
            device_calls += pc.last_run_stats()["num_device_calls"]
            step.append(bundle)
            config = pc.BundleAdjustmentConfig()
            for i in [iid] + bundle:
                config.add_image(i)
            for i in bundle:  # the new image moves, its neighbours hold the gauge
                config.set_constant_cam_pose(i)
            adjuster = pc.BundleAdjuster(pc.BundleAdjustmentOptions(refine_focal_length=False, refine_extra_params=False), config)
            if use_library:
                adjuster.solve(r)
            else:
                adjuster._solve_with(r, bc.reference_solver(ba_config_ref_lib))
            modified = t.get_modified_points3D()
            if use_library:
                step += [pc.complete_tracks(t, topts, modified), pc.merge_tracks(t, topts, modified)]
            else:
                step += [P._complete_tracks_with(t, topts, modified, trc.complete_solver), P._merge_tracks_with(t, topts, modified, trc.merge_solver)]
            step.append(r.filter_points3D(o.get("filter_max_reproj_error", 4.0), o.get("filter_min_tri_angle", 1.5), t.get_modified_points3D()))
            t.clear_modified_points3D()  # (the filter has no hook: the library's in both loops)
        step.append(k.model_snapshot(r))
        step.append({i: mp.num_reg_trials(i) for i in sorted(st["candidates"])})
        steps.append(step)
    return steps, mp.candidates, mp.num_total_reg_images(), device_calls


@pytest.mark.parametrize("name", k.scene_names())
def test_the_mappers_loop_equals_the_loop_with_the_references(name):
    lib, want = _loop(name, True), _loop(name, False)
    assert len(lib[0]) == len(want[0]) >= 1
    for n, (a, b) in enumerate(zip(lib[0], want[0])):
        assert a == b, (name, n, [x == y for x, y in zip(a, b)])
    assert lib[1:3] == want[1:3] and want[3] == 0 and lib[3] >= 2 * len(lib[0])
    registered = sum(1 for s in lib[0] if s[2])
    assert lib[2] == 2 + registered and (registered >= 1 or name == "two_view_off")


def test_a_pair_above_the_bound_is_a_value_error_and_nothing_changes():
    st = k.mapper_state("direct", 6)
    r, _, t, mp = k.mapper(st)
    before = k.model_snapshot(r)
    iid = sorted(st["images"])[0]
    with pytest.raises(ValueError, match=r"more than 2 \(AMC_MAPPER_MAX_PAIR_POINTS"):
        mp._find_local_bundle_with(dict(local_ba_num_images=2), iid, None, 2)
    assert k.model_snapshot(r) == before
    want = k.ref_scene(st).find_local_bundle(iid, local_ba_num_images=2)
    assert mp.find_local_bundle(dict(local_ba_num_images=2), iid) == want
