"""GPU parity of track completion and track merging (include/amc_tracks.h, csrc/tracks.hip): the
library against the CPU reference (tests/tracks_ref) and the frozen fixture, bit for bit, on the smallest shapes at which
the kernels can go wrong (tests/tracks_cases.py); splitting; order independence; refused input; and complete_tracks,
complete_all_tracks, merge_tracks and merge_all_tracks on top, alone and in the mapper's chain."""
from pathlib import Path

import numpy as np
import pytest

import tracks_cases as k
from pycolmap_amd import _capi

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "tracks_ref_v1.npz"


@pytest.fixture(scope="module")
def ctx():
    with _capi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _call(ctx, name, args=None, **more):
    a, kw = k.case_call(name)
    fn = ctx.complete_tracks if name.startswith("c/") else ctx.merge_tracks
    return fn(*(a if args is None else args), **{**kw, **more})


def _check_times(got, device_call):
    assert got["num_batches"] == (1 if device_call else 0)
    assert got["device_ms"] >= got["kernel_ms"] >= 0 and got["device_ms"] >= got["copy_ms"] >= 0
    assert got["host_ms"] >= got["alloc_ms"] >= 0
    assert (got["kernel_ms"] > 0) == device_call


@pytest.mark.parametrize("name", sorted(k.ALL_CASES))
def test_library_equals_reference_and_fixture(name, ctx, golden):
    got = _call(ctx, name)
    assert k.same(name, got, k.reference(name)), name  # NaNs as 16.6 F6
    assert k.digest(name, got) == str(golden[f"{name}/digest"])
    a, _ = k.case_call(name)
    _check_times(got, device_call=len(a[7]) > 0 if name.startswith("c/") else len(a[5]) > 1)
    if name.startswith("m/"):
        assert got["num_pairs_tried"] >= k.reference(name)["num_pairs_tried"]  # the one-sided stamp tries no fewer (18.2)


@pytest.mark.parametrize("name", ["c/sizes", "c/items_257", "c/all_models", "c/nonfinite"])
@pytest.mark.parametrize("batch", [1, 64, 65])
def test_split_completion_equals_unsplit(name, batch, ctx, monkeypatch):
    a, _ = k.case_call(name)
    monkeypatch.setenv("AMC_TRACKS_BATCH_CANDS", str(batch))
    split = _call(ctx, name)
    assert split["num_batches"] == -(-len(a[7]) // batch)
    assert k.same(name, split, k.reference(name)), (name, batch)


@pytest.mark.parametrize("name", ["m/comps_65", "m/mixed", "m/roots_even", "m/obs_4096"])
@pytest.mark.parametrize("batch", [1, 7, 64])
def test_split_merging_equals_unsplit(name, batch, ctx, monkeypatch):
    a, _ = k.case_call(name)
    monkeypatch.setenv("AMC_TRACKS_BATCH_COMPONENTS", str(batch))
    split = _call(ctx, name)
    assert split["num_batches"] == -(-(len(a[5]) - 1) // batch)
    assert k.same(name, split, k.reference(name)), (name, batch)


def test_calls_without_work_and_calls_in_a_row(ctx):
    for name in ("c/items_0", "m/comps_0"):
        got = _call(ctx, name)
        assert got["num_batches"] == 0 and got["device_ms"] == 0
    a, kw = k.case_call("c/sizes")
    empty = list(a)
    empty[5], empty[6], empty[7], empty[8] = np.zeros((3, 3)), np.zeros(4, np.uint64), np.zeros(0, np.uint32), np.zeros((0, 2))
    got = ctx.complete_tracks(*empty)  # items, none with a candidate
    assert got["num_batches"] == 0 and got["cand_pass"].size == 0
    for name in ("c/sizes", "m/mixed", "c/items_257", "m/comps_1", "c/sizes", "m/mixed"):  # larger calls between equal ones
        assert k.same(name, _call(ctx, name), k.reference(name)), name


def test_permuted_items_give_permuted_results(ctx):
    name = "c/sizes"
    a, _ = k.case_call(name)
    want = k.reference(name)
    off = a[6].astype(np.int64)
    perm = np.random.default_rng(5).permutation(len(off) - 1)
    cand = np.concatenate([np.arange(off[i], off[i + 1]) for i in perm]).astype(np.int64)
    p = list(a)
    p[5], p[6], p[7], p[8] = a[5][perm], np.concatenate([[0], np.cumsum((off[1:] - off[:-1])[perm])]).astype(np.uint64), a[7][cand], a[8][cand]
    got = _call(ctx, name, p)
    assert np.array_equal(k.bits(got["cand_sq_error"]), k.bits(want["cand_sq_error"][cand]))
    assert np.array_equal(got["cand_pass"], want["cand_pass"][cand])


@pytest.mark.parametrize("name", ["m/mixed", "m/roots_even"])
def test_permuted_components_give_permuted_results(name, ctx):
    a, _ = k.case_call(name)
    want = k.reference(name)
    cpo, cro, rt, X, poo, oi, xy, oco, co = (np.asarray(v) for v in a[5:])
    ncomp = len(cpo) - 1
    perm = np.random.default_rng(6).permutation(ncomp)
    i64 = lambda v: np.asarray(v, np.int64)  # noqa: E731
    cpo, cro, poo, oco = i64(cpo), i64(cro), i64(poo), i64(oco)
    pts = np.concatenate([np.arange(cpo[c], cpo[c + 1]) for c in perm])
    new_point = np.empty(len(X), np.int64)
    new_point[pts] = np.arange(len(pts))
    obs = np.concatenate([np.arange(poo[p], poo[p + 1]) for p in pts])
    new_obs = np.empty(len(oi), np.int64)
    new_obs[obs] = np.arange(len(obs))
    roots = np.concatenate([np.arange(cro[c], cro[c + 1]) for c in perm]).astype(np.int64)
    corr = [new_obs[i64(co[oco[o]:oco[o + 1]])] for o in obs]
    p = list(a[:5]) + [
        np.concatenate([[0], np.cumsum((cpo[1:] - cpo[:-1])[perm])]), np.concatenate([[0], np.cumsum((cro[1:] - cro[:-1])[perm])]),
        new_point[i64(rt)[roots]], X[pts], np.concatenate([[0], np.cumsum((poo[1:] - poo[:-1])[pts])]), oi[obs], xy[obs],
        np.concatenate([[0], np.cumsum([len(c) for c in corr])]), np.concatenate(corr) if corr else np.zeros(0, np.int64)]
    got = _call(ctx, name, p)
    assert np.array_equal(got["root_return"], want["root_return"][roots])
    moff = i64(want["root_merge_offsets"])
    merges = np.concatenate([np.arange(moff[r], moff[r + 1]) for r in roots]).astype(np.int64)
    assert np.array_equal(np.diff(i64(got["root_merge_offsets"])), (moff[1:] - moff[:-1])[roots])
    for key in ("merge_current", "merge_other"):  # slots are the component's own: they do not move
        assert np.array_equal(got[key], want[key][merges])
    assert np.array_equal(k.bits(got["merge_xyz"]), k.bits(want["merge_xyz"][merges]))


def test_refused_input(ctx):
    a, _ = k.case_call("c/item_of_1")

    def complete(i=None, value=None, **opts):
        p = list(a)
        if i is not None:
            p[i] = value
        return ctx.complete_tracks(*p, **opts)
    for bad in (lambda: complete(0, [11]), lambda: complete(0, [-1]), lambda: complete(2, np.full(len(a[2]), 7, np.uint32)),
                lambda: complete(7, np.full(len(a[7]), 1000, np.uint32)), lambda: complete(complete_max_reproj_error=-1.0),
                lambda: complete(complete_max_reproj_error=float("nan"))):
        with pytest.raises(_capi.AmcError) as e:
            bad()
        assert e.value.code == _capi.AMC_E_INVALID and "amc_complete_tracks" in str(e.value)
    assert k.same("c/item_of_1", complete(), k.reference("c/item_of_1"))

    m, _ = k.case_call("m/chain_5")

    def merge(i=None, value=None, **opts):
        p = list(m)
        if i is not None:
            p[i] = value
        return ctx.merge_tracks(*p, **opts)
    outside = np.array(m[13]).copy()
    outside[0] = len(m[10]) - 1
    two = [np.array([0, 3, 6], np.uint64), np.array([0, 3, 6], np.uint64)]  # the same points as two components
    for bad in (lambda: merge(0, [11]), lambda: merge(10, np.full(len(m[10]), 1000, np.uint32)),
                lambda: merge(merge_max_reproj_error=-1.0), lambda: merge(merge_max_reproj_error=float("nan")),
                lambda: ctx.merge_tracks(*m[:5], two[0], two[1], *m[7:]),  # roots and correspondences leave their component
                lambda: ctx.merge_tracks(*m[:5], two[0], np.array([0, 0, 6], np.uint64), *m[7:]),
                lambda: ctx.merge_tracks(*m[:5], two[0], np.array([0, 6, 6], np.uint64), m[7], *m[8:13], outside)):
        with pytest.raises(_capi.AmcError) as e:
            bad()
        assert e.value.code == _capi.AMC_E_INVALID and "amc_merge_tracks" in str(e.value)
    n = k.MAX_COMPONENT_OBS + 1
    long_comp = list(m[:5]) + [np.array([0, 1], np.uint64), np.array([0, 1], np.uint64), np.zeros(1, np.uint32), np.zeros((1, 3)),
                               np.array([0, n], np.uint64), np.zeros(n, np.uint32), np.zeros((n, 2)), np.zeros(n + 1, np.uint64),
                               np.zeros(0, np.uint32)]
    with pytest.raises(_capi.AmcError, match="4097 observations, more than 4096"):
        ctx.merge_tracks(*long_comp)
    assert k.same("m/chain_5", merge(), k.reference("m/chain_5"))


# ---- through Python ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", ["all", "subset"])
@pytest.mark.parametrize("op", ["complete", "merge", "both"])
@pytest.mark.parametrize("name", sorted(k.SCENES))
def test_functions_equal_sequential_reference(name, op, ids, golden):
    import pycolmap_amd as pc
    st, opts = k.scene_state(name)
    counts, points, p2, modified, _ = k.scene_reference(name, op, ids)
    r, _, t = k.reconstruction(st)
    survivors = dict(r.points3D)
    listed = k.subset_ids(st)
    got = []
    if op in ("complete", "both"):
        got.append(pc.complete_all_tracks(t, opts) if ids == "all" else pc.complete_tracks(t, opts, listed))
        s = pc.last_run_stats()
        assert s["call"] == ("complete_all_tracks" if ids == "all" else "complete_tracks") and s["num_device_calls"] == 1
        assert s["num_completed_observations"] == got[-1] and s["num_candidates_tested"] >= s["num_completed_observations"]
        assert s["device_ms"] >= s["kernel_ms"] > 0
    if op in ("merge", "both"):
        got.append(pc.merge_all_tracks(t, opts) if ids == "all" else pc.merge_tracks(t, opts, set(listed)))
        s = pc.last_run_stats()
        assert s["call"] == ("merge_all_tracks" if ids == "all" else "merge_tracks") and s["num_device_calls"] == 1
        assert s["num_merges"] > 0 and s["num_pairs_tried"] >= s["num_merges"] and s["largest_component"] <= k.MAX_COMPONENT_OBS
    assert got == counts
    assert k.same_points(k.recon_points(r), points)
    assert k.same_point2D_ids(k.recon_point2D_ids(r), p2)
    assert t.get_modified_points3D() == modified
    assert all(r.points3D[pid] is obj for pid, obj in survivors.items() if pid in r.points3D)
    assert k.state_digest(sum(counts), points) == str(golden[f"scene/{name}/{op}/{ids}/digest"])


def test_chain_triangulate_adjust_complete_merge_filter_equals_the_reference_chain():
    """triangulate every image, take every fourth element off the longer tracks (as a filter would have), BundleAdjuster on
    all of it with the poses fixed, complete and merge the modified points, filter_all_points3D: the library's chain
    against the same chain with the references in the library's place"""
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
        for pid, p in sorted(r.points3D.items()):
            if p.track.length() >= 4:
                for e in list(p.track.elements)[3::4]:
                    r.delete_observation(e.image_id, e.point2D_idx)
        config = pc.BundleAdjustmentConfig()
        for iid in sc["images"]:
            config.add_image(iid)
            config.set_constant_cam_pose(iid)
        options = pc.BundleAdjustmentOptions(refine_focal_length=False, refine_extra_params=False)
        adjuster = pc.BundleAdjuster(options, config)
        if use_library:
            adjuster.solve(r)
        else:
            adjuster._solve_with(r, bc.reference_solver(ba_config_ref_lib))
        modified = t.get_modified_points3D()
        if use_library:
            counts = [pc.complete_tracks(t, {}, modified), pc.merge_tracks(t, {}, modified)]
        else:
            counts = [P._complete_tracks_with(t, {}, modified, k.complete_solver), P._merge_tracks_with(t, {}, modified, k.merge_solver)]
        after = k.recon_points(r)
        counts.append(r.filter_all_points3D(4.0, 1.5))  # (the filter has no hook: the library's in both chains)
        out.append((counts, after, k.recon_points(r), k.recon_point2D_ids(r), t.get_modified_points3D()))
    lib, want = out
    assert lib[0] == want[0] and lib[0][0] > 0 and lib[0][1] > 0
    assert k.same_points(lib[1], want[1]) and k.same_points(lib[2], want[2]) and k.same_point2D_ids(lib[3], want[3])
    assert lib[4] == want[4] and len(lib[2]) >= 25


def test_model_untouched_after_a_refused_call():
    import pycolmap_amd as pc
    st = k.world(5, [[0.1, 0.2, 0.3]], {0: [1, 2, 3, 4, 5]}, [([0.1, 0.2, 0.3], [(0, 1), (0, 2)]), ([0.1, 0.2, 0.3], [(0, 3), (0, 4)])])
    r, _, t = k.reconstruction(st)
    before, ids = k.recon_points(r), k.recon_point2D_ids(r)
    t.add_modified_point3D(1)
    for fn in (pc.complete_all_tracks, pc.merge_all_tracks):
        with pytest.raises(ValueError, match="complete_max_reproj_error > 0"):
            fn(t, dict(complete_max_reproj_error=0.0))
    g2 = pc.CorrespondenceGraph()  # a graph that does not hold the images
    t2 = pc.IncrementalTriangulator(g2, r)
    for fn in (pc.complete_all_tracks, pc.merge_all_tracks):
        with pytest.raises(ValueError, match=r"Check Failed: ExistsImage"):
            fn(t2, {})
    assert k.same_points(k.recon_points(r), before) and k.same_point2D_ids(k.recon_point2D_ids(r), ids)
    assert t.get_modified_points3D() == {1}
    assert pc.complete_all_tracks(t, {}) == 1 and pc.merge_all_tracks(t, {}) == 5
