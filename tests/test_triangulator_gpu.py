"""GPU parity of the incremental triangulator (include/amc_triobs.h, csrc/triobs.hip): the library
against the CPU reference (tests/triangulator_ref) and the frozen fixture, bit for bit, on the smallest shapes at which the
kernels can go wrong (tests/triangulator_cases.py); splitting; order independence; refused input; and
IncrementalTriangulator.triangulate_image on top, alone and in a chain with bundle_adjustment and the point filter."""
from pathlib import Path

import numpy as np
import pytest

import triangulator_cases as tc
from pycolmap_amd import _capi

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "triangulator_ref_v1.npz"


@pytest.fixture(scope="module")
def ctx():
    with _capi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _assert_same(got, want, what=""):
    for k in ("continued", "cand_round", "round_offsets"):
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)), (what, k)
    assert np.array_equal(tc.bits(got["round_xyz"]), tc.bits(want["round_xyz"])), (what, "round_xyz")  # NaNs as 16.6 F6
    assert got["num_created"] == want["num_created"] and got["num_continued"] == want["num_continued"], what


@pytest.mark.parametrize("name", sorted(tc.ALL_CASES))
def test_library_equals_reference_and_fixture(name, ctx, golden):
    args, kw = tc.case_call(name)
    got = ctx.triangulate_observations(*args, **kw)
    _assert_same(got, tc.reference(name), name)
    assert tc.digest(got) == str(golden[f"{name}/digest"])
    nitems = len(args[5]) - 1
    assert got["num_batches"] == (1 if nitems else 0)
    assert got["device_ms"] >= got["kernel_ms"] >= 0 and got["device_ms"] >= got["copy_ms"] >= 0
    assert got["host_ms"] >= got["alloc_ms"] >= 0
    if nitems:
        assert got["kernel_ms"] > 0


@pytest.mark.parametrize("name", ["sizes", "items_257", "all_models"])
@pytest.mark.parametrize("batch", [1, 64, 65])
def test_split_call_equals_unsplit_call(name, batch, ctx, monkeypatch):
    args, kw = tc.case_call(name)
    nitems = len(args[5]) - 1
    monkeypatch.setenv("AMC_TRIOBS_BATCH_ITEMS", str(batch))
    split = ctx.triangulate_observations(*args, **kw)
    assert split["num_batches"] == -(-nitems // batch)
    _assert_same(split, tc.reference(name), (name, batch))


def test_call_without_items_and_two_calls_in_a_row(ctx, monkeypatch):
    args, kw = tc.case_call("items_0")
    for batch in (None, 1):
        if batch:
            monkeypatch.setenv("AMC_TRIOBS_BATCH_ITEMS", str(batch))
        got = ctx.triangulate_observations(*args, **kw)
        assert got["num_batches"] == 0 and got["num_created"] == 0 and got["round_offsets"].tolist() == [0]
    monkeypatch.delenv("AMC_TRIOBS_BATCH_ITEMS")
    for name in ("mixed", "sizes", "mixed"):  # a larger call between two equal ones
        a, k = tc.case_call(name)
        _assert_same(ctx.triangulate_observations(*a, **k), tc.reference(name), name)


@pytest.mark.parametrize("name", ["mixed", "items_257"])
def test_permuted_items_give_permuted_results(name, ctx):
    args, kw = tc.case_call(name)
    want = tc.reference(name)
    off = args[5].astype(np.int64)
    nitems = len(off) - 1
    perm = np.random.default_rng(5).permutation(nitems)
    cand = np.concatenate([np.arange(off[i], off[i + 1]) for i in perm])
    new_off = np.concatenate([[0], np.cumsum((off[1:] - off[:-1])[perm])]).astype(np.uint64)
    pargs = list(args)
    pargs[5] = new_off
    for k in (6, 7, 8, 9):
        pargs[k] = args[k][cand]
    pkw = dict(kw)
    if pkw.get("no_create_two_view") is not None:
        pkw["no_create_two_view"] = np.asarray(pkw["no_create_two_view"])[perm]
    got = ctx.triangulate_observations(*pargs, **pkw)
    assert np.array_equal(got["continued"], want["continued"][perm])
    assert np.array_equal(got["cand_round"], want["cand_round"][cand])
    roff = want["round_offsets"].astype(np.int64)
    rounds = [np.arange(roff[i], roff[i + 1]) for i in perm]
    assert np.array_equal(np.diff(got["round_offsets"].astype(np.int64)), np.array([len(r) for r in rounds]))
    assert np.array_equal(tc.bits(got["round_xyz"]), tc.bits(want["round_xyz"][np.concatenate(rounds).astype(np.int64)]))


def test_refused_input(ctx):
    args, kw = tc.case_call("items_1")

    def call(i=None, value=None, **opts):
        a = list(args)
        if i is not None:
            a[i] = value
        return ctx.triangulate_observations(*a, **{**kw, **opts})
    for bad in (lambda: call(0, [11]), lambda: call(0, [-1]), lambda: call(2, np.full(len(args[2]), 7, np.uint32)),
                lambda: call(6, np.full(len(args[6]), 1000, np.uint32)), lambda: call(create_max_angle_error=0.0),
                lambda: call(create_max_angle_error=float("nan")), lambda: call(continue_max_angle_error=-1.0),
                lambda: call(min_angle=-0.5)):
        with pytest.raises(_capi.AmcError) as e:
            bad()
        assert e.value.code == _capi.AMC_E_INVALID and "amc_triangulate_observations" in str(e.value)
    empty_item = list(args)
    empty_item[5] = np.array([0, 0, len(args[6])], np.uint64)
    with pytest.raises(_capi.AmcError, match="no candidate"):
        ctx.triangulate_observations(*empty_item, **kw)
    n = 4097
    long_item = [args[0], args[1], args[2], args[3], args[4], np.array([0, n], np.uint64), np.zeros(n, np.uint32), np.zeros((n, 2)),
                 np.zeros(n, np.uint8), np.zeros((n, 3))]
    with pytest.raises(_capi.AmcError, match="more than 4096"):
        ctx.triangulate_observations(*long_item)
    _assert_same(call(), tc.reference("items_1"), "after the refusals")


# ---- through Python ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tc.SCENES))
def test_triangulate_image_equals_sequential_reference(name, golden):
    """every image of a scene in id order against the reference's sequential result applied to the model; transitive_2
    has overlapping walks that force a cut"""
    import pycolmap_amd as pc
    sc, opts = tc.scene_case(name)
    counts, points, ids, modified, _ = tc.scene_reference(name)
    r, g = tc.reconstruction(sc)
    t = pc.IncrementalTriangulator(g, r)
    calls = 0
    for k, iid in enumerate(sc["images"]):
        assert t.triangulate_image(opts, iid) == counts[k], (name, iid)
        st = pc.last_run_stats()
        assert st["call"] == "triangulate_image" and st["device_ms"] >= st["kernel_ms"] >= 0
        calls = max(calls, st["num_device_calls"])
    got = tc.reconstruction_points(r)
    assert list(got) == list(points)
    for pid in points:
        assert np.array_equal(tc.bits(got[pid][0]), tc.bits(points[pid][0])) and got[pid][1:] == points[pid][1:], pid
    for iid, im in r.images.items():
        assert [p.point3D_id for p in im.points2D] == [int(v) for v in ids[iid]]
    assert t.get_modified_points3D() == modified
    assert tc.scene_digest(counts, got) == str(golden[f"scene/{name}/digest"])
    assert (calls > 1) == (opts.get("max_transitivity", 1) > 1)


def test_chain_triangulate_adjust_filter_keeps_the_planted_points():
    """triangulate all images, bundle_adjustment with the poses fixed, filter_all_points3D: on a scene with planted wrong
    matches the planted points and only they remain, each with a subset of its planted track"""
    import pycolmap_amd as pc
    sc = tc.scene(seed=33, nimg=12, npts=25, models=(2,), noise=0.3, wrong=3, views=(5, 12))
    r, g = tc.reconstruction(sc)
    t = pc.IncrementalTriangulator(g, r)
    for iid in sc["images"]:
        t.triangulate_image({}, iid)
    assert len(r.points3D) >= 25
    pc.bundle_adjustment(r, dict(refine_extrinsics=False, refine_focal_length=False, refine_extra_params=False))
    r.filter_all_points3D(4.0, 1.5)
    planted = {j: set(tr) for j, tr in sc["planted"].items()}
    found = set()
    for p in r.points3D.values():
        track = {(e.image_id, e.point2D_idx) for e in p.track.elements}
        owners = [j for j, tr in planted.items() if track <= tr]
        assert len(owners) == 1, sorted(track)  # only planted observations, all of one point
        assert owners[0] not in found
        found.add(owners[0])
        np.testing.assert_allclose(np.array(p.xyz), sc["xyz"][owners[0]], atol=0.02)
    assert found == set(planted)


def test_image_without_points2D_and_image_without_correspondences():
    tc.check_empty_images(lambda t, o, iid: t.triangulate_image(o, iid))
