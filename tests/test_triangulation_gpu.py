"""Track triangulation on the GPU (libamc.so's amc_triangulate_tracks, pycolmap_amd.estimate_triangulation) against
its CPU reference (tests/tri_ref/tri_ref.cc): xyz bits, masks, trial and inlier counts and success identical over
clean, noisy and outlier tracks, short and long tracks, every option, degenerate input, batches in any order; and the
same over tri_cases.EDGE_CASES, also against their frozen digests, as one shuffled call, and in split calls."""
import numpy as np
import pytest

import tri_cases
import tri_ref_lib as ref

pytestmark = pytest.mark.gpu


def run_gpu(ctx, sc, **opts):
    return ctx.triangulate_tracks(sc["poses"], sc["offsets"], sc["obs_pose"], sc["obs_xy"], **opts)


def assert_same(got, want, what=""):
    xyz, ok, mask, st = got
    wxyz, wok, wmask, wst = want
    assert np.array_equal(ok, wok), f"{what}: success differs at {np.flatnonzero(ok != wok)[:10]}"
    assert np.array_equal(st["num_trials"], wst["num_trials"]), f"{what}: num_trials differ"
    assert np.array_equal(st["num_inliers"], wst["num_inliers"]), f"{what}: num_inliers differ"
    assert np.array_equal(mask, wmask), f"{what}: masks differ"
    bad = np.flatnonzero((xyz.view(np.uint64) != wxyz.view(np.uint64)).any(axis=1))
    assert bad.size == 0, f"{what}: xyz bits differ in tracks {bad[:10]}"


CASES = tri_cases.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_exact_to_reference(amc_ctx, name):
    sc, opts = CASES[name]
    got = run_gpu(amc_ctx, sc, **opts)
    assert_same(got, ref.triangulate(sc["poses"], sc["offsets"], sc["obs_pose"], sc["obs_xy"], **opts), name)
    if name in ("clean", "noisy", "outliers30"):
        assert got[1].mean() > 0.8
    if name == "long":
        assert (got[3]["num_trials"] >= 1000).all()
    assert got[3]["device_ms"] > 0 and got[3]["num_batches"] == 1


def test_batch_equals_per_track_calls_and_any_order(amc_ctx):
    sc = tri_cases.concat(tri_cases.scene(20, 60, outlier_frac=0.2, mean_len=6.0),
                          tri_cases.fixed_length(21, 1, 120, outlier_frac=0.3))
    opts = dict(max_error=tri_cases.TIGHT)
    xyz, ok, mask, st = run_gpu(amc_ctx, sc, **opts)
    off = sc["offsets"].astype(np.int64)
    T = len(off) - 1
    for t in range(T):
        sl = slice(off[t], off[t + 1])
        one = amc_ctx.triangulate_tracks(sc["poses"], [0, off[t + 1] - off[t]], sc["obs_pose"][sl], sc["obs_xy"][sl], **opts)
        assert np.array_equal(one[0].view(np.uint64), xyz[t:t + 1].view(np.uint64)) and one[1][0] == ok[t]
        assert np.array_equal(one[2], mask[sl]) and one[3]["num_trials"][0] == st["num_trials"][t]
    perm = np.random.default_rng(0).permutation(T)
    lens = np.diff(off)[perm]
    poff = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    idx = np.concatenate([np.arange(off[t], off[t + 1]) for t in perm])
    pxyz, pok, pmask, pst = amc_ctx.triangulate_tracks(sc["poses"], poff, sc["obs_pose"][idx], sc["obs_xy"][idx], **opts)
    assert np.array_equal(pxyz.view(np.uint64), xyz[perm].view(np.uint64)) and np.array_equal(pok, ok[perm])
    assert np.array_equal(pmask, mask[idx]) and np.array_equal(pst["num_trials"], st["num_trials"][perm])


def test_two_runs_agree(amc_ctx):
    sc, opts = CASES["outliers30"]
    a, b = run_gpu(amc_ctx, sc, **opts), run_gpu(amc_ctx, sc, **opts)
    assert_same(a, b, "run 2 vs run 1")


def test_empty_batch_and_short_tracks(amc_ctx):
    sc = tri_cases.scene(30, 3)
    xyz, ok, mask, st = amc_ctx.triangulate_tracks(sc["poses"], [0], [], np.zeros((0, 2)))
    assert xyz.shape == (0, 3) and ok.shape == (0,) and mask.shape == (0,)
    # tracks of 0 and 1 observations fail with 0 trials, beside a normal one
    xy = sc["obs_xy"][:int(sc["offsets"][1])]
    n = len(xy)
    off = np.array([0, 0, 1, 1 + n], np.uint64)
    got = amc_ctx.triangulate_tracks(sc["poses"], off, np.concatenate([[0], sc["obs_pose"][:n]]),
                                     np.concatenate([xy[:1], xy]))
    assert list(got[1][:2]) == [False, False] and list(got[3]["num_trials"][:2]) == [0, 0]
    assert_same(got, ref.triangulate(sc["poses"], off, np.concatenate([[0], sc["obs_pose"][:n]]), np.concatenate([xy[:1], xy])))


def test_bad_arguments_are_value_errors(amc_ctx):
    import pycolmap_amd._capi as capi
    sc = tri_cases.scene(31, 4)
    with pytest.raises(capi.AmcError):  # pose index out of range
        amc_ctx.triangulate_tracks(sc["poses"][:1], sc["offsets"], sc["obs_pose"] + 5, sc["obs_xy"])
    with pytest.raises(capi.AmcError):
        amc_ctx.triangulate_tracks(sc["poses"], sc["offsets"], sc["obs_pose"], sc["obs_xy"], max_error=0.0)


def _pycolmap_call(pycolmap, sc, t, opts=None):
    off = sc["offsets"].astype(np.int64)
    sl = slice(off[t], off[t + 1])
    pts = [pycolmap.PointData(xy * tri_cases.F + 500.0, xy) for xy in sc["obs_xy"][sl]]
    images, cameras = [], []
    for p in sc["obs_pose"][sl]:
        P = sc["poses"][p]
        images.append(pycolmap.Image(cam_from_world=pycolmap.Rigid3d(P)))
        cameras.append(pycolmap.Camera(model="SIMPLE_PINHOLE", width=1000, height=1000, params=[tri_cases.F, 500.0, 500.0]))
    if opts is None:
        return pycolmap.estimate_triangulation(pts, images, cameras)
    return pycolmap.estimate_triangulation(pts, images, cameras, opions=opts)


def test_pycolmap_estimate_triangulation_matches_reference():
    import pycolmap
    sc = tri_cases.concat(tri_cases.scene(40, 40, outlier_frac=0.2), tri_cases.degenerate(41))
    # the reference gets the [R | t] that Rigid3d(P) round-trips through its quaternion
    Rt = np.stack([pycolmap.Rigid3d(P).matrix() for P in sc["poses"]])
    for opts, kw in ((None, {}), (pycolmap.EstimateTriangulationOptions(min_tri_angle=0.05, ransac={"max_error": tri_cases.TIGHT}),
                                  dict(min_tri_angle=0.05, max_error=tri_cases.TIGHT))):
        want = ref.triangulate(Rt, sc["offsets"], sc["obs_pose"], sc["obs_xy"], **kw)
        off = sc["offsets"].astype(np.int64)
        nones = 0
        for t in range(len(off) - 1):
            r = _pycolmap_call(pycolmap, sc, t, opts)
            if not want[1][t]:
                assert r is None
                nones += 1
                continue
            assert set(r) == {"xyz", "inliers"} and r["inliers"].dtype == bool
            assert np.array_equal(np.asarray(r["xyz"]).view(np.uint64), want[0][t].view(np.uint64))
            assert np.array_equal(r["inliers"], want[2][off[t]:off[t + 1]])
        assert nones >= 1


# ---- the edge cases (tri_cases.EDGE_CASES) -------------------------------------------------------------
EDGES = tri_cases.EDGE_CASES
_REFS = {}


def reference(name):
    """the live reference on a case of EDGES or CASES, computed once and shared"""
    if name not in _REFS:
        sc, opts = EDGES[name] if name in EDGES else CASES[name]
        _REFS[name] = ref.triangulate(sc["poses"], sc["offsets"], sc["obs_pose"], sc["obs_xy"], **opts)
    return _REFS[name]


@pytest.fixture(scope="module")
def golden_edges():
    import importlib.util
    from pathlib import Path
    spec = importlib.util.spec_from_file_location("mk_tri", Path(__file__).resolve().parent / "golden" / "make_tri_ref_golden.py")
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk.load_edges()


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_case_bit_exact_to_reference_and_fixture(amc_ctx, name, golden_edges):
    sc, opts = EDGES[name]
    got = run_gpu(amc_ctx, sc, **opts)
    assert_same(got, reference(name), name)
    assert tri_cases.digest(got) == golden_edges[name], name
    assert got[3]["num_batches"] == 1


def _option_groups():
    groups = {}
    for name in sorted(EDGES):
        groups.setdefault(tuple(sorted(EDGES[name][1].items())), []).append(name)
    return [names for names in groups.values() if len(names) > 1]


def test_edge_cases_in_one_call_in_any_order(amc_ctx):
    """the edge cases that share options as one call, tracks shuffled: every track as in its own case's call"""
    groups = _option_groups()
    assert len(groups) >= 8 and max(len(g) for g in groups) >= 20
    for gi, names in enumerate(groups):
        both = tri_cases.concat(*[EDGES[n][0] for n in names])
        want = [reference(n) for n in names]
        T = len(both["offsets"]) - 1
        perm = np.random.default_rng(1000 + gi).permutation(T)
        off = both["offsets"].astype(np.int64)
        idx = np.concatenate([np.arange(off[t], off[t + 1]) for t in perm] + [np.zeros(0, np.int64)])
        xyz, ok, mask, st = run_gpu(amc_ctx, tri_cases.reorder(both, perm), **EDGES[names[0]][1])
        wst = {k: np.concatenate([w[3][k] for w in want])[perm] for k in ("num_inliers", "num_trials")}
        assert_same((xyz, ok, mask, st), (np.concatenate([w[0] for w in want])[perm], np.concatenate([w[1] for w in want])[perm],
                                          np.concatenate([w[2] for w in want])[idx], wst), f"{names[0]} .. {names[-1]}")


def _num_batches(offsets, max_tracks, max_obs):
    """split_batches' rule: greedily, at most max_tracks tracks and max_obs observations; a longer track alone"""
    off, T, i, count = [int(o) for o in offsets], len(offsets) - 1, 0, 0
    while i < T:
        j = i + 1
        while j < T and j - i < max_tracks and off[j + 1] - off[i] <= max_obs:
            j += 1
        i, count = j, count + 1
    return count


@pytest.mark.parametrize("hook,bound", [("AMC_TRI_BATCH_TRACKS", 1), ("AMC_TRI_BATCH_TRACKS", 64), ("AMC_TRI_BATCH_TRACKS", 65),
                                        ("AMC_TRI_BATCH_OBS", 1), ("AMC_TRI_BATCH_OBS", 129)])
@pytest.mark.parametrize("name", ["len_bins", "mixed_wave", "outliers30"])
def test_split_calls_equal_the_reference(amc_ctx, monkeypatch, name, hook, bound):
    """a call split into device batches that reuse one set of buffers (the hooks are read per call)"""
    sc, opts = EDGES[name] if name in EDGES else CASES[name]
    monkeypatch.setenv(hook, str(bound))
    got = run_gpu(amc_ctx, sc, **opts)
    assert_same(got, reference(name), f"{name} {hook}={bound}")
    lens = np.diff(sc["offsets"].astype(np.int64))
    want = _num_batches(sc["offsets"], bound if hook.endswith("TRACKS") else 1 << 20, bound if hook.endswith("OBS") else 1 << 23)
    assert got[3]["num_batches"] == want
    assert (want > 1) == (hook.endswith("OBS") or len(lens) > bound)
    if (hook, bound) == ("AMC_TRI_BATCH_TRACKS", 1):
        assert want == len(lens)
    if (hook, bound) == ("AMC_TRI_BATCH_OBS", 1):  # every track of two or more observations is a batch of its own
        assert int((lens >= 2).sum()) <= want <= int((lens >= 1).sum()) + 1
