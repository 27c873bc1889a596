"""retriangulate without a GPU: the surface, the round colouring against a brute-force
restatement, the host half with the flat reference in the library's place against the literal sequential loop, the
reference against an independent Python restatement, answers worked out by hand, the fixture, and the host half in a
stand-alone program under ASan + UBSan."""
import copy
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pycolmap
import pycolmap_amd as pc
import retri_cases as k
import retri_ref_lib as ref
import tracks_cases as trc
import triangulator_cases as tc
from pycolmap_amd import _capi
from pycolmap_amd import _pycolmap as P

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "retri_ref_v1.npz"


def retri_with(t, opts, solver=k.reference_solver):
    return P._retriangulate_with(t, opts, solver)


def both_ways(st, calls=1, **opts):
    """retriangulate by the literal sequential loop and by the host half with the flat reference in the library's place,
    `calls` times over: they must agree after every call.  Returns (counts, the reference scene, the Reconstruction, the
    triangulator, the stats of the last call)."""
    rs = k.ref_scene(st)
    r, _, t = trc.reconstruction(st)
    counts = []
    for _ in range(calls):
        want = rs.retriangulate(**opts)
        got = retri_with(t, opts)
        assert got == want
        assert k.same_model(r, rs.points(), {i: rs.point2D_ids(i, len(im[3])) for i, im in st["images"].items()})
        assert t.get_modified_points3D() == rs.modified()
        assert P._retriangulate_trials(t) == rs.trials()
        counts.append(got)
    return counts, rs, r, t, pc.last_run_stats()


# ---- the surface --------------------------------------------------------------------------------------------------------------
def test_function_exists_on_both_packages_and_not_on_the_class():
    assert callable(pc.retriangulate) and pycolmap.retriangulate is pc.retriangulate
    assert "retriangulate" in pycolmap._PUBLIC and not hasattr(pc.IncrementalTriangulator, "retriangulate")
    assert "DESIGN.md section 19" in pc.retriangulate.__doc__ and "retriangulate" in pycolmap.__doc__
    for name in ("complete_image", "triangulate_points", "incremental_mapping"):
        with pytest.raises(AttributeError, match="outside pycolmap_amd's scope"):
            getattr(pycolmap, name)
    with pytest.raises(AttributeError, match="track completion and merging"):
        pycolmap.complete_image


def test_header_symbols_and_structs():
    lib = _capi.load()
    text = (ROOT / "include" / "amc_retri.h").read_text()
    for name in ("amc_retri_opts_default", "amc_retriangulate_pairs", "amc_retri_result_free"):
        assert hasattr(lib, name) and name in _capi.EXPORTED_SYMBOLS and name in text
    assert lib.amc_abi_version() == 5
    o = _capi.RetriOpts()
    lib.amc_retri_opts_default(ctypes.byref(o))
    assert (o.create_max_angle_error, o.re_max_angle_error, o.min_angle, o.re_min_ratio) == (2.0, 5.0, 1.5, 0.2)
    assert ctypes.sizeof(_capi.RetriOpts) == 4 * 8 and ctypes.sizeof(_capi.RetriProblem) == 20 * 8
    assert ctypes.sizeof(_capi.RetriResult) == 5 * 8 + 5 * 8 + 8 + 5 * 8
    for s in (_capi.RetriOpts, _capi.RetriProblem, _capi.RetriResult):
        for field, _ in s._fields_:
            assert field in text, field
    assert "AMC_RETRI_MAX_CORRS ((uint64_t)1 << 24)" in text and _capi.RETRI_MAX_CORRS == 1 << 24
    for name, value in (("NONE", 0), ("CONTINUE_1TO2", 1), ("CONTINUE_2TO1", 2), ("CREATED", 3)):
        assert f"AMC_RETRI_{name} {value}" in text and getattr(_capi, f"RETRI_{name}") == value == getattr(ref, name)
    assert "retri.hip" in (ROOT / "pycolmap_amd" / "build.py").read_text()


GOOD = np.array([[0.4, -0.2, 0.1], [-0.1, 0.4, 0.25], [0.2, -0.1, 0.35], [0.15, 0.1, -0.3], [-0.25, 0.2, 0.15]])


def world(nimg, phys, views, tracks, **kw):
    """trc.world with every pixel a fixed fraction of a pixel off its projection: at an exact pixel the cosine of the
    angular error can round above 1, whose acos is NaN, and NaN passes no test (17.2)"""
    offsets = {(p, i): (0.1 + 0.2 * ((p + i) % 3 - 1), 0.15 * ((p + 2 * i) % 3 - 1) - 0.05) for p in views for i in views[p]}
    return trc.world(nimg, phys, views, tracks, offsets=offsets, **kw)


def _small_world():
    return world(3, GOOD[:2], {0: [1, 2, 3], 1: [1, 2, 3]}, [])


def test_option_checks_and_bad_arguments():
    r, g, t = trc.reconstruction(_small_world())
    for bad, what in ((dict(re_max_angle_error=0.0), "re_max_angle_error > 0"), (dict(re_min_ratio=-0.1), "re_min_ratio >= 0"),
                      (dict(re_min_ratio=1.5), "re_min_ratio <= 1"), (dict(re_max_trials=-1), "re_max_trials >= 0"),
                      (dict(create_max_angle_error=float("nan")), "create_max_angle_error > 0"), (dict(min_angle=0.0), "min_angle > 0")):
        for call in (lambda o: retri_with(t, o), lambda o: pc.retriangulate(t, o)):
            with pytest.raises(ValueError, match="Check Failed: " + what):
                call(bad)
    with pytest.raises(TypeError):
        pc.retriangulate(r, {})  # not a triangulator
    with pytest.raises(ValueError, match="shape"):
        retri_with(t, {}, lambda d: dict(pair_ran=[1], corr_action=[0], created_offsets=[0, 0], created_xyz=[]))
    # a result that does not fit the problem: nothing of the model, the modified set or the counters changes
    for bad in (lambda d, res: res["corr_action"].__setitem__(0, 7),
                lambda d, res: res["corr_action"].__setitem__(0, ref.CONTINUE_1TO2),
                lambda d, res: res.__setitem__("created_offsets", np.zeros_like(res["created_offsets"]))):
        def solver(d, bad=bad):
            res = k.reference_solver(d)
            res["corr_action"] = res["corr_action"].copy()
            bad(d, res)
            res["created_xyz"] = np.zeros((int(res["created_offsets"][-1]), 3))
            return res
        with pytest.raises(ValueError, match="retriangulate: the result"):
            retri_with(t, dict(ignore_two_view_tracks=False), solver)
        assert len(r.points3D) == 0 and t.get_modified_points3D() == set() and P._retriangulate_trials(t) == {}
    # (1, 2) creates two points, (1, 3) continues both into image 3, and (2, 3) is no longer under-reconstructed
    assert retri_with(t, dict(ignore_two_view_tracks=False)) == 6
    assert P._retriangulate_trials(t) == {(1, 2): 1, (1, 3): 1}


def test_without_a_gpu_the_function_raises_and_leaves_the_model():
    if _capi.device_count() > 0:
        pytest.skip("a GPU is visible; this test covers the CPU-only container")
    st, opts = k.scene_state("direct")
    r, _, t = trc.reconstruction(st)
    before, ids = trc.recon_points(r), trc.recon_point2D_ids(r)
    with pytest.raises(_capi.AmcError):
        pc.retriangulate(t, opts)
    assert trc.same_points(trc.recon_points(r), before) and trc.same_point2D_ids(trc.recon_point2D_ids(r), ids)
    assert t.get_modified_points3D() == set() and P._retriangulate_trials(t) == {}


# ---- 19.3: the colouring -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_round_colouring_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    nimg = int(rng.integers(2, 14))
    every = [(a, b) for a in range(1, nimg + 1) for b in range(a + 1, nimg + 1)]
    pairs = [p for p in every if rng.random() < (0.2, 0.5, 1.0)[seed % 3]]  # ascending pair id, as the host takes them
    got = P._retriangulate_rounds(pairs)
    assert got == k.brute_colour(pairs) == ref.colour(pairs).tolist() == P._retriangulate_rounds(list(pairs))
    for r in set(got):
        images = [i for p, q in zip(pairs, got) if q == r for i in p]
        assert len(images) == len(set(images))  # a round's pairs share no image
    for i, (p, r) in enumerate(zip(pairs, got)):  # every lower round is blocked by an earlier pair
        for lower in range(r):
            assert any(got[j] == lower and set(pairs[j]) & set(p) for j in range(i))
    # the order is by the list given, not by the ids: the reversed list is coloured from its own front
    assert P._retriangulate_rounds(pairs[::-1]) == k.brute_colour(pairs[::-1])


# ---- whole scenes ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", k.SCENES)
def test_host_half_with_reference_in_the_librarys_place(name, golden):
    st, opts = k.scene_state(name)
    calls, _ = k.scene_reference(name)
    counts, rs, r, t, stats = both_ways(st, calls=2, **opts)
    assert counts == [c[0] for c in calls] and counts[0] > 0  # the cut left work
    assert stats["call"] == "retriangulate" and stats["num_device_calls"] == 0
    assert k.state_digest(calls[1][0], calls[1][1], calls[1][4]) == str(golden[f"scene/{name}/digest"])
    if name == "bogus_camera":  # the pairs of the bogus camera's images spend trials and change nothing
        bogus = {i for i, im in st["images"].items() if tc.bogus(st["cameras"][im[0]], dict(zip(ref.OPTION_FIELDS, ref.OPTION_DEFAULTS)))}
        assert bogus and any(set(p) & bogus for p in calls[0][4])


def test_copies_carry_the_trial_counters():
    st, opts = k.scene_state("direct")
    _, _, t = trc.reconstruction(st)
    retri_with(t, opts)
    trials = P._retriangulate_trials(t)
    assert trials and P._retriangulate_trials(copy.copy(t)) == trials and P._retriangulate_trials(copy.deepcopy(t)) == trials
    u = copy.deepcopy(t)
    retri_with(u, opts)
    assert P._retriangulate_trials(t) == trials  # the copy's counters are its own


# left out: the two cases that put Continue's angle on the threshold and one double above it, on purpose
RESTATED = [n for n in sorted(k.ALL_CASES) if n not in ("continue_at_threshold", "continue_above_threshold")]
RATIO_AT_THRESHOLD = ("ratio_0", "ratio_fifth_skipped", "ratio_fifth_runs")


@pytest.mark.parametrize("name", RESTATED)
def test_reference_equals_python_restatement(name):
    args, kw = k.case_call(name)
    res = k.reference(name)
    # 18.6's margin: no deciding angle or ratio within 1e-9 relative of its threshold; only the cases that put a ratio on
    # or next to the threshold on purpose are let through (the ratio is one IEEE division of two integers on both sides)
    assert res["margins"][0] > 1e-9 and res["margins"][1] > 1e-9
    assert res["margins"][2] > 1e-9 or name in RATIO_AT_THRESHOLD
    assert k.same(res, k.py_retriangulate_pairs(args, kw))


def test_reference_reproduces_fixture(golden):
    assert sorted(golden["cases"].tolist()) == sorted(k.ALL_CASES) and sorted(golden["scenes"].tolist()) == sorted(k.SCENES)
    for name in sorted(k.ALL_CASES):
        res = k.reference(name)
        assert k.digest(res) == str(golden[f"{name}/digest"]), name
        for key in k.RESULT_KEYS:
            if f"{name}/{key}" in golden:
                a, b = np.asarray(res[key]), golden[f"{name}/{key}"]
                assert np.array_equal(k.bits(a), k.bits(b)) if a.dtype == np.float64 else np.array_equal(a, b), (name, key)
    # what the flat cases are for
    for name, tri, ran in (("filled_pair_skipped", [0, 0, 6], [True, True, False]), ("filled_pair_runs", [0, 0, 1], [True, True, True])):
        res = k.reference(name)  # the last pair's ratio is taken on what the earlier rounds left, not on the uploaded state
        assert k.initial_num_tri(k.case_call(name)[0]) == [0, 0, 0] and res["pair_num_tri"].tolist() == tri and res["pair_ran"].tolist() == ran
        assert f"{name}/pair_num_tri" in golden
    assert k.reference("filled_pair_skipped")["corr_action"].tolist() == [ref.CONTINUE_1TO2] * 12 + [ref.NONE] * 6
    assert k.reference("filled_pair_runs")["corr_action"].tolist() == [ref.CONTINUE_1TO2] * 2 + [ref.NONE] + [ref.CREATED] * 5
    acts = set(k.reference("mixed")["corr_action"].tolist())
    assert acts == {ref.NONE, ref.CONTINUE_1TO2, ref.CONTINUE_2TO1, ref.CREATED}
    assert 0 < k.reference("rounds_65")["pair_ran"].sum() < 65  # pairs that ran and pairs the ratio test stopped
    assert [len(k.case_call("sizes")[0][11][int(a):int(b)]) for a, b in zip(k.case_call("sizes")[0][10][:-1], k.case_call("sizes")[0][10][1:])] == [0, 1, 63, 64, 65, 257]
    assert k.reference("sizes")["pair_ran"][0]  # 0 / 0 is not >= re_min_ratio: the empty pair runs, on nothing
    assert len(k.case_call("rounds_65")[0][12]) == 66 and len(k.case_call("pairs_257")[0][9]) == 257


# ---- answers by hand -----------------------------------------------------------------------------------------------------------
def test_a_ratio_of_exactly_one_fifth_is_skipped_and_runs_at_the_next_double():
    skipped, runs = k.reference("ratio_fifth_skipped"), k.reference("ratio_fifth_runs")
    assert skipped["pair_num_tri"].tolist() == [1] and not skipped["pair_ran"][0] and not skipped["corr_action"].any()
    assert runs["pair_num_tri"].tolist() == [1] and runs["pair_ran"][0]
    assert runs["corr_action"].tolist() == [ref.NONE] + [ref.CREATED] * 4
    assert np.float64(1) / np.float64(5) == 0.2 < k.case_call("ratio_fifth_runs")[1]["re_min_ratio"]


def test_an_angle_exactly_at_re_max_angle_error_continues_and_one_double_above_does_not():
    assert k.reference("continue_at_threshold")["corr_action"].tolist() == [ref.CONTINUE_1TO2]
    assert k.reference("continue_above_threshold")["corr_action"].tolist() == [ref.NONE]
    assert k.reference("continue_at_threshold")["margins"][0] == 0.0


def test_create_uses_create_max_angle_error_not_re_max_angle_error():
    args, kw = k.case_call("between_thresholds_wide")
    wide, narrow = k.reference("between_thresholds_wide"), k.reference("between_thresholds")
    assert narrow["corr_action"].tolist() == [ref.NONE] and narrow["pair_ran"][0]
    assert wide["corr_action"].tolist() == [ref.CREATED]
    a = dict(zip(k.ARG_NAMES, args))
    for o in (0, 1):  # each observation's error under the point lies between the two defaults
        nxy = ref.lift(a["camera_models"][0], a["camera_params"][0], [a["obs_xy"][o]])[0]
        e = tc.np_angular_error(nxy, tc.pose_matrix(a["qvec"][a["obs_image"][o]], a["tvec"][a["obs_image"][o]]), wide["created_xyz"][0])
        assert 2.0 * k.DEG < e < 5.0 * k.DEG


def _tracked_world():
    """five points seen by images 1 to 4, each with the model point [(p, 1), (p, 4)]; correspondences among images 1, 2, 3"""
    phys = np.array([[0.1, 0.2, 0.3], [-0.3, 0.1, 0.0], [0.4, -0.2, 0.1], [0.0, 0.0, -0.4], [-0.2, -0.3, 0.2]])
    views = {p: [1, 2, 3, 4] for p in range(5)}
    edges = {p: [(1, 2), (1, 3), (2, 3)] for p in range(5)}
    return world(4, phys, views, [(phys[p], [(p, 1), (p, 4)]) for p in range(5)], edges=edges)


def test_a_pair_under_reconstructed_at_the_start_is_skipped_when_earlier_rounds_filled_it():
    st = _tracked_world()
    seen = []

    def solver(d):
        seen.append((d, k.reference_solver(d)))
        return seen[-1][1]
    r, _, t = trc.reconstruction(st)
    assert retri_with(t, {}, solver) == 10  # rounds 1 and 2 continue five observations each
    d, res = seen[0]
    assert d["pair_images"].tolist() == [[0, 1], [0, 2], [1, 2]] and d["round_offsets"].reshape(-1).tolist() == [0, 1, 2, 3]
    assert res["pair_ran"].tolist() == [True, True, False] and res["pair_num_tri"].tolist() == [0, 0, 5]
    assert res["corr_action"].tolist() == [ref.CONTINUE_1TO2] * 10 + [ref.NONE] * 5
    assert P._retriangulate_trials(t) == {(1, 2): 1, (1, 3): 1}  # the skipped pair spends nothing
    assert all(len(p.track.elements) == 4 for p in r.points3D.values()) and t.get_modified_points3D() == {1, 2, 3, 4, 5}
    st_ = pc.last_run_stats()
    assert (st_["num_pairs"], st_["num_pairs_run"], st_["num_rounds"], st_["num_correspondences"]) == (3, 2, 3, 15)
    assert (st_["num_continued_observations"], st_["num_created_points"]) == (10, 0)
    both_ways(st)


def test_a_continue_in_round_two_joins_a_point_created_in_round_one():
    st = world(3, GOOD[:1], {0: [1, 2, 3]}, [], edges={0: [(1, 2), (1, 3)]})
    counts, rs, r, t, stats = both_ways(st)
    assert counts == [3] and stats["num_rounds"] == 2 and stats["num_created_points"] == 1 and stats["num_continued_observations"] == 1
    (pid, p), = r.points3D.items()
    assert pid == 1 and [(e.image_id, e.point2D_idx) for e in p.track.elements] == [(1, 0), (2, 0), (3, 0)]
    assert np.allclose(p.xyz, GOOD[0], atol=1e-2)


def _wrong_world(**kw):
    """images 1 and 2 matched through two wrong correspondences only: nothing can be triangulated, the pair stays at ratio 0"""
    phys = [[0.5, 0.2, 0.3], [-0.5, 0.4, -0.3], [0.1, -0.6, 0.5]]
    return world(3, phys, {0: [1, 2, 3], 1: [1, 2, 3], 2: [1, 2, 3]}, [], edges={0: [], 1: [], 2: []},
                     extra=[((0, 1), (1, 2)), ((1, 1), (2, 2))], **kw)


@pytest.mark.parametrize("max_trials, want", [(0, [{}, {}]), (1, [{(1, 2): 1}, {(1, 2): 1}]), (2, [{(1, 2): 1}, {(1, 2): 2}])])
def test_re_max_trials_over_two_calls(max_trials, want):
    st = _wrong_world()
    r, _, t = trc.reconstruction(st)
    rs = k.ref_scene(st)
    runs = []
    for call in range(2):
        assert retri_with(t, dict(re_max_trials=max_trials)) == rs.retriangulate(re_max_trials=max_trials) == 0
        assert P._retriangulate_trials(t) == rs.trials() == want[call]
        runs.append(pc.last_run_stats()["num_pairs_run"])
    assert runs == [min(max_trials, 1), 1 if max_trials == 2 else 0] and len(r.points3D) == 0


def test_the_counter_is_spent_on_a_pair_with_a_bogus_camera():
    st = _wrong_world(bogus_images=(2,))
    counts, rs, r, t, stats = both_ways(st, calls=2)
    assert counts == [0, 0] and P._retriangulate_trials(t) == {(1, 2): 1} and stats["num_pairs"] == 0 and len(r.points3D) == 0


def test_points_on_both_sides_the_ratio_and_the_two_view_rule():
    phys = GOOD
    views = {p: [1, 2, 3] for p in range(5)}
    tracks = [(phys[0], [(0, 1), (0, 2)]), (phys[1], [(1, 1), (1, 3)]), (phys[1] + 1e-4, [(1, 2), (1, 3)])]
    # (point 3 takes (1, 3) from point 2: the world writes the later id; neither matters below)
    st = world(3, phys, views, tracks, edges={p: [(1, 2)] for p in range(5)})
    st["points"][2] = (st["points"][2][0], st["points"][2][1], st["points"][2][2], st["points"][2][3][:1])
    seen = []

    def solver(d):
        seen.append(k.reference_solver(d))
        return seen[-1]
    # tri_ratio is 1 / 5: the same point on both sides counts, two different points do not
    r, _, t = trc.reconstruction(st)
    assert retri_with(t, {}, solver) == 0 and seen[-1]["pair_num_tri"].tolist() == [1] and not seen[-1]["pair_ran"][0]
    assert P._retriangulate_trials(t) == {}
    # it runs under a larger re_min_ratio; every remaining correspondence is a two-view observation
    assert retri_with(t, dict(re_min_ratio=0.5), solver) == 0 and seen[-1]["pair_ran"][0] and not seen[-1]["corr_action"].any()
    assert P._retriangulate_trials(t) == {(1, 2): 1} and len(r.points3D) == 3
    # without the two-view rule the three free correspondences create points; the two with points stay as they are
    r, _, t = trc.reconstruction(st)
    assert retri_with(t, dict(re_min_ratio=0.5, ignore_two_view_tracks=False), solver) == 6
    assert seen[-1]["corr_action"].tolist() == [ref.NONE, ref.NONE, ref.CREATED, ref.CREATED, ref.CREATED]
    assert sorted(r.points3D) == [1, 2, 3, 4, 5, 6] and t.get_modified_points3D() == {4, 5, 6}
    both_ways(st, re_min_ratio=0.5, ignore_two_view_tracks=False)


def test_an_image_outside_the_model_and_a_graph_without_pairs():
    st = _tracked_world()
    st["graph_images"][9] = 3
    st["matches"].append((1, 9, np.array([[0, 0], [1, 1]], np.uint32)))
    st["matches"].append((9, 2, np.array([[2, 2]], np.uint32)))
    counts, rs, r, t, stats = both_ways(st)
    assert counts == [10] and stats["num_pairs"] == 3 and all(9 not in p for p in P._retriangulate_trials(t))
    st = _tracked_world()
    st["matches"] = []
    rr, g, t = trc.reconstruction(st, finalize=False)
    assert g.num_image_pairs() == 0 and pc.retriangulate(t, {}) == 0  # no device call is made: this runs anywhere
    stats = pc.last_run_stats()
    assert stats["call"] == "retriangulate" and stats["num_pairs"] == stats["num_rounds"] == stats["num_device_calls"] == 0
    assert len(rr.points3D) == 5 and P._retriangulate_trials(t) == {}


def test_a_call_above_the_bound_is_refused_by_name_and_leaves_the_model():
    st, opts = k.scene_state("direct")
    r, _, t = trc.reconstruction(st)
    t.add_modified_point3D(2)
    before, ids = trc.recon_points(r), trc.recon_point2D_ids(r)
    seen = []

    def solver(d):
        seen.append(len(d["corr_obs"]))
        return k.reference_solver(d)
    u = copy.deepcopy(t)
    retri_with(u, opts, solver)  # the size of the call, on a copy
    n = seen.pop()
    assert n > 1 and not seen
    with pytest.raises(ValueError, match=f"hold {n} correspondences, more than {n - 1} "):
        P._retriangulate_with(t, opts, solver, max_correspondences=n - 1)
    assert not seen  # refused before anything is sent
    assert trc.same_points(trc.recon_points(r), before) and trc.same_point2D_ids(trc.recon_point2D_ids(r), ids)
    assert t.get_modified_points3D() == {2} and P._retriangulate_trials(t) == {}
    assert P._retriangulate_with(t, opts, solver, max_correspondences=n) == k.scene_reference("direct")[0][0][0] and seen == [n]


def test_host_half_under_asan(tmp_path):
    """The host half (csrc/host/retriangulate_host.h, csrc/retri_plan.h) in a stand-alone program under ASan + UBSan
    (tests/shim/retriangulate_host_fuzz.cc)."""
    import os
    import shutil
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    flags = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined"]
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("sanitizer runtime not installed")
    exe = tmp_path / "retriangulate_host_fuzz"
    b = subprocess.run(flags + [str(ROOT / "tests" / "shim" / "retriangulate_host_fuzz.cc"),
                                str(ROOT / "pycolmap_amd" / "csrc" / "host" / "model_io.cc"),
                                str(ROOT / "pycolmap_amd" / "csrc" / "host" / "reconstruction.cc"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[1]) >= 1000
