"""CPU checks of the incremental triangulator: the surface of CorrespondenceGraph, Correspondence,
IncrementalTriangulatorOptions and IncrementalTriangulator; the graph and the reference's graph against a brute-force
restatement; the sequential reference (tests/triangulator_ref) against an independent Python restatement, hand-built
answers and the frozen fixture; the host half of triangulate_image (Find, the cut into runs, the write-back) with the
reference in the library's place; and the same host half in a stand-alone program under ASan + UBSan."""
import copy
import ctypes
import pickle
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pycolmap_amd as pc
import triangulator_cases as tc
import triangulator_ref_lib as ref
from pycolmap_amd import _capi

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "triangulator_ref_v1.npz"
NOT_DEFINED = ("complete_image", "complete_tracks", "complete_all_tracks", "merge_tracks", "merge_all_tracks", "retriangulate")


# ---- the surface -------------------------------------------------------------------------------------------------------------
def test_options_defaults_protocol_and_checks():
    o = pc.IncrementalTriangulatorOptions()
    assert o.todict() == dict(zip(ref.OPTION_FIELDS, ref.OPTION_DEFAULTS))
    assert isinstance(o.max_transitivity, int) and isinstance(o.ignore_two_view_tracks, bool)
    o2 = pc.IncrementalTriangulatorOptions(max_transitivity=3, min_angle=2.5)
    assert (o2.max_transitivity, o2.min_angle, o2.create_max_angle_error) == (3, 2.5, 2.0)
    o3 = pc.IncrementalTriangulatorOptions({"re_min_ratio": 0.5})
    o3.mergedict({"re_max_trials": 4})
    assert (o3.re_min_ratio, o3.re_max_trials) == (0.5, 4)
    assert pickle.loads(pickle.dumps(o2)).todict() == o2.todict()
    assert copy.deepcopy(o2).todict() == o2.todict() and copy.copy(o3).todict() == o3.todict()
    assert "max_transitivity" in o.summary() and "IncrementalTriangulatorOptions" in repr(o)
    with pytest.raises((TypeError, ValueError, AttributeError)):
        pc.IncrementalTriangulatorOptions(no_such_field=1)
    sc = tc.scene(seed=1, nimg=4, npts=3, views=(4, 4), wrong=0)
    r, g = tc.reconstruction(sc)
    t = pc.IncrementalTriangulator(g, r)
    for bad in (dict(max_transitivity=-1), dict(create_max_angle_error=0.0), dict(continue_max_angle_error=-1.0),
                dict(re_min_ratio=1.5), dict(min_angle=0.0), dict(min_angle=float("nan"))):
        with pytest.raises(ValueError, match="Check Failed"):
            t.triangulate_image(bad, 1)
    assert len(r.points3D) == 0


def test_classes_reprs_copies_and_absent_methods():
    import pycolmap
    for name in ("Correspondence", "CorrespondenceGraph", "IncrementalTriangulator", "IncrementalTriangulatorOptions"):
        assert getattr(pycolmap, name) is getattr(pc, name)
    c = pc.Correspondence(3, 7)
    assert (c.image_id, c.point2D_idx) == (3, 7) and repr(c) == "Correspondence(image_id=3, point2D_idx=7)"
    d = copy.deepcopy(c)
    d.image_id = 4
    assert c.image_id == 3 and copy.copy(c).point2D_idx == 7
    assert pc.Correspondence().image_id == 0xFFFFFFFF
    g = pc.CorrespondenceGraph()
    assert repr(g) == "CorrespondenceGraph(num_images=0, num_image_pairs=0)"
    g.add_image(1, 3)
    g.add_image(2, 3)
    g.add_correspondences(1, 2, np.array([[0, 1]], np.uint32))
    h = copy.deepcopy(g)
    h.add_correspondences(1, 2, np.array([[1, 2]], np.uint32))
    assert g.num_correspondences_between_images(1, 2) == 1 and h.num_correspondences_between_images(1, 2) == 2
    assert copy.copy(g).num_images() == 2
    r = pc.Reconstruction()
    t = pc.IncrementalTriangulator(g, r)
    assert t.correspondence_graph is g and t.reconstruction is r
    assert repr(t) == "IncrementalTriangulator(num_images=0, num_points3D=0, num_modified_points3D=0)"
    t.add_modified_point3D(5)
    assert t.get_modified_points3D() == set()  # recorded, but the point does not exist
    assert "num_modified_points3D=1" in repr(t)
    t2, t3 = copy.copy(t), copy.deepcopy(t)
    assert t2.reconstruction is r and t3.reconstruction is not r and t3.correspondence_graph is not g
    t.clear_modified_points3D()
    assert "num_modified_points3D=0" in repr(t) and "num_modified_points3D=1" in repr(t2)
    with pytest.raises(TypeError):
        pc.IncrementalTriangulator(r, g)
    for name in NOT_DEFINED:
        assert not hasattr(t, name), name
    for name in ("triangulate_points", "incremental_mapping"):
        with pytest.raises(AttributeError, match="outside pycolmap_amd's scope"):
            getattr(pycolmap, name)
    for name in ("add_observation", "merge_points3D", "transform"):
        assert not hasattr(r, name)


def test_header_symbols_and_structs():
    lib = _capi.load()
    for name in ("amc_triobs_opts_default", "amc_triangulate_observations", "amc_triobs_result_free"):
        assert hasattr(lib, name) and name in _capi.EXPORTED_SYMBOLS
    assert lib.amc_abi_version() == 5
    o = _capi.TriobsOpts()
    lib.amc_triobs_opts_default(ctypes.byref(o))
    assert (o.create_max_angle_error, o.continue_max_angle_error, o.min_angle) == (2.0, 2.0, 1.5)
    assert ctypes.sizeof(_capi.TriobsOpts) == 32 and ctypes.sizeof(_capi.TriobsProblem) == 14 * 8
    assert ctypes.sizeof(_capi.TriobsResult) == 4 * 8 + 4 * 8 + 8 + 5 * 8
    text = (ROOT / "include" / "amc_triobs.h").read_text()
    for field, _ in _capi.TriobsProblem._fields_ + _capi.TriobsResult._fields_ + _capi.TriobsOpts._fields_:
        assert field in text, field


def test_wrapper_refuses_inconsistent_arrays():
    args, kw = tc.case_call("items_1")
    bad = list(args)
    bad[7] = bad[7][:-1]
    with pytest.raises(ValueError, match="candidates"):
        _capi.triobs_inputs(*bad)
    bad = list(args)
    bad[5] = np.array([0, 3], np.uint64)
    with pytest.raises(ValueError, match="item_offsets ends"):
        _capi.triobs_inputs(*bad)
    with pytest.raises(ValueError, match="two-view flags"):
        _capi.triobs_inputs(*args, no_create_two_view=[1, 0])


# ---- the graph ---------------------------------------------------------------------------------------------------------------
def _random_lists(seed, nimg=6, npts=8, nlists=30):
    rng = np.random.default_rng(seed)
    images = {10 + 2 * i: npts for i in range(nimg)}
    images[99] = 5  # never matched: leaves at finalize
    lists = []
    ids = list(images)[:-1]
    for _ in range(nlists):
        a, b = (int(v) for v in rng.choice(ids, 2, replace=bool(rng.random() < 0.1)))
        m = rng.integers(0, npts + 2, (int(rng.integers(0, 7)), 2))  # two indices out of range
        if rng.random() < 0.3 and len(m):
            m = np.concatenate([m, m[:2]])  # duplicates in the same direction
        lists.append((a, b, m.astype(np.uint32)))
        if rng.random() < 0.2:
            lists.append((b, a, m[:, ::-1].astype(np.uint32)))  # and in the other
    return images, lists


def _graphs(seed, finalize=True):
    images, lists = _random_lists(seed)
    g, p = pc.CorrespondenceGraph(), tc.PyGraph()
    sc = dict(cameras={}, images={}, points={}, graph_images=images, matches=lists)
    for iid, n in images.items():
        g.add_image(iid, n)
        p.add_image(iid, n)
    for a, b, m in lists:
        g.add_correspondences(a, b, m)
        p.add_correspondences(a, b, m)
    if finalize:
        g.finalize()
        p.finalize()
    return images, g, p, tc.ref_scene(sc, finalize=finalize)


@pytest.mark.parametrize("seed", range(6))
def test_graph_equals_brute_force(seed):
    images, g, p, rs = _graphs(seed)
    assert g.num_images() == len(p.npts) == rs.num_images()
    assert not g.exists_image(99) and g.exists_image(10) and not rs.exists_image(99)
    assert g.num_image_pairs() == len(p.pairs)
    for iid in p.npts:
        assert g.num_observations_for_image(iid) == p.nobs[iid] == rs.image_counts(iid)[0] > 0
        assert g.num_correspondences_for_image(iid) == p.ncorr[iid] == rs.image_counts(iid)[1]
        for k in range(images[iid]):
            direct = p.direct(iid, k)
            assert [(c.image_id, c.point2D_idx) for c in g.extract_correspondences(iid, k)] == direct
            assert g.has_correspondences(iid, k) == bool(direct)
            assert len({c[0] for c in direct}) == len(direct)  # at most one correspondence per other image
            assert g.is_two_view_observation(iid, k) == p.is_two_view(iid, k) == rs.is_two_view(iid, k)
            for t in (0, 1, 2, 3, 5):
                want = p.transitive(iid, k, t)
                got = [(c.image_id, c.point2D_idx) for c in g.extract_transitive_correspondences(iid, k, t)]
                assert got == want == rs.transitive(iid, k, t), (iid, k, t)
    for (a, b), n in p.pairs.items():
        assert g.num_correspondences_between_images(a, b) == g.num_correspondences_between_images(b, a) == n == rs.pair_count(a, b)
        m = g.find_correspondences_between_images(a, b)
        assert m.dtype == np.uint32 and m.shape == (n, 2)
        assert sorted(map(tuple, m.tolist())) == sorted((k, c[1]) for k in range(images[a]) for c in p.corrs.get((a, k), []) if c[0] == b)
        assert sorted(map(tuple, g.find_correspondences_between_images(b, a)[:, ::-1].tolist())) == sorted(map(tuple, m.tolist()))
    assert g.num_correspondences_between_images(10, 99) == 0 and g.find_correspondences_between_images(10, 99).shape == (0, 2)


def test_graph_walks_close_cycles_and_end_early():
    g = pc.CorrespondenceGraph()
    for i in (1, 2, 3, 4):
        g.add_image(i, 2)
    g.add_correspondences(1, 2, [[0, 0]])
    g.add_correspondences(2, 3, [[0, 0]])
    g.add_correspondences(3, 1, [[0, 0]])  # the cycle 1 - 2 - 3 - 1
    g.add_correspondences(3, 4, [[0, 1]])
    g.add_correspondences(1, 1, [[0, 1]])  # a self pair: ignored
    g.finalize()
    walk = lambda t: [(c.image_id, c.point2D_idx) for c in g.extract_transitive_correspondences(1, 0, t)]  # noqa: E731
    assert walk(1) == [(2, 0), (3, 0)]
    assert walk(2) == [(4, 1), (2, 0), (3, 0)]  # level 2 finds (4, 1) only: the cycle closes; it takes the seed's place
    assert walk(5) == walk(2)  # level 3 adds nothing: the walk ends early
    assert g.extract_transitive_correspondences(1, 1, 3) == []
    assert not g.is_two_view_observation(1, 0) and g.is_two_view_observation(4, 1) is False  # (3, 0) has three
    assert g.num_correspondences_for_image(1) == 2 and g.num_image_pairs() == 4


def test_graph_before_finalize_and_unknown_images():
    images, g, p, rs = _graphs(2, finalize=False)
    assert g.exists_image(99) and g.num_images() == len(images)
    assert g.num_observations_for_image(10) == 0  # counted by finalize
    assert g.num_correspondences_for_image(10) == p.ncorr[10]
    g.finalize()
    for call in (lambda: g.num_observations_for_image(99), lambda: g.num_correspondences_for_image(7),
                 lambda: g.has_correspondences(99, 0), lambda: g.extract_correspondences(99, 0),
                 lambda: g.extract_transitive_correspondences(99, 0, 2), lambda: g.is_two_view_observation(99, 0),
                 lambda: g.add_correspondences(10, 99, [[0, 0]]), lambda: g.extract_correspondences(10, 1000),
                 lambda: g.add_image(10, 3)):
        with pytest.raises(ValueError, match=r"\[correspondence_graph.h:\d+\] Check Failed"):
            call()
    with pytest.raises(ValueError, match="N x 2"):
        g.add_correspondences(10, 12, [1, 2, 3])


# ---- the reference -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tc.SCENES))
def test_reference_equals_python_restatement(name):
    """Find, Continue and Create restated in Python (numpy for the angle, tests/tri_ref for the RANSAC) create the same
    tracks and make the same continuations; first, no deciding angle of the reference is within 1e-9 rad of its
    threshold, so that numpy's arccos may decide."""
    sc, opts = tc.scene_case(name)
    counts, points, ids, modified, margins = tc.scene_reference(name)
    assert min(margins) > 1e-9, margins
    state, graph = tc.PyState(sc), tc.py_graph(sc)
    got = [state.triangulate_image(graph, i, **opts) for i in sc["images"]]
    assert got == counts
    assert state.tracks() == {pid: p[2] for pid, p in points.items()}
    for i in sc["images"]:
        assert state.ids[i] == [int(v) for v in ids[i]]
    for pid, (xyz, err, track) in points.items():
        np.testing.assert_allclose(state.points[pid][0], xyz, rtol=0, atol=1e-12)
        assert err == -1.0 and pid in modified
    assert sum(counts) > 0 and any(d[3] for d in state.decisions)
    if name != "bogus_camera":  # (there the first image creates every track whole)
        assert any(d[2] is not None for d in state.decisions)


def test_reference_noise_free_planted_tracks_come_back():
    """(0.01 px of noise, not none: an exact observation can give a cosine of 1 + 2^-52, whose acos is NaN and so an
    outlier, T6 of section 11.6)"""
    sc = tc.scene(seed=21, nimg=12, npts=20, models=(1,), noise=0.01, wrong=0, extra_keypoints=2)
    rs = tc.ref_scene(sc)
    for i in sc["images"]:
        rs.triangulate_image(i)
    points = rs.points()
    assert len(points) == 20
    planted = sorted(sorted(t) for t in sc["planted"].values())
    assert sorted(sorted(p[2]) for p in points.values()) == planted
    for xyz, _, track in points.values():
        j = next(j for j, t in sc["planted"].items() if sorted(t) == sorted(track))
        np.testing.assert_allclose(xyz, sc["xyz"][j], atol=1e-3)


def _hand(seed, sizes, **kw):
    args, k = tc.hand_problem(seed=seed, sizes=sizes, models=(1,), noise=0.01, p_out=0.0, **kw)  # (0.01 px: see above)
    return args, k, ref.triangulate_observations(*args, **k)


def test_reference_hand_built_answers():
    # two consistent groups of 3 give two points; the candidates were dealt to the groups in turn
    _, _, r = _hand(50, [6], groups=2)
    rounds = r["cand_round"].tolist()  # (which group wins round 1 is the residual sums' business)
    assert rounds in ([1, 2, 1, 2, 1, 2], [2, 1, 2, 1, 2, 1]) and r["num_created"] == 2
    # three rounds in one item
    _, _, r = _hand(51, [9], groups=3)
    rounds = r["cand_round"].tolist()
    assert rounds == rounds[:3] * 3 and sorted(rounds[:3]) == [1, 2, 3]
    # a left-over of 2 gives none
    _, _, r = _hand(52, [5], groups=2)
    assert r["cand_round"].tolist() == [1, 0, 1, 0, 1] and r["num_created"] == 1
    # a two-view observation is ignored, and is created with the flag off
    args, _, r = _hand(53, [2], two_view=[1])
    assert r["num_created"] == 0
    assert ref.triangulate_observations(*args, no_create_two_view=[0])["cand_round"].tolist() == [1, 1]
    # the flag does not reach an item of three
    _, _, r = _hand(54, [3], two_view=[1])
    assert r["cand_round"].tolist() == [1, 1, 1]
    # a Continue tie goes to the first candidate
    args, kw, _ = _hand(55, [4])
    args[8][:] = [0, 1, 1, 0]
    args[9][1] = args[9][2] = [0.1, 0.2, 0.3]
    r = ref.triangulate_observations(*args, continue_max_angle_error=180.0)
    assert r["continued"].tolist() == [1] and r["num_created"] == 0  # one observation is left: nothing to create
    # a reference observation that already has a point neither continues nor joins a track
    args[8][:] = [0, 1, 0, 1]
    r = ref.triangulate_observations(*args, continue_max_angle_error=180.0)
    assert r["continued"].tolist() == [-1] and r["cand_round"].tolist() == [1, 0, 1, 0]
    # Continue at its threshold and one double above it
    assert tc.reference("continue_at_threshold")["continued"].tolist() == [0]
    assert tc.reference("continue_above_threshold")["continued"].tolist() == [-1]
    assert max(np.diff(tc.reference("three_rounds")["round_offsets"].astype(np.int64))) >= 3


def test_reference_reproduces_fixture():
    golden = np.load(GOLDEN)
    assert sorted(golden["cases"]) == sorted(tc.CASES) and sorted(golden["edge_cases"]) == sorted(tc.EDGE_CASES)
    assert sorted(golden["scenes"]) == sorted(tc.SCENES)
    for name in tc.ALL_CASES:
        res = tc.reference(name)
        assert tc.digest(res) == str(golden[f"{name}/digest"]), name
        if name in tc.CASES:
            for k in tc.RESULT_KEYS:
                assert np.array_equal(tc.bits(res[k]) if k == "round_xyz" else np.asarray(res[k]),
                                      tc.bits(golden[f"{name}/{k}"]) if k == "round_xyz" else golden[f"{name}/{k}"]), (name, k)
    for name in tc.SCENES:
        counts, points, _, _, _ = tc.scene_reference(name)
        assert counts == golden[f"scene/{name}/counts"].tolist()
        assert tc.scene_digest(counts, points) == str(golden[f"scene/{name}/digest"]), name


# ---- the host half -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tc.SCENES))
def test_host_half_with_reference_in_the_librarys_place(name):
    """triangulate_image's Find, cut into runs and write-back around the reference's arithmetic equal the sequential
    reference: ids, tracks, positions bit for bit, errors, point2D ids, the modified set; surviving Python objects stay the
    same objects."""
    sc, opts = tc.scene_case(name)
    counts, points, ids, modified, _ = tc.scene_reference(name)
    r, g = tc.reconstruction(sc)
    t = pc.IncrementalTriangulator(g, r)
    images = dict(r.images)
    calls, seen = 0, {}
    for k, iid in enumerate(sc["images"]):
        assert t._triangulate_image_with(opts, iid, tc.reference_solver) == counts[k]
        st = pc.last_run_stats()
        assert st["call"] == "triangulate_image" and st["host_ms"] >= 0
        assert st["num_created_points"] + st["num_continued_observations"] <= counts[k]
        calls = max(calls, st["num_device_calls"])
        for pid, p in r.points3D.items():
            assert seen.setdefault(pid, p) is p
    got = tc.reconstruction_points(r)
    assert list(got) == list(points)
    for pid in points:
        assert np.array_equal(tc.bits(got[pid][0]), tc.bits(points[pid][0])) and got[pid][1:] == points[pid][1:], pid
    for iid, im in r.images.items():
        assert im is images[iid]
        assert [p.point3D_id for p in im.points2D] == [int(v) for v in ids[iid]]
    assert t.get_modified_points3D() == modified
    assert (calls > 1) == (opts.get("max_transitivity", 1) > 1), "overlapping walks must force a cut, direct lists never"
    t.clear_modified_points3D()
    assert t.get_modified_points3D() == set()


def test_triangulate_image_refusals_leave_the_model_untouched():
    sc, _ = tc.scene_case("direct")
    r, g = tc.reconstruction(sc)
    t = pc.IncrementalTriangulator(g, r)
    with pytest.raises(ValueError, match="Check Failed"):
        t._triangulate_image_with({}, 999, tc.reference_solver)  # not in the reconstruction
    lonely = pc.Image(name="lonely.png", camera_id=1, id=500)
    lonely.points2D = [pc.Point2D([1.0, 2.0])]
    r.add_image(lonely)
    with pytest.raises(ValueError, match="correspondence_graph.h"):
        t._triangulate_image_with({}, 500, tc.reference_solver)  # not in the graph
    with pytest.raises(ValueError, match="shape"):
        t._triangulate_image_with({}, 1, lambda d: dict(continued=[], cand_round=[], round_offsets=[0], round_xyz=[]))
    assert len(r.points3D) == 0 and t.get_modified_points3D() == set()


def test_bogus_camera_on_the_image_returns_zero():
    sc, opts = tc.scene_case("bogus_camera")
    r, g = tc.reconstruction(sc)
    t = pc.IncrementalTriangulator(g, r)
    assert t._triangulate_image_with(opts, 2, tc.reference_solver) == 0  # image 2 has the bogus camera
    assert pc.last_run_stats()["num_device_calls"] == 0 and len(r.points3D) == 0
    n = t._triangulate_image_with(opts, 1, tc.reference_solver)
    assert n > 0
    for p in r.points3D.values():  # a correspondence with a bogus camera joins nothing
        assert all(sc["images"][e.image_id][0] == 1 for e in p.track.elements)


def test_host_half_under_asan(tmp_path):
    """The host half (csrc/host/correspondence_graph.h, triangulator_host.h, csrc/triobs_plan.h) in a stand-alone program
    under ASan + UBSan (tests/shim/triangulator_host_fuzz.cc)."""
    import os
    import shutil
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    flags = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined"]
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("sanitizer runtime not installed")
    exe = tmp_path / "triangulator_host_fuzz"
    b = subprocess.run(flags + [str(ROOT / "tests" / "shim" / "triangulator_host_fuzz.cc"),
                                str(ROOT / "pycolmap_amd" / "csrc" / "host" / "model_io.cc"),
                                str(ROOT / "pycolmap_amd" / "csrc" / "host" / "reconstruction.cc"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[1]) >= 1000


def test_image_without_points2D_and_image_without_correspondences():
    tc.check_empty_images(lambda t, o, iid: t._triangulate_image_with(o, iid, tc.reference_solver))
