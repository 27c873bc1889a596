"""GPU parity tests of the relative pose (pose.hip: amc_pose_pairs and amc_verify_pairs with
compute_relative_pose) against the oracle's EstimateTwoViewGeometryPose on identical inputs.
Bit-exact: R, t, quaternion, tri_angle, the number of points in front of both cameras, config.
First on random scenes, then on the named cases of tests/pose_cases.py."""
import ctypes as C
import sys

import numpy as np
import pytest

import oracle_lib as o
import pose_cases as pc
from pycolmap_amd import _capi, synth

sys.path.insert(0, str(o.ROOT / "tests" / "golden"))
import make_pose_ref_golden as pose_golden  # noqa: E402

pytestmark = pytest.mark.gpu

CAM_A = dict(model="PINHOLE", width=1600, height=1200, params=(1200.0, 1190.0, 800.0, 600.0))
CAM_B = dict(model="SIMPLE_PINHOLE", width=1600, height=1200, params=(1210.0, 801.0, 599.0))


def bits(a):
    a = np.ascontiguousarray(a, dtype=np.float64).copy()
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def ocam(c, prior=True):
    return o.make_camera(c["model"], c["width"], c["height"], c["params"], prior=prior)


def assert_pose_equal(got, want, tag=""):
    assert bool(got["ok"]) == want["pose_ok"], tag
    assert int(got["config"]) == want["config"], f"{tag}: {got['config']} vs {want['config_name']}"
    assert int(got["num_points3D"]) == want["num_points3D"], tag
    np.testing.assert_array_equal(bits(got["R"]), bits(want["R"]), err_msg=f"{tag} R")
    np.testing.assert_array_equal(bits(got["tvec"]), bits(want["tvec"]), err_msg=f"{tag} t")
    np.testing.assert_array_equal(bits(got["qvec"]), bits(want["qvec"]), err_msg=f"{tag} q")
    assert bits(got["tri_angle"]) == bits(want["tri_angle"]), f"{tag}: {got['tri_angle']} vs {want['tri_angle']}"


def test_pose_pairs_all_configs_bit_exact(amc_ctx):
    """A batch of general / planar / panoramic scenes with mixed cameras, every config value and small
    correspondence counts (empty, one, two, three) through amc_pose_pairs."""
    rng = np.random.default_rng(2024)
    kinds = [dict(), dict(planar=True), dict(pure_rotation=True, noise=0.05)]
    scenes, cams, geoms = [], [], []
    for i in range(9):
        sc = synth.two_view_scene(rng, num_inliers=int(rng.integers(30, 400)), num_outliers=int(rng.integers(0, 80)),
                                  **kinds[i % 3])
        c1, c2 = CAM_A, (CAM_B if i % 2 else CAM_A)
        r = o.estimate_two_view_geometry(ocam(c1), sc["pts1"], ocam(c2), sc["pts2"], sc["matches"])
        scenes.append(sc)
        cams.append((c1, c2))
        geoms.append(r)
    amc_ctx.reserve_slots(2 * len(scenes))
    for i, (sc, (c1, c2)) in enumerate(zip(scenes, cams)):
        amc_ctx.upload_points_f64(2 * i, sc["pts1"])
        amc_ctx.upload_points_f64(2 * i + 1, sc["pts2"])
        amc_ctx.upload_camera(2 * i, c1["model"], c1["width"], c1["height"], c1["params"], True)
        amc_ctx.upload_camera(2 * i + 1, c2["model"], c2["width"], c2["height"], c2["params"], True)
    jobs = []  # (scene, config, inlier matches)
    for i, (sc, r) in enumerate(zip(scenes, geoms)):
        m = sc["matches"][r["inlier_mask"]]
        for cfg in range(9):
            jobs.append((i, cfg, m))
        for n in (0, 1, 2, 3, 64, 65):
            jobs.append((i, 2, m[:n]))
            jobs.append((i, 6, m[:n]))
    s1 = np.array([2 * j[0] for j in jobs], dtype=np.uint32)
    off = np.zeros(len(jobs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(j[2]) for j in jobs])
    mm = np.concatenate([j[2] for j in jobs])
    cfgs = np.array([j[1] for j in jobs], dtype=np.int32)
    E = np.stack([geoms[j[0]]["E"] for j in jobs])
    H = np.stack([geoms[j[0]]["H"] for j in jobs])
    got = amc_ctx.pose_pairs(s1, s1 + 1, off, mm, cfgs, E, H)
    seen = set()
    for k, (i, cfg, m) in enumerate(jobs):
        c1, c2 = cams[i]
        want = o.estimate_two_view_geometry_pose(ocam(c1), scenes[i]["pts1"], ocam(c2), scenes[i]["pts2"], m, cfg,
                                                 E=geoms[i]["E"], H=geoms[i]["H"])
        assert_pose_equal(got[k], want, f"job {k} scene {i} cfg {cfg} n {len(m)}")
        seen.add(want["config_name"])
    assert {"CALIBRATED", "UNCALIBRATED", "PLANAR", "PANORAMIC"} <= seen


def test_verify_with_relative_pose_bit_exact(amc_ctx):
    """TwoViewGeometryOptions.compute_relative_pose through amc_verify_pairs: the estimation as before,
    then the pose; PLANAR_OR_PANORAMIC resolves to PLANAR / PANORAMIC in tvg.config as well."""
    rng = np.random.default_rng(31)
    scenes, priors = [], []
    for i in range(12):
        kind = [dict(), dict(planar=True), dict(pure_rotation=True, noise=0.05), dict(num_inliers=0, num_outliers=30)][i % 4]
        kw = dict(num_inliers=int(rng.integers(40, 350)), num_outliers=int(rng.integers(0, 120)))
        kw.update(kind)
        scenes.append(synth.two_view_scene(rng, **kw))
        priors.append(i % 3 != 2)
    amc_ctx.reserve_slots(2 * len(scenes))
    for i, sc in enumerate(scenes):
        for s, pts in ((2 * i, sc["pts1"]), (2 * i + 1, sc["pts2"])):
            amc_ctx.upload_keypoints(s, pts.astype(np.float32))
            amc_ctx.upload_camera(s, CAM_A["model"], CAM_A["width"], CAM_A["height"], CAM_A["params"], priors[i])
    s1 = np.arange(0, 2 * len(scenes), 2, dtype=np.uint32)
    off = np.zeros(len(scenes) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(sc["matches"]) for sc in scenes])
    mm = np.concatenate([sc["matches"] for sc in scenes])
    for multiple in (0, 1):
        tvg, mask, st = amc_ctx.verify_pairs(s1, s1 + 1, off, mm,
                                             _capi.tvg_options(compute_relative_pose=1, multiple_models=multiple), seed=0)
        assert "pose" in st and len(st["pose"]) == len(scenes)
        names = set()
        for p, sc in enumerate(scenes):
            cam = ocam(CAM_A, priors[p])
            w = o.estimate_two_view_geometry(cam, sc["pts1"], cam, sc["pts2"], sc["matches"],
                                             o.tvg_default_options(compute_relative_pose=1, multiple_models=multiple), seed=0)
            assert _capi.CONFIG_NAMES[tvg[p]["config"]] == w["config_name"], f"pair {p}"
            np.testing.assert_array_equal(mask[int(off[p]):int(off[p + 1])], w["inlier_mask"], err_msg=f"pair {p}")
            if w["config_name"] != "MULTIPLE":
                for k in "EFH":
                    np.testing.assert_array_equal(bits(tvg[p][k]), bits(w[k]), err_msg=f"pair {p} {k}")
            assert_pose_equal(st["pose"][p], w, f"pair {p} multiple={multiple}")
            names.add(w["config_name"])
        if not multiple:
            assert {"CALIBRATED", "UNCALIBRATED", "PLANAR", "DEGENERATE"} <= names, names
            assert "PLANAR_OR_PANORAMIC" not in names
    # without the option the result carries no poses and PLANAR_OR_PANORAMIC stays
    tvg, mask, st = amc_ctx.verify_pairs(s1, s1 + 1, off, mm, _capi.tvg_options(), seed=0)
    assert "pose" not in st and "PLANAR_OR_PANORAMIC" in {_capi.CONFIG_NAMES[c] for c in tvg["config"]}


def test_pose_many_inliers_and_planted_motion(amc_ctx):
    """Thousands of inliers (the median selection runs over many 64-wide chunks) and the result is the
    planted motion."""
    rng = np.random.default_rng(8)
    sc = synth.two_view_scene(rng, num_inliers=6000, num_outliers=500, noise=0.3)
    amc_ctx.reserve_slots(2)
    amc_ctx.upload_keypoints(0, sc["pts1"].astype(np.float32))
    amc_ctx.upload_keypoints(1, sc["pts2"].astype(np.float32))
    cam = ("PINHOLE", 1600, 1200, (1200.0, 1200.0, 800.0, 600.0))
    amc_ctx.upload_camera(0, *cam, True)
    amc_ctx.upload_camera(1, *cam, True)
    off = np.array([0, len(sc["matches"])], dtype=np.uint64)
    tvg, mask, st = amc_ctx.verify_pairs([0], [1], off, sc["matches"], _capi.tvg_options(compute_relative_pose=1), seed=0)
    oc = o.make_camera("PINHOLE", 1600, 1200, (1200.0, 1200.0, 800.0, 600.0), prior=True)
    w = o.estimate_two_view_geometry(oc, sc["pts1"], oc, sc["pts2"], sc["matches"],
                                     o.tvg_default_options(compute_relative_pose=1), seed=0)
    assert w["config_name"] == "CALIBRATED" and w["num_points3D"] > 5000
    assert_pose_equal(st["pose"][0], w, "large")
    R = st["pose"][0]["R"]
    assert np.degrees(np.arccos(np.clip((np.trace(R.T @ sc["R"]) - 1) / 2, -1, 1))) < 0.3
    assert float(st["pose"][0]["tvec"] @ (sc["t"] / np.linalg.norm(sc["t"]))) > 0.999


def test_pose_rejects_unsupported_input(amc_ctx):
    rng = np.random.default_rng(1)
    sc = synth.two_view_scene(rng, num_inliers=50, num_outliers=0)
    amc_ctx.reserve_slots(2)
    amc_ctx.upload_points_f64(0, sc["pts1"])
    amc_ctx.upload_points_f64(1, sc["pts2"])
    off = np.array([0, len(sc["matches"])], dtype=np.uint64)
    with pytest.raises(_capi.AmcError):   # no cameras uploaded
        amc_ctx.pose_pairs([0], [1], off, sc["matches"], [2], [sc["E_true"]])
    amc_ctx.upload_camera(0, *("PINHOLE", 1600, 1200, (1200.0, 1200.0, 800.0, 600.0)), True)
    amc_ctx.upload_camera(1, *("PINHOLE", 1600, 1200, (1200.0, 1200.0, 800.0, 600.0)), True)
    bad = sc["matches"].copy()
    bad[3, 1] = 10 ** 6
    with pytest.raises(_capi.AmcError):   # match index past the keypoints
        amc_ctx.pose_pairs([0], [1], off, bad, [2], [sc["E_true"]])
    got = amc_ctx.pose_pairs(np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(1, np.uint64),
                             np.zeros((0, 2), np.uint32), [], None)
    assert len(got) == 0


# ------------------------------------------------------------------------------------------------
# The named cases of tests/pose_cases.py ("what is pinned"): lane edges of the ballots and the
# compaction, ranks of the median selection, the branches of the decompositions, the slices of the workspace.
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pose_ctx():
    """one context for the new tests: every case of pose_cases.cases() in its own pair of slots (2 i, 2 i + 1), then
    the masked scenes"""
    ctx = _capi.Context(0)
    cs = pc.cases()
    masked = pc.masked_scenes()
    ctx.reserve_slots(2 * (len(cs) + len(masked)))
    slots = {}
    for i, (name, c) in enumerate(cs.items()):
        for s, cam, pts in ((2 * i, c["cam1"], c["pts1"]), (2 * i + 1, c["cam2"], c["pts2"])):
            if c["f32"]:
                ctx.upload_keypoints(s, pts.astype(np.float32))
            else:
                ctx.upload_points_f64(s, pts)
            ctx.upload_camera(s, cam[0], cam[1], cam[2], cam[3], True)
        slots[name] = 2 * i
    for j, (M, sc) in enumerate(masked.items()):
        base = 2 * (len(cs) + j)
        for s, pts in ((base, sc["pts1"]), (base + 1, sc["pts2"])):
            ctx.upload_keypoints(s, pts.astype(np.float32))
            ctx.upload_camera(s, *sc["cam"], True)
        slots[M] = base
    yield ctx, slots
    ctx.close()


def run_cases(ctx, slots, names, matches=None):
    """amc_pose_pairs on the listed cases, in that order, in one call; matches: name -> rows instead of the case's"""
    cs = pc.cases()
    mm = [cs[n]["matches"] if matches is None or n not in matches else matches[n] for n in names]
    s1 = np.array([slots[n] for n in names], dtype=np.uint32)
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in mm])
    return ctx.pose_pairs(s1, s1 + 1, off, np.concatenate(mm).reshape(-1, 2), [cs[n]["config"] for n in names],
                          np.stack([cs[n]["E"] for n in names]), np.stack([cs[n]["H"] for n in names]))


def record_bits(rec):
    return tuple(bits(rec[k]).tobytes() for k in ("R", "tvec", "qvec", "tri_angle")) + (int(rec["ok"]), int(rec["config"]),
                                                                                         int(rec["num_points3D"]))


@pytest.fixture(scope="module")
def all_at_once(pose_ctx):
    ctx, slots = pose_ctx
    return run_cases(ctx, slots, list(pc.cases()))


def test_named_cases_bit_exact_against_the_oracle_and_the_fixture(all_at_once):
    cs, want = pc.build_cases()
    poses, _ = pose_golden.load()
    assert list(poses) == list(cs)
    for k, name in enumerate(cs):
        assert_pose_equal(all_at_once[k], want[name], name)
        assert_pose_equal(all_at_once[k], poses[name], f"{name} (fixture)")
    # the same values through either upload
    names = list(cs)
    assert record_bits(all_at_once[names.index("cameras_float32")]) == record_bits(all_at_once[names.index("cameras_float64")])


def test_one_call_each_equals_all_in_one_call(pose_ctx, all_at_once):
    ctx, slots = pose_ctx
    for k, name in enumerate(pc.cases()):
        assert record_bits(run_cases(ctx, slots, [name])[0]) == record_bits(all_at_once[k]), name


def test_a_permuted_order_gives_the_permuted_result(pose_ctx, all_at_once):
    ctx, slots = pose_ctx
    names = list(pc.cases())
    perm = np.random.default_rng(5).permutation(len(names))
    got = run_cases(ctx, slots, [names[i] for i in perm])
    for k, i in enumerate(perm):
        assert record_bits(got[k]) == record_bits(all_at_once[i]), names[i]
    back = run_cases(ctx, slots, names[::-1])
    for k, name in enumerate(names[::-1]):
        assert record_bits(back[k]) == record_bits(all_at_once[len(names) - 1 - k]), name


def test_an_empty_pair_between_two_full_ones_changes_neither(pose_ctx, all_at_once):
    ctx, slots = pose_ctx
    names = list(pc.cases())
    a, b = "rotation_x", "angles_above_90"
    got = run_cases(ctx, slots, [a, "rotation_small", b], matches={"rotation_small": np.zeros((0, 2), np.uint32)})
    assert record_bits(got[0]) == record_bits(all_at_once[names.index(a)])
    assert record_bits(got[2]) == record_bits(all_at_once[names.index(b)])
    c = pc.cases()["rotation_small"]
    want = o.estimate_two_view_geometry_pose(pc.ocam(c["cam1"]), c["pts1"], pc.ocam(c["cam2"]), c["pts2"],
                                             np.zeros((0, 2), np.uint32), c["config"], E=c["E"], H=c["H"])
    assert_pose_equal(got[1], want, "the empty pair")


def test_thirty_pairs_on_one_pair_of_slots_agree_with_the_single_call(pose_ctx, all_at_once):
    ctx, slots = pose_ctx
    names = list(pc.cases())
    for name in ("survivors_edges", "duplicates_halves_130"):
        got = run_cases(ctx, slots, [name] * 30)
        for k in range(30):
            assert record_bits(got[k]) == record_bits(all_at_once[names.index(name)]), (name, k)


def test_masked_path_with_a_hole_in_every_chunk(pose_ctx):
    """amc_verify_pairs with compute_relative_pose hands the pose kernel the estimation's mask.  The mask is the
    planted one - rows 0, 63, 64 and M - 1 cleared - or the test fails; then the pose, bit for bit."""
    ctx, slots = pose_ctx
    masked = pc.masked_scenes()
    s1 = np.array([slots[M] for M in masked], dtype=np.uint32)
    off = np.zeros(len(masked) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(sc["matches"]) for sc in masked.values()])
    mm = np.concatenate([sc["matches"] for sc in masked.values()])
    tvg, mask, st = ctx.verify_pairs(s1, s1 + 1, off, mm, _capi.tvg_options(compute_relative_pose=1), seed=0)
    for p, (M, sc) in enumerate(masked.items()):
        w = pc.oracle_verify(sc)
        pc.check_masked(sc, w["inlier_mask"])
        got = mask[int(off[p]):int(off[p + 1])]
        np.testing.assert_array_equal(got, w["inlier_mask"], err_msg=f"M {M}")
        pc.check_masked(sc, got)
        assert _capi.CONFIG_NAMES[tvg[p]["config"]] == w["config_name"] == "CALIBRATED", M
        assert_pose_equal(st["pose"][p], w, f"masked M {M}")
        assert int(st["pose"][p]["num_points3D"]) == M - len(sc["holes"])


def test_refused_input_leaves_the_context_usable(pose_ctx, all_at_once):
    ctx, slots = pose_ctx
    names = list(pc.cases())
    cs = pc.cases()
    a = "rotation_y"
    c = cs[a]

    def still_works():
        assert record_bits(run_cases(ctx, slots, [a])[0]) == record_bits(all_at_once[names.index(a)])

    off = np.array([0, len(c["matches"])], dtype=np.uint64)
    past = 2 * (len(cs) + len(pc.masked_scenes()))
    with pytest.raises(_capi.AmcError, match="slot out of range"):      # a slot past the table
        ctx.pose_pairs([slots[a]], [past], off, c["matches"], [c["config"]], [c["E"]], [c["H"]])
    still_works()
    with pytest.raises(_capi.AmcError, match="slot out of range"):
        ctx.pose_pairs([0xFFFFFFFF], [slots[a] + 1], off, c["matches"], [c["config"]], [c["E"]], [c["H"]])
    still_works()
    # offsets that are not monotone: the second pair ends before it begins (every row read before the refusal exists)
    s1 = np.array([slots[a]] * 3, dtype=np.uint32)
    bad = np.array([0, 60, 50, 130], dtype=np.uint64)
    with pytest.raises(_capi.AmcError, match="not monotone"):
        ctx.pose_pairs(s1, s1 + 1, bad, c["matches"], [c["config"]] * 3, [c["E"]] * 3, [c["H"]] * 3)
    still_works()
    # ... and a first pair that ends past the last offset: refused before any row of it is looked at
    with pytest.raises(_capi.AmcError, match="not monotone at 0"):
        ctx.pose_pairs(s1[:2], s1[:2] + 1, np.array([0, 100, 50], dtype=np.uint64), c["matches"][:50], [c["config"]] * 2,
                       [c["E"]] * 2, [c["H"]] * 2)
    still_works()
    # a NULL geometry array, through the C entry point
    s = np.array([slots[a]], dtype=np.uint32)
    s2 = s + 1
    m = np.ascontiguousarray(c["matches"], dtype=np.uint32)
    out = np.zeros(1, dtype=_capi.POSE_DTYPE)
    v = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = ctx._lib.amc_pose_pairs(ctx._h, v(s), v(s2), C.c_size_t(1), v(off), v(m), None, v(out))
    assert rc != 0 and b"NULL" in ctx._lib.amc_last_error()
    assert not out["ok"][0]
    still_works()
