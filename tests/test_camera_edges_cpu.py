"""The camera models beyond the narrow cone, without a GPU: the edge cases of
tests/camera_edge_cases.py reach the branches they are named for (the census floors); the CPU references (tests/ba_ref,
tests/filter_ref, tests/abspose_ref, the oracle's lifts) agree there with an independent 60-digit mpmath restatement
(tests/ref2/camera_edges_ref2.py) within the measured deviation budget (tests/ref2/camera_edges_deviation_budget.json,
written by tests/ref2/compare_camera_edges.py) and still reproduce the fixture tests/golden/camera_edges_ref_v1.npz that
tests/test_camera_edges_gpu.py holds the device to."""
import functools
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest

import camera_edge_cases as ce
from ref2 import camera_edges_ref2 as r2
from ref2 import compare_camera_edges as cmp

ROOT = Path(__file__).resolve().parent.parent
BUDGET = json.loads(cmp.BUDGET.read_text())
# the only regimes whose references may hold an entry that is not finite or not comparable
NONFINITE_REGIMES = ("rational_pole", "behind")


@functools.lru_cache(maxsize=None)
def measured(name):
    return cmp.measure(name)


def allowed(worst):
    """twice the recorded worst and never less than one unit more: another libm or numpy build may move the last bit of
    the comparison side"""
    return max(2.0 * worst, worst + 1.0)


# ---- the cases and the census --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ce.CASES)
def test_scene_is_small_exact_and_reaches_its_branches(name):
    sc = ce.case_scene(name)
    assert len(sc["image_cameras"]) <= 6 and len(sc["xyz"]) <= 130 and len(sc["obs_image"]) <= 600
    assert np.array_equal(sc["qvec"][0], [0, 0, 0, 1]) and not sc["tvec"][0].any()
    assert np.isfinite(sc["obs_xy"]).all()
    c = ce.census(sc)
    fl = ce.floors(name)
    assert fl or ce.regime(name) == "strong_poly"
    for branch, floor in fl.items():
        assert floor >= (8 if branch.startswith(("atan_", "depth_", "denominator_p", "denominator_n", "fov_omega", "fov_atan",
                                                  "fov_radius_series", "rem_pio2", "r_gt")) else 2), (branch, floor)
        assert c.get(branch, 0) >= floor, (name, branch, c)
    if ce.regime(name) != "behind":
        assert "depth_negative" not in c and "depth_below_eps" not in c  # the other images see every point in front


def test_every_regime_and_model_has_its_cases():
    have = {(ce.regime(n), ce.SPECS[n][1]) for n in ce.CASES}
    for reg in ("wide_50_68", "wide_68_89", "axis", "behind"):
        assert all((reg, m) in have for m in range(11))
    for reg in ("atan_cuts", "axis_tiny", "depth_tiny"):
        assert all((reg, m) in have for m in ce.ATAN_MODELS)
    assert all(("axis_eps", m) in have for m in ce.FISHEYE) and all(("strong_poly", m) in have for m in ce.POLYNOMIAL)
    assert set(ce.REGIMES) == {"atan_cuts", "wide_50_68", "wide_68_89", "axis", "axis_eps", "axis_tiny", "depth_tiny", "behind",
                               "fov_small_omega", "fov_small_radius", "fov_large_omega", "rational_pole", "strong_poly"}
    wide = [n for n in ce.ITERATION_CASES if ce.regime(n).startswith("wide_")]
    assert {ce.SPECS[n][1] for n in wide} == set(ce.WIDE_ITERATION_MODELS) and len(wide) == 2 * len(ce.WIDE_ITERATION_MODELS)


def test_selectors_at_their_cuts():
    assert [ce.atan_branch(x) for x in (0.0, ce._prev(2.0 ** -29), 2.0 ** -29, ce._prev(0.4375), 0.4375, ce._prev(0.6875),
                                         0.6875, ce._prev(1.1875), 1.1875, ce._prev(2.4375), 2.4375, ce._prev(2.0 ** 66),
                                         2.0 ** 66, -3.0)] == \
        ["atan_tiny", "atan_tiny", "atan_poly", "atan_poly", "atan_id0", "atan_id0", "atan_id1", "atan_id1", "atan_id2",
         "atan_id2", "atan_id3", "atan_id3", "atan_huge", "atan_id3"]
    assert ce.SQ_LO * ce.SQ_LO < 1e-4 <= ce.SQ_HI * ce.SQ_HI and ce.SQ_HI == ce._next(ce.SQ_LO)
    # both cancellation rounds of the reduction are reached: omega / 2 = pi / 2 + 2^-20 ends in the second, fl(pi) / 2 in
    # the third; 0.3 needs none and 0.8, 1.0, 1.5 end in the first
    omega = {t: float(ce.case_scene(f"fov_large_omega/{t}")["camera_params"][0][4]) for t in ("1.6", "2.0", "3.0", "round2",
                                                                                              "round3")}
    assert [ce.rem_pio2_round(omega[t] / 2) for t in ("1.6", "2.0", "3.0", "round2", "round3")] == [1, 1, 1, 2, 3]
    assert ce.rem_pio2_round(0.3) == 0 and ce.rem_pio2_round(-0.8) == 1
    pole = ce.case_scene("rational_pole/FULL_OPENCV")
    lo, hi = ce.pole_radius(pole["camera_params"][0][4:])
    d = [ce.rational_denominator(pole["camera_params"][0][4:], r * r) for r in (lo, hi)]
    assert d[0] > 0 > d[1] and max(abs(d[0]), abs(d[1])) < 1e-12
    for m in ce.POLYNOMIAL:
        c = ce.strong_census(m)
        assert c["principal_point"] >= 2 and c["principal_point_neighbour"] >= 2 and c["past_fold"] >= 8 and \
            c["inside_fold"] >= 8 and len(ce.strong_pixels(m)) == 257


# ---- the references against the restatement ------------------------------------------------------------------------------
def test_restatement_against_known_answers():
    """the mpmath side by itself: a pinhole by hand, the equidistant fisheye at 45 degrees, FOV's two series against the
    function, and the derivative of a pinhole"""
    mp = r2.mp
    x, y, _ = r2.img_from_cam(1, [r2.M(v) for v in (800, 808, 500, 400)], r2.M(0.25), r2.M(-0.5))
    assert (float(x), float(y)) == (700.0, -4.0)
    x, y, _ = r2.img_from_cam(8, [r2.M(v) for v in (800, 500, 400, 0)], r2.M(1), r2.M(0))
    assert abs(x - (800 * mp.pi / 4 + 500)) < mp.mpf(10) ** -50 and y == 400
    p = [r2.M(v) for v in (800, 808, 500, 400, 0.01)]
    a = r2.img_from_cam(7, p, r2.M(0.3), r2.M(0.1), ("series",))[0]
    b = r2.img_from_cam(7, p, r2.M(0.3), r2.M(0.1), ("atan",))[0]
    # COLMAP's small-omega series, 1 + omega^2 r^2 / 3 - omega^2 / 12, is the expansion of the inverse map's factor: it
    # mirrors the function's 1 - omega^2 r^2 / 3 + omega^2 / 12 about 1.  The branch is the specification as it stands.
    assert abs(a - b) > 1e-3 and abs((a - 740) + (b - 740)) < 1e-6
    p[4] = r2.M(0.6)
    a = r2.img_from_cam(7, p, r2.M(0.006), r2.M(0.008), ("radius_series",))[0]
    b = r2.img_from_cam(7, p, r2.M(0.006), r2.M(0.008), ("atan",))[0]
    assert 0 < abs(a - b) < 1e-7
    Jp, Jc, Jx = r2.jacobians(0, [800.0, 500.0, 400.0], [0, 0, 0, 1.0], [0, 0, 0], [0.5, -0.25, 2.0])
    np.testing.assert_allclose(Jx, [[400.0, 0, -100.0], [0, 400.0, 50.0]], rtol=1e-15)
    np.testing.assert_allclose(Jc[:, :3], [[0.25, 1, 0], [-0.125, 0, 1]], rtol=1e-15)
    np.testing.assert_allclose(Jp[:, 3:], Jx, rtol=1e-15)


@pytest.mark.parametrize("name", ce.CASES)
def test_references_agree_with_the_restatement_within_the_budget(name):
    worst, nonfinite, ill, counts = measured(name)
    budget = BUDGET["worst"][cmp.key(name)]
    quantities = cmp.VALUE_QUANTITIES + (cmp.JACOBIAN_QUANTITIES if ce.iteration_safe(name) else ()) + \
        ((cmp.ROW_QUANTITY,) if ce.regime(name) != "depth_tiny" else ())  # (compare_camera_edges.py says why not there)
    for q in quantities:
        print(f"{name} {q}: worst {worst.get(q, 0.0):.3f} of {counts.get(q, 0)} (budget {budget[q]})")
    for q in quantities:
        assert counts.get(q, 0) > 0 and worst[q] <= allowed(budget[q]), (name, q, worst[q], budget[q])
    # what is not finite or not comparable: only where the budget lists it by name, only in the two regimes allowed any
    assert set(nonfinite) <= set(BUDGET["nonfinite"]) and set(ill) <= set(BUDGET["ill_conditioned"])
    if nonfinite or ill:
        assert ce.regime(name) in NONFINITE_REGIMES
    n = len(ce.case_scene(name)["obs_image"])
    assert counts["sq_error_filter"] + len(ill) == n  # every other observation was compared


@pytest.mark.parametrize("name", ce.ITERATION_CASES)
def test_bundle_adjustment_accepts_a_step_on_every_iteration_case(name):
    """A run whose steps are all rejected returns its inputs, and a wrong Jacobian would show in nothing but a PCG count:
    under trivial_6 (and CAUCHY where it runs) the reference accepts at least one step and moves every block."""
    sc = ce.case_scene(name)
    for opt in ce.ba_options_of(name):
        res = ce.ba_reference(name, opt)
        print(f"{name} {opt}: {res['num_successful_steps']} accepted, {res['num_unsuccessful_steps']} rejected")
        if opt in ("trivial_6", "cauchy_2"):
            assert res["num_successful_steps"] >= 1 and res["final_cost"] < res["initial_cost"], (name, opt)
            n = len(sc["camera_params"][0])
            assert not np.array_equal(res["camera_params"][0, :n], sc["camera_params"][0])
            assert not np.array_equal(res["xyz"], sc["xyz"]) and not np.array_equal(res["qvec"][2], sc["qvec"][2])
            if sc["model"] == ce.FOV:
                assert res["camera_params"][0, 4] != sc["camera_params"][0][4] or sc["camera_params"][0][4] == 0.0


def test_rational_pole_at_the_zero_has_the_sign_and_size_of_its_quotient():
    """The four observations whose denominator is a rounding error are compared with no restatement (the budget lists them
    as ill_conditioned, in place of the issue's list of non-finite entries: the reference is finite there).  What can be
    said: along the point's axis the pixel's offset from the principal point is f u numerator / denominator with the
    denominator as the projection's own order of operations rounds it, in sign and within a factor of two."""
    import ba_ref_lib
    name = "rational_pole/FULL_OPENCV"
    sc = ce.case_scene(name)
    prm = sc["camera_params"][0]
    e = prm[4:]
    rows = [int(s.split("#")[1]) for s in BUDGET["ill_conditioned"]]
    assert len(rows) == 4 and all(sc["obs_image"][k] == 0 for k in rows)
    for k in rows:
        X = sc["xyz"][ce.obs_point(sc)[k]]
        _, r, _, _, _ = ba_ref_lib.observation(6, prm, sc["qvec"][0], sc["tvec"][0], X, [0.0, 0.0])
        assert np.isfinite(r).all()
        a = 0 if X[0] != 0 else 1
        u = X[a] / X[2]
        r2 = u * u
        want = prm[a] * u * (1.0 + e[0] * r2 + e[1] * r2 * r2 + e[4] * r2 * r2 * r2) / ce.rational_denominator(e, r2)
        got = r[a] - prm[2 + a]
        assert abs(want) > 1e14 and np.sign(got) == np.sign(want) and 0.5 < got / want < 2.0, (k, got, want)


def test_budget_covers_the_cases_and_lists_the_exceptions():
    assert set(BUDGET["worst"]) == {cmp.key(n) for n in ce.CASES}
    for entry in BUDGET["nonfinite"] + BUDGET["ill_conditioned"]:
        assert entry.split("/")[0] in NONFINITE_REGIMES
    assert len(BUDGET["ill_conditioned"]) == ce.census("rational_pole/FULL_OPENCV")["denominator_zero"]
    # a value beyond ten ulps is budgeted only where DESIGN.md 15.3a says why: next to the rational pole, and for the
    # polynomial models in wide_68_89, where a rotated image's small coordinate is a difference of terms a hundred times
    # its size and the radial factor of ten and more carries it far from the principal point
    conditioned = {"rational_pole/FULL_OPENCV"} | {f"wide_68_89/{ce.MODEL_NAMES[m]}" for m in ce.POLYNOMIAL}
    for k, w in BUDGET["worst"].items():
        for q in cmp.VALUE_QUANTITIES:
            assert w[q] <= 10.0 or k in conditioned, (k, q, w[q])


@pytest.mark.parametrize("model", ce.POLYNOMIAL, ids=[ce.MODEL_NAMES[m] for m in ce.POLYNOMIAL])
def test_oracle_lifts_on_strong_distortion(model):
    lm = cmp.lift_measure(model)
    n = len(lm["iterations"])
    inside = np.arange(n) < 126  # strong_pixels: the principal point, its neighbours and the pixels inside the fold
    # the float64 restatement of the Newton iteration reproduces the oracle, so its iteration counts are the oracle's
    assert lm["same_bits"].all()
    # inside the fold the iteration ends by its step bound, and its last step, below 1e-5, leaves an error of the order
    # of its square: 1e-6 pixels is ten times f * 1e-10 / (1 - 0.9 r^2) at the largest radius there
    assert (lm["iterations"][inside] < 100).all() and (lm["reprojection"][inside] <= 1e-6).all()
    assert lm["iterations"][:6].max() <= 2 and np.array_equal(ce.lift_reference(model)[0][:2], np.zeros((2, 2)))
    # past the fold nothing is promised: the bits are pinned by the fixture alone (below)
    rec = BUDGET["lifts"][ce.MODEL_NAMES[model]]
    assert int(lm["nonfinite"].sum()) <= rec["nonfinite_lifts"]
    assert cmp.project_measure(model) <= allowed(rec["img_from_cam_ulps"])
    print(f"strong_poly {ce.MODEL_NAMES[model]}: {int((lm['iterations'] == 100).sum())} lifts ran 100 iterations, "
          f"{int(lm['nonfinite'].sum())} not finite, worst reprojection inside the fold "
          f"{np.nanmax(lm['reprojection'][inside]):.3g} px")


# ---- the fixture ---------------------------------------------------------------------------------------------------------
def test_references_reproduce_the_fixture():
    spec = importlib.util.spec_from_file_location("make_camera_edges_ref_golden",
                                                  ROOT / "tests" / "golden" / "make_camera_edges_ref_golden.py")
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    digests, arrays = ce.golden()
    assert mk.digests() == digests
    live = mk.arrays()
    assert set(live) | {"digest_keys", "digest_values"} == set(arrays.files)
    for k, a in live.items():
        assert np.array_equal(ce.bits(a), ce.bits(arrays[k])), k
    assert ce.GOLDEN.stat().st_size < 100 * 1024


def test_summary_line():
    """per regime: observations, branches hit, worst deviations (values in ulps, Jacobians in DBL_EPSILON of the row)"""
    parts = []
    for reg in ce.REGIMES:
        names = [n for n in ce.CASES if ce.regime(n) == reg]
        nobs, branches, wv, wj = 0, {}, 0.0, 0.0
        for n in names:
            nobs += len(ce.case_scene(n)["obs_image"])
            for b, c in ce.census(n).items():
                if not b.startswith(("depth_ok", "r_gt_eps")):
                    branches[b] = branches.get(b, 0) + c
            for b, c in ce.observed_fov_atan(ce.case_scene(n)).items():
                branches["fov_arg_" + b] = branches.get("fov_arg_" + b, 0) + c
            w = measured(n)[0]
            wv = max([wv] + [w.get(q, 0.0) for q in cmp.VALUE_QUANTITIES])
            wj = max([wj] + [w.get(q, 0.0) for q in cmp.JACOBIAN_QUANTITIES + (cmp.ROW_QUANTITY,)])
        hit = ",".join(f"{b}:{c}" for b, c in sorted(branches.items()))
        lifts = ""
        if reg == "strong_poly":  # observed, not selected: the Newton iteration counts of the lifts and the non-finite lifts
            for m in ce.POLYNOMIAL:
                lm = cmp.lift_measure(m)
                it = lm["iterations"]
                lifts += (f"; {ce.MODEL_NAMES[m]} lifts: iterations median {int(np.median(it))} max inside fold "
                          f"{int(it[:126].max())}, {int((it == 100).sum())} ran 100, {int(lm['nonfinite'].sum())} non-finite")
        parts.append(f"{reg}[obs {nobs}; {hit}; values {wv:.2f} ulp; jacobians {wj:.1f} eps{lifts}]")
    print("camera edges: " + " | ".join(parts))
    assert len(parts) == len(ce.REGIMES)
