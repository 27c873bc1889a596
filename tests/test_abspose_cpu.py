"""Absolute pose without a GPU: the pycolmap surface (names, defaults, option protocol, THROW_CHECK errors, the
out-of-scope options), the C header, and the CPU reference (tests/abspose_ref) against known answers, independent
numpy / scipy restatements, numpy's transcendentals and the frozen fixture."""
import math
import pickle
from pathlib import Path

import numpy as np
import pytest

import abspose_cases
import abspose_ref_lib as ref
from pycolmap_amd import synth

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "abspose_ref_v1.npz"
RECORDED = ROOT / "tests" / "golden" / "absolute_pose_reference_v1.npz"


# ---- the pycolmap surface -------------------------------------------------------------------------------------------
def test_names_defaults_and_option_protocol():
    import pycolmap
    import pycolmap_amd as pc
    for n in ("absolute_pose_estimation", "pose_refinement", "AbsolutePoseEstimationOptions",
              "AbsolutePoseRefinementOptions"):
        assert getattr(pycolmap, n) is getattr(pc, n)
    e = pc.AbsolutePoseEstimationOptions()
    assert (e.estimate_focal_length, e.num_focal_length_samples, e.min_focal_length_ratio, e.max_focal_length_ratio) == \
        (False, 30, 0.1, 10.0)
    r0 = pc.RANSACOptions()
    assert e.ransac.max_error == 12.0
    for k in ("min_inlier_ratio", "confidence", "dyn_num_trials_multiplier", "min_num_trials", "max_num_trials"):
        assert getattr(e.ransac, k) == getattr(r0, k)
    r = pc.AbsolutePoseRefinementOptions()
    assert r.todict() == dict(gradient_tolerance=1.0, max_num_iterations=100, loss_function_scale=1.0,
                              refine_focal_length=False, refine_extra_params=False, print_summary=False)
    e2 = pc.AbsolutePoseEstimationOptions({"estimate_focal_length": True, "ransac": {"max_error": 3.0}})
    assert e2.estimate_focal_length and e2.ransac.max_error == 3.0 and e2.ransac.min_num_trials == 1000
    e3 = pc.AbsolutePoseEstimationOptions(num_focal_length_samples=7)
    e3.mergedict({"min_focal_length_ratio": 0.5})
    assert (e3.num_focal_length_samples, e3.min_focal_length_ratio) == (7, 0.5)
    assert e3.todict()["ransac"]["max_error"] == 12.0 and "num_focal_length_samples" in e3.summary()
    e4 = pickle.loads(pickle.dumps(e3))
    assert e4.todict() == e3.todict()
    r2 = pickle.loads(pickle.dumps(pc.AbsolutePoseRefinementOptions(max_num_iterations=5)))
    assert r2.max_num_iterations == 5


def test_throw_check_and_out_of_scope_options_raise():
    import pycolmap_amd as pc
    cam = pc.Camera(model="SIMPLE_PINHOLE", width=100, height=100, params=[100.0, 50.0, 50.0])
    with pytest.raises(ValueError, match=r"points2D.size\(\) == points3D.size\(\) \(3 vs. 4\)"):
        pc.absolute_pose_estimation(np.zeros((3, 2)), np.zeros((4, 3)), cam)
    with pytest.raises(ValueError, match=r"inlier_mask.size\(\) == points2D.size\(\) \(2 vs. 3\)"):
        pc.pose_refinement(pc.Rigid3d(), np.zeros((3, 2)), np.zeros((3, 3)), [True, False], cam)
    with pytest.raises(ValueError, match="N x 2"):
        pc.absolute_pose_estimation(np.zeros((3, 3)), np.zeros((3, 3)), cam)
    for k in ("refine_focal_length", "refine_extra_params"):
        ro = pc.AbsolutePoseRefinementOptions({k: True})
        with pytest.raises(ValueError, match=f"{k}=True is not supported"):
            pc.absolute_pose_estimation(np.zeros((3, 2)), np.zeros((3, 3)), cam, refinement_options=ro)
        with pytest.raises(ValueError, match=f"{k}=True is not supported"):
            pc.pose_refinement(pc.Rigid3d(), np.zeros((3, 2)), np.zeros((3, 3)), [True] * 3, cam, ro)


def test_header_names_the_entry_points():
    h = (ROOT / "include" / "amc_abspose.h").read_text()
    for name in ("amc_estimate_absolute_poses", "amc_refine_absolute_poses", "amc_abspose_result_free",
                 "amc_abspose_opts_default", "amc_abspose_refine_opts_default"):
        assert name in h


# ---- transcendentals and the focal loop -----------------------------------------------------------------------------
def ulps(a, b):
    ia = np.array([a]).view(np.int64)[0]
    ib = np.array([b]).view(np.int64)[0]
    ia = ia if ia >= 0 else -(ia & 0x7fffffffffffffff)
    ib = ib if ib >= 0 else -(ib & 0x7fffffffffffffff)
    return abs(int(ia) - int(ib))


@pytest.mark.parametrize("fn,lo,hi", [("atan", -50.0, 50.0), ("sin", -20.0, 20.0), ("cos", -20.0, 20.0),
                                      ("log", 1.0, 1e6)])
def test_own_transcendentals_within_one_ulp_of_numpy(fn, lo, hi):
    rng = np.random.default_rng(7)
    xs = np.concatenate([rng.uniform(lo, hi, 20000), rng.uniform(-1e-3, 1e-3, 2000) + (1.0 if fn == "log" else 0.0),
                         [0.4375, 1.1875, 2.4375, math.pi / 4, math.pi / 2, 3 * math.pi / 4] if fn != "log" else
                         [1.0, 2.0, 1.0 + 2 ** -30, math.e]])
    npf = {"atan": np.arctan, "sin": np.sin, "cos": np.cos, "log": np.log}[fn]
    worst = max(ulps(ref.scalar(fn, x), float(npf(x))) for x in xs)
    assert worst <= 1, f"{fn}: {worst} ulp"
    assert math.isnan(ref.scalar(fn, float("nan")))


@pytest.mark.parametrize("k", [1, 3, 7, 10, 30, 49, 100])
def test_focal_factor_count_matches_the_literal_loop(k):
    want, f = [], 0.0
    while f <= 1.0:  # for (double f = 0; f <= 1.0; f += 1.0 / k) with host doubles
        want.append(0.1 + (10.0 - 0.1) * f * f)
        f += 1.0 / k
    got = ref.focal_factors(estimate_focal_length=1, num_focal_length_samples=k)
    assert np.array_equal(got, np.array(want))
    assert np.array_equal(ref.focal_factors(), [1.0])


# ---- the reference against known answers ----------------------------------------------------------------------------
def rel_pose_error(r, sc):
    dq = np.abs(np.abs((r["qvec"] * sc["qvec"]).sum(1)) - 1.0)
    dt = np.linalg.norm(r["tvec"] - sc["tvec"], axis=1) / np.linalg.norm(sc["tvec"], axis=1)
    return dq.max(), dt.max()


@pytest.mark.parametrize("model", range(11))
def test_noise_free_queries_recover_the_pose(model):
    sc = abspose_cases.scene(100 + model, 2, 150, outlier_frac=0.25, noise_px=0.0, model=model)
    r = ref.estimate(sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"], sc["points3D"])
    assert r["success"].all()
    dq, dt = rel_pose_error(r, sc)
    assert dq < 1e-12 and dt < 1e-9, (dq, dt)
    assert np.array_equal(r["inlier_mask"], ~sc["outlier"])


def random_triangle(rng):
    R, q = synth.random_rotation(rng)
    t = rng.normal(size=3)
    Xc = np.stack([rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3), rng.uniform(2, 6, 3)], axis=1)
    X = (Xc - t) @ R
    return R, t, Xc[:, :2] / Xc[:, 2:], X


def test_p3p_returns_the_true_pose_on_random_triangles():
    rng = np.random.default_rng(3)
    hits = 0
    for _ in range(200):
        R, t, uv, X = random_triangle(rng)
        models = ref.p3p(uv, X)
        assert len(models) <= 4
        err = [np.abs(m[:, :3] - R).max() + np.abs(m[:, 3] - t).max() for m in models]
        hits += bool(err) and min(err) < 1e-7
    assert hits >= 198


def p3p_numpy(uv, X):
    """P3P restated independently: the same two law-of-cosines quadratics in y, but their resultant in x is the
    determinant of the 4 x 4 Sylvester matrix, evaluated at 9 points and interpolated (np.polyfit), roots by np.roots,
    distances back-substituted by solving the quadratic pair numerically, Umeyama by np.linalg.svd."""
    b = np.hstack([uv, np.ones((3, 1))])
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    cuv, cuw, cvw = b[0] @ b[1], b[0] @ b[2], b[1] @ b[2]
    AB2, AC2, BC2 = [np.sum((X[i] - X[j]) ** 2) for i, j in ((0, 1), (0, 2), (1, 2))]
    a, bb = BC2 / AB2, AC2 / AB2
    p, q, r = 2 * cvw, 2 * cuw, 2 * cuv

    def quads(x):  # y^2, y, 1 coefficients of both equations at x
        return (np.array([1 - a, a * r * x - p, 1 - a * x * x]),
                np.array([-bb, bb * r * x, (1 - bb) * x * x - q * x + 1]))

    def sylvester(x):
        f, g = quads(x)
        return np.linalg.det(np.array([[*f, 0], [0, *f], [*g, 0], [0, *g]]))

    xs = np.linspace(-2.0, 2.0, 9)
    quart = np.polyfit(xs, [sylvester(x) for x in xs], 4)
    out = []
    for x in np.roots(quart):
        if abs(x.imag) > 1e-8 or x.real < 0:
            continue
        x = x.real
        f, g = quads(x)
        yr = [y.real for y in np.roots(f) if abs(y.imag) < 1e-6]
        if not yr:
            continue
        y = min(yr, key=lambda y: abs(np.polyval(g, y)))  # the common root of both quadratics
        nu = x * x + y * y - 2 * x * y * cuv
        if nu <= 0:
            continue
        PC = math.sqrt(AB2) / math.sqrt(nu)
        Xc = np.stack([b[0] * x * PC, b[1] * y * PC, b[2] * PC])
        ms, md = X.mean(0), Xc.mean(0)
        U, _, Vt = np.linalg.svd((Xc - md).T @ (X - ms))
        S = np.diag([1, 1, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
        Rm = U @ S @ Vt
        out.append(np.hstack([Rm, (md - Rm @ ms)[:, None]]))
    return out


def test_p3p_matches_a_numpy_restatement():
    rng = np.random.default_rng(4)
    for _ in range(100):
        _, _, uv, X = random_triangle(rng)
        mine, theirs = ref.p3p(uv, X), p3p_numpy(uv, X)
        # both directions: every solution of one is a solution of the other (up to the conditioning of the root)
        for m in theirs:
            assert min(np.abs(m - k).max() for k in mine) < 1e-5
        for k in mine:
            if np.isfinite(k).all() and np.abs(k).max() < 1e6:
                assert min((np.abs(m - k).max() for m in theirs), default=np.inf) < 1e-5


def test_epnp_is_exact_on_noise_free_points():
    rng = np.random.default_rng(5)
    for n in (6, 10, 50, 500):
        R, _ = synth.random_rotation(rng)
        t = rng.normal(size=3)
        Xc = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(3, 8, n)], axis=1)
        X = (Xc - t) @ R
        P = ref.epnp(Xc[:, :2] / Xc[:, 2:], X)
        assert P is not None
        assert np.abs(P[:, :3] - R).max() < 1e-8 and np.abs(P[:, 3] - t).max() < 1e-8, n


def robust_cost(sc, q, t, mask, scale=1.0):
    R, _ = quat_to_R(q), None
    Xc = sc["points3D"] @ R.T + t
    x, y = synth.img_from_cam(sc["camera_models"][0], sc["camera_params"][0], Xc[:, :2] / Xc[:, 2:]).T
    s = (x - sc["points2D"][:, 0]) ** 2 + (y - sc["points2D"][:, 1]) ** 2
    return 0.5 * np.sum(scale ** 2 * np.log1p(s[mask] / scale ** 2))


def quat_to_R(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def perturbed(sc, seed, rot=0.02, trans=0.1):
    rng = np.random.default_rng(seed)
    q = sc["qvec"] + rng.normal(scale=rot, size=sc["qvec"].shape)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q, sc["tvec"] + rng.normal(scale=trans, size=sc["tvec"].shape)


def test_refinement_lowers_the_robust_cost_and_converges():
    sc = abspose_cases.scene(200, 1, 300, outlier_frac=0.2, noise_px=1.0, model=1)
    mask = ~sc["outlier"]
    q0, t0 = perturbed(sc, 1)
    r = ref.refine(sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"], sc["points3D"], q0, t0,
                   mask, dict(gradient_tolerance=1e-10))
    assert r["success"][0]
    c0, c1 = robust_cost(sc, q0[0], t0[0], mask), robust_cost(sc, r["qvec"][0], r["tvec"][0], mask)
    assert c1 < 0.5 * c0 and c1 <= robust_cost(sc, sc["qvec"][0], sc["tvec"][0], mask)
    assert np.linalg.norm(r["tvec"][0] - sc["tvec"][0]) < 0.05
    # from two different starts to the same minimum, up to where the function tolerance (1e-6 of the cost) stops LM
    q1, t1 = perturbed(sc, 2)
    r2 = ref.refine(sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"], sc["points3D"], q1, t1,
                    mask, dict(gradient_tolerance=1e-10))
    assert np.abs(r2["tvec"] - r["tvec"]).max() < 1e-4


def test_refinement_matches_scipy_least_squares_cauchy():
    scipy_opt = pytest.importorskip("scipy.optimize")
    from scipy.spatial.transform import Rotation
    converged = 0
    for seed, model, scale in ((201, 1, 1.0), (202, 4, 2.0), (203, 9, 1.0)):
        sc = abspose_cases.scene(seed, 1, 300, outlier_frac=0.2, noise_px=1.0, model=model)
        mask = ~sc["outlier"]
        q0, t0 = perturbed(sc, seed, rot=0.005, trans=0.02)
        r = ref.refine(sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"], sc["points3D"], q0, t0,
                       mask, dict(gradient_tolerance=1e-12, loss_function_scale=scale))
        prm = sc["camera_params"][0]

        def fun(z):
            R = Rotation.from_rotvec(z[:3]).as_matrix()
            Xc = sc["points3D"][mask] @ R.T + z[3:]
            x, y = synth.img_from_cam(model, prm, Xc[:, :2] / Xc[:, 2:]).T
            # Ceres robustifies the squared norm of each 2-vector block; scipy each scalar: one residual per block
            return np.hypot(x - sc["points2D"][mask, 0], y - sc["points2D"][mask, 1])

        z0 = np.concatenate([Rotation.from_quat(q0[0]).as_rotvec(), t0[0]])
        sol = scipy_opt.least_squares(fun, z0, loss="cauchy", f_scale=scale, xtol=1e-15, ftol=1e-15, gtol=1e-15,
                                      max_nfev=5000)
        # LM stops once a step changes the cost by less than 1e-6 of it (Ceres' function tolerance), so the two agree
        # on the cost to that order and on the pose to about 1e-5 of the scene's scale
        Rs = Rotation.from_rotvec(sol.x[:3])
        dang = (Rs.inv() * Rotation.from_quat(r["qvec"][0])).magnitude()
        mine = robust_cost(sc, r["qvec"][0], r["tvec"][0], mask, scale)
        assert mine <= sol.cost * (1 + 2e-6), (model, mine, sol.cost)
        if not sol.success:  # (scipy's trust region may crawl on the norm residual's kink; ours is not worse)
            continue
        assert abs(mine - sol.cost) <= 2e-6 * sol.cost, (model, mine, sol.cost)
        assert dang < 5e-5 and np.abs(sol.x[3:] - r["tvec"][0]).max() < 5e-4, (model, dang, sol.x[3:] - r["tvec"][0])
        converged += 1
    assert converged >= 2


def test_covariance_is_symmetric_positive_and_shrinks_with_more_points():
    covs = []
    for n in (50, 800):
        sc = abspose_cases.scene(300, 1, n, outlier_frac=0.0, noise_px=1.0)
        r = ref.estimate(sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"], sc["points3D"],
                         return_covariance=True)
        c = r["covariance"][0]
        assert r["success"][0] and np.allclose(c, c.T, rtol=1e-9, atol=0) and np.linalg.eigvalsh(c).min() > 0
        covs.append(np.trace(c))
    assert covs[1] < covs[0]


# ---- the frozen fixture and the real-pycolmap recording -------------------------------------------------------------
def test_reference_matches_frozen_fixture():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mk", ROOT / "tests" / "golden" / "make_abspose_ref_golden.py")
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    g = np.load(GOLDEN)
    for name, (sc, est, rf, cov) in mk.fixture_cases(g).items():
        r = ref.estimate(sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"], sc["points3D"], est,
                         rf, cov)
        for k in mk.FIELDS:
            if k in r:
                assert np.array_equal(np.asarray(r[k]), g[f"{name}/{k}"]), f"{name}: {k}"


@pytest.mark.skipif(not RECORDED.exists(), reason="no recording of real pycolmap (tests/golden/"
                                                  "make_absolute_pose_reference_golden.py writes it)")
def test_agreement_with_recorded_pycolmap():
    g = np.load(GOLDEN)
    rec = np.load(RECORDED)
    agree, poses = [], 0
    for name in sorted({k.split("/")[0] for k in rec.files}):
        if f"{name}/qvec" not in g.files:
            continue
        ok = rec[f"{name}/success"] & g[f"{name}/success"]
        dq = np.abs(np.abs((rec[f"{name}/qvec"] * g[f"{name}/qvec"]).sum(1)) - 1.0)
        poses += int((ok & (dq < 1e-6)).sum())
        agree.append((rec[f"{name}/inlier_mask"] == g[f"{name}/inlier_mask"]).mean())
    both = sum(int((rec[f"{n}/success"] & g[f"{n}/success"]).sum()) for n in sorted({k.split("/")[0] for k in rec.files})
               if f"{n}/qvec" in g.files)
    print(f"pycolmap agreement: {poses} of {both} poses within 1e-6, inlier-mask agreement {np.mean(agree):.4f}")
    assert np.mean(agree) > 0.95
    assert poses >= 0.9 * both


# ---- the edge cases: what abspose_cases.cases() leaves out ---------------------------------------------
GOLDEN_EDGES = ROOT / "tests" / "golden" / "abspose_ref_edges_v1.npz"
EDGES = abspose_cases.EDGE_CASES


def maker():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mk", ROOT / "tests" / "golden" / "make_abspose_ref_golden.py")
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk


@pytest.fixture(scope="module")
def golden_edges():
    return maker().load_edges()


@pytest.fixture(scope="module")
def solved_edges():
    """the reference on every edge case, once: name -> (result, trace rows or None)"""
    mk = maker()
    return {name: mk.edge_reference(name) for name in EDGES}


def test_edge_fixture_lists_the_edge_cases(golden_edges):
    assert sorted(golden_edges) == sorted(EDGES)
    assert GOLDEN_EDGES.stat().st_size < 20_000
    assert len(abspose_cases.cases()) == 23


@pytest.mark.parametrize("name", sorted(EDGES))
def test_reference_equals_its_edge_fixture_bit_for_bit(name, golden_edges, solved_edges):
    r, tr = solved_edges[name]
    want_digest, want_trace = golden_edges[name]
    assert abspose_cases.digest(r) == want_digest
    assert (tr is None) == (want_trace is None) and (tr is None or np.array_equal(tr, want_trace))


def test_trace_records_and_does_not_compute(solved_edges):
    for name in ("refine_model4", "refine_count1_cov", "refine_nan_quat", "refine_min_radius"):
        plain = abspose_cases.edge_run(name, ref.estimate, ref.refine)
        assert abspose_cases.digest(plain) == abspose_cases.digest(solved_edges[name][0]), name


def test_edge_cases_reach_the_exits_and_paths(solved_edges):
    """by the reference's own results and trace and the cases' own shapes, so that the list cannot decay"""
    res = {n: solved_edges[n][0] for n in EDGES}
    trace = {n: dict(zip(ref.TRACE_FIELDS, solved_edges[n][1].T)) for n in EDGES if solved_edges[n][1] is not None}
    exits = lambda n: [ref.EXITS[e] for e in trace[n]["exit"]]  # noqa: E731
    sizes = lambda n: np.diff(EDGES[n][1]["offsets"].astype(np.int64)).tolist()  # noqa: E731
    kinds = {n: EDGES[n][0] for n in EDGES}
    assert set(trace) == {n for n in EDGES if kinds[n] == "refine"}
    for n in EDGES:
        assert max(sizes(n)) <= (200 if kinds[n] == "estimate" else 129), n

    # the lane edges
    for n in (63, 64, 65, 127, 128, 129):
        kind, _, est, _, cov = EDGES[f"n{n}"]
        assert sizes(f"n{n}") == [n] and est == abspose_cases.FAST and cov == (n % 2 == 1)
        assert res[f"n{n}"]["success"].all()
    for k in (64, 65):
        sc = EDGES[f"inliers{k}"][1]
        assert sizes(f"inliers{k}") == [100] and int(sc["outlier"].sum()) == 100 - k
        assert res[f"inliers{k}"]["num_inliers"].tolist() == [k] and res[f"inliers{k}"]["success"].all()
        assert np.array_equal(res[f"inliers{k}"]["inlier_mask"], ~sc["outlier"])

    # RANSAC control
    assert EDGES["trials_equal"][2] == dict(min_num_trials=50, max_num_trials=50)
    assert res["trials_equal"]["num_trials"].tolist() == [50] and res["trials_equal"]["success"].all()
    assert EDGES["one_trial"][2]["max_num_trials"] == 1 and res["one_trial"]["num_trials"].tolist() == [1]
    est = EDGES["ratio_clamp"][2]
    eo, _ = ref.abspose_options(est, None)
    clamp = math.ceil(math.log(1.0 - eo.confidence) / math.log(1.0 - est["min_inlier_ratio"] ** 3)
                      * eo.dyn_num_trials_multiplier)
    assert est["min_inlier_ratio"] == 0.5 and abs(EDGES["ratio_clamp"][1]["outlier"].mean() - 0.6) < 0.1
    assert res["ratio_clamp"]["num_trials"].tolist() == [clamp] and clamp < est["max_num_trials"]
    # confidence 0: ComputeNumTrials is 0 for every inlier count, so the constructor's clamp leaves no trial at all;
    # confidence 1: it is the largest count, so nothing stops a run before max_num_trials
    assert EDGES["confidence0"][2]["confidence"] == 0.0 and EDGES["confidence1"][2]["confidence"] == 1.0
    assert res["confidence0"]["num_trials"].tolist() == [0] and not res["confidence0"]["success"].any()
    assert res["confidence1"]["num_trials"].tolist() == [abspose_cases.FAST["max_num_trials"]]
    assert res["confidence1"]["success"].all()
    # the sample stream's overrun: the middle query alone draws past the first table
    assert EDGES["overrun_shared_launch"][2] == abspose_cases.OVERRUN and sizes("overrun_shared_launch") == [40, 120, 200]
    assert abspose_cases.FIRST_STREAM_WORDS == 3 * 2000 + 1024
    assert (3 * res["overrun_shared_launch"]["num_trials"] > abspose_cases.FIRST_STREAM_WORDS).tolist() == \
        [False, True, False]
    assert res["overrun_shared_launch"]["success"].all()
    sc, est, rf, cov = abspose_cases.cases()["outliers80"]
    r80 = ref.estimate(sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"], sc["points3D"], est, rf,
                       cov)
    assert est == {} and (3 * r80["num_trials"] > abspose_cases.FIRST_STREAM_WORDS).all()

    # focal-length estimation
    for m in (1, 4, 5, 7, 8, 10):
        kind, sc, est, _, cov = EDGES[f"focal_model{m}"]
        assert sc["camera_models"].tolist() == [m] and sizes(f"focal_model{m}") == [150] and cov
        assert est == dict(estimate_focal_length=1, num_focal_length_samples=4, min_num_trials=30, max_num_trials=500)
        assert res[f"focal_model{m}"]["success"].all() and res[f"focal_model{m}"]["focal_factor"][0] != 1.0
    kind, sc, est, rf, cov = EDGES["focal_tie"]
    factors = ref.focal_factors(**{k: v for k, v in est.items() if "focal" in k})
    assert len(factors) == 7 and factors[0] == 0.9 and sizes("focal_tie") == [80]
    alone = dict({k: v for k, v in est.items() if "focal" not in k})
    for f in factors:  # each factor alone, as a camera scaled beforehand: all count every correspondence
        prm = [sc["camera_params"][0] * np.array([f, 1.0, 1.0])]
        one = ref.estimate(sc["offsets"], sc["camera_models"], prm, sc["points2D"], sc["points3D"], alone, rf, cov)
        assert one["success"].all() and one["num_inliers"].tolist() == [80], f
    assert res["focal_tie"]["focal_factor"].tolist() == [0.9] and res["focal_tie"]["num_inliers"].tolist() == [80]
    assert res["focal_tie"]["success"].all()
    r = res["focal_all_fail"]
    assert EDGES["focal_all_fail"][2]["estimate_focal_length"] == 1 and sizes("focal_all_fail") == [2, 60]
    assert not r["success"].any() and r["focal_factor"].tolist() == [0.0, 0.0] and not r["inlier_mask"].any()
    assert r["num_inliers"].tolist() == [0, 0] and not r["qvec"].any() and not r["tvec"].any()
    sc = EDGES["focal_mixed_batch"][1]
    assert sc["camera_models"].tolist() == [0, 5, 4, 7, 1, 10, 2, 8, 6, 9]
    n = sizes("focal_mixed_batch")
    assert n[6] == 0 and n[7] == 2 and all(40 <= v <= 130 for i, v in enumerate(n) if i not in (6, 7))
    assert EDGES["focal_mixed_batch"][2]["num_focal_length_samples"] == 4
    assert res["focal_mixed_batch"]["success"].tolist() == [i not in (6, 7) for i in range(10)]

    # refinement alone
    for m in range(11):
        assert EDGES[f"refine_model{m}"][1]["camera_models"].tolist() == [m] and sizes(f"refine_model{m}") == [120]
        assert res[f"refine_model{m}"]["success"].all() and trace[f"refine_model{m}"]["accepted"][0] > 0
    for k in (0, 1, 2, 3, 4, 64, 65):
        for suffix, cov in (("", False), ("_cov", True)):
            name = f"refine_count{k}{suffix}"
            sc = EDGES[name][1]
            assert sc["camera_models"].tolist() == [4] and sizes(name) == [100] and EDGES[name][4] == cov
            assert int(sc["mask"].sum()) == k and res[name]["num_inliers"].tolist() == [k]
            assert res[name]["success"].tolist() == [not (cov and k in (1, 2))], name
            assert trace[name]["rank_failed"].tolist() == [int(cov and k in (1, 2))], name
        assert exits(f"refine_count{k}") == exits(f"refine_count{k}_cov")
    for suffix in ("", "_cov"):
        name = f"refine_count0{suffix}"
        assert exits(name) == ["NOTHING_TO_REFINE"]
        assert np.array_equal(res[name]["qvec"].view(np.uint64), EDGES[name][1]["start_q"].view(np.uint64))
        assert np.array_equal(res[name]["tvec"].view(np.uint64), EDGES[name][1]["start_t"].view(np.uint64))
    assert not res["refine_count0_cov"]["covariance"].any() and not res["refine_count1_cov"]["covariance"].any()
    for n in (63, 64, 65, 129):
        assert sizes(f"refine_n{n}") == [n] and EDGES[f"refine_n{n}"][1]["mask"].all()
        assert res[f"refine_n{n}"]["success"].all()
    assert sizes("refine_empty_between")[1] == 0 and min(sizes("refine_empty_between")[::2]) > 0
    assert res["refine_empty_between"]["success"].all() and exits("refine_empty_between")[1] == "NOTHING_TO_REFINE"
    assert trace["refine_empty_between"]["accepted"][[0, 2]].min() > 0
    assert np.isnan(EDGES["refine_nan_quat"][1]["start_q"][0]).any()
    for name, ok in (("refine_nan_quat", False), ("refine_nan_point_in_mask", False),
                     ("refine_nan_point_outside_mask", True)):
        assert res[name]["success"].tolist() == [ok, True], name
        assert (exits(name)[0] == "NOT_FINITE_START") == (not ok), name
    for name, inside in (("refine_nan_point_in_mask", True), ("refine_nan_point_outside_mask", False)):
        sc = EDGES[name][1]
        bad = np.isnan(sc["points3D"]).any(axis=1)
        assert bad.sum() == 1 and bad[:60].any() and sc["mask"][bad].tolist() == [inside]

    # the exits
    for it in (0, 1, 3):
        name = f"refine_iterations{it}"
        assert EDGES[name][3] == dict(gradient_tolerance=0.0, max_num_iterations=it)
        assert exits(name) == ["MAX_ITERATIONS"] and trace[name]["iterations"].tolist() == [it]
    moved = lambda name: (np.abs(res[name]["tvec"] - EDGES[name][1]["start_t"]).max())  # noqa: E731
    assert moved("refine_iterations0") == 0.0 and moved("refine_iterations1") > 0.0
    assert EDGES["refine_far_start"][3] == dict(gradient_tolerance=0.0) and trace["refine_far_start"]["accepted"][0] >= 5
    assert np.abs(EDGES["refine_far_start"][1]["start_t"] - EDGES["refine_far_start"][1]["tvec"]).max() > 1.0
    assert EDGES["refine_at_optimum"][3] == {} and exits("refine_at_optimum") == ["GRADIENT_AT_START"]
    assert trace["refine_at_optimum"]["iterations"].tolist() == [0] and moved("refine_at_optimum") == 0.0
    assert exits("refine_function_tolerance") == ["FUNCTION_TOLERANCE"]
    assert exits("refine_parameter_tolerance") == ["PARAMETER_TOLERANCE"]
    assert trace["refine_function_tolerance"]["accepted"][0] > 0 and trace["refine_parameter_tolerance"]["accepted"][0] > 0
    t = trace["refine_rejected_then_accepted"]
    assert t["accepted"][0] > 0 and t["rejected"][0] > 0 and res["refine_rejected_then_accepted"]["success"].all()
    assert exits("refine_invalid_steps") == ["INVALID_STEPS"] and trace["refine_invalid_steps"]["invalid"].tolist() == [5]
    assert not res["refine_invalid_steps"]["success"].any() and moved("refine_invalid_steps") == 0.0
    assert exits("refine_min_radius") == ["MIN_RADIUS"] and trace["refine_min_radius"]["rejected"].tolist() == [15]
    assert res["refine_min_radius"]["success"].all() and moved("refine_min_radius") == 0.0
    reached = {e for n in trace for e in exits(n)}
    assert reached == set(ref.EXITS), sorted(set(ref.EXITS) - reached)
    assert any(trace[n]["exit"][i] == ref.EXITS.index("GRADIENT_AFTER_STEP") and trace[n]["accepted"][i] > 0
               for n in trace for i in range(len(trace[n]["exit"])))
    assert any(t["rank_failed"].any() for t in trace.values())
    assert any(((t["accepted"] > 0) & (t["rejected"] > 0)).any() for t in trace.values())
