"""Bundle-adjustment covariance without a GPU: the pycolmap surface and the option protocol, the
header against _capi, the sequential reference (tests/bacov_ref) against its frozen fixture, against an independent numpy
restatement (tests/ref2/bacov_ref2.py) within the recorded budget, against hand-built problems whose answers are exact and
against section 12.8's single-image covariance; the relative-pose propagation against central differences; the host plan
under ASan + UBSan in a stand-alone program; estimate_ba_covariance with the reference in the library's place."""
import copy
import ctypes as C
import json
import pickle
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "ref2"))

import bacov_cases  # noqa: E402
import bacov_ref2  # noqa: E402
import bacov_ref_lib as ref  # noqa: E402
import pycolmap  # noqa: E402
import pycolmap_amd  # noqa: E402
from pycolmap_amd import _ba_covariance, _capi  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "bacov_ref_v1.npz"
BUDGET_PATH = ROOT / "tests" / "ref2" / "bacov_deviation_budget.json"
OK_CASES = [c["name"] for c in bacov_cases.cases() if c["expect"] == "ok" and c["m"] > 0]


@pytest.fixture(scope="module")
def budget():
    """the committed record of tests/golden/make_bacov_ref_golden.py --budget: the bounds below are read, not recomputed"""
    return json.loads(BUDGET_PATH.read_text())


@pytest.fixture(scope="module")
def results():
    return {c["name"]: ref.ba_covariance(*c["problem"], options=c["options"], point_const=c["point_const"])
            for c in bacov_cases.cases()}


# ---- surface ------------------------------------------------------------------------------------------------------------
def test_names_resolve_through_import_pycolmap():
    for name in ("BACovariance", "BACovarianceOptions", "BACovarianceOptionsParams", "estimate_ba_covariance"):
        assert getattr(pycolmap, name) is getattr(pycolmap_amd, name) and name in pycolmap._PUBLIC
    assert "estimate_ba_covariance" in pycolmap.__doc__ and "BACovarianceOptions" in pycolmap.__doc__
    assert [p.name for p in pycolmap.BACovarianceOptionsParams] == ["POSES", "POINTS", "POSES_AND_POINTS", "ALL"]
    with pytest.raises(AttributeError, match="estimate_ba_covariance.*DESIGN.md section 24"):
        pycolmap.Sim3d
    # helpers of the module are not part of the surface
    assert not hasattr(pycolmap, "relative_pose_jacobian") and not hasattr(pycolmap, "FLAT_KEYS")
    for name in ("get_cam_from_world_cov", "get_point_cov", "get_camera_cov", "variable_camera_param_idxs",
                 "get_cam_cross_cov", "get_cam2_from_cam1_cov", "last_run_stats"):
        assert callable(getattr(pycolmap.BACovariance, name))


def test_option_protocol():
    P = pycolmap.BACovarianceOptionsParams
    o = pycolmap.BACovarianceOptions()
    assert o.params == P.ALL and o.damping == 1e-8 and o.todict() == {"params": P.ALL, "damping": 1e-8}
    assert not hasattr(o, "experimental_custom_poses")
    assert pycolmap.BACovarianceOptions({"params": P.POSES}).params == P.POSES
    assert pycolmap.BACovarianceOptions(damping=1, params="points").todict() == {"params": P.POINTS, "damping": 1.0}
    o.mergedict({"damping": 0.5})
    o.params = P.POSES_AND_POINTS
    assert "params = POSES_AND_POINTS" in o.summary() and "damping: float = 0.5" in o.summary(True)
    for clone in (copy.copy(o), copy.deepcopy(o), pickle.loads(pickle.dumps(o)), pycolmap.BACovarianceOptions(o)):
        assert clone == o and clone is not o
    clone.damping = 2.0
    assert clone != o and o.damping == 0.5
    with pytest.raises(ValueError, match="unknown option 'dampin'"):
        pycolmap.BACovarianceOptions(dampin=1.0)
    with pytest.raises(TypeError):
        o.damping = "1"
    with pytest.raises(TypeError):
        o.params = 1.5
    with pytest.raises(ValueError):
        o.params = "CAMERAS"
    with pytest.raises(TypeError):
        pycolmap.BACovarianceOptions({}, damping=1.0)
    bad = pycolmap.BACovarianceOptions(damping=-1.0)
    with pytest.raises(ValueError, match="damping"):
        bad.check()


def test_header_agrees_with_capi():
    header = (ROOT / "include" / "amc_bacov.h").read_text()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for struct, cls in (("amc_bacov_opts", _capi.BacovOpts), ("amc_bacov_result", _capi.BacovResult)):
        text = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), body, flags=re.S).group(1)
        names = [n for decl in text.split(";") for n in re.findall(r"\**(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.strip())]
        assert names == [f[0] for f in cls._fields_], (struct, names)
    assert "#define AMC_BACOV_MAX_COLUMNS 8192" in header and _capi.BACOV_MAX_COLUMNS == 8192
    assert "enum { AMC_BACOV_PHASES = 5 }" in header and len(_capi.BACOV_PHASES) == 5
    assert ("int amc_ba_covariance(amc_ctx* ctx, const amc_ba_problem* problem, const uint8_t* point_const,\n"
            "                      const amc_bacov_opts* options, amc_bacov_result* result);") in header
    lib = _capi.load()
    for name in ("amc_bacov_opts_default", "amc_ba_covariance", "amc_bacov_result_free"):
        assert hasattr(lib, name) and name in _capi.EXPORTED_SYMBOLS and name in header
    assert lib.amc_abi_version() == 5
    o = _capi.BacovOpts()
    lib.amc_bacov_opts_default(C.byref(o))
    d = _capi.bacov_options()
    for name, _ in _capi.BacovOpts._fields_:
        assert getattr(o, name) == getattr(d, name), name
    assert (o.loss_function_type, o.want_points, o.want_matrix, o.loss_function_scale, o.damping) == (0, 1, 1, 1.0, 1e-8)
    assert C.sizeof(_capi.BacovOpts) == 32 and C.sizeof(_capi.BacovResult) == 152
    assert "bacov.hip" in __import__("pycolmap_amd.build", fromlist=["x"]).HIP_SOURCES


def test_input_helpers_refuse_malformed_input():
    c = bacov_cases.by_name("columns_5")
    for bad in (dict(damping=-1.0), dict(damping=float("inf")), dict(loss_function_scale=-2.0),
                dict(loss_function_type="huber"), dict(loss_function_type=5), dict(reserved=1), dict(nope=0)):
        with pytest.raises(ValueError, match="ba_covariance"):
            _capi.bacov_options(bad)
    assert _capi.bacov_options(dict(loss_function_type="cauchy", want_points=0)).loss_function_type == 2
    args = list(c["problem"])
    with pytest.raises(ValueError, match="ba_covariance"):
        _capi.bacov_inputs(*args[:4], np.zeros((1, 4)), *args[5:])
    with pytest.raises(ValueError, match="ba_covariance.*point_const"):
        _capi.bacov_inputs(*args, point_const=[0, 1])
    out = _capi.bacov_inputs(*args, point_const=np.arange(12) % 2)
    assert out[-1].dtype == np.uint8 and out[-1].tolist() == [0, 1] * 6 and len(out) == 12


def test_without_a_gpu_the_entry_point_raises():
    if _capi.device_count() > 0:
        pytest.skip("a GPU is visible; this test covers the CPU-only container")
    import ba_config_cases as cc
    rec, adj = cc.adjuster(pycolmap, "pose_only")
    before = cc.model_bits(rec)
    with pytest.raises(_capi.AmcError):
        pycolmap.estimate_ba_covariance(pycolmap.BACovarianceOptions(), rec, adj)
    assert cc.model_bits(rec) == before


# ---- the reference --------------------------------------------------------------------------------------------------------
def test_reference_matches_frozen_fixture(results):
    g = np.load(GOLDEN)
    assert list(g["names"]) == [c["name"] for c in bacov_cases.cases()]
    for c in bacov_cases.cases():
        r = results[c["name"]]
        assert bacov_cases.digest(r) == str(g[f'{c["name"]}/digest']), c["name"]
        want = g[f'{c["name"]}/scalars']
        assert [float(r["success"]), r["failed_column"], r["num_columns"]] == list(want[:3]), c["name"]
        assert np.float64(r["min_pivot_ratio"]).view(np.uint64) == want[3:].view(np.uint64)[0], c["name"]


def test_case_list_has_every_kind(results):
    """the list covers what DESIGN.md 24.8 says it covers, by the reference's own results"""
    ms = {c["m"] for c in bacov_cases.cases()}
    assert {0, 1, 5, 6, 63, 64, 65, 127, 128, 129, 257, 599} <= ms
    for c in bacov_cases.cases():
        r = results[c["name"]]
        assert r["num_columns"] == c["m"], c["name"]
        assert r["success"] == (c["expect"] == "ok"), c["name"]
        if c["expect"] == "fail":
            assert r["failed_column"] == c["column"] and r["matrix"] is None
    e = bacov_cases.by_name("empty_image_variable")
    r = results["empty_image_variable"]
    assert r["column_owner"][r["failed_column"]] == 3 and not (np.asarray(e["problem"][8]) == 3).any()
    assert results["empty_image_constant"]["success"]
    # track lengths and the twice-seen point
    t = bacov_cases.by_name("track_lengths")["problem"]
    assert {2, 3, 63, 64, 65} <= set(np.bincount(np.asarray(t[9])).tolist())
    d = bacov_cases.by_name("duplicate_observations")["problem"]
    pairs = list(zip(np.asarray(d[8]).tolist(), np.asarray(d[9]).tolist()))
    assert len(set(pairs)) < len(pairs)
    assert np.bincount(np.asarray(bacov_cases.by_name("segment_70")["problem"][8])).max() > 64
    assert len(bacov_cases.by_name("eleven_models")["problem"][0]) == 11
    r0 = results["no_columns"]
    assert r0["success"] and r0["matrix"].shape == (0, 0) and not r0["point_present"].any()
    for c in bacov_cases.refused_cases():
        with pytest.raises(ValueError):
            ref.ba_covariance(*c["problem"], options=c["options"], point_const=c["point_const"])
    # the loss and the damping change the answer
    assert not np.array_equal(results["loss_trivial"]["matrix"], results["loss_cauchy"]["matrix"])
    assert not np.array_equal(results["loss_soft_l1"]["matrix"], results["loss_cauchy"]["matrix"])
    assert not np.array_equal(results["damping_0"]["matrix"], results["damping_default"]["matrix"])
    assert not np.array_equal(results["damping_1"]["point_cov"], results["damping_default"]["point_cov"])


@pytest.mark.parametrize("name", OK_CASES)
def test_blocks_are_symmetric_with_positive_diagonals(name, results):
    r = results[name]
    M = r["matrix"]
    assert np.array_equal(M, M.T) and (np.diag(M) > 0).all() and np.isfinite(M).all()
    assert 0 < r["min_pivot_ratio"] <= 1.0
    assert np.linalg.eigvalsh(M).min() > -64 * np.finfo(float).eps * np.abs(M).max() * M.shape[0]
    blocks = r["point_cov"][r["point_present"]]
    if blocks.size:
        assert (blocks[:, [0, 1, 2], [0, 1, 2]] > 0).all()
        # a point block's two triangles are sums of the same terms in two orders: they agree to the rounding of those
        # sums, which the conditioning of the reduced matrix amplifies (24.6)
        bound = max(1e-12, 64 * np.finfo(float).eps * np.linalg.cond(M))
        asym = np.abs(blocks - blocks.transpose(0, 2, 1)).max(axis=(1, 2)) / np.abs(blocks).max(axis=(1, 2))
        assert asym.max() <= bound, (asym.max(), bound)
    c = bacov_cases.by_name(name)
    if c["point_const"] is not None:
        assert np.array_equal(r["point_present"], np.asarray(c["point_const"]) == 0)
        assert not r["point_cov"][~r["point_present"]].any()


@pytest.mark.parametrize("name", OK_CASES)
def test_reference_agrees_with_the_numpy_restatement(name, results, budget):
    """bound: twice the deviation measured on the CPU when the budget was written (make_bacov_ref_golden.py --budget),
    relative to the largest entry of each block; the figures are in tests/ref2/bacov_deviation_budget.json"""
    c = bacov_cases.by_name(name)
    M2, P2 = bacov_ref2.ba_covariance(*c["problem"], options=c["options"], point_const=c["point_const"])
    dev = bacov_ref2.deviation(results[name], M2, P2)
    b = budget["cases"][name]
    print(f"{name}: deviation {dev:.3e}, measured {b['measured']:.3e}, bound {b['bound']:.3e}")
    assert b["bound"] == 2.0 * b["measured"]
    assert dev <= b["bound"], (dev, b)


# ---- exact answers --------------------------------------------------------------------------------------------------------
def _dyadic_problem(variable):
    """One PINHOLE image (f = 2, identity pose) over constant points at depths 1 and 2: d(pixel) / d(t_x) = f / z is 2 or 1,
    exactly, and d(pixel_x) / d(t_y) = 0."""
    X = np.array([[0.5, 0.25, 1.0], [-0.5, 0.5, 1.0], [0.25, -0.5, 1.0], [1.0, 0.5, 2.0], [-1.0, 1.0, 2.0],
                  [0.5, -1.0, 2.0], [-0.5, -0.5, 2.0]])
    pc = np.ones((1, 6), np.uint8)
    pc[0, list(variable)] = 0
    xy = np.array([[2.0 * x / z + 0.125, 2.0 * y / z - 0.25] for x, y, z in X])
    return ([1], [np.array([2.0, 2.0, 0.0, 0.0])], np.ones((1, 12), np.uint8), [0], [[0.0, 0.0, 0.0, 1.0]], [[0.0, 0.0, 0.0]],
            pc, X, np.zeros(7, np.uint32), np.arange(7, dtype=np.uint32), xy)


def test_single_column_is_the_reciprocal_of_a_sum_of_dyadic_squares():
    r = ref.ba_covariance(*_dyadic_problem([3]), point_const=np.ones(7, np.uint8))
    # S = 3 * 2^2 + 4 * 1^2 = 16, L = 4, Z = 1/4, Sigma = 1/16: every step exact
    assert r["success"] and r["num_columns"] == 1 and r["matrix"].tolist() == [[0.0625]]
    assert r["min_pivot_ratio"] == 1.0 and r["column_owner"].tolist() == [0] and r["column_coord"].tolist() == [3]
    assert not r["point_present"].any()


def test_two_columns_with_a_diagonal_reduced_matrix():
    r = ref.ba_covariance(*_dyadic_problem([3, 4]), point_const=np.ones(7, np.uint8))
    assert r["success"] and r["matrix"].tolist() == [[0.0625, 0.0], [0.0, 0.0625]] and r["min_pivot_ratio"] == 1.0
    assert r["column_coord"].tolist() == [3, 4]


# ---- section 12.8's covariance ----------------------------------------------------------------------------------------------
def test_one_image_equals_the_pose_refinement_covariance(budget):
    """The same inliers, Cauchy scale and pose; no point is variable, so the damping does not enter.  12.8 inverts by an
    eigen-decomposition, section 24 by Cholesky: they agree within the recorded figure, doubled."""
    dev = abspose_deviation()
    b = budget["abspose"]
    print(f"abspose: deviation {dev:.3e}, measured {b['measured']:.3e}, bound {b['bound']:.3e}")
    assert b["bound"] == 2.0 * b["measured"] and dev <= b["bound"], (dev, b)


def abspose_problem():
    import abspose_cases
    import abspose_ref_lib
    sc = abspose_cases.scene(300, 1, 60, outlier_frac=0.0, noise_px=1.0)
    n = int(sc["offsets"][-1])
    r = abspose_ref_lib.refine(sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"], sc["points3D"],
                               sc["qvec"], sc["tvec"], np.ones(n, bool), return_covariance=True)
    assert r["success"][0]
    args = ([int(sc["camera_models"][0])], [sc["camera_params"][0]], np.ones((1, 12), np.uint8), [0], r["qvec"][:1],
            r["tvec"][:1], np.zeros((1, 6), np.uint8), sc["points3D"], np.zeros(n, np.uint32),
            np.arange(n, dtype=np.uint32), sc["points2D"])
    opts = dict(loss_function_type="CAUCHY", loss_function_scale=_capi.abspose_options(None, None)[1].loss_function_scale)
    return args, opts, np.ones(n, np.uint8), np.asarray(r["covariance"][0]).reshape(6, 6)


def abspose_deviation():
    args, opts, mask, want = abspose_problem()
    got = ref.ba_covariance(*args, options=opts, point_const=mask)
    assert got["success"] and got["num_columns"] == 6
    return float(np.abs(got["matrix"] - want).max() / np.abs(want).max())


# ---- relative pose --------------------------------------------------------------------------------------------------------
def _quat_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                     a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def _relative(q1, t1, q2, t2):
    """cam2_from_world * cam1_from_world.inverse() for unit quaternions (x, y, z, w)"""
    from ba_cases import rotate
    inv1 = np.array([-q1[0], -q1[1], -q1[2], q1[3]])
    q21 = _quat_mul(q2, inv1)
    return q21, t2 - rotate(q21, t1)


def relative_pose_jacobian_deviation():
    """central differences of the composition in numpy against relative_pose_jacobian: the relative pose's tangent step is
    read off q21(x) q21(0)^-1 = (sin|d| d / |d|, cos|d|)"""
    from ba_cases import quat_plus
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(5):
        q1, q2 = quat_plus([0, 0, 0, 1.0], rng.uniform(-0.6, 0.6, 3)), quat_plus([0, 0, 0, 1.0], rng.uniform(-0.6, 0.6, 3))
        t1, t2 = rng.uniform(-2, 2, 3), rng.uniform(-2, 2, 3)
        q21, t21 = _relative(q1, t1, q2, t2)
        inv21 = np.array([-q21[0], -q21[1], -q21[2], q21[3]])

        def step(x):
            qa, ta = _relative(quat_plus(q1, x[0:3]), t1 + x[3:6], quat_plus(q2, x[6:9]), t2 + x[9:12])
            dq = _quat_mul(qa, inv21)
            n = np.linalg.norm(dq[:3])
            return np.concatenate([dq[:3] * (np.arctan2(n, dq[3]) / n if n else 1.0), ta - t21])
        h = 1e-6
        num = np.stack([(step(h * e) - step(-h * e)) / (2 * h) for e in np.eye(12)], axis=1)
        J = _ba_covariance.relative_pose_jacobian(q1, t1, q2, t2)
        worst = max(worst, float(np.abs(J - num).max() / np.abs(num).max()))
    return worst


def test_relative_pose_jacobian_against_central_differences(budget):
    dev = relative_pose_jacobian_deviation()
    b = budget["relative_pose_jacobian"]
    print(f"relative pose: deviation {dev:.3e}, measured {b['measured']:.3e}, bound {b['bound']:.3e}")
    assert b["bound"] == 2.0 * b["measured"] and dev <= b["bound"], (dev, b)
    # a rotation of image 1 alone by d turns the relative rotation by -R21 d; a translation of image 2 alone adds to t21
    J = _ba_covariance.relative_pose_jacobian([0, 0, 0, 1.0], [1.0, 2.0, 3.0], [0, 0, 0, 1.0], [0.0, 0.0, 0.0])
    assert np.array_equal(J[:3, :3], -np.eye(3)) and np.array_equal(J[3:, 9:], np.eye(3)) and np.array_equal(J[:3, 6:9], np.eye(3))
    assert np.array_equal(J[3:, 6:9], 2.0 * np.array([[0, -3.0, 2.0], [3.0, 0, -1.0], [-2.0, 1.0, 0]]))


# ---- the host plan ----------------------------------------------------------------------------------------------------------
def test_host_plan_under_asan(tmp_path):
    """The host half (pycolmap_amd/csrc/bacov_plan.h over ba_plan.h) in a stand-alone program under ASan + UBSan
    (tests/shim/bacov_plan_fuzz.cc): 200 seeded problems and nine corruptions of each; every corruption is refused without a
    read through it, every valid plan has 24.1's columns and 24.3's slots and destination blocks."""
    from test_ba_cpu import _run_sanitized, _sanitized_program
    r = _run_sanitized(_sanitized_program(tmp_path, "bacov_plan_fuzz", []))
    assert r.returncode == 0 and r.stdout.startswith("ok 2000 "), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    blocks, none, twice = (int(v) for v in r.stdout.split()[2:5])
    assert blocks > 1000 and none >= 30 and twice > 50


# ---- estimate_ba_covariance with the reference in the library's place --------------------------------------------------------
def reference_solver(d):
    import ba_config_cases as cc
    return ref.ba_covariance(*cc.flat_args(d), options=dict(d["options"]), point_const=np.asarray(d["point_const"]).reshape(-1))


@pytest.mark.parametrize("scene", ["local", "pose_only"])
def test_estimate_with_the_reference_serves_blocks_by_id(scene):
    import ba_config_cases as cc
    import ba_config_ref_lib
    rec, adj = cc.adjuster(pycolmap, scene)
    assert adj._solve_with(rec, cc.reference_solver(ba_config_ref_lib)) is True
    before = cc.model_bits(rec)
    cov = _ba_covariance._estimate_ba_covariance_with(pycolmap.BACovarianceOptions(), rec, adj, reference_solver)
    assert isinstance(cov, pycolmap.BACovariance) and cc.model_bits(rec) == before
    d = adj._problem(rec)
    want = reference_solver(dict(d, options=dict(loss_function_type=int(adj.options.loss_function_type),
                                                 loss_function_scale=adj.options.loss_function_scale, damping=1e-8)))
    assert want["success"]
    # the flat problem's images, cameras and points by id: *_at are places in the reconstruction's maps
    image_at = np.array(list(rec.images))[np.asarray(d["image_at"]).reshape(-1)]
    camera_at = np.array(list(rec.cameras))[np.asarray(d["camera_at"]).reshape(-1)]
    point_at = np.array(list(rec.points3D))[np.asarray(d["point_at"]).reshape(-1)]
    assert not np.array_equal(image_at, np.asarray(d["image_at"]).reshape(-1))  # (ids start at 1, places at 0)
    nimg = image_at.size
    pc, ccst = np.asarray(d["pose_const"]), np.asarray(d["camera_const"])
    owner, coord, M = want["column_owner"], want["column_coord"], want["matrix"]
    served = 0
    for i, iid in enumerate(image_at):
        cols = np.flatnonzero(owner == i)
        block = cov.get_cam_from_world_cov(int(iid))
        if cols.size == 0:
            assert block is None and pc[i].all()
            continue
        assert block.shape == (6, 6) and np.array_equal(block[np.ix_(coord[cols], coord[cols])], M[np.ix_(cols, cols)])
        const = np.flatnonzero(pc[i])
        assert not block[const].any() and not block[:, const].any()
        served += 1
    assert served >= 2
    ids = [int(iid) for i, iid in enumerate(image_at) if (owner == i).any()]
    a, b = ids[0], ids[1]
    ca, cb = np.flatnonzero(owner == list(image_at).index(a)), np.flatnonzero(owner == list(image_at).index(b))
    cross = cov.get_cam_cross_cov(a, b)
    assert np.array_equal(cross[np.ix_(coord[ca], coord[cb])], M[np.ix_(ca, cb)])
    assert np.array_equal(cov.get_cam_cross_cov(b, a), cross.T)
    rel = cov.get_cam2_from_cam1_cov(a, b)
    assert rel.shape == (6, 6) and np.allclose(rel, rel.T, rtol=0, atol=1e-12 * np.abs(rel).max())
    assert np.linalg.eigvalsh(0.5 * (rel + rel.T)).min() > -1e-12 * np.abs(rel).max()
    for c, cid in enumerate(camera_at):
        cols = np.flatnonzero(owner == nimg + c)
        if cols.size == 0:
            assert cov.get_camera_cov(int(cid)) is None and cov.variable_camera_param_idxs(int(cid)) is None
        else:
            assert cov.variable_camera_param_idxs(int(cid)) == coord[cols].tolist()
            assert np.array_equal(cov.get_camera_cov(int(cid)), M[np.ix_(cols, cols)])
            assert list(np.flatnonzero(ccst[c] == 0)) == coord[cols].tolist()
    mask = np.asarray(d["point_const"]).reshape(-1)
    for j, pid in enumerate(point_at):
        block = cov.get_point_cov(int(pid))
        if mask[j]:
            assert block is None
        else:
            assert np.array_equal(block, want["point_cov"][j])
    assert (mask == 0).any() or scene == "pose_only"
    assert cov.get_cam_from_world_cov(10 ** 6) is None and cov.get_point_cov(10 ** 6) is None
    assert cov.get_cam2_from_cam1_cov(a, 10 ** 6) is None and cov.get_camera_cov(10 ** 6) is None
    s = cov.last_run_stats()
    assert s == pycolmap.last_run_stats() or {k: s[k] for k in s if k != "total_ms"} == {k: v for k, v in pycolmap.last_run_stats().items() if k != "total_ms"}
    assert s["num_columns"] == want["num_columns"] and s["min_pivot_ratio"] == want["min_pivot_ratio"] and s["params"] == "ALL"
    # params selects what is served, not what is solved
    poses = _ba_covariance._estimate_ba_covariance_with(dict(params="POSES"), rec, adj, reference_solver)
    assert np.array_equal(poses.get_cam_from_world_cov(a), cov.get_cam_from_world_cov(a))
    assert all(poses.get_point_cov(int(p)) is None for p in point_at) and all(poses.get_camera_cov(int(c)) is None for c in camera_at)
    points = _ba_covariance._estimate_ba_covariance_with(dict(params="POINTS"), rec, adj, reference_solver)
    assert points.get_cam_from_world_cov(a) is None
    assert cc.model_bits(rec) == before


def test_a_failed_factorisation_is_none_with_a_warning(capfd):
    """a config that leaves the gauge free: every pose and point variable, nothing constant"""
    import ba_cases
    import ba_config_cases as cc
    rec = ba_cases.reconstruction(cc.structure_only_scene())
    cfg = pycolmap.BundleAdjustmentConfig()
    for iid in rec.images:
        cfg.add_image(iid)
    for pid in rec.points3D:
        cfg.add_variable_point(pid)
    o = pycolmap.BundleAdjustmentOptions()
    o.refine_focal_length = o.refine_extra_params = False
    adj = pycolmap.BundleAdjuster(o, cfg)
    got = _ba_covariance._estimate_ba_covariance_with(dict(damping=0.0), rec, adj, reference_solver)
    if got is not None:  # rounding may leave the seven gauge pivots tiny and positive: then the ratio says so
        assert got.summary["min_pivot_ratio"] < 1e-9
    else:
        assert "rank deficient" in capfd.readouterr().err
