"""pycolmap.homography_decomposition = PoseFromHomographyMatrix (/root/reference/pycolmap/geometry/homography_matrix.h:13-40):
the oracle's restatement against the geometry it must recover (CPU), the device path against the oracle bit for bit (GPU)."""
import sys

import numpy as np
import pytest

import oracle_lib as o
import pose_cases as pc

sys.path.insert(0, str(o.ROOT / "tests" / "golden"))
import make_pose_ref_golden as pose_golden  # noqa: E402


def rot(rng, angle):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def plane_scene(rng, n=60, pure_rotation=False, angle=0.2):
    """Points on the plane nrm . X = d seen by camera 1 = [I | 0] and camera 2 = [R | t]; H maps pixels of 1 to pixels of 2."""
    K1 = np.array([[900.0, 0, 640], [0, 910.0, 360], [0, 0, 1]])
    K2 = np.array([[1100.0, 0, 600], [0, 1090.0, 400], [0, 0, 1]])
    R = rot(rng, angle)
    t = np.zeros(3) if pure_rotation else rng.normal(size=3) * 0.3
    nrm = np.array([0.1, -0.2, 1.0])
    nrm /= np.linalg.norm(nrm)
    d = 5.0
    xy = rng.uniform(-0.4, 0.4, (n, 2))
    rays = np.column_stack([xy, np.ones(n)])
    X = rays * (d / (rays @ nrm))[:, None]                      # on the plane, in front of camera 1
    X2 = X @ R.T + t
    assert (X2[:, 2] > 0.5).all()
    p1 = X[:, :2] / X[:, 2:]
    p2 = X2[:, :2] / X2[:, 2:]
    H = K2 @ (R + np.outer(t, nrm) / d) @ np.linalg.inv(K1)
    return dict(H=H * rng.uniform(0.5, 2.0), K1=K1, K2=K2, R=R, t=t, n=nrm, d=d, p1=p1, p2=p2, X=X)


@pytest.mark.parametrize("seed", range(6))
def test_oracle_recovers_the_plane_and_the_motion(seed):
    rng = np.random.default_rng(seed)
    s = plane_scene(rng)
    if seed % 2:
        s["H"] = -s["H"]                                         # the sign of H is arbitrary
    r = o.pose_from_homography(s["H"], s["K1"], s["K2"], s["p1"], s["p2"])
    # a plane seen from two views has two decompositions with every point in front of both cameras; whichever COLMAP's
    # tie rule picks, (R, t, n) is a rotation, a unit normal, and reproduces H up to scale: Hn = R - t n^T (COLMAP's
    # HomographyMatrixFromPose convention: the plane is n . X + d = 0, so n points away from the true normal)
    R, t, n = r["R"], r["t"], r["n"]
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-9)
    assert abs(np.linalg.det(R) - 1) < 1e-9 and abs(np.linalg.norm(n) - 1) < 1e-9
    Hn = np.linalg.inv(s["K2"]) @ s["H"] @ s["K1"]
    Hn = Hn / np.linalg.svd(Hn, compute_uv=False)[1]
    if np.linalg.det(Hn) < 0:
        Hn = -Hn
    np.testing.assert_allclose(R - np.outer(t, n), Hn, atol=1e-9)
    assert len(r["points3D"]) == len(s["p1"])
    X = r["points3D"]
    np.testing.assert_allclose(X[:, :2] / X[:, 2:], s["p1"], atol=1e-9)          # the points reproject
    X2 = X @ R.T + t
    np.testing.assert_allclose(X2[:, :2] / X2[:, 2:], s["p2"], atol=1e-9)
    # and the true motion is one of the two: either this one ...
    truth = np.allclose(R, s["R"], atol=1e-8) and np.allclose(t, s["t"] / s["d"], atol=1e-8) and np.allclose(n, -s["n"], atol=1e-8)
    # ... or the other, which then shares the plane-induced homography
    assert truth or not np.allclose(R, s["R"], atol=1e-3)


def test_oracle_pure_rotation_has_one_candidate():
    rng = np.random.default_rng(11)
    s = plane_scene(rng, pure_rotation=True)
    r = o.pose_from_homography(s["H"], s["K1"], s["K2"], s["p1"], s["p2"])
    np.testing.assert_allclose(r["R"], s["R"], atol=1e-9)
    assert (r["t"] == 0).all() and (r["n"] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(8))
def test_device_matches_the_oracle(seed):
    from pycolmap_amd import _capi
    rng = np.random.default_rng(100 + seed)
    s = plane_scene(rng, n=int(rng.integers(1, 300)), pure_rotation=seed == 7, angle=float(rng.uniform(0.01, 0.6)))
    p2 = s["p2"] + rng.normal(0, 1e-3, s["p2"].shape)           # noise: some points fail the cheirality test
    if seed == 5:
        p2[::3] = -p2[::3] * 5                                   # garbage correspondences
    H = s["H"] if seed % 2 else -s["H"]
    ctx = _capi.Context(0)
    g = ctx.homography_decomposition(H, s["K1"], s["K2"], s["p1"], p2)
    w = o.pose_from_homography(H, s["K1"], s["K2"], s["p1"], p2)
    for k in ("R", "t", "n", "points3D"):
        assert g[k].shape == w[k].shape, k
        np.testing.assert_array_equal(g[k].view(np.uint64), w[k].view(np.uint64), err_msg=k)
    ctx.close()


@pytest.fixture(scope="module")
def hom_ctx():
    from pycolmap_amd import _capi
    ctx = _capi.Context(0)
    yield ctx
    ctx.close()


def same_bits(got, want, tag):
    for k in ("R", "t", "n", "points3D"):
        assert got[k].shape == want[k].shape, f"{tag} {k}"
        np.testing.assert_array_equal(pc.bits(got[k]), pc.bits(want[k]), err_msg=f"{tag} {k}")


@pytest.mark.gpu
def test_named_cases_bit_exact_order_included(hom_ctx):
    """pose_cases.homography_cases(): counts at the lane edges, garbage rows at lanes 0, 63, 64, 127 and 129 (the
    points3D compaction), the three formula sets, +-H, the pure rotation and both sides of its threshold - against the
    oracle and against tests/golden/pose_ref_v1.npz; points3D row for row"""
    hs, want = pc.build_homography_cases()
    _, homs = pose_golden.load()
    assert list(homs) == list(hs)
    got = {}
    for name, c in hs.items():
        g = got[name] = hom_ctx.homography_decomposition(c["H"], c["K1"], c["K2"], c["p1"], c["p2"])
        same_bits(g, want[name], name)
        same_bits(g, homs[name], f"{name} (fixture)")
        assert len(g["points3D"]) == c["survivors"], name
        # two calls in a row on one context give the same bits
        same_bits(hom_ctx.homography_decomposition(c["H"], c["K1"], c["K2"], c["p1"], c["p2"]), g, f"{name} (again)")
    # the survivors of the garbage case are the other rows, in input order: each point reprojects to its own row
    X = got["garbage_edges"]["points3D"]
    keep = sorted(set(range(130)) - set(pc.EDGE_ROWS))
    np.testing.assert_allclose(X[:, :2] / X[:, 2:], hs["garbage_edges"]["p1"][keep], atol=1e-9)


@pytest.mark.gpu
def test_binding():
    import pycolmap_amd as pycolmap
    rng = np.random.default_rng(42)
    s = plane_scene(rng)
    r = pycolmap.homography_decomposition(s["H"], s["K1"], s["K2"], s["p1"], [tuple(p) for p in s["p2"]])
    assert set(r) == {"R", "t", "n", "points3D"}
    w = o.pose_from_homography(s["H"], s["K1"], s["K2"], s["p1"], s["p2"])
    np.testing.assert_array_equal(r["R"], w["R"])
    np.testing.assert_array_equal(r["t"], w["t"])
    np.testing.assert_array_equal(r["n"], w["n"])
    np.testing.assert_array_equal(np.array(r["points3D"]), w["points3D"])
    e = pycolmap.homography_decomposition(s["H"], s["K1"], s["K2"], np.zeros((0, 2)), np.zeros((0, 2)))
    assert e["points3D"] == [] and e["R"].shape == (3, 3)
    with pytest.raises(ValueError):
        pycolmap.homography_decomposition(s["H"], s["K1"], s["K2"], s["p1"], s["p2"][:-1])
