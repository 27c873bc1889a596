"""The relative pose (pose_math.h, pose.hip) on the named cases of tests/pose_cases.py, without a GPU:

  * the oracle reproduces tests/golden/pose_ref_v1.npz;
  * the host shim over pose_math.h (tests/shim/tvg_shim.cc shim_pose: the kernel's lane-local functions and its
    selection median, run serially) equals the oracle bit for bit on every case;
  * the oracle agrees with the independent restatement tests/ref2/pose_ref2.py within twice the measured budget
    tests/ref2/pose_deviation_budget.json (the margin of two is for libm and LAPACK differences between machines);
  * the coverage the cases are there for holds; the planted motion comes back.

`python tests/test_pose_cpu.py --write-budgets` measures and rewrites the budget file: per path (E, H, the
homography_decomposition entry point) and quantity the worst deviation measured over the compared cases, and under
`truth` the restatement's own worst error against the planted motion.  The file holds the figures as measured; several
are one to three ulps of a unit quantity, and twice that is all the tests allow.

Floats are compared with the restatement only where the result is clear of ties (pose_ref2.clear_of_ties) and the case
has no garbage row and no degenerate input; ok, config and num_points3D are compared on every case that is not
degenerate.  One clean case is not clear and cannot be made so: count_calibrated_0 is a four-way tie at zero points, and
which of an essential matrix's two rotations comes later is a matter of the SVD's sign convention, so it has no winner
by definition.  Every other clean case is compared (asserted below); count_calibrated_1 counts as clear because its
winner is the only candidate that keeps a point.
"""
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
if __name__ == "__main__":
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
sys.path.insert(0, str(ROOT / "tests" / "golden"))

import make_pose_ref_golden as golden  # noqa: E402
import oracle_lib as o  # noqa: E402
import pose_cases as pc  # noqa: E402

BUDGET = ROOT / "tests" / "ref2" / "pose_deviation_budget.json"
SHIM = ROOT / "tests" / "shim" / "_build" / "libtvgshim.so"
NOT_CLEAR = {"count_calibrated_0"}
bits = pc.bits


def same_pose(got, want, tag):
    assert got["pose_ok"] == want["pose_ok"] and got["config"] == want["config"], tag
    assert got["num_points3D"] == want["num_points3D"], tag
    for k in ("R", "tvec", "qvec", "tri_angle"):
        np.testing.assert_array_equal(bits(got[k]), bits(want[k]), err_msg=f"{tag} {k}")


@pytest.fixture(scope="module")
def built():
    return pc.build_cases()


@pytest.fixture(scope="module")
def built_h():
    return pc.build_homography_cases()


@pytest.fixture(scope="module")
def shim():
    SHIM.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "shim" / "tvg_shim.cc"
    hdrs = [ROOT / "pycolmap_amd" / "csrc" / "tvg_math.h", ROOT / "pycolmap_amd" / "csrc" / "pose_math.h"]
    if not SHIM.exists() or SHIM.stat().st_mtime < max(f.stat().st_mtime for f in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-shared", "-fPIC", str(src),
                        "-o", str(SHIM)], check=True)
    return C.CDLL(str(SHIM))


def shim_pose(shim, c):
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    iout, dout = np.zeros(3, dtype=np.int32), np.zeros(17)
    prm = [np.zeros(12) for _ in range(2)]
    for dst, cam in zip(prm, (c["cam1"], c["cam2"])):
        dst[:len(cam[3])] = cam[3]
    a = np.ascontiguousarray(c["pts1"][c["matches"][:, 0]]).reshape(-1, 2)
    b = np.ascontiguousarray(c["pts2"][c["matches"][:, 1]]).reshape(-1, 2)
    E, H = np.ascontiguousarray(c["E"]).reshape(9), np.ascontiguousarray(c["H"]).reshape(9)
    shim.shim_pose(C.c_int(o.CAMERA_MODELS[c["cam1"][0]]), p(prm[0]), C.c_int(o.CAMERA_MODELS[c["cam2"][0]]), p(prm[1]),
                   p(a), p(b), C.c_int(len(a)), C.c_int(c["config"]), p(E), p(H), p(iout), p(dout))
    return dict(pose_ok=bool(iout[0]), config=int(iout[1]), num_points3D=int(iout[2]), R=dout[:9].reshape(3, 3),
                tvec=dout[9:12].copy(), qvec=dout[12:16].copy(), tri_angle=float(dout[16]))


# ---------------------------------------------------------------------------------------------- measurements
def quaternion_gap(a, b):
    return float(min(np.abs(a - b).max(), np.abs(a + b).max()))


def path_of(c):
    return "E" if c["config"] in (pc.CALIBRATED, pc.UNCALIBRATED) else "H"


def measure_deviation(cs, want, hs, hwant):
    """(worst deviation of the oracle from the restatement per path and quantity, the names compared)"""
    worst = {"E": dict(R=0.0, t=0.0, q=0.0, tri_angle=0.0), "H": dict(R=0.0, t=0.0, q=0.0, tri_angle=0.0),
             "homography_decomposition": dict(R=0.0, t=0.0, n=0.0, points3D=0.0)}
    compared = []
    for name, c in cs.items():
        if c["kind"] != "clean":
            continue
        r, w = pc.restated(c), want[name]
        if not r["clear"]:
            continue
        assert r["num_points3D"] == w["num_points3D"], name
        d = worst[path_of(c)]
        d["R"] = max(d["R"], float(np.abs(r["R"] - w["R"]).max()))
        d["t"] = max(d["t"], float(np.abs(r["t"] - w["tvec"]).max()))
        # Eigen's conversion and the restatement's eigenvector agree on rotations only; the R of a nearly pure rotation
        # below the threshold is Hn itself, orthonormal to 1e-3 and no better (homography_threshold_below)
        if np.abs(r["R"].T @ r["R"] - np.eye(3)).max() < 1e-9:
            d["q"] = max(d["q"], quaternion_gap(r["q"], w["qvec"]))
        else:
            assert name == "homography_threshold_below", name
        d["tri_angle"] = max(d["tri_angle"], abs(r["tri_angle"] - w["tri_angle"]))
        compared.append(name)
    d = worst["homography_decomposition"]
    for name, c in hs.items():
        if c["kind"] != "clean":
            continue
        r, w = pc.restated_h(c), hwant[name]
        if not r["clear"]:
            continue
        assert len(r["points3D"]) == len(w["points3D"]), name
        for k in ("R", "t", "n"):
            d[k] = max(d[k], float(np.abs(r[k] - w[k]).max()))
        if len(r["points3D"]):
            d["points3D"] = max(d["points3D"], float(np.abs(r["points3D"] - w["points3D"]).max()))
        compared.append("h/" + name)
    return worst, compared


def truth_errors(cs, result_of):
    """worst (max |R - planted R|, max |t / |t| - planted t / |t||) over the cases that carry a planted motion"""
    eR = et = 0.0
    for name, c in cs.items():
        if c["truth"] is None:
            continue
        R, t = result_of(name, c)
        eR = max(eR, float(np.abs(R - c["truth"][0]).max()))
        et = max(et, float(np.abs(t / np.linalg.norm(t) - c["truth"][1] / np.linalg.norm(c["truth"][1])).max()))
    return dict(R=eR, t=et)


def measure_truth(cs):
    def run(name, c):
        r = pc.restated(c)
        return r["R"], r["t"]
    return truth_errors(cs, run)


# ---------------------------------------------------------------------------------------------- tests
def test_the_cases_cover_what_they_are_there_for(built, built_h):
    """build_cases() and build_homography_cases() assert it; here once more with the figures in the failure message"""
    cs, want = built
    cov = pc.coverage(cs, want)
    pc.check_coverage(cs, cov)
    assert {n for n, c in cs.items() if c["survivors"] is not None} >= {f"survivors_{k}" for k in pc.SURVIVOR_SETS}
    assert [want[f"survivors_{k}"]["num_points3D"] for k in ("edges", "64", "65", "1", "2", "0")] == [125, 64, 65, 1, 2, 0]
    assert cov["negative_cosines"] >= 1 and set(cov["branches"].values()) == {"trace", 0, 1, 2}
    assert all(abs(v - 1e-3) >= 1e-4 for v in cov["inf_norm"].values())
    # the rows that survive are the planted ones (the restatement's mask)
    for k, keep in pc.SURVIVOR_SETS.items():
        assert list(np.flatnonzero(pc.restated(cs[f"survivors_{k}"])["keep"])) == keep, k
    # the pure rotation and the two threshold sides resolve as stated
    assert want["homography_pure_rotation_por"]["config_name"] == "PANORAMIC"
    assert want["homography_pure_rotation_por"]["tri_angle"] == 0.0 and (want["homography_pure_rotation_por"]["tvec"] == 0).all()
    assert want["homography_pure_rotation_planar"]["config_name"] == "PLANAR"
    assert want["homography_pure_rotation_panoramic"]["config_name"] == "PANORAMIC"
    assert want["homography_threshold_below"]["config_name"] == "PANORAMIC"
    assert want["homography_threshold_above"]["config_name"] == "PLANAR"
    for n in ("undefined", "degenerate", "watermark", "multiple"):
        assert not want[f"degenerate_config_{n}"]["pose_ok"]
    pc.check_homography_coverage(*built_h)


def test_oracle_reproduces_the_fixture(built, built_h):
    (cs, want), (hs, hwant) = built, built_h
    poses, homs = golden.load()
    assert list(poses) == list(cs) and list(homs) == list(hs), "the case list changed: rewrite the fixture"
    for name in cs:
        same_pose(want[name], poses[name], name)
    for name in hs:
        for k in ("R", "t", "n", "points3D"):
            assert hwant[name][k].shape == homs[name][k].shape, f"{name} {k}"
            np.testing.assert_array_equal(bits(hwant[name][k]), bits(homs[name][k]), err_msg=f"{name} {k}")


def test_host_shim_equals_the_oracle_bit_for_bit(built, shim):
    cs, want = built
    for name, c in cs.items():
        same_pose(shim_pose(shim, c), want[name], name)


def test_float32_and_float64_uploads_of_the_same_values_agree(built):
    _, want = built
    same_pose(want["cameras_float32"], want["cameras_float64"], "float32 against float64")


def test_oracle_agrees_with_the_restatement_within_the_budget(built, built_h):
    (cs, want), (hs, hwant) = built, built_h
    budget = json.loads(BUDGET.read_text())
    for name, c in cs.items():   # what must be equal, not close
        if c["kind"] == "degenerate":
            continue
        r, w = pc.restated(c), want[name]
        assert (r["ok"], r["config"], r["num_points3D"]) == (w["pose_ok"], w["config"], w["num_points3D"]), name
    for name, c in hs.items():
        assert len(pc.restated_h(c)["points3D"]) == len(hwant[name]["points3D"]), name
    worst, compared = measure_deviation(cs, want, hs, hwant)
    clean = {n for n, c in cs.items() if c["kind"] == "clean"} | {"h/" + n for n, c in hs.items() if c["kind"] == "clean"}
    assert clean - set(compared) == NOT_CLEAR, sorted(clean - set(compared))
    print(json.dumps(worst))
    for group, d in worst.items():
        for k, v in d.items():
            assert v <= 2.0 * budget[group][k], f"{group} {k}: {v} against a budget of {budget[group][k]}"


def test_masked_scenes_have_a_hole_in_every_chunk():
    """the scenes of the GPU suite's masked path: the oracle's inlier mask clears exactly the planted rows, and its pose
    is the one EstimateTwoViewGeometryPose gives for the inlier matches alone"""
    for M, sc in pc.masked_scenes().items():
        w = pc.oracle_verify(sc)
        pc.check_masked(sc, w["inlier_mask"])
        assert w["config_name"] == "CALIBRATED" and w["pose_ok"] and w["num_points3D"] == M - len(sc["holes"]), M
        cam = pc.ocam(sc["cam"])
        alone = o.estimate_two_view_geometry_pose(cam, sc["pts1"], cam, sc["pts2"], sc["matches"][w["inlier_mask"]],
                                                  w["config"], E=w["E"], H=w["H"])
        same_pose(w, alone, f"M {M}")


def test_planted_motion_comes_back(built):
    """R is the planted R and t is parallel to the planted t, for the restatement and for the oracle, each within twice
    the restatement's worst error as measured and committed under the budget's `truth` entry"""
    cs, want = built
    budget = json.loads(BUDGET.read_text())
    assert sum(c["truth"] is not None for c in cs.values()) >= 20
    got = measure_truth(cs)
    ora = truth_errors(cs, lambda name, c: (want[name]["R"], want[name]["tvec"]))
    print(json.dumps(dict(restatement=got, oracle=ora)))
    for who, e in (("restatement", got), ("oracle", ora)):
        assert e["R"] <= 2.0 * budget["truth"]["R"] and e["t"] <= 2.0 * budget["truth"]["t"], (who, e)


if __name__ == "__main__":
    if "--write-budgets" in sys.argv:
        cs_, want_ = pc.build_cases()
        hs_, hwant_ = pc.build_homography_cases()
        worst_, compared_ = measure_deviation(cs_, want_, hs_, hwant_)
        worst_["truth"] = measure_truth(cs_)
        BUDGET.write_text(json.dumps(worst_, indent=1) + "\n")
        print(worst_, "compared", len(compared_))
