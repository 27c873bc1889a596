"""Stereo fusion without a GPU: the Python surface and the option protocol, the C ABI's header
against _capi, the sequential reference (tests/fusion_ref) against its fixture, against a numpy float64 restatement of
lift, projection and the three tests (budget in tests/ref2/fusion_deviation_budget.json), against answers worked out by
hand and against ground truth (tests/ref2/fusion_accuracy_budget.json), and the host half of StereoFusion with the
reference in the library's place.

`python tests/test_stereo_fusion_cpu.py --write-budgets` measures and rewrites the two budget files."""
import copy
import ctypes
import json
import pickle
import struct
import sys
from pathlib import Path

import numpy as np
import pytest

import fusion_cases as fc
import fusion_ref_lib as ref
import patchmatch_cases as pc
import pycolmap
import pycolmap_amd
from pycolmap_amd import _capi, _fusion as F
from pycolmap_amd._patch_match import write_array

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "fusion_ref_v1.npz"
DEVIATION = ROOT / "tests" / "ref2" / "fusion_deviation_budget.json"
ACCURACY = ROOT / "tests" / "ref2" / "fusion_accuracy_budget.json"
FMAX = float(np.finfo(np.float32).max)


# ---- surface, options, header ---------------------------------------------------------------------------------------------------
def test_surface():
    for name in ("StereoFusion", "FusionOptions"):
        assert getattr(pycolmap, name) is getattr(pycolmap_amd, name) and name in pycolmap._PUBLIC
    assert "StereoFusion" in pycolmap.__doc__ and "DESIGN.md section 23" in pycolmap.__doc__
    for name in ("stereo_fusion", "StereoFusionOptions"):
        with pytest.raises(AttributeError, match="outside pycolmap_amd's scope.*StereoFusion.*DESIGN.md section 23"):
            getattr(pycolmap, name)
        assert not hasattr(pycolmap_amd, name)


def test_options_follow_the_protocol():
    o = pycolmap.FusionOptions()
    want = dict(mask_path="", num_threads=-1, max_image_size=-1, min_num_pixels=5, max_num_pixels=10000, max_traversal_depth=100,
                max_reproj_error=2.0, max_depth_error=0.01, max_normal_error=10.0, check_num_images=50, use_cache=False,
                cache_size=32.0, bounding_box=((-FMAX,) * 3, (FMAX,) * 3))
    assert o.todict() == want and len(want) == 13 and list(o.todict()) == list(want)  # the binding's fields, in its order
    for name, value in want.items():
        doc = getattr(pycolmap.FusionOptions, name).__doc__
        shown = f'"{value}"' if isinstance(value, str) else value
        assert doc.endswith(f"({type(value).__name__}, default: {shown})"), name
    assert pycolmap.FusionOptions.min_num_pixels.__doc__.startswith("Minimum number of fused pixels to produce a point.")
    a = pycolmap.FusionOptions(dict(min_num_pixels=3, use_cache=True))
    b = pycolmap.FusionOptions(min_num_pixels=3, use_cache=True)
    assert a == b and a.min_num_pixels == 3 and a.use_cache is True and a != o
    b.mergedict(dict(check_num_images=7))
    assert b.check_num_images == 7 and a.check_num_images == 50
    with pytest.raises(ValueError, match="unknown option 'min_pixels'"):
        pycolmap.FusionOptions(min_pixels=3)
    with pytest.raises(TypeError, match="min_num_pixels"):
        o.min_num_pixels = 2.5
    with pytest.raises(TypeError, match="use_cache"):
        o.use_cache = 1
    with pytest.raises(TypeError, match="mask_path"):
        o.mask_path = 3
    with pytest.raises(TypeError, match="bounding_box"):
        o.bounding_box = (1.0, 2.0, 3.0)
    o.max_depth_error = 1  # an int where a float is wanted converts, as in the binding
    assert o.max_depth_error == 1.0 and isinstance(o.max_depth_error, float)
    o.bounding_box = (np.array([-1, -2, -3]), [1, 2, 3])
    assert o.bounding_box == ((-1.0, -2.0, -3.0), (1.0, 2.0, 3.0))
    for twin in (copy.copy(b), copy.deepcopy(b), pickle.loads(pickle.dumps(b))):
        assert twin == b and twin is not b
        twin.check_num_images = 9
        assert b.check_num_images == 7
    text = a.summary()
    assert text.startswith("FusionOptions:\n    mask_path = \n    num_threads = -1\n") and "\n    min_num_pixels = 3\n" in text
    assert "\n    min_num_pixels: int = 3\n" in a.summary(True) and repr(a) == text


@pytest.mark.parametrize("change, text", [
    (dict(min_num_pixels=-1), "min_num_pixels >= 0"), (dict(min_num_pixels=6, max_num_pixels=5), "min_num_pixels <= max_num_pixels"),
    (dict(max_traversal_depth=0), "max_traversal_depth > 0"), (dict(max_reproj_error=-1.0), "max_reproj_error >= 0"),
    (dict(max_depth_error=-1.0), "max_depth_error >= 0"), (dict(max_normal_error=-1.0), "max_normal_error >= 0"),
    (dict(check_num_images=0), "check_num_images > 0"), (dict(cache_size=0.0), "cache_size > 0")])
def test_options_check(change, text):
    pycolmap.FusionOptions().check()
    with pytest.raises(ValueError, match=r"\[_fusion.py:\d+\] Check Failed: " + text):
        pycolmap.FusionOptions(change).check()


def test_header_symbols_and_structs():
    lib = _capi.load()
    text = (ROOT / "include" / "amc_fusion.h").read_text()
    for name in ("amc_fusion_opts_default", "amc_fuse_depth_maps", "amc_fusion_result_free"):
        assert hasattr(lib, name) and name in _capi.EXPORTED_SYMBOLS and name in text
    assert lib.amc_abi_version() == 5
    o = _capi.FusionOpts()
    lib.amc_fusion_opts_default(ctypes.byref(o))
    for name, value in _capi.FUSION_DEFAULTS.items():
        if name == "bounding_box":
            assert tuple(o.bounding_box) == tuple(value[0]) + tuple(value[1]) == (-FMAX,) * 3 + (FMAX,) * 3
        else:
            assert getattr(o, name) == value, name
    assert o.reserved == 0
    assert ctypes.sizeof(_capi.FusionOpts) == 4 * 4 + 9 * 8 and ctypes.sizeof(_capi.FusionProblem) == 13 * 8
    assert ctypes.sizeof(_capi.FusionResult) == 11 * 8 + 8 + 5 * 8
    for s in (_capi.FusionOpts, _capi.FusionProblem, _capi.FusionResult):
        for field, _ in s._fields_:
            assert field in text, field
    for name, value in (("MAX_NEIGHBOURS", _capi.FUSION_MAX_NEIGHBOURS), ("MAX_TRAVERSAL_DEPTH", _capi.FUSION_MAX_TRAVERSAL_DEPTH),
                        ("MAX_CLUSTER", _capi.FUSION_MAX_CLUSTER)):
        assert f"AMC_FUSION_{name} {value}" in " ".join(text.split())
    assert fc.MAX_CLUSTER == _capi.FUSION_MAX_CLUSTER
    assert "fusion.hip" in (ROOT / "pycolmap_amd" / "build.py").read_text()
    source = (ROOT / "pycolmap_amd" / "csrc" / "fusion.hip").read_text() + (ROOT / "pycolmap_amd" / "csrc" / "fusion_core.h").read_text()
    assert "atomic" not in source.replace("No atomics", "").replace("no atomics", "")
    assert "AMC_FUSION_BATCH_SEEDS" in source and "AMC_FUSION_BATCH_SEEDS" in text and "AMC_FUSION_BATCH_SEEDS" in (ROOT / "README.md").read_text()
    res = _capi.FusionResult()  # NULL arguments are refused before a device is looked for
    assert lib.amc_fuse_depth_maps(None, None, None, ctypes.byref(res)) == _capi.AMC_E_INVALID
    assert lib.amc_fuse_depth_maps(None, None, None, None) == _capi.AMC_E_INVALID
    lib.amc_fusion_result_free(ctypes.byref(res))
    lib.amc_fusion_result_free(None)
    lib.amc_fusion_opts_default(None)


def test_flat_input_is_checked_before_the_library():
    good = fc.stack(3)
    for at, value in ((1, good[1][:2]), (2, good[2][:2]), (0, [np.zeros((2, 2), np.uint8)] * 3), (4, good[4][:2]), (6, [[1]] * 2),
                      (4, [np.zeros((3, 2), np.float32)] * 3), (5, [None] + good[5][1:]), (6, [[-1], [], []]), (6, [[1] * 65, [], []])):
        args = list(good)
        args[at] = value
        with pytest.raises(ValueError, match="fuse_depth_maps"):
            _capi.fusion_inputs(*args)
    with pytest.raises(ValueError, match="unknown option 'min_pixels'"):
        _capi.fusion_options(min_pixels=1)
    with pytest.raises(ValueError, match="bounding_box"):
        _capi.fusion_options(bounding_box=(1, 2, 3))


# ---- the reference against its fixture --------------------------------------------------------------------------------------------
CASES = fc.build_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_reproduces_the_fixture(name):
    args, opts = CASES[name]
    out = ref.fuse_depth_maps(*args, trace=True, **opts)
    assert fc.result_digest(out) == str(np.load(GOLDEN)[f"digest/{name}"])
    reasons = {ref.REASONS[r] for r in out["trace"][:, 5]}
    for wanted in fc.EXPECT.get(name, ()):  # the case reaches what its name says
        assert wanted in reasons, (name, wanted)
    assert not np.isnan(out["xyz"]).any() and not np.isnan(out["normal"]).any()


def test_reference_thresholds_to_the_float():
    golden = np.load(GOLDEN)
    for name, (args, opts, (spix, image, row, col), taken) in fc.threshold_cases(ref).items():
        out = ref.fuse_depth_maps(*args, trace=True, **opts)
        assert fc.result_digest(out) == str(golden[f"digest/threshold_{name}"])
        line = [ln for ln in out["trace"] if out["seed_pixel"][ln[0]] == spix and out["seed_image"][ln[0]] == 0 and ln[1] == 0
                and tuple(ln[2:5]) == (image, row, col)]
        assert len(line) == 1
        assert ref.REASONS[line[0][5]] == ("taken" if taken else name.split("_")[0] + "_error"), name


def test_reference_and_core_header_under_asan(tmp_path):
    """The C++ of fusion that runs on a host (fusion_core.h, which the kernel shares, and the reference) in a stand-alone
    program under ASan + UBSan (tests/shim/fusion_ref_fuzz.cc): 300 seeded problems on heap arrays of their exact sizes,
    with bad map values, repeated and backward neighbours, images without maps and options down to their least; every
    result is checked for what section 23 promises of any input.  (The host half of StereoFusion is Python: M14.)"""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    flags = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-ffp-contract=off", "-fno-fast-math"]
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("sanitizer runtime not installed")
    exe = tmp_path / "fusion_ref_fuzz"
    b = subprocess.run(flags + [str(ROOT / "tests" / "shim" / "fusion_ref_fuzz.cc"), "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    import os
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0 and r.stdout.startswith("ok 300"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])


# ---- the reference against a float64 restatement ----------------------------------------------------------------------------------
def restate(args, seed_image, srow, scol, image, row, col):
    """section 23.1 - 23.2 in numpy float64 from the section's formulas, not from fusion_core.h: the seed's point, the
    child's point, the relative depth error, the normals' cosine, the squared reprojection error"""
    images, K, R, t, dm, nm, nb = args

    def Kmat(i):
        fx, fy, cx, cy = K[i]
        return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])

    def lift(i, r, c):
        z = float(dm[i][r, c])
        return R[i].T @ (np.linalg.solve(Kmat(i), np.array([c + 0.5, r + 0.5, 1.0]) * z) - t[i])

    def project(i, X):
        p = Kmat(i) @ (R[i] @ X + t[i])
        return p[0] / p[2], p[1] / p[2], p[2]

    Xs, Xc = lift(seed_image, srow, scol), lift(image, row, col)
    z = float(dm[image][row, col])
    derr = abs(project(image, Xs)[2] - z) / z
    cosn = float((R[seed_image].T @ nm[seed_image][:, srow, scol].astype(np.float64)) @ (R[image].T @ nm[image][:, row, col].astype(np.float64)))
    u, v, _ = project(seed_image, Xc)
    return Xs, Xc, derr, cosn, (u - (scol + 0.5)) ** 2 + (v - (srow + 0.5)) ** 2


RESTATED = {"slanted": ("slanted", 4, 24, 18), "step": ("step", 4, 24, 18), "fronto": ("fronto", 3, 16, 12)}
RESTATED_OPTIONS = dict(min_num_pixels=1, max_reproj_error=2.0, max_depth_error=0.01, max_normal_error=10.0)


def measure_deviation():
    """the largest deviation of the reference's float32 quantities from the restatement over every child the reference
    looked at with a depth, and the share of those children within `margin` of a threshold"""
    worst = dict(point=0.0, depth_error=0.0, cosine=0.0, reproj_sq=0.0)
    rows = []
    for kind, cams, w, h in RESTATED.values():
        args = fc.rendered(kind, cams, w, h)
        out = ref.fuse_depth_maps(*args, trace=True, **RESTATED_OPTIONS)
        seeds = list(zip(out["seed_image"], out["seed_pixel"]))  # (min_num_pixels = 1: a point per seed)
        assert len(seeds) == out["num_seeds"]
        for cluster, parent, image, row, col, why, _ in out["trace"]:
            name = ref.REASONS[why]
            if name not in ("taken", "depth_error", "normal_error", "reproj_error"):
                continue
            si, spix = seeds[cluster]
            srow, scol = divmod(int(spix), w)
            d32, c32, r32, Xs32, Xc32 = ref.measure(args, int(si), srow, scol, int(image), int(row), int(col))
            Xs, Xc, derr, cosn, rsq = restate(args, int(si), srow, scol, int(image), int(row), int(col))
            worst["point"] = max(worst["point"], float(np.abs(Xs32 - Xs).max()), float(np.abs(Xc32 - Xc).max()))
            worst["depth_error"] = max(worst["depth_error"], abs(d32 - derr))
            worst["cosine"] = max(worst["cosine"], abs(c32 - cosn))
            worst["reproj_sq"] = max(worst["reproj_sq"], abs(r32 - rsq))
            rows.append((name, derr, cosn, rsq))
    return worst, rows


def membership(rows, budget):
    """compares the reference's verdict with the restatement's wherever the restatement is farther than twice the budget
    from every threshold; returns (compared, left out, disagreements)"""
    o = RESTATED_OPTIONS
    cos_max = np.cos(np.radians(o["max_normal_error"]))
    compared = left_out = wrong = 0
    for name, derr, cosn, rsq in rows:
        near = (abs(derr - o["max_depth_error"]) <= 2 * budget["depth_error"] or abs(cosn - cos_max) <= 2 * budget["cosine"]
                or abs(rsq - o["max_reproj_error"] ** 2) <= 2 * budget["reproj_sq"])
        if near:
            left_out += 1
            continue
        verdict = ("depth_error" if derr > o["max_depth_error"] else "normal_error" if cosn < cos_max
                   else "reproj_error" if rsq > o["max_reproj_error"] ** 2 else "taken")
        compared += 1
        wrong += verdict != name
    return compared, left_out, wrong


def test_reference_equals_the_float64_restatement_within_the_budget():
    budget = json.loads(DEVIATION.read_text())
    worst, rows = measure_deviation()
    for key, value in worst.items():
        print(key, value, "budget", budget[key])
        assert value <= 2 * budget[key], key
    compared, left_out, wrong = membership(rows, budget)
    print("candidates", len(rows), "compared", compared, "left out", left_out, "wrong", wrong)
    assert len(rows) > 2000 and wrong == 0
    assert left_out <= 0.05 * len(rows)


# ---- answers by hand ----------------------------------------------------------------------------------------------------------------
def test_identical_cameras_fuse_one_pixel_per_image():
    for n in (2, 3):
        args = fc.stack(n, 2, 2, depth=2.0, focal=4.0)
        out = ref.fuse_depth_maps(*args, min_num_pixels=n)
        assert out["num_points"] == 4 and out["num_seeds"] == 4 and list(out["num_fused"]) == [n] * 4
        # pixel (row, col) at depth 2: ((col + 0.5 - 1) / 4 * 2, (row + 0.5 - 1) / 4 * 2, 2)
        want = [[(c - 0.5) / 2, (r - 0.5) / 2, 2.0] for r in range(2) for c in range(2)]
        assert out["xyz"].tolist() == want and out["normal"].tolist() == [[0.0, 0.0, -1.0]] * 4
        assert out["vis_images"].tolist() == list(range(n)) * 4 and out["vis_offsets"].tolist() == [n * k for k in range(5)]
        assert list(out["seed_image"]) == [0] * 4 and list(out["seed_pixel"]) == [0, 1, 2, 3]
        assert ref.fuse_depth_maps(*args, min_num_pixels=n + 1)["num_points"] == 0


def test_medians_of_odd_and_even_counts_and_colour_rounding():
    # one pixel per image at one pose; depths within max_depth_error of the seed's, so that all of them fuse
    depths = [2.0, 2.0 + 2 ** -7, 2.0 - 2 ** -7, 2.0 + 2 ** -6]
    colors = [(10, 0, 255), (11, 1, 0), (13, 1, 255), (20, 2, 1)]
    for n, z, rgb in ((3, 2.0, (11, 1, 255)), (4, 2.0 + 2 ** -8, (12, 1, 128)), (2, 2.0 + 2 ** -8, (11, 1, 128))):
        args = fc.stack(n, 1, 1, focal=4.0, colors=colors)
        for i in range(n):
            args[4][i][...] = depths[i]
        out = ref.fuse_depth_maps(*args, min_num_pixels=n, max_depth_error=0.5)
        # the pixel's centre is the principal point: x = y = 0, z = the median depth
        assert out["num_points"] == 1 and out["num_fused"][0] == n and out["xyz"].tolist() == [[0.0, 0.0, z]]
        assert tuple(out["color"][0]) == rgb  # of four: (11 + 13) / 2 = 12, (1 + 255) / 2 = 128; of two: (10 + 11) / 2 = 10.5 -> 11
    args = fc.stack(2, 1, 1, focal=4.0, colors=[(0, 1, 2), (1, 2, 3)])
    assert tuple(ref.fuse_depth_maps(*args, min_num_pixels=2)["color"][0]) == (1, 2, 3)  # .5 goes up


def test_a_point_on_the_bounding_box_and_one_float_beyond():
    args = fc.stack(2, 1, 1, depth=2.0)
    up, down = float(np.nextafter(np.float32(2.0), np.float32(3))), float(np.nextafter(np.float32(2.0), np.float32(1)))
    for box, kept in ((((-1, -1, 2.0), (1, 1, 2.0)), True), (((-1, -1, up), (1, 1, 3)), False), (((-1, -1, 1), (1, 1, down)), False),
                      (((0, 0, 2.0), (0, 0, 2.0)), True), (((-FMAX,) * 3, (FMAX,) * 3), True)):
        assert ref.fuse_depth_maps(*args, min_num_pixels=2, bounding_box=box)["num_points"] == (1 if kept else 0), box


def test_chain_and_claims_by_hand():
    chain = [[1], [2], [3], [4], []]
    for depth, sizes in ((1, [1] * 5), (2, [2, 2, 1]), (3, [3, 2]), (5, [5]), (100, [5])):
        out = ref.fuse_depth_maps(*fc.stack(5, 1, 1, neighbours=chain), min_num_pixels=1, max_traversal_depth=depth)
        assert list(out["num_fused"]) == sizes, depth
    # two seeds of one step share a member, and the step after finds it claimed
    args, opts = CASES["two_seeds_share_a_member"]
    out = ref.fuse_depth_maps(*args, **opts)
    assert list(out["seed_image"]) == [0] * 8 and list(out["num_fused"]) == [2] * 8 and out["num_seeds"] == 8
    assert out["vis_images"].tolist() == [0, 1] * 8


# ---- ground truth -------------------------------------------------------------------------------------------------------------------
TRUTH = {"fronto": ("fronto", 4, 48, 36), "slanted": ("slanted", 4, 48, 36), "step": ("step", 4, 48, 36)}
TRUTH_RELATIVE = 1e-3  # of the distance to the plane over the point's depth


def measure_accuracy(kind):
    """the share of fused points within TRUTH_RELATIVE of their plane, and the points per pixel of one image"""
    _, cams, w, h = TRUTH[kind]
    out = ref.fuse_depth_maps(*fc.rendered(kind, cams, w, h), min_num_pixels=3)
    X = out["xyz"].astype(np.float64)
    dist = np.full(len(X), np.inf)
    for n, off, side in pc.SCENES[kind]:
        n = np.asarray(n, np.float64)
        dist = np.minimum(dist, np.abs(X @ n - off) / np.linalg.norm(n))
    share = float(np.mean(dist / X[:, 2] <= TRUTH_RELATIVE)) if len(X) else 0.0
    return share, len(X) / float(w * h)


@pytest.mark.parametrize("kind", sorted(TRUTH))
def test_fused_points_against_ground_truth(kind):
    budget = json.loads(ACCURACY.read_text())[kind]
    share, density = measure_accuracy(kind)
    print(kind, "share", share, "density", density, "budget", budget)
    assert share >= budget["share_within"] - 0.02 and density >= 0.9 * budget["points_per_pixel"]


# ---- the host half of StereoFusion --------------------------------------------------------------------------------------------------
def tree(path):
    return {str(p.relative_to(path)): p.read_bytes() for p in sorted(Path(path).rglob("*")) if p.is_file()}


def write_dense_workspace(path, sc, stage="geometric", skip=()):
    """write_workspace, fusion.cfg in image order and the scene's exact maps as `stage` maps; `skip`: images without"""
    pc.write_workspace(str(path), sc, "")
    n = len(sc["images"])
    with open(path / "stereo" / "fusion.cfg", "w") as f:
        f.write("# the fusion order\n" + "".join(f"im{i}.pgm\n" for i in range(n)) + "\n")
    for i in range(n):
        if i in skip:
            continue
        write_array(path / "stereo" / "depth_maps" / f"im{i}.pgm.{stage}.bin", sc["depth"][i])
        write_array(path / "stereo" / "normal_maps" / f"im{i}.pgm.{stage}.bin", np.transpose(sc["normal"][i], (1, 2, 0)))


def test_config_parsing():
    names = ["a.png", "b.png", "c.png"]
    assert F.parse_config("# order\n\nb.png\n a.png \n", names) == ["b.png", "a.png"]
    assert F.parse_config("", names) == []
    with pytest.raises(ValueError, match="d.png is not in the sparse model"):
        F.parse_config("a.png\nd.png\n", names)
    with pytest.raises(ValueError, match="a.png is listed twice"):
        F.parse_config("a.png\nb.png\na.png\n", names)


def test_neighbour_selection_against_brute_force():
    rng = np.random.default_rng(5)
    order = [7, 3, 9, 4, 12, 1]
    seen = {i: sorted(set(rng.integers(0, 30, rng.integers(0, 25)).tolist())) for i in order}
    seen[12] = []
    for k in (1, 2, 5, 64):
        got = F.select_neighbours(order, seen, k)
        for at, i in enumerate(order):
            counts = [(len(set(seen[i]) & set(seen[j])), j) for j in order if j != i]
            brute = [order.index(j) for c, j in sorted(counts, key=lambda cj: (-cj[0], cj[1])) if c > 0][:k]
            assert got[at] == brute, (k, i)
    assert F.select_neighbours(order, seen, 3)[4] == []


def test_ply_and_vis_bytes():
    pts = np.zeros(2, F.POINT_DTYPE)
    pts[0] = (1.0, 2.0, 3.0, 0.0, 0.0, -1.0, 10, 20, 30)
    pts[1] = (-1.5, 0.25, 8.0, 0.0, 1.0, 0.0, 255, 0, 7)
    head = (b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
            b"property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
            b"end_header\n")
    body = struct.pack("<6f3B", 1.0, 2.0, 3.0, 0.0, 0.0, -1.0, 10, 20, 30) + struct.pack("<6f3B", -1.5, 0.25, 8.0, 0.0, 1.0, 0.0, 255, 0, 7)
    assert F.ply_bytes(pts) == head + body and len(body) == 2 * 27
    assert F.vis_bytes([[0, 2], [], [5]]) == struct.pack("<Q", 3) + struct.pack("<III", 2, 0, 2) + struct.pack("<I", 0) + struct.pack("<II", 1, 5)
    assert F.ply_bytes(pts[:0]).endswith(b"element vertex 0\n" + head.split(b"element vertex 2\n")[1]) and F.vis_bytes([]) == struct.pack("<Q", 0)


def test_without_a_gpu_run_raises_and_writes_nothing(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: test_stereo_fusion_gpu.py runs the class on it")
    write_dense_workspace(tmp_path, pc.scene("fronto", 3, 16, 12))
    before = tree(tmp_path)
    f = pycolmap.StereoFusion({}, str(tmp_path))
    with pytest.raises(Exception):
        f.run()
    assert not hasattr(f, "fused_points") and tree(tmp_path) == before
    with pytest.raises(ValueError, match="run"):
        f.write(str(tmp_path / "out.ply"))


def test_walk_with_the_reference_in_the_library_place(tmp_path):
    sc = pc.scene("slanted", 4, 24, 18)
    ws = tmp_path / "ws"
    ws.mkdir()
    write_dense_workspace(ws, sc, skip=(2,))
    before = tree(ws)
    f = pycolmap.StereoFusion(dict(min_num_pixels=2, check_num_images=2), str(ws))
    f._context_factory = ref.Context
    f.run()
    assert tree(ws) == before  # run() writes nothing
    pts, vis = f.fused_points, f.fused_points_visibility
    assert pts.dtype == F.POINT_DTYPE and len(pts) == len(vis) > 100
    assert f.summary["images_without_maps"] == 1 and f.summary["num_images"] == 3 and f.summary["num_points"] == len(pts)
    assert f.last_run_stats() == f.summary and pycolmap.last_run_stats()["num_points"] == len(pts)
    # the same call by hand: the images in fusion.cfg's order without image 2, neighbours from the shared points
    rec = pycolmap.Reconstruction(str(ws / "sparse"))
    keep = [0, 1, 3]
    seen = {i + 1: sorted({p.point3D_id for p in rec.images[i + 1].points2D if p.has_point3D()}) for i in keep}
    nb = F.select_neighbours([i + 1 for i in keep], seen, 2)
    rgb = [np.repeat(sc["images"][i][..., None], 3, axis=2) for i in keep]
    want = ref.fuse_depth_maps(rgb, sc["K"][keep], sc["R"][keep], sc["t"][keep], [np.asarray(sc["depth"][i], np.float32) for i in keep],
                               [np.asarray(sc["normal"][i], np.float32) for i in keep], nb, min_num_pixels=2)
    assert want["num_points"] == len(pts)
    assert np.array_equal(np.stack([pts["x"], pts["y"], pts["z"]], 1), want["xyz"]) and np.array_equal(np.stack([pts["r"], pts["g"], pts["b"]], 1), want["color"])
    assert np.array_equal(np.stack([pts["nx"], pts["ny"], pts["nz"]], 1), want["normal"])
    # the visibility names fusion.cfg's lines: image 3 is index 3, not 2
    flat = np.concatenate(vis)
    assert set(flat.tolist()) <= {0, 1, 3} and 3 in flat
    assert [len(v) for v in vis] == np.diff(want["vis_offsets"]).tolist()
    # a .ply path: the two files, byte for byte
    out = tmp_path / "fused.ply"
    model = f.write(str(out))
    assert out.read_bytes() == F.ply_bytes(pts) and (tmp_path / "fused.ply.vis").read_bytes() == F.vis_bytes(vis)
    assert model.num_points3D() == len(pts) and model.num_images() == 4
    assert tree(ws) == before
    # an existing directory: the sparse model with the fused points, read back
    (tmp_path / "model").mkdir()
    f.write(tmp_path / "model")
    assert sorted(p.name for p in (tmp_path / "model").iterdir()) == ["cameras.bin", "images.bin", "points3D.bin"]
    back = pycolmap.Reconstruction(str(tmp_path / "model"))
    assert back.num_points3D() == len(pts) and back.num_images() == 4 and back.num_cameras() == 4
    for k in (0, len(pts) // 2, len(pts) - 1):
        p = back.points3D[k + 1]
        assert list(p.xyz) == [float(pts[k]["x"]), float(pts[k]["y"]), float(pts[k]["z"])]
        assert list(p.color) == [int(pts[k]["r"]), int(pts[k]["g"]), int(pts[k]["b"])] and p.track.length() == 0
    assert not any(p.has_point3D() for im in back.images.values() for p in im.points2D)
    assert (tmp_path / "model" / "cameras.bin").read_bytes() == (ws / "sparse" / "cameras.bin").read_bytes()
    with pytest.raises(ValueError, match=r"\.ply"):
        f.write(str(tmp_path / "fused.txt"))
    # the photometric maps are other files: none here, so every image is left out
    g = pycolmap.StereoFusion({}, str(ws), input_type="photometric")
    g._context_factory = ref.Context
    g.run()
    assert len(g.fused_points) == 0 and g.summary["images_without_maps"] == 4 and g.fused_points_visibility == []


@pytest.mark.parametrize("options, kwargs, text", [
    ({}, dict(workspace_format="PMVS"), "workspace_format 'PMVS' is not supported"),
    ({}, dict(workspace_format="other"), "Invalid `workspace_format` - supported values are 'COLMAP' or 'PMVS'."),
    ({}, dict(input_type="both"), "Invalid input type - supported values are 'photometric' and 'geometric'."),
    (dict(mask_path="masks"), {}, "mask_path"),
    (dict(max_image_size=16), {}, "max_image_size"),
    (dict(check_num_images=65), {}, "check_num_images=65 is more than 64"),
    (dict(max_traversal_depth=129), {}, "max_traversal_depth=129 is more than 128"),
    (dict(min_num_pixels=-1), {}, "Check Failed: min_num_pixels >= 0"),
])
def test_refusals_leave_the_folder_untouched(options, kwargs, text, tmp_path):
    write_dense_workspace(tmp_path, pc.scene("fronto", 3, 24, 18))
    before = tree(tmp_path)
    f = pycolmap.StereoFusion(options, str(tmp_path), **kwargs)
    f._context_factory = ref.Context
    with pytest.raises(ValueError, match=text):
        f.run()
    assert tree(tmp_path) == before and not hasattr(f, "fused_points")


def test_refuses_a_camera_that_is_not_pinhole_and_a_map_of_another_size(tmp_path):
    sc = pc.scene("fronto", 3, 24, 18)
    write_dense_workspace(tmp_path, sc)
    write_array(tmp_path / "stereo" / "depth_maps" / "im1.pgm.geometric.bin", sc["depth"][1][:, :-1])
    before = tree(tmp_path)
    f = pycolmap.StereoFusion({}, str(tmp_path))
    f._context_factory = ref.Context
    with pytest.raises(ValueError, match="im1.pgm: the image is 24 x 18, its depth map 23 x 18"):
        f.run()
    assert tree(tmp_path) == before
    rec = pycolmap.Reconstruction()
    rec.read(str(tmp_path / "sparse"))
    cam = rec.cameras[1]
    rec.cameras[1] = pycolmap.Camera("SIMPLE_RADIAL", cam.width, cam.height, [26.0, 12.0, 9.0, 0.01], 1)
    rec.write(str(tmp_path / "sparse"))
    before = tree(tmp_path)
    with pytest.raises(ValueError, match="PINHOLE"):
        f.run()
    assert tree(tmp_path) == before and not hasattr(f, "fused_points")


if __name__ == "__main__":
    if "--write-budgets" in sys.argv:
        worst, rows = measure_deviation()
        DEVIATION.write_text(json.dumps(worst, indent=1) + "\n")
        compared, left_out, wrong = membership(rows, worst)
        print(worst, "candidates", len(rows), "compared", compared, "left out", left_out, f"({left_out / len(rows):.2%})", "wrong", wrong)
        acc = {}
        for kind in sorted(TRUTH):
            share, density = measure_accuracy(kind)
            acc[kind] = {"share_within": share, "points_per_pixel": density, "relative_distance": TRUTH_RELATIVE}
        ACCURACY.write_text(json.dumps(acc, indent=1) + "\n")
        print(acc)
