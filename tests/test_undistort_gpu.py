"""GPU checks of undistortion: Context.undistort_images against the CPU reference
(tests/undistort_ref) and the frozen fixtures on the warp cases and on the edge list (group tails, wave and block
boundaries, long windows, exact ties, coordinates that are not finite), the edge list's known answers in integer
arithmetic, batch independence and the batch count at its bound, the pybind building blocks, undistort_images end to
end on a tiny workspace and through several device calls, and the error paths.  Every comparison is exact: uint8
arrays equal, camera parameters equal bit for bit."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import undistort_cases as cases
import undistort_ref_lib as ref

import pycolmap_amd
from pycolmap_amd import _capi

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "undistort_ref_v1.npz"
EDGES_GOLDEN = ROOT / "tests" / "golden" / "undistort_ref_edges_v1.npz"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_camera(a, b):
    return tuple(int(v) for v in a[:3]) == tuple(int(v) for v in b[:3]) and np.array_equal(bits(a[3]), bits(b[3]))


def cam_tuple(c):
    return (int(c.model), int(c.width), int(c.height), np.array(c.params, dtype=np.float64))


@pytest.fixture(scope="module")
def reference():
    """[(name, image, source camera, target camera, reference image)], computed once and left unchanged."""
    out = []
    for name, img, cam, opts in cases.warp_cases():
        und = ref.undistort_camera(cam, **opts)
        want = ref.warp(img, cam, und)
        want.setflags(write=False)
        out.append((name, img, cam, und, want))
    return out


def test_case_list_covers_the_shapes_that_can_break_the_kernel(reference):
    by = {r[0]: r for r in reference}
    assert {n.split("-")[0] for n in by} >= set(cases.CAMERAS)  # the eleven models
    assert any(r[1].ndim == 2 for r in reference) and any(r[1].ndim == 3 for r in reference)
    assert by["PINHOLE-2x2"][1].shape == (2, 2)
    assert not by["OPENCV-stride-3ch"][1].flags.c_contiguous and by["OPENCV-stride-3ch"][1].strides[0] > cases.W * 3
    larger = [r for r in reference if r[3][1] * r[3][2] > r[1].shape[0] * r[1].shape[1]]
    smaller = [r for r in reference if r[3][1] * r[3][2] < r[1].shape[0] * r[1].shape[1]]
    assert len(larger) >= 8 and len(smaller) >= 6  # without and with the pre-pass
    assert "SIMPLE_RADIAL-default-1ch" in {r[0] for r in smaller}  # default options, barrel distortion
    assert (by["OPENCV_FISHEYE-strong-3ch"][4] == 0).mean() > 0.25  # many pixels outside
    assert by["RADIAL-roi-3ch"][3][1] < cases.W


@pytest.mark.parametrize("index", range(len(cases.warp_cases())), ids=[c[0] for c in cases.warp_cases()])
def test_warp_equals_reference_and_fixture(amc_ctx, reference, index):
    name, img, cam, und, want = reference[index]
    assert same_camera(_capi.undistort_camera(cam, **cases.warp_cases()[index][3]), und)
    outs, st = amc_ctx.undistort_images([img], [cam], [und])
    assert outs[0].shape == want.shape and outs[0].dtype == np.uint8
    assert np.array_equal(outs[0], want), f"{name}: {int((outs[0] != want).sum())} bytes differ"
    fx = np.load(GOLDEN)
    assert bytes(fx[f"{name}/digest"]).decode() == cases.digest(outs[0])
    assert st["num_batches"] == 1 and st["num_resized"] == int(want.shape[0] * want.shape[1] < img.shape[0] * img.shape[1])
    assert st["device_ms"] > 0 and st["kernel_ms"] > 0


BATCH_CHILD = """
import json, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import undistort_cases as cases, undistort_ref_lib as ref
from pycolmap_amd import _capi
cs = cases.warp_cases()
imgs = [c[1] for c in cs]; src = [c[2] for c in cs]; dst = [ref.undistort_camera(c[2], **c[3]) for c in cs]
with _capi.Context(0) as ctx:
    outs, st = ctx.undistort_images(imgs, src, dst)
print(json.dumps(dict(num_batches=st["num_batches"], digests=[cases.digest(o) for o in outs])))
"""


def test_batch_independence(amc_ctx, reference):
    imgs, src, dst = [r[1] for r in reference], [r[2] for r in reference], [r[3] for r in reference]
    outs, st = amc_ctx.undistort_images(imgs, src, dst)  # a mixed batch: sizes, cameras, channel counts
    assert st["num_batches"] == 1
    for r, o in zip(reference, outs):
        assert np.array_equal(o, r[4]), r[0]  # = the per-image calls' results (each equals the reference, above)
    single = [amc_ctx.undistort_images([i], [s], [d])[0][0] for i, s, d in list(zip(imgs, src, dst))[::5]]
    for o, s in zip(outs[::5], single):
        assert np.array_equal(o, s)
    order = np.random.default_rng(3).permutation(len(imgs))
    shuffled, _ = amc_ctx.undistort_images([imgs[k] for k in order], [src[k] for k in order], [dst[k] for k in order])
    for k, o in zip(order, shuffled):
        assert np.array_equal(o, outs[k]), reference[k][0]
    # the same batch split into device batches: the bound is read per call from the environment, so a fresh child
    child = subprocess.run([sys.executable, "-c", BATCH_CHILD.format(root=str(ROOT), tests=str(ROOT / "tests"))],
                           capture_output=True, text=True, timeout=120, env=dict(os.environ, AMC_UNDISTORT_BATCH_BYTES="60000"))
    assert child.returncode == 0, child.stderr[-2000:]
    got = json.loads(child.stdout.strip().splitlines()[-1])
    assert got["num_batches"] >= 3
    assert got["digests"] == [cases.digest(o) for o in outs]


def test_pybind_building_blocks_equal_the_capi(amc_ctx, reference):
    for name, img, cam, und, want in reference[::3]:
        opts = cases.warp_cases()[[r[0] for r in reference].index(name)][3]
        o = pycolmap_amd.UndistortCameraOptions(opts)
        c = pycolmap_amd.Camera(cam[0], cam[1], cam[2], [float(v) for v in cam[3]])
        assert same_camera(cam_tuple(pycolmap_amd.undistort_camera(o, c)), und), name
        out, ucam = pycolmap_amd.undistort_image(o, img, c)
        assert same_camera(cam_tuple(ucam), und) and out.dtype == np.uint8 and np.array_equal(out, want), name
    with pytest.raises(ValueError, match="the image is 2 x 2, the camera 67 x 45"):
        pycolmap_amd.undistort_image({}, np.zeros((2, 2), np.uint8), pycolmap_amd.Camera("PINHOLE", 67, 45, [60, 60, 33, 22]))
    with pytest.raises(ValueError, match="uint8"):
        pycolmap_amd.undistort_image({}, np.zeros((45, 67), np.float32), pycolmap_amd.Camera("PINHOLE", 67, 45, [60, 60, 33, 22]))


# ---- the edge list: targets given directly ---------------------------------------------------------------------
EDGE_NAMES = [c[0] for c in cases.edge_cases()]


@pytest.fixture(scope="module")
def edge_reference():
    """[(name, image, source camera, target camera, reference image)], computed once and left unchanged."""
    out = []
    for name, img, cam, dst in cases.edge_cases():
        want = ref.warp(img, cam, dst)
        want.setflags(write=False)
        out.append((name, img, cam, dst, want))
    return out


@pytest.fixture(scope="module")
def edge_fixture_digests():
    fx = np.load(EDGES_GOLDEN)
    return {name: bytes(fx[f"{name}/digest"]).decode() for name in EDGE_NAMES}


def takes_the_prepass(cam, dst):
    return dst[1] * dst[2] < cam[1] * cam[2]  # 14.4


@pytest.mark.parametrize("index", range(len(EDGE_NAMES)), ids=EDGE_NAMES)
def test_edge_case_equals_reference_and_fixture(amc_ctx, edge_reference, edge_fixture_digests, index):
    name, img, cam, dst, want = edge_reference[index]
    outs, st = amc_ctx.undistort_images([img], [cam], [dst])
    assert outs[0].shape == (dst[2], dst[1]) + img.shape[2:] and outs[0].shape == want.shape and outs[0].dtype == np.uint8
    assert np.array_equal(outs[0], want), f"{name}: {int((outs[0] != want).sum())} bytes differ"
    assert cases.digest(outs[0]) == edge_fixture_digests[name]
    assert st["num_batches"] == 1 and st["num_resized"] == int(takes_the_prepass(cam, dst))


def test_known_answers_on_the_device(amc_ctx):
    """The (g) cases against integer arithmetic alone (cases.known_answers), whatever the reference says."""
    by = {c[0]: c for c in cases.edge_cases()}
    answers = cases.known_answers()
    assert len(answers) == 8
    for name, (want, pinned) in answers.items():
        _, img, cam, dst = by[name]
        outs, _ = amc_ctx.undistort_images([img], [cam], [dst])
        assert pinned.all() and np.array_equal(outs[0], want), (name, int((outs[0] != want).sum()))


def test_edge_batch_independence(amc_ctx, edge_reference):
    imgs, src, dst = [r[1] for r in edge_reference], [r[2] for r in edge_reference], [r[3] for r in edge_reference]
    single = [amc_ctx.undistort_images([i], [s], [d])[0][0] for i, s, d in zip(imgs, src, dst)]
    resized = sum(takes_the_prepass(s, d) for s, d in zip(src, dst))
    assert 40 <= resized <= len(imgs) - 40  # both paths many times in one batch
    outs, st = amc_ctx.undistort_images(imgs, src, dst)
    assert st["num_batches"] == 1 and st["num_resized"] == resized
    for r, o, s in zip(edge_reference, outs, single):
        assert np.array_equal(o, s) and np.array_equal(o, r[4]), r[0]
    order = np.random.default_rng(5).permutation(len(imgs))
    shuffled, st = amc_ctx.undistort_images([imgs[k] for k in order], [src[k] for k in order], [dst[k] for k in order])
    assert st["num_batches"] == 1 and st["num_resized"] == resized
    for k, o in zip(order, shuffled):
        assert np.array_equal(o, single[k]), edge_reference[k][0]


def test_one_array_as_two_jobs_of_a_call(amc_ctx, edge_reference):
    by = {r[0]: r for r in edge_reference}
    a, b = by["e-window-67x45-to-22x15-3ch"], by["k-fortran-order-3ch"]  # both RADIAL on 67 x 45, three channels
    assert a[2][0] == b[2][0] and np.array_equal(a[2][3], b[2][3]) and a[1].shape == b[1].shape
    img = a[1]
    jobs = [a[3], b[3], cases.pinhole(67, 45, 58.0, 58.0, 33.25, 22.5), a[3]]  # with and without the pre-pass, one twice
    want = [ref.warp(img, a[2], d) for d in jobs]
    outs, st = amc_ctx.undistort_images([img] * len(jobs), [a[2]] * len(jobs), jobs)
    assert st["num_resized"] == 2
    for o, w in zip(outs, want):
        assert np.array_equal(o, w)
    assert np.array_equal(outs[0], outs[3]) and outs[0] is not outs[3] and np.array_equal(outs[0], a[4])


EDGE_CHILD = """
import json, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import undistort_cases as cases
from pycolmap_amd import _capi
cs = {cases_expr}
with _capi.Context(0) as ctx:
    outs, st = ctx.undistort_images([c[1] for c in cs], [c[2] for c in cs], [c[3] for c in cs])
print(json.dumps(dict(num_batches=st["num_batches"], num_resized=st["num_resized"], digests=[cases.digest(o) for o in outs])))
"""


def run_child(cases_expr, batch_bytes):
    """One Context.undistort_images call in a fresh process under AMC_UNDISTORT_BATCH_BYTES (read per call)."""
    code = EDGE_CHILD.format(root=str(ROOT), tests=str(ROOT / "tests"), cases_expr=cases_expr)
    child = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120,
                           env=dict(os.environ, AMC_UNDISTORT_BATCH_BYTES=str(batch_bytes)))
    assert child.returncode == 0, child.stderr[-2000:]
    return json.loads(child.stdout.strip().splitlines()[-1])


def test_every_edge_case_a_batch_of_its_own(edge_reference, edge_fixture_digests):
    """A bound below the smallest image: one batch per image, each at offset 0 of the one allocation, the pre-pass
    tables in memory that earlier batches used."""
    got = run_child("cases.edge_cases()", 1)
    assert got["num_batches"] == len(edge_reference)
    assert got["num_resized"] == sum(takes_the_prepass(r[2], r[3]) for r in edge_reference)
    assert got["digests"] == [edge_fixture_digests[r[0]] for r in edge_reference]


def align256(n):
    return (n + 255) // 256 * 256


SEVEN = ("[('seven-%d' % k, cases.make_image(cases.H, cases.W, 3, 900 + k), cases.camera('OPENCV'), "
         "cases.pinhole(70, 50, 62.0, 64.0, 35.0, 24.75)) for k in range(7)]")


@pytest.mark.parametrize("short_by, per_batch", [(0, 2), (1, 1)])
def test_batch_count_at_the_bound(short_by, per_batch):
    """14.5: an image without the pre-pass takes align256(source bytes) + align256(target bytes) of a batch; batches are
    greedy runs under the bound, the bound included."""
    per_image = align256(cases.W * cases.H * 3) + align256(70 * 50 * 3)
    assert per_image == 9216 + 10752 and 70 * 50 >= cases.W * cases.H
    want_batches = -(-7 // per_batch)
    assert want_batches == (4, 7)[short_by]
    got = run_child(SEVEN, 2 * per_image - short_by)
    assert got["num_batches"] == want_batches and got["num_resized"] == 0
    cam, dst = cases.camera("OPENCV"), cases.pinhole(70, 50, 62.0, 64.0, 35.0, 24.75)
    assert got["digests"] == [cases.digest(ref.warp(cases.make_image(cases.H, cases.W, 3, 900 + k), cam, dst)) for k in range(7)]


def test_degenerate_undistorted_camera_is_refused_as_a_target(amc_ctx):
    """14.2 step 5: max_image_size = 1 on 67 x 20 rounds the height to 0 samples: fy = cy = 0, which no image can be
    warped onto."""
    cam = cases.camera("OPENCV", height=20)
    und = _capi.undistort_camera(cam, max_image_size=1)
    assert (und[1], und[2]) == (1, 1) and und[3][1] == 0.0
    img = cases.make_image(20, cases.W, 3, 950)
    with pytest.raises(ValueError, match="target focal length is 0"):
        pycolmap_amd.undistort_image(dict(max_image_size=1), img, pycolmap_amd.Camera("OPENCV", cases.W, 20, [float(v) for v in cam[3]]))
    with pytest.raises(_capi.AmcError) as e:
        amc_ctx.undistort_images([img], [cam], [und])
    assert e.value.code == _capi.AMC_E_INVALID
    und_ok = _capi.undistort_camera(cases.camera("OPENCV"), max_image_size=1)  # 67 x 45: 1 x 1 with fy > 0, all black
    outs, _ = amc_ctx.undistort_images([cases.make_image(cases.H, cases.W, 3, 951)], [cases.camera("OPENCV")], [und_ok])
    assert outs[0].shape == (1, 1, 3) and not outs[0].any()


# ---- undistort_images end to end ---------------------------------------------------------------------------------------------
def have_pillow():
    try:
        import PIL  # noqa: F401
        return True
    except ImportError:
        return False


@pytest.fixture(scope="module")
def workspace(tmp_path_factory):
    """The tiny model plus a PINHOLE image (copied, not warped) and, with Pillow, a PNG; images as PPM / PGM."""
    root = tmp_path_factory.mktemp("undistort")
    cameras, images, points3D = cases.tiny_model()
    cameras[9] = (1, 40, 30, [35.0, 36.0, 20.0, 15.0])
    images[7] = (images[1][0], images[1][1], 9, "deep/er/p.pgm", [(3.0, 4.0, -1)])
    if have_pillow():
        images[8] = (images[2][0], images[2][1], 1, "d.png", [])
    cases.write_model_bin(root / "model", cameras, images, points3D)
    pixels = {}
    for iid, (_, _, cid, name, _) in images.items():
        _, w, h, _ = cameras[cid]
        img = cases.make_image(h, w, 1 if name.endswith(".pgm") else 3, 400 + iid)
        pixels[name] = img
        if name.endswith(".png"):
            from PIL import Image
            Image.fromarray(img).save(root / "images" / name)
        else:
            cases.write_pnm(root / "images" / name, img)
    return root, cameras, images, points3D, pixels


def read_any(path):
    if str(path).endswith(".png"):
        from PIL import Image
        return np.asarray(Image.open(path))
    return cases.read_pnm(path)


def tree(path):
    return sorted(str(p.relative_to(path)) + ("/" if p.is_dir() else "") for p in Path(path).rglob("*"))


def test_undistort_images_end_to_end(workspace, tmp_path):
    root, cameras, images, points3D, pixels = workspace
    opts = dict(blank_pixels=0.25)
    out = tmp_path / "dense"
    pycolmap_amd.undistort_images(out, root / "model", root / "images", num_patch_match_src_images=7, undistort_options=opts)
    names = [im[3] for im in images.values()]
    want_tree = ["images/", "sparse/", "stereo/", "sparse/cameras.bin", "sparse/images.bin", "sparse/points3D.bin",
                 "stereo/patch-match.cfg", "stereo/fusion.cfg"] + [f"images/{n}" for n in names]
    for sub in ("images", "stereo/depth_maps", "stereo/normal_maps", "stereo/consistency_graphs"):
        want_tree += [f"{sub}/", f"{sub}/sub/", f"{sub}/deep/", f"{sub}/deep/er/"]
    assert tree(out) == sorted(set(want_tree))
    assert (out / "stereo" / "patch-match.cfg").read_text() == "".join(f"{n}\n__auto__, 7\n" for n in names)
    assert (out / "stereo" / "fusion.cfg").read_text() == "".join(f"{n}\n" for n in names)
    # the undistorted model
    ucams, uimages, upoints = cases.parse_model_bin(out / "sparse")
    assert upoints == points3D and list(uimages) == list(images)
    und = {cid: ref.undistort_camera(c, **opts) for cid, c in cameras.items()}
    for cid, c in ucams.items():
        assert same_camera((c[0], c[1], c[2], np.array(c[3])), und[cid]), cid
    for iid, (q, t, cid, name, pts) in images.items():
        uq, ut, ucid, uname, upts = uimages[iid]
        assert (uq, ut, ucid, uname) == (q, t, cid, name) and [p[2] for p in upts] == [p[2] for p in pts]
        if cameras[cid][0] == 1:
            assert upts == pts
        elif pts:
            want = ref.undistort_points(cameras[cid], und[cid], [[p[0], p[1]] for p in pts])
            assert np.array_equal(bits([[p[0], p[1]] for p in upts]), bits(want)), name
        # the pixels
        got = read_any(out / "images" / name)
        if cameras[cid][0] == 1:
            assert np.array_equal(got, pixels[name])
        else:
            assert np.array_equal(got, ref.warp(pixels[name], cameras[cid], und[cid])), name
        assert got.ndim == pixels[name].ndim  # colour stays colour, grey stays grey
    st = pycolmap_amd.last_run_stats()
    for k in ("images", "pixels", "decode_ms", "device_ms", "kernel_ms", "encode_ms", "total_ms"):
        assert k in st, k
    assert st["images"] == len(names) and st["warped"] == len(names) - 1 and st["copied"] == 1
    assert st["pixels"] == sum(und[im[2]][1] * und[im[2]][2] for im in images.values() if cameras[im[2]][0] != 1)


def test_copy_policy_and_image_list(workspace, tmp_path, capfd):
    root, cameras, images, points3D, pixels = workspace
    src = root / "images" / "deep/er/p.pgm"
    for policy, check in (("copy", lambda p: not p.is_symlink() and p.stat().st_ino != src.stat().st_ino),
                          (getattr(pycolmap_amd.CopyType, "soft-link"), lambda p: os.path.islink(p) and p.resolve() == src.resolve()),
                          ("hard-link", lambda p: not os.path.islink(p) and p.stat().st_nlink >= 2 and p.stat().st_ino == src.stat().st_ino)):
        out = tmp_path / f"dense-{policy}"
        capfd.readouterr()
        pycolmap_amd.undistort_images(out, root / "model", root / "images", ["deep/er/p.pgm", "nope.ppm", "a.ppm"],
                                      copy_policy=policy)
        assert "Cannot find image nope.ppm" in capfd.readouterr().err
        assert check(out / "images" / "deep/er/p.pgm"), policy
        assert np.array_equal(cases.read_pnm(out / "images" / "deep/er/p.pgm"), pixels["deep/er/p.pgm"])
        # the list restricts images/ and the two cfg files, not sparse/
        assert sorted(str(p.relative_to(out / "images")) for p in (out / "images").rglob("*") if not p.is_dir()) == \
            ["a.ppm", "deep/er/p.pgm"]
        assert (out / "stereo" / "fusion.cfg").read_text() == "deep/er/p.pgm\na.ppm\n"
        assert (out / "stereo" / "patch-match.cfg").read_text() == "deep/er/p.pgm\n__auto__, 20\na.ppm\n__auto__, 20\n"
        assert list(cases.parse_model_bin(out / "sparse")[1]) == list(images)
        und = ref.undistort_camera(cameras[1])
        assert np.array_equal(cases.read_pnm(out / "images" / "a.ppm"), ref.warp(pixels["a.ppm"], cameras[1], und))


def test_driver_batches_write_the_same_workspace(tmp_path, monkeypatch):
    """undistort_images' own batch loop (BATCH_BYTES of source pixels a device call; the previous batch's files are
    written while the next is warped): six distorted images in four device calls give the files of one call."""
    from pycolmap_amd import _undistortion
    cameras, images, points3D = cases.tiny_model()
    for iid, cid, name in ((6, 1, "d.ppm"), (7, 3, "sub/e.pgm"), (8, 1, "f.ppm")):
        images[iid] = (images[1][0], images[2][1], cid, name, [(5.0 + iid, 6.0, -1)])
    cases.write_model_bin(tmp_path / "model", cameras, images, points3D)
    sizes = []
    for iid, (_, _, cid, name, _) in images.items():
        _, w, h, _ = cameras[cid]
        cases.write_pnm(tmp_path / "images" / name, cases.make_image(h, w, 1 if name.endswith(".pgm") else 3, 800 + iid))
        sizes.append(w * h * 3)
    assert len(sizes) == 6 and all(c[0] > 1 for c in cameras.values())  # six images, every one warped
    pycolmap_amd.undistort_images(tmp_path / "one", tmp_path / "model", tmp_path / "images")
    st = pycolmap_amd.last_run_stats()
    assert st["warped"] == 6 and st["num_batches"] == 1
    bound = 16000
    calls, i = 0, 0
    while i < len(sizes):  # the loop of 14.8, restated: greedy runs of whole images under the bound, at least one each
        j, total = i, 0
        while j < len(sizes) and (j == i or total + sizes[j] <= bound):
            total += sizes[j]
            j += 1
        calls, i = calls + 1, j
    assert calls == 4
    monkeypatch.setattr(_undistortion, "BATCH_BYTES", bound)
    pycolmap_amd.undistort_images(tmp_path / "many", tmp_path / "model", tmp_path / "images")
    st = pycolmap_amd.last_run_stats()
    assert st["warped"] == 6 and st["num_batches"] == calls >= 3
    assert tree(tmp_path / "many") == tree(tmp_path / "one")
    files = [p for p in tree(tmp_path / "one") if not p.endswith("/")]
    assert sum(p.startswith("images/") for p in files) == 6 and "stereo/patch-match.cfg" in files and "stereo/fusion.cfg" in files
    assert sum(p.startswith("sparse/") for p in files) == 3
    for p in files:
        assert (tmp_path / "many" / p).read_bytes() == (tmp_path / "one" / p).read_bytes(), p
    und = ref.undistort_camera(cameras[1])
    assert np.array_equal(cases.read_pnm(tmp_path / "many" / "images" / "f.ppm"),
                          ref.warp(cases.make_image(cases.H, cases.W, 3, 808), cameras[1], und))  # the last batch's file


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_context_usable(amc_ctx, reference):
    import ctypes as C
    name, img, cam, und, want = reference[8]
    lib = _capi.load()

    def call(**change):
        a = np.ascontiguousarray(img)
        out = np.zeros_like(want)
        ch = 1 if a.ndim == 2 else 3
        job = _capi.UndistortImage(a.ctypes.data, a.strides[0], ch, 0, _capi._undistort_cam(cam), _capi._undistort_cam(und),
                                   out.ctypes.data)
        for k, v in change.items():
            if k in ("src", "dst", "channels", "src_stride"):
                setattr(job, k, v)
            elif k == "dst_model":
                job.dst_camera.model = v
            elif k == "src_width":
                job.src_camera.width = v
            elif k == "dst_height":
                job.dst_camera.height = v
        res = _capi.UndistortResult()
        rc = lib.amc_undistort_images(amc_ctx._h, 1, C.byref(job), C.byref(res))
        return rc, out

    for change in (dict(src=None), dict(dst=None), dict(src_width=0), dict(dst_height=0), dict(channels=2), dict(channels=4),
                   dict(dst_model=0), dict(dst_model=4), dict(src_stride=3)):
        rc, _ = call(**change)
        assert rc == _capi.AMC_E_INVALID, change
        assert "amc_undistort_images" in lib.amc_last_error().decode()
    res = _capi.UndistortResult()
    assert lib.amc_undistort_images(amc_ctx._h, 1, None, C.byref(res)) == _capi.AMC_E_INVALID
    assert lib.amc_undistort_images(amc_ctx._h, 0, None, C.byref(res)) == _capi.AMC_OK and res.num_batches == 0
    rc, out = call()
    assert rc == _capi.AMC_OK and np.array_equal(out, want)
    outs, _ = amc_ctx.undistort_images([img], [cam], [und])
    assert np.array_equal(outs[0], want)
    with pytest.raises(ValueError, match="takes 8 parameters"):
        amc_ctx.undistort_images([img], [("OPENCV", 67, 45, [1.0, 2.0])], [und])
