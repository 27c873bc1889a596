"""GPU checks of undistortion: Context.undistort_images against the CPU reference
(tests/undistort_ref) and the frozen fixture, batch independence, the pybind building blocks, undistort_images end to
end on a tiny workspace, and the error paths.  Every comparison is exact: uint8 arrays equal, camera parameters equal
bit for bit."""
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
