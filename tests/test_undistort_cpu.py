"""CPU-only checks of undistortion: the public surface, undistort_camera against known answers
and the frozen fixture, the CPU reference's warp and resize against independent float64 numpy restatements, the
sparse-model reader and writer against an independent struct.pack writer and parser, and the workspace plan.  Nothing
here needs a device: undistort_camera, the points2D map, the model I/O and the plan are host computations."""
import inspect
from pathlib import Path

import numpy as np
import pytest

import undistort_cases as cases
import undistort_ref_lib as ref

import pycolmap_amd
from pycolmap_amd import _capi

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "undistort_ref_v1.npz"
EDGES_GOLDEN = ROOT / "tests" / "golden" / "undistort_ref_edges_v1.npz"
RECORDED = ROOT / "tests" / "golden" / "undistort_pycolmap_v1.npz"
OPTION_FIELDS = dict(blank_pixels=0.0, min_scale=0.2, max_scale=2.0, max_image_size=-1, roi_min_x=0.0, roi_min_y=0.0,
                     roi_max_x=1.0, roi_max_y=1.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_camera(a, b):
    return tuple(int(v) for v in a[:3]) == tuple(int(v) for v in b[:3]) and np.array_equal(bits(a[3]), bits(b[3]))


def py_camera(cam):
    return pycolmap_amd.Camera(cam[0], cam[1], cam[2], [float(v) for v in cam[3]])


def cam_tuple(c):
    return (int(c.model), int(c.width), int(c.height), np.array(c.params, dtype=np.float64))


# ---- surface ------------------------------------------------------------------------------------------------------------
def test_surface_names_defaults_and_protocol():
    for name in ("UndistortCameraOptions", "CopyType", "undistort_images", "undistort_camera", "undistort_image",
                 "_undistort_plan", "last_run_stats"):
        assert hasattr(pycolmap_amd, name), name
    o = pycolmap_amd.UndistortCameraOptions()
    assert o.todict() == OPTION_FIELDS
    assert pycolmap_amd.UndistortCameraOptions({"blank_pixels": 0.5}).blank_pixels == 0.5
    assert pycolmap_amd.UndistortCameraOptions(max_image_size=100).max_image_size == 100
    o.mergedict({"roi_max_x": 0.5})
    assert o.roi_max_x == 0.5 and "roi_max_x = 0.5" in o.summary()
    with pytest.raises(ValueError, match="unknown option"):
        pycolmap_amd.UndistortCameraOptions({"nope": 1})
    sig = inspect.signature(pycolmap_amd.undistort_images)
    assert list(sig.parameters) == ["output_path", "input_path", "image_path", "image_list", "output_type", "copy_policy",
                                    "num_patch_match_src_images", "undistort_options"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["image_list"] == [] and d["output_type"] == "COLMAP" and d["num_patch_match_src_images"] == 20
    assert d["copy_policy"] == pycolmap_amd.CopyType.copy and d["undistort_options"].todict() == OPTION_FIELDS


def test_copy_type_from_string():
    ct = pycolmap_amd.CopyType
    assert sorted(ct.__members__) == ["copy", "hard-link", "soft-link"]
    assert ct("copy") == ct.copy and ct("soft-link") == getattr(ct, "soft-link") and ct("hard-link") == getattr(ct, "hard-link")
    with pytest.raises(ValueError, match="Invalid string value link for enum CopyType"):
        ct("link")


def test_resolves_through_import_pycolmap():
    import pycolmap
    for name in ("UndistortCameraOptions", "CopyType", "undistort_images", "undistort_camera", "undistort_image"):
        assert getattr(pycolmap, name) is getattr(pycolmap_amd, name)
    assert "undistort_images" in pycolmap.__doc__
    with pytest.raises(AttributeError, match="outside pycolmap_amd's scope.*undistortion"):
        pycolmap.patch_match_stereo


def test_abi_symbols_are_listed_and_exported():
    new = {"amc_undistort_opts_default", "amc_undistort_camera", "amc_undistort_points", "amc_undistort_images"}
    assert new <= set(_capi.EXPORTED_SYMBOLS)
    lib = _capi.load()
    assert all(hasattr(lib, n) for n in new) and lib.amc_abi_version() == 5
    o = _capi.undistort_options()
    assert {k: getattr(o, k) for k in OPTION_FIELDS} == OPTION_FIELDS


@pytest.mark.parametrize("bad, expr", [
    (dict(blank_pixels=-0.1), "blank_pixels >= 0"), (dict(blank_pixels=1.5), "blank_pixels <= 1"),
    (dict(min_scale=0.0), "min_scale > 0"), (dict(min_scale=3.0), "min_scale <= max_scale"),
    (dict(max_image_size=0), "max_image_size != 0"), (dict(roi_min_x=-0.1), "roi_min_x >= 0"),
    (dict(roi_min_y=-0.1), "roi_min_y >= 0"), (dict(roi_max_x=1.1), "roi_max_x <= 1"), (dict(roi_max_y=1.1), "roi_max_y <= 1"),
    (dict(roi_min_x=0.5, roi_max_x=0.5), "roi_min_x < roi_max_x"), (dict(roi_min_y=0.6, roi_max_y=0.5), "roi_min_y < roi_max_y")])
def test_option_checks_are_throw_check_errors(bad, expr):
    cam = py_camera(cases.camera("OPENCV"))
    with pytest.raises(ValueError, match=r"^\[undistort_host\.h:\d+\] Check Failed: " + expr.replace("(", r"\(")):
        pycolmap_amd.undistort_camera(bad, cam)
    with pytest.raises(_capi.AmcError) as e:  # the C ABI refuses them too
        _capi.undistort_camera(cases.camera("OPENCV"), **bad)
    assert e.value.code == _capi.AMC_E_INVALID


def test_undistort_images_argument_errors(tmp_path):
    (tmp_path / "model").mkdir()
    (tmp_path / "images").mkdir()
    with pytest.raises(ValueError, match=r"Check Failed: ExistsDir\(input_path\) : Directory .*nowhere does not exist\."):
        pycolmap_amd.undistort_images(tmp_path / "out", tmp_path / "nowhere", tmp_path / "images")
    with pytest.raises(ValueError, match=r"Check Failed: ExistsDir\(image_path\) : Directory .*nowhere does not exist\."):
        pycolmap_amd.undistort_images(tmp_path / "out", tmp_path / "model", tmp_path / "nowhere")
    with pytest.raises(ValueError, match=r"Invalid `output_type` - supported values are \{'COLMAP', 'PMVS', 'CMP-MVS'\}\."):
        pycolmap_amd.undistort_images(tmp_path / "out", tmp_path / "model", tmp_path / "images", output_type="MVE")
    for t in ("PMVS", "CMP-MVS"):
        with pytest.raises(ValueError, match="not supported by pycolmap_amd"):
            pycolmap_amd.undistort_images(tmp_path / "out", tmp_path / "model", tmp_path / "images", output_type=t)
    with pytest.raises(ValueError, match="do not exist as .bin or .txt"):  # an empty model folder
        pycolmap_amd.undistort_images(tmp_path / "out", tmp_path / "model", tmp_path / "images")


# ---- undistort_camera -----------------------------------------------------------------------------------------------------
def test_pinhole_models_come_back_as_pinhole_with_the_same_numbers():
    for model in ("PINHOLE", "SIMPLE_PINHOLE"):
        cam = cases.camera(model)
        p = cases.CAMERAS[model]
        want = (1, cases.W, cases.H, np.array(p if model == "PINHOLE" else [p[0], p[0], p[1], p[2]]))
        assert same_camera(_capi.undistort_camera(cam), want)
        assert same_camera(ref.undistort_camera(cam), want)
        assert same_camera(cam_tuple(pycolmap_amd.undistort_camera(pycolmap_amd.UndistortCameraOptions(), py_camera(cam))), want)


def test_simple_radial_without_distortion_loses_one_column():
    """k = 0, W = 100, cx = 50: the borders lift to themselves, left x = 0.5 and right x = 99.5, so min_scale_x =
    min(50 / 49.5, 49.5 / 49.5) = 1 and max_scale_x = 50 / 49.5; blank_pixels = 0 takes 1 / max_scale_x =
    (cx - 0.5) / cx = 0.99, hence width size_t(99.0) = 99 and cx = 50 * 99 / 100.  Likewise H = 80, cy = 40: 79."""
    und = _capi.undistort_camera(("SIMPLE_RADIAL", 100, 80, [90.0, 50.0, 40.0, 0.0]))
    assert same_camera(und, (1, 99, 79, np.array([90.0, 90.0, 50.0 * 99.0 / 100.0, 40.0 * 79.0 / 80.0])))
    # blank_pixels = 1 takes 1 / min_scale = 1: the source's size
    und = _capi.undistort_camera(("SIMPLE_RADIAL", 100, 80, [90.0, 50.0, 40.0, 0.0]), blank_pixels=1.0)
    assert same_camera(und, (1, 100, 80, np.array([90.0, 90.0, 50.0, 40.0])))


def test_roi_halves():
    """PINHOLE 100 x 80 with the right half, then the bottom half: round(0.5 * 100) = 50 columns from x = 50, the
    principal point moves by 50.  The border walk of a PINHOLE ROI gives left 0.5 - 50 + ... : both scales come out
    as those of the full image seen through the window, so only size and principal point are pinned here by hand for
    the exact window (fx 64, cx 75: left x = 0.5 - 50, right x = 99.5 - 50, min/max scale_x = min/max(25 / 74.5,
    24.5 / 24.5) -> blank_pixels 1 gives 1 / (25 / 74.5) clamped to max_scale 2: 100 columns)."""
    cam = ("PINHOLE", 100, 80, [64.0, 64.0, 75.0, 40.0])
    und = _capi.undistort_camera(cam, roi_min_x=0.5, blank_pixels=1.0)
    assert und[1] == 100 and und[2] == 80  # scale_x clamped to 2 on 50 columns; scale_y = 1 / min(40/39.5, 1) = 1
    assert und[3][2] == 25.0 * 100.0 / 50.0 and und[3][0] == 64.0
    und = _capi.undistort_camera(cam, roi_min_x=0.5, blank_pixels=0.0)
    # max_scale_x = max(25 / 74.5, 1) = 1 -> 50 columns, cx = 75 - 50; max_scale_y = max(40 / 39.5, 1) -> 79 rows
    assert same_camera(und, (1, 50, 79, np.array([64.0, 64.0, 25.0, 40.0 * 79.0 / 80.0])))
    und = _capi.undistort_camera(cam, roi_min_y=0.5, blank_pixels=0.0)
    assert und[2] == 40 and und[3][3] == 0.0  # rows 40 .. 79, cy = 40 - 40
    assert same_camera(und, ref.undistort_camera(cam, roi_min_y=0.5, blank_pixels=0.0))


def test_max_image_size_below_the_image():
    """PINHOLE 100 x 80, max_image_size 50: factor min(0.5, 0.625) = 0.5, Rescale gives round(50) x round(40) and
    scales focal lengths and principal point by 50 / 100 and 40 / 80."""
    und = _capi.undistort_camera(("PINHOLE", 100, 80, [64.0, 60.0, 48.0, 42.0]), max_image_size=50)
    assert same_camera(und, (1, 50, 40, np.array([32.0, 30.0, 24.0, 21.0])))
    und = _capi.undistort_camera(("PINHOLE", 100, 80, [64.0, 60.0, 48.0, 42.0]), max_image_size=100)
    assert same_camera(und, (1, 100, 80, np.array([64.0, 60.0, 48.0, 42.0])))  # factor 1: unchanged


def test_blank_pixels_ordering_and_scale_clamps():
    for model in cases.CAMERAS:
        cam = cases.camera(model)
        u0, u1 = _capi.undistort_camera(cam, blank_pixels=0.0), _capi.undistort_camera(cam, blank_pixels=1.0)
        assert u1[1] >= u0[1] and u1[2] >= u0[2], model  # keeping every source pixel never gives a smaller image
        lo = _capi.undistort_camera(cam, min_scale=1.5, max_scale=1.5)
        if model not in ("PINHOLE", "SIMPLE_PINHOLE"):  # (they skip the border walk)
            assert (lo[1], lo[2]) == (int(1.5 * cases.W), int(1.5 * cases.H)), model
            hi = _capi.undistort_camera(cam, min_scale=0.25, max_scale=0.25)
            assert (hi[1], hi[2]) == (int(0.25 * cases.W), int(0.25 * cases.H)), model


def test_undistort_camera_product_equals_reference_on_every_case():
    for name, img, cam, opts in cases.warp_cases():
        und = _capi.undistort_camera(cam, **opts)
        assert same_camera(und, ref.undistort_camera(cam, **opts)), name
        o = pycolmap_amd.UndistortCameraOptions(opts)
        assert same_camera(cam_tuple(pycolmap_amd.undistort_camera(o, py_camera(cam))), und), name


def test_reference_against_frozen_fixture():
    fx = np.load(GOLDEN)
    names = [c[0] for c in cases.warp_cases()]
    assert sorted({k.split("/")[0] for k in fx.files}) == sorted(names)
    full = 0
    for name, img, cam, opts in cases.warp_cases():
        assert bytes(fx[f"{name}/input_digest"]).decode() == cases.digest(img), name  # the seeded inputs are the frozen ones
        und = ref.undistort_camera(cam, **opts)
        assert same_camera(und, (1, *fx[f"{name}/size"], fx[f"{name}/params"])), name
        warped = ref.warp(img, cam, und)
        assert bytes(fx[f"{name}/digest"]).decode() == cases.digest(warped), name
        if f"{name}/image" in fx.files:
            assert np.array_equal(fx[f"{name}/image"], warped), name
            full += 1
    assert full == 4


# ---- the reference against independent numpy restatements ------------------------------------------------------------------
def np_img_from_cam(model, p, u, v):
    """Camera::ImgFromCam of colmap/sensor/models.h for arrays, with numpy's arctan / tan."""
    nf = 1 if model in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE") else 2
    f1, f2, c1, c2 = p[0], p[nf - 1], p[nf], p[nf + 1]
    e = p[nf + 2:]
    eps = np.finfo(np.float64).eps
    if model in ("SIMPLE_PINHOLE", "PINHOLE"):
        return f1 * u + c1, f2 * v + c2
    if model == "FOV":
        omega, r2 = e[0], u * u + v * v
        if omega * omega < 1e-4:
            factor = omega * omega * r2 / 3 - omega * omega / 12 + 1
        else:
            t = np.tan(omega / 2)
            r = np.sqrt(np.maximum(r2, 1e-300))
            factor = np.where(r2 < 1e-4, (-2 * t * (4 * r2 * t * t - 3)) / (3 * omega), np.arctan(r * 2 * t) / (r * omega))
        return f1 * u * factor + c1, f2 * v * factor + c2
    if model == "THIN_PRISM_FISHEYE":
        r = np.sqrt(u * u + v * v)
        s = np.where(r > eps, np.arctan(r) / np.maximum(r, 1e-300), 1.0)
        u, v = u * s, v * s
    u2, uv, v2 = u * u, u * v, v * v
    r2 = u2 + v2
    if model == "SIMPLE_RADIAL":
        du, dv = u * e[0] * r2, v * e[0] * r2
    elif model == "RADIAL":
        rad = e[0] * r2 + e[1] * r2 ** 2
        du, dv = u * rad, v * rad
    elif model == "OPENCV":
        rad = e[0] * r2 + e[1] * r2 ** 2
        du = u * rad + 2 * e[2] * uv + e[3] * (r2 + 2 * u2)
        dv = v * rad + 2 * e[3] * uv + e[2] * (r2 + 2 * v2)
    elif model == "FULL_OPENCV":
        rad = (1 + e[0] * r2 + e[1] * r2 ** 2 + e[4] * r2 ** 3) / (1 + e[5] * r2 + e[6] * r2 ** 2 + e[7] * r2 ** 3)
        du = u * rad + 2 * e[2] * uv + e[3] * (r2 + 2 * u2) - u
        dv = v * rad + 2 * e[3] * uv + e[2] * (r2 + 2 * v2) - v
    elif model == "THIN_PRISM_FISHEYE":
        rad = e[0] * r2 + e[1] * r2 ** 2 + e[4] * r2 ** 3 + e[5] * r2 ** 4
        du = u * rad + 2 * e[2] * uv + e[3] * (r2 + 2 * u2) + e[6] * r2
        dv = v * rad + 2 * e[3] * uv + e[2] * (r2 + 2 * v2) + e[7] * r2
    else:  # the equidistant fisheye family
        nk = {"SIMPLE_RADIAL_FISHEYE": 1, "RADIAL_FISHEYE": 2}.get(model, 4)
        k = list(e[:nk]) + [0.0] * (4 - nk)
        r = np.sqrt(r2)
        th = np.arctan(r)
        thd = th * (1 + k[0] * th ** 2 + k[1] * th ** 4 + k[2] * th ** 6 + k[3] * th ** 8)
        s = np.where(r > eps, thd / np.maximum(r, 1e-300), 1.0)
        du, dv = u * s - u, v * s - v
    return f1 * (u + du) + c1, f2 * (v + dv) + c2


def np_warp(img, model, params, pin, dw, dh):
    """DESIGN.md 14.3 for a whole image: (values before rounding (dh, dw, ch), inside mask, distance to the nearest
    inside / outside bound in pixels)."""
    sh, sw = img.shape[:2]
    a = img.reshape(sh, sw, -1).astype(np.float64)
    y, x = np.mgrid[0:dh, 0:dw].astype(np.float64)
    sx, sy = np_img_from_cam(model, np.asarray(params, np.float64), (x + 0.5 - pin[2]) / pin[0], (y + 0.5 - pin[3]) / pin[1])
    xs, iy = sx - 0.5, (sh - 1) - (sy - 0.5)
    with np.errstate(invalid="ignore"):
        x0, y0 = np.floor(xs), np.floor(iy)
        inside = (x0 >= 0) & (x0 + 1 < sw) & (y0 >= 0) & (y0 + 1 < sh)
    margin = np.minimum(np.minimum(np.abs(xs), np.abs(xs - (sw - 1))), np.minimum(np.abs(iy), np.abs(iy - (sh - 1))))
    xi, yi = np.where(inside, x0, 0).astype(int), np.where(inside, y0, 0).astype(int)
    dx, dy = (xs - x0)[..., None], (iy - y0)[..., None]
    r0, r1 = sh - 1 - yi, np.maximum(sh - 2 - yi, 0)  # bottom-up rows y0 and y0 + 1
    xj = np.minimum(xi + 1, sw - 1)
    v0 = (1 - dx) * a[r0, xi] + dx * a[r0, xj]
    v1 = (1 - dx) * a[r1, xi] + dx * a[r1, xj]
    return (1 - dy) * v0 + dy * v1, inside, margin


def np_rescaled(model, params, sx, sy):
    p = np.array(params, np.float64)
    nf = 1 if model in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE") else 2
    p[nf] *= sx
    p[nf + 1] *= sy
    if nf == 1:
        p[0] *= (sx + sy) / 2
    else:
        p[0] *= sx
        p[1] *= sy
    return p


@pytest.mark.parametrize("case", cases.warp_cases() + cases.edge_cases(), ids=lambda c: c[0])
def test_reference_warp_against_numpy_restatement(case):
    """Conditions, not measurements: where both call a pixel inside, the reference's byte is the numpy value rounded
    (|byte - value| <= 0.5 + 1e-6: the project's atan is within one ulp of numpy's, which moves a coordinate by parts in
    1e-13 and a value by less than 1e-9); inside / outside may differ only within 1e-9 of a bound.  A case carries
    either undistort_camera's options or (the edge list) the target camera itself."""
    name, img, cam, target = case
    model, sw, sh, params = cam
    und = ref.undistort_camera(cam, **target) if isinstance(target, dict) else target
    dw, dh = und[1], und[2]
    out, vals, coords = ref.warp(img, cam, und, details=True)
    src = np.ascontiguousarray(img)
    if dw * dh < sw * sh:  # the pre-pass (checked on its own below): resized pixels, Camera::Rescale(dw, dh)
        src = ref.resize(src, dw, dh)
        params = np_rescaled(model, params, dw / sw, dh / sh)
    with np.errstate(all="ignore"):  # the (h) cases overflow on purpose
        want, inside, margin = np_warp(src, model, params, und[3], dw, dh)
    ref_inside = vals[..., 0] >= 0
    differ = ref_inside != inside
    assert np.all(margin[differ] <= 1e-9), (name, int(differ.sum()))
    both = ref_inside & inside
    assert both.any() or name == "SIMPLE_RADIAL-2x2-3ch" or "black" in name
    o3 = out.reshape(dh, dw, -1).astype(np.float64)
    assert np.all(np.abs(o3[both] - want[both]) <= 0.5 + 1e-6), name
    assert np.all(np.abs(vals[both] - want[both]) <= 1e-6), name
    assert np.all(out.reshape(dh, dw, -1)[~ref_inside] == 0), name


def np_axis_matrix(n_in, n_out):
    """DESIGN.md 14.4 as a dense n_out x n_in weight matrix."""
    scale = n_out / n_in
    width, fscale = (1 / scale, scale) if scale < 1 else (1.0, 1.0)
    m = np.zeros((n_out, n_in))
    for u in range(n_out):
        center = u / scale + 0.5 / scale
        left, right = max(0, int(center - width + 0.5)), min(int(center + width + 0.5), n_in)
        i = np.arange(left, right)
        m[u, left:right] = fscale * np.maximum(0.0, 1 - np.abs(fscale * (i + 0.5 - center)))
    return m / m.sum(axis=1, keepdims=True)


def window_shapes():
    """The (source, target) shapes of the edge list's windows as (array shape, dw, dh)."""
    return [((sh, sw) + ((3,) if ch == 3 else ()), dw, dh) for (sw, sh), (dw, dh), ch in cases.WINDOWS]


@pytest.mark.parametrize("shape, dw, dh", [((45, 67, 3), 30, 45), ((45, 67), 67, 20), ((45, 67), 66, 42), ((9, 5, 3), 2, 9),
                                           ((7, 40), 13, 7)] + window_shapes())
def test_reference_resize_against_numpy_restatement(shape, dw, dh):
    img = cases.make_image(shape[0], shape[1], 1 if len(shape) == 2 else 3, 500 + dw)
    a = img.reshape(shape[0], shape[1], -1).astype(np.float64)
    mx, my = np_axis_matrix(shape[1], dw), np_axis_matrix(shape[0], dh)
    assert np.allclose(mx.sum(1), 1) and np.allclose(my.sum(1), 1)
    rows = ref.resize(img, dw, shape[0]).reshape(shape[0], dw, -1)  # the first pass alone (the second is the identity)
    assert np.all(np.abs(rows - np.einsum("ux,yxc->yuc", mx, a)) <= 0.5 + 1e-6)
    both = ref.resize(img, dw, dh).reshape(dh, dw, -1)  # the second pass reads the first one's bytes
    assert np.all(np.abs(both - np.einsum("vy,yuc->vuc", my, rows.astype(np.float64))) <= 0.5 + 1e-6)
    assert np.array_equal(ref.resize(img, shape[1], shape[0]), img)  # same size: every window is one sample


def test_identity_warp_blanks_the_top_row_and_the_last_column():
    """PINHOLE onto itself with fx = fy = 64 and a half-integer principal point, so that (x + 0.5 - cx) / fx * fx + cx is
    exact: s = (x + 0.5, y + 0.5), the bilinear corner is x0 = x with dx = 0 and, bottom-up, y0 = H - 1 - y with dy = 0.
    The rule blanks x1 = x + 1 >= W, the last column, and y1 = H - y >= H, the top row y = 0; every other pixel is
    (1 - 0) p[y0][x0] = the input."""
    for ch in (1, 3):
        img = cases.make_image(cases.H, cases.W, ch, 600 + ch)
        cam = ("PINHOLE", cases.W, cases.H, np.array([64.0, 64.0, 33.5, 22.5]))
        out = ref.warp(img, cam, (1, cases.W, cases.H, cam[3]))
        assert np.array_equal(out[1:, :-1], img[1:, :-1])
        assert np.all(out[0] == 0) and np.all(out[:, -1] == 0)


# ---- the edge list ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_reference():
    """{name: (image, source camera, target camera, reference image, values before rounding, source coordinates)},
    computed once and left unchanged."""
    out = {}
    for name, img, cam, dst in cases.edge_cases():
        warped, vals, coords = ref.warp(img, cam, dst, details=True)
        for a in (warped, vals, coords):
            a.setflags(write=False)
        out[name] = (img, cam, dst, warped, vals, coords)
    return out


def axis_window_lengths(n_in, n_out):
    """14.4's window of every output sample, zero weights included: min(int(c + width + 0.5), n) - max(0, int(c - width + 0.5))."""
    scale = n_out / n_in
    width = 1 / scale if scale < 1 else 1.0
    centers = [u / scale + 0.5 / scale for u in range(n_out)]
    return np.array([min(int(c + width + 0.5), n_in) - max(0, int(c - width + 0.5)) for c in centers])


# the longest window per (in, out) pair, counted by hand from 14.4: about 2 in / out samples for a reduction (1000 -> 3:
# centres 166.67, 500, 833.33 and width 333.33, the middle window is int(833.83) - int(167.17) = 833 - 167), three for
# an enlargement at most (width 1 around a centre: int(c + 1.5) - int(c - 0.5), here 2 as no centre of 7 -> 100 has a
# fraction of exactly one half); 64 -> 63 has width 64 / 63 and int(c + 1.516) - int(c - 0.516) = 2 for its centres
# u + 0.5 + (u + 0.5) / 63; 67 -> 22 would reach 7 only at u = 21, where the image's end clips it
LONGEST_WINDOW = {(1000, 3): 666, (300, 7): 86, (300, 2): 225, (257, 1): 257, (64, 1): 64, (64, 16): 8, (64, 32): 4,
                  (64, 63): 2, (67, 22): 6, (45, 15): 6, (7, 100): 2}


def test_edge_case_list_reaches_what_it_names(edge_reference):
    """From the shapes and the reference's details alone: the list holds the edges 14.6 names."""
    names = [c[0] for c in cases.edge_cases()]
    assert len(set(names)) == len(names) == len(edge_reference) and 100 <= len(names) <= 160
    shape = {n: (r[1][1], r[1][2], r[2][1], r[2][2]) for n, r in edge_reference.items()}  # sw, sh, dw, dh
    inside = {n: r[4][..., 0] >= 0 for n, r in edge_reference.items()}
    prepass = {n: s[2] * s[3] < s[0] * s[1] for n, s in shape.items()}
    for n, (sw, sh, dw, dh) in shape.items():
        assert max(sw * sh, dw * dh) <= 12000, n  # a few thousand pixels each
        img, warped = edge_reference[n][0], edge_reference[n][3]
        assert img.shape[:2] == (sh, sw) and warped.shape[:2] == (dh, dw) and warped.shape[2:] == img.shape[2:], n
        if "black" in n:  # a side of 1 in the image the warp reads: nothing can be inside
            assert not inside[n].any() and not warped.any() and prepass[n] and min(dw, dh) == 1, n
        else:
            assert inside[n].any(), n

    def tail_is_inside_with_data(n):
        dw, dh = shape[n][2:]
        k = (dw * dh) % 4 or 4  # the last group: the partial one, or a full one
        flat_inside = inside[n].reshape(-1)
        flat = edge_reference[n][3].reshape(dw * dh, -1)
        assert flat_inside[-k:].all() and flat[-k:].any(axis=1).all(), n

    # a. every tail length for both channel counts, without and with the pre-pass, data in the tail pixels
    for ch in (1, 3):
        for pre in ("", "-prepass"):
            tails = set()
            for dw, dh in cases.GROUP_TAILS:
                n = f"a-tail-{dw}x{dh}-{ch}ch{pre}"
                assert prepass[n] == bool(pre) and edge_reference[n][0].reshape(shape[n][1], shape[n][0], -1).shape[2] == ch
                tail_is_inside_with_data(n)
                tails.add((dw * dh) % 4)
            assert tails == {0, 1, 2, 3}
    assert min(s[2] * s[3] for s in shape.values()) == 1 and sorted({s[2] for n, s in shape.items() if n[0] == "b"}) == [1, 2, 3, 5]
    # b. one group of four pixels spans 4, 2, 2 and 1 to 2 rows
    assert [-(-4 // dw) for (dw, dh), _ in cases.NARROW] == [4, 2, 2, 1]
    for n in names:
        if n.startswith("b-narrow"):
            assert not prepass[n] and inside[n].all(), n
    # c. the warp's pixel counts: 63 | 64 | 65 and 255 | 256 | 257 groups, each also with a one-pixel tail
    c_counts = {}
    for n in names:
        if n.startswith("c-"):
            c_counts.setdefault(shape[n][2] * shape[n][3], []).append(n)
            ch = edge_reference[n][0].reshape(shape[n][1], shape[n][0], -1).shape[2]
            assert ch == (3 if shape[n][2] * shape[n][3] % 4 == 1 else 1), n
            if "black" not in n:
                assert not prepass[n]
                tail_is_inside_with_data(n)
    assert sorted(c_counts) == [252, 253, 256, 257, 260, 1020, 1021, 1024, 1025, 1028]
    assert sorted({-(-k // 4) for k in c_counts}) == [63, 64, 65, 255, 256, 257]
    assert all(any("black" not in n for n in v) for v in c_counts.values())  # every count also with pixels in it
    # d. the resize kernels' sample counts
    first = sorted(shape[n][2] * shape[n][1] for n in names if n.startswith("d-first"))
    second = sorted(shape[n][2] * shape[n][3] for n in names if n.startswith("d-second"))
    assert first == [255, 256, 257] and second == [255, 256, 257]
    assert all(prepass[n] for n in names if n.startswith("d-"))
    assert sum("black" not in n for n in names if n.startswith("d-")) == 5  # 257 = 1 x 257 only: that one is black
    # e. every window pair on x and on y, the longest window restated from 14.4 and within the device's table bound
    on_x = {(shape[n][0], shape[n][2]) for n in names if n.startswith("e-")}
    on_y = {(shape[n][1], shape[n][3]) for n in names if n.startswith("e-")}
    assert all(prepass[n] for n in names if n.startswith("e-"))
    assert set(cases.WINDOW_PAIRS) == set(LONGEST_WINDOW)
    for n_in, n_out in cases.WINDOW_PAIRS:
        assert (n_in, n_out) in on_x and (n_in, n_out) in on_y, (n_in, n_out)
        lengths = axis_window_lengths(n_in, n_out)
        m = np_axis_matrix(n_in, n_out)
        assert lengths.max() == LONGEST_WINDOW[(n_in, n_out)] and lengths.min() >= 1, (n_in, n_out, lengths.max())
        assert np.all((m > 0).sum(axis=1) <= lengths) and np.all((m > 0).sum(axis=1) >= 1)  # no empty window (14.4's fallback)
        assert lengths.max() <= 2 * (n_in // n_out + 1) + 3  # undistort.hip sizes a batch's weight table by this
    sw, sh, dw, dh = shape["e-window-7x300-to-100x2-1ch"]
    assert dw > sw and dw * dh < sw * sh  # an axis enlarged inside a resized image
    # f. the eleven models through a pre-pass that enlarges x and reduces y; 11 % .. 100 % inside
    f_names = [n for n in names if n.startswith("f-")]
    assert {n.split("-")[2] for n in f_names} == set(cases.CAMERAS)
    for n in f_names:
        assert shape[n] == (cases.W, cases.H, 100, 9) and prepass[n] and 0.11 <= inside[n].mean() <= 1.0, (n, inside[n].mean())
    # g. the half-pixel shifts decide many bytes by round half up
    a = edge_reference["g-halfx-1ch"][0].astype(int)
    assert ((a[1:, :-1] + a[1:, 1:]) % 2 == 1).mean() > 0.3
    a = edge_reference["g-halfy-3ch"][0].astype(int)
    assert ((a[:-1, :-1] + a[1:, :-1]) % 2 == 1).mean() > 0.3
    a = edge_reference["g-halfxy-1ch"][0].astype(int)
    quarters = (a[:-1, :-1] + a[:-1, 1:] + a[1:, :-1] + a[1:, 1:]) % 4
    assert (quarters == 2).mean() > 0.15 and ((quarters == 1) | (quarters == 3)).mean() > 0.3  # .5 up, .25 and .75 not
    for n in names:
        if n.startswith("g-"):  # every coordinate is a multiple of 1 / 8
            co = edge_reference[n][5]
            assert np.array_equal(co * 8, np.round(co * 8)), n
    # h. the split of the huge coordinates
    h_names = [n for n in names if n.startswith("h-")]
    assert len(h_names) == 11 * len(cases.HUGE_FOCALS) * len(cases.HUGE_TARGETS)
    for n in h_names:
        model, focal = n.split("-")[2], float("-".join(n.split("-")[3:5]))
        co = edge_reference[n][5]
        assert prepass[n] == (shape[n][2:] == (21, 15)) and inside[n][7, 10], n  # u = v = 0 on pixel (10, 7)
        if model in ("RADIAL", "OPENCV", "FULL_OPENCV"):
            assert np.isnan(co).any(), n
        if model in ("SIMPLE_PINHOLE", "PINHOLE") or (model == "SIMPLE_RADIAL" and focal == 1e-150):
            assert not np.isnan(co).any() and (np.isinf(co).any() or np.abs(co).max() > 1e100), n
        if model in cases.POLYNOMIAL:
            assert inside[n].sum() == 1, n
        elif model in ("FOV", "THIN_PRISM_FISHEYE") and focal == 1e-150:
            # r is finite here: atan(r) / r leaves a point about pi / 2 (FOV: pi / (2 omega)) from the axis, which is
            # finite, ordinary and far outside the 67 x 45 source; only the pixel on the principal point is inside
            assert np.isfinite(co).all() and inside[n].sum() == 1 and np.abs(co).max() < 1e3, n
        else:  # r overflows to infinity, or u * theta_d / r - u absorbs into -u: every pixel lands on the principal point
            assert np.isfinite(co).all() and inside[n].all(), n
    # i. u = v = 0 exactly on a pixel centre: the source coordinate is the (rescaled) principal point, bit for bit
    for model in ("OPENCV_FISHEYE", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE"):
        (n,) = [k for k in names if k.startswith(f"i-centre-{model}-")]
        _, _, cx, cy = cases.focal_and_principal_point(edge_reference[n][1])
        assert np.array_equal(edge_reference[n][5][7, 10], [cx * (21 / cases.W), cy * (15 / cases.H)]) and inside[n][7, 10], n
    for n in names:
        if n.startswith("i-fov-omega"):
            assert edge_reference[n][1][3][4] ** 2 < 1e-4
    dst = edge_reference["i-fov-small-radius-1ch"][2][3]
    y, x = np.mgrid[0:50, 0:70]
    r2 = ((x + 0.5 - dst[2]) / dst[0]) ** 2 + ((y + 0.5 - dst[3]) / dst[1]) ** 2
    assert 4 <= (r2 < 1e-4).sum() < r2.size / 4  # both of FOV's radius branches in one image
    # j. saturation: the inside bytes are exactly 255 and 0
    for value in (255, 0):
        for size in ("130x90", "30x20"):
            n = f"j-all-{value}-{size}-3ch"
            assert inside[n].all() and np.all(edge_reference[n][3] == value) and prepass[n] == (size == "30x20"), n
    board = edge_reference["j-checkerboard-64-to-63-1ch"][0]
    assert set(np.unique(board)) == {0, 255} and np.all(board[:, 1:] != board[:, :-1]) and np.all(board[1:] != board[:-1])
    # k. the layouts
    assert edge_reference["k-rows-subsampled-3ch"][0].strides[0] == 2 * cases.W * 3
    assert edge_reference["k-trailing-1-axis"][0].shape == (cases.H, cases.W, 1)
    assert edge_reference["k-fortran-order-3ch"][0].flags.f_contiguous and not edge_reference["k-fortran-order-3ch"][0].flags.c_contiguous
    assert edge_reference["k-negative-row-stride-1ch"][0].strides[0] < 0


def test_known_answers_on_the_reference(edge_reference):
    """The (g) cases against integer arithmetic (cases.known_answers): round half up at exact ties, the strict bounds,
    a negative focal length, and the pre-pass seen through an identity warp."""
    answers = cases.known_answers()
    assert sorted(answers) == sorted(n for n in edge_reference if n.startswith("g-")) and len(answers) == 8
    for name, (want, pinned) in answers.items():
        got = edge_reference[name][3]
        assert pinned.all(), name  # (the pre-pass seeds leave no byte to an FP tie)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        assert np.all(got[:, -1] == 0) and (np.all(got[-1] == 0) if "halfy" in name or "halfxy" in name else np.all(got[0] == 0))


def test_int_resize_is_the_numpy_restatement():
    """The integer statement of 14.4 for a reduction by 4 against the dense float64 matrix: the same windows, weights
    equal to within rounding."""
    for n_in, n_out in ((64, 16), (48, 12)):
        m = np_axis_matrix(n_in, n_out)
        for u, (left, w, d) in enumerate(cases.int_axis_weights(n_in, n_out)):
            row = np.zeros(n_in)
            row[left:left + len(w)] = np.array(w) / d
            assert np.allclose(m[u], row, rtol=0, atol=1e-15), (n_in, u)


def test_saturated_images_stay_saturated_through_the_resize():
    """Normalised weights may sum to just above 1: 255 times that sum must clamp to 255, not wrap."""
    above = 0
    for n_in, n_out in cases.WINDOW_PAIRS + [(67, 30), (45, 20)]:
        m = np_axis_matrix(n_in, n_out)
        above += int(np.any(np.array([sum(row[row > 0]) for row in m]) > 1.0))
    assert above > 0  # (sequential sums of the normalised weights, as the reference accumulates them)
    for shape, dw, dh in window_shapes() + [((45, 67, 3), 30, 20)]:
        for value in (255, 0):
            assert np.all(ref.resize(np.full(shape, value, np.uint8), dw, dh) == value), (shape, dw, dh)


def test_edge_reference_against_frozen_fixture(edge_reference):
    fx = np.load(EDGES_GOLDEN)
    assert sorted({k.split("/")[0] for k in fx.files}) == sorted(edge_reference)
    full = 0
    for name, (img, cam, dst, warped, vals, coords) in edge_reference.items():
        assert bytes(fx[f"{name}/input_digest"]).decode() == cases.digest(img), name
        assert bytes(fx[f"{name}/digest"]).decode() == cases.digest(warped), name
        assert int(fx[f"{name}/inside"]) == int((vals[..., 0] >= 0).sum()), name
        if f"{name}/image" in fx.files:
            assert np.array_equal(fx[f"{name}/image"], warped), name
            full += 1
    assert full == 6


# ---- undistort_camera at its edges (14.2) --------------------------------------------------------------------------------------
CAMERA_EDGES = [
    ("roi-1x1", {}, dict(roi_min_x=0.5, roi_max_x=0.505, roi_min_y=0.5, roi_max_y=0.51)),  # round(33.5) = round(33.8) = 34
    ("roi-min-near-1", {}, dict(roi_min_x=0.999, roi_min_y=0.999)),                        # round(66.9) = 67 -> W - 1
    ("one-scale-blank-0", {}, dict(blank_pixels=0.0, min_scale=0.7, max_scale=0.7)),
    ("one-scale-blank-half", {}, dict(blank_pixels=0.5, min_scale=0.7, max_scale=0.7)),
    ("one-scale-blank-1", {}, dict(blank_pixels=1.0, min_scale=0.7, max_scale=0.7)),
    ("max_image_size-1", {}, dict(max_image_size=1)),
    ("max_image_size-1-flat", dict(height=20), dict(max_image_size=1)),
]


@pytest.mark.parametrize("model", list(cases.CAMERAS))
@pytest.mark.parametrize("label, size, opts", CAMERA_EDGES, ids=[c[0] for c in CAMERA_EDGES])
def test_undistort_camera_edges_equal_the_reference(model, label, size, opts):
    cam = cases.camera(model, height=size.get("height", cases.H))
    und = _capi.undistort_camera(cam, **opts)
    assert same_camera(und, ref.undistort_camera(cam, **opts)), (und, ref.undistort_camera(cam, **opts))
    if label == "roi-1x1":       # a one-pixel window times a scale of at most max_scale = 2
        assert 1 <= und[1] <= 2 and 1 <= und[2] <= 2
    elif label == "roi-min-near-1":
        # x0 = W - 1, y0 = H - 1: a one-pixel window again, the principal point moved by (W - 1, H - 1)
        assert 1 <= und[1] <= 2 and 1 <= und[2] <= 2 and und[3][2] < 0 and und[3][3] < 0
    elif label.startswith("one-scale") and model not in ("PINHOLE", "SIMPLE_PINHOLE"):
        assert (und[1], und[2]) == (int(0.7 * cases.W), int(0.7 * cases.H))  # whatever blank_pixels weighs
    elif label == "max_image_size-1":      # s = 1 / W'': round(s W'') = 1 and round(s H'') = round(H'' / W'') = 1
        assert (und[1], und[2]) == (1, 1) and und[3][1] > 0
    elif label == "max_image_size-1-flat":
        # 14.2 step 5: round(s H'') = 0 for H'' < W'' / 2; the size is clamped to 1, the factor 0 / H'' is not
        assert (und[1], und[2]) == (1, 1) and und[3][1] == 0.0 and und[3][3] == 0.0 and und[3][0] > 0


def test_undistort_camera_with_a_nan_scale():
    """SIMPLE_RADIAL without distortion and cx = 0.5: the left border lifts to x = cx, so cx / (cx - left) = inf on both
    the min and the max side; max_scale_x = inf.  blank_pixels = 1 weighs it with 0: inf * 0 = NaN.  14.2 step 4: a NaN
    passes min(max(scale, min_scale), max_scale) unchanged (every comparison with it is false) and max(1.0, NaN * W) is
    1.0: the axis gets one sample.  blank_pixels < 1 gives 1 / inf = 0, clamped to min_scale."""
    cam = ("SIMPLE_RADIAL", cases.W, cases.H, [58.0, 0.5, 22.5, 0.0])
    for blank, width in ((1.0, 1), (0.5, int(0.2 * cases.W)), (0.0, int(0.2 * cases.W))):
        und = _capi.undistort_camera(cam, blank_pixels=blank)
        assert same_camera(und, ref.undistort_camera(cam, blank_pixels=blank)) and und[1] == width, (blank, und)
        assert und[3][2] == 0.5 * width / cases.W
    cam = ("SIMPLE_RADIAL", cases.W, cases.H, [58.0, 33.5, 0.5, 0.0])  # the same on y
    und = _capi.undistort_camera(cam, blank_pixels=1.0, min_scale=0.5)
    assert same_camera(und, ref.undistort_camera(cam, blank_pixels=1.0, min_scale=0.5)) and und[2] == 1


def test_own_atan_within_one_ulp_of_numpy():
    xs = np.concatenate([np.linspace(-8, 8, 4001), np.logspace(-12, 6, 500)])
    got = np.array([ref.load().undistort_ref_atan(float(x)) for x in xs])
    assert np.all(np.abs(got - np.arctan(xs)) <= np.spacing(np.abs(np.arctan(xs))))


# ---- model I/O ---------------------------------------------------------------------------------------------------------------
def plan_cameras(plan):
    return {p["name"]: (p["image_id"], cam_tuple(p["camera"])) for p in plan}


def test_bin_and_txt_models_read_back_to_the_same_values(tmp_path):
    cameras, images, points3D = cases.tiny_model()
    cases.write_model_bin(tmp_path / "bin", cameras, images, points3D)
    cases.write_model_txt(tmp_path / "txt", cameras, images, points3D)
    pb, pt = pycolmap_amd._undistort_plan(tmp_path / "bin"), pycolmap_amd._undistort_plan(tmp_path / "txt")
    assert [p["name"] for p in pb] == [im[3] for im in images.values()] == [p["name"] for p in pt]
    for p, q, (iid, im) in zip(pb, pt, images.items()):
        mid, w, h, params = cameras[im[2]]
        for got in (p, q):
            assert got["image_id"] == iid and got["camera"].camera_id == im[2]
            assert same_camera(cam_tuple(got["camera"]), (mid, w, h, np.array(params)))
    # the whole model, points2D and points3D included: both spellings give the same undistorted .bin files
    from pycolmap_amd import _pycolmap
    for d in ("out_bin", "out_txt"):
        (tmp_path / d).mkdir()
    o = pycolmap_amd.UndistortCameraOptions()
    assert _pycolmap._write_undistorted_model(tmp_path / "bin", tmp_path / "out_bin", o) == (2, 3, 12)
    _pycolmap._write_undistorted_model(tmp_path / "txt", tmp_path / "out_txt", o)
    for f in ("cameras.bin", "images.bin", "points3D.bin"):
        assert (tmp_path / "out_bin" / f).read_bytes() == (tmp_path / "out_txt" / f).read_bytes(), f
    # .bin wins when both spellings lie in one folder
    cases.write_model_txt(tmp_path / "bin", *cases.pinhole_model())
    assert same_camera(cam_tuple(pycolmap_amd._undistort_plan(tmp_path / "bin")[0]["camera"]), cam_tuple(pb[0]["camera"]))


def test_written_model_is_the_undistorted_one(tmp_path):
    cameras, images, points3D = cases.tiny_model()
    cases.write_model_bin(tmp_path / "in", cameras, images, points3D)
    (tmp_path / "out").mkdir()
    from pycolmap_amd import _pycolmap
    opts = dict(blank_pixels=0.3)
    _pycolmap._write_undistorted_model(tmp_path / "in", tmp_path / "out", pycolmap_amd.UndistortCameraOptions(opts))
    ucams, uimages, upoints = cases.parse_model_bin(tmp_path / "out")
    assert upoints == points3D and list(ucams) == list(cameras) and list(uimages) == list(images)
    und = {}
    for cid, (mid, w, h, params) in cameras.items():
        und[cid] = ref.undistort_camera((mid, w, h, params), **opts)
        assert same_camera((ucams[cid][0], ucams[cid][1], ucams[cid][2], np.array(ucams[cid][3])), und[cid])
    for iid, (q, t, cid, name, pts) in images.items():
        uq, ut, ucid, uname, upts = uimages[iid]
        assert (uq, ut, ucid, uname) == (q, t, cid, name) and [p[2] for p in upts] == [p[2] for p in pts]
        mid, w, h, params = cameras[cid]
        want = ref.undistort_points((mid, w, h, params), und[cid], [[p[0], p[1]] for p in pts])
        assert np.array_equal(bits([[p[0], p[1]] for p in upts]), bits(want)), name
        assert np.array_equal(bits(_capi.undistort_points((mid, w, h, params), und[cid], [[p[0], p[1]] for p in pts])), bits(want))


def test_pinhole_model_is_rewritten_byte_for_byte(tmp_path):
    cases.write_model_bin(tmp_path / "in", *cases.pinhole_model())
    (tmp_path / "out").mkdir()
    from pycolmap_amd import _pycolmap
    _pycolmap._write_undistorted_model(tmp_path / "in", tmp_path / "out", pycolmap_amd.UndistortCameraOptions())
    for f in ("cameras.bin", "images.bin", "points3D.bin"):
        assert (tmp_path / "out" / f).read_bytes() == (tmp_path / "in" / f).read_bytes(), f
    assert cases.parse_model_bin(tmp_path / "out") == cases.pinhole_model()


def test_damaged_model_files_are_refused(tmp_path):
    cases.write_model_bin(tmp_path / "m", *cases.tiny_model())
    d = (tmp_path / "m" / "images.bin").read_bytes()
    (tmp_path / "m" / "images.bin").write_bytes(d[:-5])
    with pytest.raises(ValueError, match="images.bin: (is truncated|holds a count larger than the file)"):
        pycolmap_amd._undistort_plan(tmp_path / "m")
    (tmp_path / "m" / "images.bin").write_bytes(b"\xff" * 8 + d[8:])
    with pytest.raises(ValueError, match="count larger than the file"):
        pycolmap_amd._undistort_plan(tmp_path / "m")


# ---- the plan ------------------------------------------------------------------------------------------------------------------
def test_plan_filters_warns_and_decides_copies(tmp_path, capfd):
    cameras, images, points3D = cases.tiny_model()
    cameras[9] = (1, 40, 30, [35.0, 36.0, 20.0, 15.0])                    # PINHOLE: copied
    cameras[10] = (cases.MODEL_IDS["RADIAL"], 40, 30, [35.0, 20.0, 15.0, 0.0, 0.0])  # no distortion, but 39 x 29: warped
    images[7] = (images[1][0], images[1][1], 9, "p.pgm", [])
    images[8] = (images[1][0], images[1][1], 10, "z.pgm", [])
    cases.write_model_bin(tmp_path / "m", cameras, images, points3D)
    plan = pycolmap_amd._undistort_plan(tmp_path / "m")
    assert [p["name"] for p in plan] == ["a.ppm", "sub/b.pgm", "c.ppm", "p.pgm", "z.pgm"]
    assert [p["copy"] for p in plan] == [False, False, False, True, False]
    z = plan[4]["undistorted_camera"]
    assert (z.width, z.height) == (39, 29)
    full = pycolmap_amd._undistort_plan(tmp_path / "m", [], dict(blank_pixels=1.0))
    assert full[4]["copy"] and (full[4]["undistorted_camera"].width, full[4]["undistorted_camera"].height) == (40, 30)
    opts = dict(blank_pixels=0.5, max_image_size=50)
    for p in pycolmap_amd._undistort_plan(tmp_path / "m", [], opts):
        assert same_camera(cam_tuple(p["undistorted_camera"]), _capi.undistort_camera(cam_tuple(p["camera"]), **opts)), p["name"]
        assert same_camera(cam_tuple(p["undistorted_camera"]), ref.undistort_camera(cam_tuple(p["camera"]), **opts)), p["name"]
    # max_image_size 50 shrinks the 67 x 45 cameras only: the 40 x 30 PINHOLE image is still a copy
    assert [p["copy"] for p in pycolmap_amd._undistort_plan(tmp_path / "m", [], opts)] == [False, False, False, True, False]
    capfd.readouterr()
    some = pycolmap_amd._undistort_plan(tmp_path / "m", ["c.ppm", "missing.png", "sub/b.pgm"])
    assert [p["name"] for p in some] == ["c.ppm", "sub/b.pgm"]
    err = capfd.readouterr().err
    assert "Cannot find image missing.png" in err and err.lstrip().startswith("W")
    with pytest.raises(ValueError, match="Check Failed: blank_pixels <= 1"):
        pycolmap_amd._undistort_plan(tmp_path / "m", [], dict(blank_pixels=2.0))


@pytest.mark.skipif(not RECORDED.exists(), reason="no recording of real pycolmap (tests/golden/"
                    "make_undistort_reference_golden.py)")
def test_reference_against_pycolmap_recording():
    """Reports how far COLMAP's own undistort_images is from the reference on the tiny model: the deviations of DESIGN.md
    14.9 that are marked "to confirm" are settled by this comparison.  Cameras and points2D must agree to 1e-9."""
    rec = np.load(RECORDED)
    cameras, images, _ = cases.tiny_model()
    for cid, (mid, w, h, params) in cameras.items():
        und = ref.undistort_camera((mid, w, h, params))
        got = rec[f"camera/{cid}"]
        assert (int(got[0]), int(got[1]), int(got[2])) == und[:3], cid
        assert np.allclose(got[3:], und[3], rtol=0, atol=1e-9), cid
    for iid, (_, _, cid, name, pts) in images.items():
        mid, w, h, params = cameras[cid]
        und = ref.undistort_camera((mid, w, h, params))
        want = ref.undistort_points((mid, w, h, params), und, [[p[0], p[1]] for p in pts])
        assert np.allclose(rec[f"points2D/{iid}"], want, rtol=0, atol=1e-9), name
        mine = ref.warp(cases.make_image(h, w, 3, 400 + iid), (mid, w, h, params), und)
        diff = np.abs(mine.astype(int) - rec[f"image/{iid}"].astype(int))
        print(f"{name}: {int((diff > 0).sum())} of {diff.size} bytes differ from COLMAP's, largest difference {int(diff.max())}")


def test_workspace_of_copied_images_needs_no_device(tmp_path):
    """An image_list of already-undistorted images is copied or linked, never warped: the whole workspace is host work."""
    import os
    cameras, images, points3D = cases.tiny_model()
    cameras[9] = (1, 40, 30, [35.0, 36.0, 20.0, 15.0])
    images[7] = (images[1][0], images[1][1], 9, "deep/p.pgm", [(3.0, 4.0, -1)])
    cases.write_model_bin(tmp_path / "model", cameras, images, points3D)
    img = cases.make_image(30, 40, 1, 700)
    cases.write_pnm(tmp_path / "images" / "deep/p.pgm", img)
    out = tmp_path / "dense"
    pycolmap_amd.undistort_images(out, tmp_path / "model", tmp_path / "images", ["deep/p.pgm"], copy_policy="soft-link",
                                  num_patch_match_src_images=5)
    assert os.path.islink(out / "images" / "deep/p.pgm") and np.array_equal(cases.read_pnm(out / "images" / "deep/p.pgm"), img)
    assert (out / "stereo" / "patch-match.cfg").read_text() == "deep/p.pgm\n__auto__, 5\n"
    assert (out / "stereo" / "fusion.cfg").read_text() == "deep/p.pgm\n"
    for sub in ("depth_maps", "normal_maps", "consistency_graphs"):
        assert (out / "stereo" / sub / "deep").is_dir()
    ucams, uimages, upoints = cases.parse_model_bin(out / "sparse")  # the whole model, undistorted
    assert list(uimages) == list(images) and upoints == points3D and all(c[0] == 1 for c in ucams.values())
    st = pycolmap_amd.last_run_stats()
    assert st["images"] == 1 and st["copied"] == 1 and st["warped"] == 0 and st["pixels"] == 0
    for k in ("decode_ms", "device_ms", "kernel_ms", "encode_ms", "total_ms"):
        assert k in st
