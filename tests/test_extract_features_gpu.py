"""extract_features on the GPU: database contents (cameras, names, N x 6 keypoints whose first columns are the
extractor's, descriptors), image_list, camera modes, downscaling; and the end-to-end path from rendered pixels through
extract_features and match_exhaustive to the homography of the views."""
import numpy as np
import pytest

import sift_images as si

pytestmark = pytest.mark.gpu


def write_pgm(path, img):
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_bytes(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())


def by_name(db):
    return {im.name: im for im in db.read_all_images()}


def test_database_contents_equal_the_extractor(tmp_path, amc_ctx):
    import pycolmap_amd as pycolmap
    imgs = {"a/1.pgm": si.textured(60, 120, 160), "a/2.pgm": si.textured(61, 120, 160),
            "b/3.pgm": si.textured(62, 100, 90)}
    for n, im in imgs.items():
        write_pgm(tmp_path / "img" / n, im)
    pycolmap.extract_features(tmp_path / "f.db", tmp_path / "img")
    st = pycolmap.last_run_stats()
    assert st["images"] == 3 and st["features"] > 0 and st["device_ms"] > 0 and "sqlite_ms" in st
    db = pycolmap.Database(tmp_path / "f.db")
    ims = by_name(db)
    assert sorted(ims) == sorted(imgs)
    cams = {c.camera_id: c for c in db.read_all_cameras()}
    assert len(cams) == 2  # AUTO: a new camera when the size changes
    nfeat = 0
    for n, im in imgs.items():
        rec = ims[n]
        cam = cams[rec.camera_id]
        assert (cam.width, cam.height) == (im.shape[1], im.shape[0])
        assert cam.model.name == "SIMPLE_RADIAL" and not cam.has_prior_focal_length
        assert np.allclose(cam.params, [1.2 * max(im.shape), im.shape[1] / 2, im.shape[0] / 2, 0.0])
        (kp, desc), _ = amc_ctx.sift_extract(im)
        kp6 = db.read_keypoints(rec.image_id)
        assert kp6.shape == (len(kp), 6)
        assert np.array_equal(kp6[:, :2].view(np.uint32), kp[:, :2].view(np.uint32))
        assert np.allclose(kp6[:, 2:], np.stack([kp[:, 2] * np.cos(kp[:, 3]), -kp[:, 2] * np.sin(kp[:, 3]),
                                                 kp[:, 2] * np.sin(kp[:, 3]), kp[:, 2] * np.cos(kp[:, 3])], 1),
                           atol=1e-5)
        assert np.array_equal(db.read_descriptors(rec.image_id), desc)
        # Sift.extract's float descriptors are these bytes / 512
        nfeat += len(kp)
    assert st["features"] == nfeat
    db.close()


@pytest.mark.parametrize("mode,ncams", [("SINGLE", 1), ("PER_FOLDER", 2), ("PER_IMAGE", 3), ("AUTO", 1)])
def test_camera_modes(tmp_path, mode, ncams):
    import pycolmap_amd as pycolmap
    for k, n in enumerate(("a/1.pgm", "a/2.pgm", "b/3.pgm")):
        write_pgm(tmp_path / "img" / n, si.textured(70 + k, 64, 80))
    pycolmap.extract_features(tmp_path / "f.db", tmp_path / "img", camera_mode=mode,
                              reader_options={"camera_params": "100,40,32,0.01"})
    db = pycolmap.Database(tmp_path / "f.db")
    cams = db.read_all_cameras()
    assert len(cams) == ncams and all(np.allclose(c.params, [100, 40, 32, 0.01]) for c in cams)
    db.close()


def test_image_list_subset(tmp_path):
    import pycolmap_amd as pycolmap
    for k in range(4):
        write_pgm(tmp_path / "img" / f"{k}.pgm", si.textured(80 + k, 70, 90))
    pycolmap.extract_features(tmp_path / "f.db", tmp_path / "img", image_list=["3.pgm", "1.pgm"])
    db = pycolmap.Database(tmp_path / "f.db")
    assert [im.name for im in db.read_all_images()] == ["3.pgm", "1.pgm"]
    db.close()


def test_downscaled_image_keypoints_in_original_pixels(tmp_path, amc_ctx):
    import pycolmap_amd as pycolmap
    from pycolmap_amd import _extraction as ex
    img = si.textured(90, 200, 300)
    write_pgm(tmp_path / "img" / "big.pgm", img)
    pycolmap.extract_features(tmp_path / "f.db", tmp_path / "img", sift_options={"max_image_size": 160})
    small = ex.downscale(img, 160)
    assert small.shape == (106, 160)
    (kp, desc), _ = amc_ctx.sift_extract(small)
    db = pycolmap.Database(tmp_path / "f.db")
    cam = db.read_all_cameras()[0]
    assert (cam.width, cam.height) == (300, 200)
    kp6 = db.read_keypoints(1)
    assert np.allclose(kp6[:, 0], kp[:, 0] * (300 / 160)) and np.allclose(kp6[:, 1], kp[:, 1] * (200 / 106))
    assert np.array_equal(db.read_descriptors(1), desc)
    db.close()


def _colmap_coords(H):
    T = np.array([[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1.0]])
    return T @ H @ np.linalg.inv(T)


def _apply(H, pts):
    p = np.c_[pts, np.ones(len(pts))] @ H.T
    return p[:, :2] / p[:, 2:]


def test_end_to_end_rendered_plane_to_homography(tmp_path):
    import pycolmap_amd as pycolmap
    tex = si.plane_texture(7, 900)
    w, h = 640, 480
    crop = np.array([[1, 0, -130.0], [0, 1, -210.0], [0, 0, 1]])  # texture -> base view
    views = {"0_base.pgm": crop,
             "1_mild.pgm": crop @ si.similarity(4.0, 1.05, 6.0, -4.0, 450, 450),
             "2_rot30.pgm": crop @ si.similarity(30.0, 0.8, 0.0, 0.0, 450, 450)}
    for n, H in views.items():
        write_pgm(tmp_path / "img" / n, si.render(tex, H, h, w))
    pycolmap.extract_features(tmp_path / "f.db", tmp_path / "img")
    pycolmap.match_exhaustive(tmp_path / "f.db")
    db = pycolmap.Database(tmp_path / "f.db")
    ids = {im.name: im.image_id for im in db.read_all_images()}
    corners = np.array([[0, 0], [w, 0], [w, h], [0, h]], float)
    for n in ("1_mild.pgm", "2_rot30.pgm"):
        g = db.read_two_view_geometry(ids["0_base.pgm"], ids[n])
        assert g.config.name in ("PLANAR", "PANORAMIC", "PLANAR_OR_PANORAMIC"), (n, g.config.name)
        assert len(g.inlier_matches) >= 100, (n, len(g.inlier_matches))
        H_true = _colmap_coords(views[n] @ np.linalg.inv(crop))  # base view -> this view, COLMAP pixel coordinates
        err = np.linalg.norm(_apply(np.asarray(g.H), corners) - _apply(H_true, corners), axis=1)
        assert err.max() < 1.0, (n, err)
    db.close()
