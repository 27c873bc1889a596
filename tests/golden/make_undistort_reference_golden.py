"""Record COLMAP's own undistort_images for a later comparison with this project's (tests/test_undistort_cpu.py::
test_reference_against_pycolmap_recording).  Needs the real pycolmap 0.6.x (COLMAP 3.9.1) with Pillow or FreeImage's
PNG support; writes tests/golden/undistort_pycolmap_v1.npz: the tiny model of tests/undistort_cases.py and its three
seeded images go through pycolmap.undistort_images with default options, and the undistorted cameras, points2D and
pixels are stored.  Run from the repository root on a machine that has that package:
python tests/golden/make_undistort_reference_golden.py"""
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))


def main():
    import pycolmap  # the reference package, not this repository's alias
    if "pycolmap_amd" in (getattr(pycolmap, "__doc__", "") or "") or not hasattr(pycolmap, "undistort_images"):
        raise SystemExit("this needs the real pycolmap 0.6.x, not pycolmap_amd's alias")
    from PIL import Image

    import undistort_cases as cases
    cameras, images, points3D = cases.tiny_model()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        # PNG names: FreeImage reads them everywhere; the pixels are those of the PPM / PGM files the tests use
        images = {iid: (q, t, cid, Path(name).with_suffix(".png").as_posix(), pts) for iid, (q, t, cid, name, pts) in images.items()}
        cases.write_model_bin(tmp / "sparse", cameras, images, points3D)
        for iid, (_, _, cid, name, _) in images.items():
            _, w, h, _ = cameras[cid]
            (tmp / "images" / name).parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray(cases.make_image(h, w, 3, 400 + iid)).save(tmp / "images" / name)
        pycolmap.undistort_images(tmp / "dense", tmp / "sparse", tmp / "images")
        ucams, uimages, _ = cases.parse_model_bin(tmp / "dense" / "sparse")
        for cid, (mid, w, h, params) in ucams.items():
            out[f"camera/{cid}"] = np.array([mid, w, h] + list(params), np.float64)
        for iid, (_, _, _, name, pts) in uimages.items():
            out[f"points2D/{iid}"] = np.array([[x, y] for x, y, _ in pts], np.float64)
            out[f"image/{iid}"] = np.asarray(Image.open(tmp / "dense" / "images" / name))
            print(name, out[f"image/{iid}"].shape)
    np.savez_compressed(ROOT / "tests" / "golden" / "undistort_pycolmap_v1.npz", **out)


if __name__ == "__main__":
    main()
