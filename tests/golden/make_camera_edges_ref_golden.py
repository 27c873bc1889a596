"""Freeze the CPU references on the camera-model edge cases (tests/camera_edge_cases.py) into
tests/golden/camera_edges_ref_v1.npz: per case the digests of the filter reference (both modes) and, for the cases that
run iterations, of the bundle adjustment and pose refinement references; the squared errors of the regimes whose radii
are exact doubles; strong_poly's lifts and projections by the oracle and the digest of its pose estimation.  Made from
the references alone, never from a GPU run.  The GPU tests compare the library with the live references and with this
file; tests/test_camera_edges_cpu.py checks that the references still reproduce it.

    python tests/golden/make_camera_edges_ref_golden.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import camera_edge_cases as ce  # noqa: E402

OUT = Path(__file__).resolve().parent / "camera_edges_ref_v1.npz"


def digests():
    """key -> digest, every digest the fixture holds"""
    d = {}
    for name in ce.CASES:
        for mode, errors_only in (("filter", False), ("errors", True)):
            d[f"{name}/{mode}"] = ce.filter_digest(ce.filter_reference(name, errors_only))
    for name in ce.ITERATION_CASES:
        for opt in ce.ba_options_of(name):
            d[f"{name}/ba/{opt}"] = ce.ba_digest(ce.ba_reference(name, opt))
        for tag, off_axis in (("exact", False), ("off_axis", True)):
            d[f"{name}/abspose/{tag}"] = ce.abspose_digest(ce.abspose_reference(name, off_axis))
    for m in ce.POLYNOMIAL:
        lift, proj = ce.lift_reference(m)
        d[f"strong_poly/{ce.MODEL_NAMES[m]}/cam_from_img"] = ce.lift_digest(lift)
        d[f"strong_poly/{ce.MODEL_NAMES[m]}/img_from_cam"] = ce.lift_digest(proj)
        d[f"strong_poly/{ce.MODEL_NAMES[m]}/estimate"] = ce.abspose_digest(ce.estimate_reference(m))
    return d


def arrays():
    a = {}
    for name in ce.CASES:
        if ce.regime(name) in ce.EXACT_REGIMES:
            a[f"{name}/obs_sq_error"] = np.asarray(ce.filter_reference(name, True)["obs_sq_error"])
    for m in ce.POLYNOMIAL:
        lift, proj = ce.lift_reference(m)
        a[f"strong_poly/{ce.MODEL_NAMES[m]}/cam_from_img"] = np.asarray(lift)
        a[f"strong_poly/{ce.MODEL_NAMES[m]}/img_from_cam"] = np.asarray(proj)
    return a


def main():
    d = digests()
    data = {"digest_keys": np.array(sorted(d)), "digest_values": np.array([d[k] for k in sorted(d)])}
    data.update(arrays())
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(d)} digests)")


if __name__ == "__main__":
    main()
