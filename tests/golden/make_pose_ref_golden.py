"""Writes tests/golden/pose_ref_v1.npz: what the project's oracle (oracle/tvg_oracle.cc) returns for every case of
tests/pose_cases.py, so that a later change of the oracle or of a case shows up as a diff.  The inputs are seeded and
rebuilt by pose_cases, so none are stored.

    python tests/golden/make_pose_ref_golden.py

A few arrays for all the cases, since an archive member per case would cost more than what it holds: names (C,), ok,
config, num_points3D, R (C, 3, 3), t, q, tri_angle for cases(); h_names, h_R, h_t, h_n, h_rows and the concatenated
h_points3D for homography_cases().
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import pose_cases  # noqa: E402

OUT = ROOT / "tests" / "golden" / "pose_ref_v1.npz"
CONFIG_NAMES = ["UNDEFINED", "DEGENERATE", "CALIBRATED", "UNCALIBRATED", "PLANAR", "PANORAMIC", "PLANAR_OR_PANORAMIC",
                "WATERMARK", "MULTIPLE"]


def main():
    cs, want = pose_cases.build_cases()
    hs, hwant = pose_cases.build_homography_cases()
    names, hnames = list(cs), list(hs)
    np.savez_compressed(
        OUT, names=np.array(names), ok=np.array([want[n]["pose_ok"] for n in names]),
        config=np.array([want[n]["config"] for n in names], np.int32),
        num_points3D=np.array([want[n]["num_points3D"] for n in names], np.int32),
        R=np.stack([want[n]["R"] for n in names]), t=np.stack([want[n]["tvec"] for n in names]),
        q=np.stack([want[n]["qvec"] for n in names]), tri_angle=np.array([want[n]["tri_angle"] for n in names]),
        h_names=np.array(hnames), h_R=np.stack([hwant[n]["R"] for n in hnames]), h_t=np.stack([hwant[n]["t"] for n in hnames]),
        h_n=np.stack([hwant[n]["n"] for n in hnames]), h_rows=np.array([len(hwant[n]["points3D"]) for n in hnames], np.int32),
        h_points3D=np.concatenate([hwant[n]["points3D"] for n in hnames]))
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


def load():
    """(name -> the oracle's pose dict, name -> the oracle's homography dict) of the fixture"""
    g = np.load(OUT)
    poses = {str(n): dict(pose_ok=bool(g["ok"][i]), config=int(g["config"][i]), config_name=CONFIG_NAMES[int(g["config"][i])],
                          num_points3D=int(g["num_points3D"][i]), R=g["R"][i], tvec=g["t"][i], qvec=g["q"][i],
                          tri_angle=float(g["tri_angle"][i]))
             for i, n in enumerate(g["names"])}
    ends = np.cumsum(g["h_rows"])
    homs = {str(n): dict(R=g["h_R"][i], t=g["h_t"][i], n=g["h_n"][i], points3D=g["h_points3D"][ends[i] - g["h_rows"][i]:ends[i]])
            for i, n in enumerate(g["h_names"])}
    return poses, homs


if __name__ == "__main__":
    main()
