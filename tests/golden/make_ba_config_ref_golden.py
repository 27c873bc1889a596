"""Freeze the reference of bundle adjustment with constant points (tests/ba_config_ref) into
tests/golden/ba_config_ref_v1.npz: per case of tests/ba_config_cases.py the sha256 digest of the refined arrays and
statistics and the statistics themselves as float64 (costs bit for bit), and per Reconstruction scene the digest of the
reference's result on the flat problem BundleAdjuster sets up.  Run from the repository root after the build:
python tests/golden/make_ba_config_ref_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import ba_cases  # noqa: E402
import ba_config_cases as cc  # noqa: E402
import ba_config_ref_lib as ref  # noqa: E402


def stats(r):
    return np.array([ref.TERMINATIONS.index(r[k]) if k == "termination" else r[k] for k in ba_cases.RESULT_STATS], np.float64)


def main():
    import pycolmap_amd as pc
    out = {"names": np.array(sorted(cc.CASES)), "scenes": np.array(sorted(cc.SCENES))}
    for name in sorted(cc.CASES):
        args, pm, options = cc.case_problem(name)
        r = ref.bundle_adjust(*args, options=options, point_const=pm)
        out[f"{name}/digest"] = np.array(ba_cases.digest(r))
        out[f"{name}/stats"] = stats(r)
    for name in sorted(cc.SCENES):
        rec, adj = cc.adjuster(pc, name)
        d = adj._problem(rec)
        r = ref.bundle_adjust(*cc.flat_args(d), options=cc.SCENES[name][2], point_const=np.asarray(d["point_const"]).reshape(-1))
        out[f"scene/{name}/digest"] = np.array(ba_cases.digest(r))
        out[f"scene/{name}/stats"] = stats(r)
        out[f"scene/{name}/point_const"] = np.asarray(d["point_const"]).reshape(-1)
    np.savez_compressed(ROOT / "tests" / "golden" / "ba_config_ref_v1.npz", **out)


if __name__ == "__main__":
    main()
