"""Freeze the bundle adjustment reference (tests/ba_ref) on tests/ba_cases.py's cases into tests/golden/ba_ref_v1.npz:
per case the sha256 digest of the refined arrays and statistics, and the statistics themselves as float64 (costs bit
for bit).  Run from the repository root: python tests/golden/make_ba_ref_golden.py
With --edges it writes tests/golden/ba_ref_edges_v1.npz for ba_cases.EDGE_CASES instead (digest and statistics per
case) and leaves ba_ref_v1.npz alone."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import ba_cases  # noqa: E402
import ba_ref_lib  # noqa: E402


def edges():
    out = {"names": np.array(sorted(ba_cases.EDGE_CASES))}
    for name in sorted(ba_cases.EDGE_CASES):
        args, options = ba_cases.edge_problem(name)
        r = ba_ref_lib.bundle_adjust(*args, options=options)
        out[f"{name}/digest"] = np.array(ba_cases.digest(r))
        out[f"{name}/stats"] = np.array([ba_ref_lib.TERMINATIONS.index(r[k]) if k == "termination" else r[k]
                                         for k in ba_cases.RESULT_STATS], np.float64)
    np.savez_compressed(ROOT / "tests" / "golden" / "ba_ref_edges_v1.npz", **out)


def main():
    out = {"names": np.array(sorted(ba_cases.CASES))}
    for name in sorted(ba_cases.CASES):
        args, options = ba_cases.case_problem(name)
        r = ba_ref_lib.bundle_adjust(*args, options=options)
        out[f"{name}/digest"] = np.array(ba_cases.digest(r))
        out[f"{name}/stats"] = np.array([ba_ref_lib.TERMINATIONS.index(r[k]) if k == "termination" else r[k]
                                         for k in ba_cases.RESULT_STATS], np.float64)
        out[f"{name}/qvec"] = r["qvec"]
        out[f"{name}/tvec"] = r["tvec"]
    np.savez_compressed(ROOT / "tests" / "golden" / "ba_ref_v1.npz", **out)


if __name__ == "__main__":
    edges() if "--edges" in sys.argv[1:] else main()
