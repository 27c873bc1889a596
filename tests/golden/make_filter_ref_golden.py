"""Freeze the point filter's CPU reference (tests/filter_ref/filter_ref.cc, written from DESIGN.md section 16) into
tests/golden/filter_ref_v1.npz: for every case of tests/filter_cases.py the digests of the filter call and of the
errors-only call, and for CASES the result arrays themselves.  The GPU tests compare the library with the live reference
and with this file; tests/test_filter_cpu.py checks that the reference still reproduces it.

    python tests/golden/make_filter_ref_golden.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import filter_cases as fc  # noqa: E402

OUT = Path(__file__).resolve().parent / "filter_ref_v1.npz"


def main():
    data = {"cases": np.array(sorted(fc.CASES)), "edge_cases": np.array(sorted(fc.EDGE_CASES))}
    for name in sorted(fc.ALL_CASES):
        for mode, errors_only in (("filter", False), ("errors", True)):
            res = fc.reference(name, errors_only)
            data[f"{name}/{mode}/digest"] = np.array(fc.digest(res))
            if name in fc.CASES:
                for k in fc.RESULT_KEYS:
                    data[f"{name}/{mode}/{k}"] = np.asarray(res[k])
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(fc.ALL_CASES)} cases)")


if __name__ == "__main__":
    main()
