"""Writes tests/golden/absrefine_ref_v1.npz: for every case of absrefine_cases.CASES the sha256 digest of what the joint
pose and camera refinement's CPU reference (tests/absrefine_ref) returns and, for a refinement, the reference's trace,
so that a later change of the reference shows up as a diff.  The inputs are seeded, so none are stored.

    python tests/golden/make_absrefine_ref_golden.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import absrefine_cases as cases  # noqa: E402

OUT = ROOT / "tests" / "golden" / "absrefine_ref_v1.npz"


def compute():
    import absrefine_ref_lib as ref
    names, digests, traces = [], [], []
    for name in cases.CASES:
        if cases.CASES[name][0] == "refine":
            r, tr = cases.run(name, None, ref.refine, trace=True)
            row = np.stack([tr[k] for k in ref.TRACE_FIELDS], axis=1)[0]  # (the first query's)
        else:
            r, row = cases.run(name, ref.estimate, None), np.full(len(ref.TRACE_FIELDS), -1, np.int32)
        names.append(name)
        digests.append(cases.digest(r))
        traces.append(row.astype(np.int32))
    return dict(names=np.array(names), digests=np.array(digests), traces=np.stack(traces))


def main():
    np.savez_compressed(OUT, **compute())
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
