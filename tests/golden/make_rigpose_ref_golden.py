"""Writes tests/golden/rigpose_ref_v1.npz: the CPU reference (tests/rigpose_ref) on every case of tests/rigpose_cases.py,
one array per case and field ("<case>/<field>").  The fixture freezes the reference: tests/test_rigpose_cpu.py compares
a fresh run with it bit for bit, tests/test_rigpose_gpu.py the GPU.  Run from the repository root after a deliberate
change of DESIGN.md section 13: python tests/golden/make_rigpose_ref_golden.py

With --edges it writes tests/golden/rigpose_ref_edges_v1.npz for rigpose_cases.EDGE_CASES instead: per case the sha256
digest of the result and the reference's refinement trace (the inputs are seeded, so none are stored), and leaves
rigpose_ref_v1.npz alone.  Both come from the reference only, never from the GPU."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import rigpose_cases  # noqa: E402
import rigpose_ref_lib as ref  # noqa: E402

FIELDS = ("success", "qvec", "tvec", "num_inliers", "num_all_inliers", "num_trials", "inlier_mask", "covariance")
OUT_EDGES = ROOT / "tests" / "golden" / "rigpose_ref_edges_v1.npz"


def main():
    out = {}
    for name, (sc, est, rf, cov) in sorted(rigpose_cases.cases().items()):
        r = ref.estimate(*rigpose_cases.args(sc), est, rf, cov)
        for k in FIELDS:
            if k in r:
                out[f"{name}/{k}"] = np.asarray(r[k])
    path = ROOT / "tests" / "golden" / "rigpose_ref_v1.npz"
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {path.stat().st_size} bytes")


def edge_reference(name):
    """(result, trace (Q, 6) int32 by rigpose_ref_lib.TRACE_FIELDS) of the reference on one edge case"""
    sc, est, rf, cov = rigpose_cases.EDGE_CASES[name]
    r, tr = ref.estimate(*rigpose_cases.args(sc), est, rf, cov, trace=True)
    return r, np.stack([tr[k] for k in ref.TRACE_FIELDS], axis=1)


def edges():
    """names (C,), digests (C, 32) uint8, trace_rows (C,) rows of each case in trace (R, 6): a few arrays for all the
    cases, since an archive member per case would cost more than what it holds"""
    names = sorted(rigpose_cases.EDGE_CASES)
    digests, rows, traces = [], [], []
    for name in names:
        r, tr = edge_reference(name)
        digests.append(np.frombuffer(bytes.fromhex(rigpose_cases.digest(r)), np.uint8))
        rows.append(len(tr))
        traces.append(tr)
    np.savez_compressed(OUT_EDGES, names=np.array(names), digests=np.stack(digests),
                        trace_rows=np.array(rows, np.int32), trace=np.concatenate(traces))
    print(f"wrote {OUT_EDGES} ({OUT_EDGES.stat().st_size} bytes)")


def load_edges():
    """name -> (digest as hex, trace (Q, 6)) of the edge fixture"""
    g = np.load(OUT_EDGES)
    ends = np.cumsum(g["trace_rows"])
    return {str(n): (bytes(g["digests"][i]).hex(), g["trace"][ends[i] - g["trace_rows"][i]:ends[i]])
            for i, n in enumerate(g["names"])}


if __name__ == "__main__":
    edges() if "--edges" in sys.argv[1:] else main()
