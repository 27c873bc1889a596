"""Freeze the triangulation CPU reference (tests/tri_ref/tri_ref.cc) on seeded batches of tests/tri_cases.py: inputs
and outputs -> tests/golden/tri_ref_v1.npz, and for tri_cases.EDGE_CASES one sha256 per case over the bits of xyz,
success, the mask, num_inliers and num_trials (tri_cases.digest) -> tests/golden/tri_ref_edges_v1.npz.
tests/test_triangulation_cpu.py checks that the reference still computes exactly this.  Run from the repository root:
python tests/golden/make_tri_ref_golden.py"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

CASES = ["clean", "outliers30", "three_obs", "long_trial_caps", "min_tri_angle", "degenerate"]
OUT_EDGES = ROOT / "tests" / "golden" / "tri_ref_edges_v1.npz"


def main():
    import tri_cases
    import tri_ref_lib as ref
    all_cases = tri_cases.cases()
    out = {}
    for name in CASES:
        sc, opts = all_cases[name]
        xyz, ok, mask, st = ref.triangulate(sc["poses"], sc["offsets"], sc["obs_pose"], sc["obs_xy"], **opts)
        for k in ("poses", "offsets", "obs_pose", "obs_xy"):
            out[f"{name}/{k}"] = sc[k]
        out[f"{name}/options"] = np.frombuffer(json.dumps(opts).encode(), np.uint8)
        out[f"{name}/xyz"] = xyz
        out[f"{name}/success"] = ok
        out[f"{name}/inlier_mask"] = mask
        out[f"{name}/num_inliers"] = st["num_inliers"]
        out[f"{name}/num_trials"] = st["num_trials"]
        print(name, len(ok), "tracks", len(mask), "observations", int(ok.sum()), "successful")
    np.savez_compressed(ROOT / "tests" / "golden" / "tri_ref_v1.npz", **out)
    edges()


def edges():
    """names (C,), digests (C, 32) uint8: two arrays for all the cases"""
    import tri_cases
    import tri_ref_lib as ref
    names = sorted(tri_cases.EDGE_CASES)
    digests = []
    for name in names:
        sc, opts = tri_cases.EDGE_CASES[name]
        r = ref.triangulate(sc["poses"], sc["offsets"], sc["obs_pose"], sc["obs_xy"], **opts)
        digests.append(np.frombuffer(bytes.fromhex(tri_cases.digest(r)), np.uint8))
    np.savez_compressed(OUT_EDGES, names=np.array(names), digests=np.stack(digests))
    print(f"wrote {OUT_EDGES} ({OUT_EDGES.stat().st_size} bytes)")


def load_edges():
    """name -> digest as hex, of the edge fixture"""
    g = np.load(OUT_EDGES)
    return {str(n): bytes(g["digests"][i]).hex() for i, n in enumerate(g["names"])}


if __name__ == "__main__":
    main()
