"""Writes tests/golden/abspose_ref_v1.npz: a few localisation queries (inputs included) and what the absolute pose CPU
reference (tests/abspose_ref) returns for them, so that a later change of the reference shows up as a diff.

    python tests/golden/make_abspose_ref_golden.py

With --edges it writes tests/golden/abspose_ref_edges_v1.npz for abspose_cases.EDGE_CASES instead: per case the sha256
digest of the result and, for a refinement, the reference's trace (its inputs are seeded, so none are stored), and
leaves abspose_ref_v1.npz alone.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import abspose_cases  # noqa: E402

OUT = ROOT / "tests" / "golden" / "abspose_ref_v1.npz"
OUT_EDGES = ROOT / "tests" / "golden" / "abspose_ref_edges_v1.npz"
FIELDS = ("success", "qvec", "tvec", "num_inliers", "num_trials", "focal_factor", "inlier_mask", "covariance")
INPUTS = ("offsets", "camera_models", "points2D", "points3D")
OPTS = {"outliers40": ({}, {}, True), "focal": (dict(estimate_focal_length=1, num_focal_length_samples=6), {}, False),
        "models": ({}, dict(loss_function_scale=2.0), True), "degenerate": ({}, {}, True)}


def fresh_scenes():
    return {"outliers40": abspose_cases.scene(500, 3, 400, outlier_frac=0.4),
            "focal": abspose_cases.scene(501, 2, 200, outlier_frac=0.2),
            "models": abspose_cases.concat(*[abspose_cases.scene(510 + m, 1, 120, outlier_frac=0.3, model=m)
                                             for m in range(11)]),
            "degenerate": abspose_cases.degenerate()}


def fixture_cases(g=None):
    """name -> (scene, estimation options, refinement options, return_covariance); the scenes from the fixture itself
    when it is given, else freshly generated"""
    out = {}
    scenes = fresh_scenes() if g is None else None
    for name, (est, rf, cov) in OPTS.items():
        if g is None:
            sc = scenes[name]
        else:
            sc = {k: g[f"{name}/in_{k}"] for k in INPUTS}
            sc["camera_params"] = list(g[f"{name}/in_camera_params"])
        out[name] = (sc, est, rf, cov)
    return out


def main():
    import abspose_ref_lib as ref
    arrays = {}
    for name, (sc, est, rf, cov) in fixture_cases().items():
        for k in INPUTS:
            arrays[f"{name}/in_{k}"] = np.asarray(sc[k])
        arrays[f"{name}/in_camera_params"] = np.stack([np.pad(np.asarray(p, np.float64), (0, 12 - len(p)))
                                                       for p in sc["camera_params"]])
        r = ref.estimate(sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"], sc["points3D"], est,
                         rf, cov)
        for k in FIELDS:
            if k in r:
                arrays[f"{name}/{k}"] = np.asarray(r[k])
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


def edge_reference(name):
    """(result, trace (Q, 6) int32 by abspose_ref_lib.TRACE_FIELDS or None) of the reference on one edge case"""
    import abspose_ref_lib as ref
    if abspose_cases.EDGE_CASES[name][0] == "estimate":
        return abspose_cases.edge_run(name, ref.estimate, ref.refine), None
    r, tr = abspose_cases.edge_run(name, ref.estimate, lambda *a: ref.refine(*a, trace=True))
    return r, np.stack([tr[k] for k in ref.TRACE_FIELDS], axis=1)


def edges():
    """names (C,), digests (C, 32) uint8, trace_rows (C,) rows of each case in trace (R, 6): a few arrays for all the
    cases, since an archive member per case would cost more than what it holds"""
    names = sorted(abspose_cases.EDGE_CASES)
    digests, rows, traces = [], [], [np.zeros((0, 6), np.int32)]
    for name in names:
        r, tr = edge_reference(name)
        digests.append(np.frombuffer(bytes.fromhex(abspose_cases.digest(r)), np.uint8))
        rows.append(0 if tr is None else len(tr))
        if tr is not None:
            traces.append(tr)
    np.savez_compressed(OUT_EDGES, names=np.array(names), digests=np.stack(digests),
                        trace_rows=np.array(rows, np.int32), trace=np.concatenate(traces))
    print(f"wrote {OUT_EDGES} ({OUT_EDGES.stat().st_size} bytes)")


def load_edges():
    """name -> (digest as hex, trace (Q, 6) or None) of the edge fixture"""
    g = np.load(OUT_EDGES)
    ends = np.cumsum(g["trace_rows"])
    return {str(n): (bytes(g["digests"][i]).hex(), g["trace"][ends[i] - g["trace_rows"][i]:ends[i]]
                     if g["trace_rows"][i] else None) for i, n in enumerate(g["names"])}


if __name__ == "__main__":
    edges() if "--edges" in sys.argv[1:] else main()
