"""Timings of the mapper's two device calls and three methods.  It asserts no time.

Workload, generated here: --images cameras (default 200) 0.2 apart along a path with one shared SIMPLE_RADIAL camera and
--points planted points (default 10,000), each seen by 4 to 12 neighbouring cameras, 0.5 px noise.  The first half of the
images is the model, with every planted point at least two of them see at its true position; the other half are the
mapper's candidates; the graph holds the planted matches of every two images with a common point.  Reports, for the best of
--reps repetitions after two untimed calls:

  visibility    one Context.image_visibility call on all candidates (the flat problem the host layer plans) against the
                single-threaded CPU reference (tests/mapper_ref) on the same input, compared bit for bit;
  angles        one Context.shared_point_angles call on the pairs of every model image's local bundle, against the reference;
  methods       find_next_images, register_next_image of the best candidate and find_local_bundle around it through Python,
                against the same three calls of the sequential reference scene, with the lists compared.

Prints one JSON line; --out writes it too.

    python tools/image_registration_bench.py [--reps 3] [--out profiles/mapper/image_registration_bench.json]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def path_state(nimg, npts, seed=0, noise=0.5):
    """a state in the form of tests/mapper_cases.mapper_state"""
    import ba_cases
    import ba_scipy
    rng = np.random.default_rng(seed)
    prm = np.array([800.0, 500.0, 400.0, 0.05])
    q = np.array([ba_cases.quat_plus([0, 0, 0, 1.0], rng.uniform(-0.03, 0.03, 3)) for _ in range(nimg)])
    centre = np.stack([0.2 * np.arange(nimg), np.zeros(nimg), np.zeros(nimg)], axis=1)
    t = np.array([-ba_cases.rotate(q[i], centre[i]) for i in range(nimg)])
    L = np.minimum(rng.integers(4, 13, npts), nimg)
    c = rng.integers(0, nimg, npts)
    first = np.clip(c - L // 2, 0, nimg - L)
    X = np.stack([0.2 * c + rng.uniform(-1.0, 1.0, npts), rng.uniform(-1.0, 1.0, npts), rng.uniform(5.0, 7.0, npts)], axis=1)
    seen = [[] for _ in range(nimg)]  # per image the planted points, its point2D order
    for j in range(npts):
        for i in range(first[j], first[j] + L[j]):
            seen[i].append(j)
    index = [{j: p for p, j in enumerate(s)} for s in seen]
    xy = [ba_scipy.project(2, prm, ba_cases.rotate(q[i], X[seen[i]]) + t[i]) + noise * rng.standard_normal((len(seen[i]), 2)) for i in range(nimg)]
    nmodel = nimg // 2
    images = {i + 1: [1, q[i], t[i], xy[i], np.full(len(seen[i]), (1 << 64) - 1, np.uint64)] for i in range(nmodel)}
    points = {}
    for j in range(npts):
        track = [(i + 1, index[i][j]) for i in range(first[j], min(first[j] + L[j], nmodel))]
        if len(track) >= 2:
            pid = len(points) + 1
            points[pid] = (X[j], track)
            for i, p in track:
                images[i][4][p] = pid
    matches = []
    for a in range(nimg):
        for b in range(a + 1, min(nimg, a + 12)):
            m = [(index[a][j], index[b][j]) for j in seen[a] if j in index[b]]
            if m:
                matches.append((a + 1, b + 1, np.array(m, np.uint32)))
    return dict(cameras={1: (2, 1000, 800, prm, True)}, images={i: tuple(v) for i, v in images.items()}, points=points,
                candidates={i + 1: (1, xy[i]) for i in range(nmodel, nimg)}, graph_images={i + 1: len(seen[i]) for i in range(nimg)}, matches=matches)


def best_of(reps, fn):
    out, best = None, None
    for rep in range(reps + 2):
        t0 = time.perf_counter()
        out = fn()
        ms = 1e3 * (time.perf_counter() - t0)
        if rep >= 2:
            best = ms if best is None else min(best, ms)
    return out, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import mapper_cases as k
    import mapper_ref_lib as ref
    import pycolmap_amd as pc
    from pycolmap_amd import _capi

    pc.logging.minloglevel = 2
    st = path_state(a.images, a.points)
    opts = dict(local_ba_num_images=6)
    _, _, _, mp = k.mapper(st)
    # the flat problems, as the host layer plans them
    seen = []
    mp._find_next_images_with(opts, lambda d: (seen.append(d), k.vis_solver(d))[1])
    vis = [seen[0][f] for f in ("image_point_offsets", "point2D_point3D", "cand_width", "cand_height", "cand_point_offsets", "cand_xy", "corr_offsets",
                                "corr_image", "corr_point2D")]
    vis = [v.reshape(-1) if f != 5 else v for f, v in enumerate(vis)]
    bundles = []
    for iid in sorted(st["images"]):
        mp._find_local_bundle_with(opts, iid, lambda d: (bundles.append(d), k.angle_solver(d))[1])
    q = np.concatenate([d["qvec"] for d in bundles])
    t = np.concatenate([d["tvec"] for d in bundles])
    X = np.concatenate([d["point_xyz"] for d in bundles])
    io = np.cumsum([0] + [len(d["qvec"]) for d in bundles])
    po = np.cumsum([0] + [len(d["point_xyz"]) for d in bundles])
    pimg = np.concatenate([d["pair_images"] + io[n] for n, d in enumerate(bundles)]).astype(np.uint32)
    shared = np.concatenate([d["shared_points"].reshape(-1) + po[n] for n, d in enumerate(bundles)]).astype(np.uint32)
    sizes = np.concatenate([np.diff(d["pair_offsets"].reshape(-1).astype(np.int64)) for d in bundles])
    poff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ang = (q, t, X, pimg, poff, shared)

    out = {"workload": {"images": a.images, "planted_points": a.points, "model_images": len(st["images"]), "points3D": len(st["points"]),
                        "candidates": len(st["candidates"]), "candidate_points2D": int(vis[4][-1]), "candidate_correspondences": int(vis[6][-1]),
                        "pairs": len(pimg), "shared_points": int(poff[-1]), "largest_pair": int(sizes.max())}}
    with _capi.Context(0) as ctx:
        def pick(call):
            best = None
            for rep in range(a.reps + 2):
                t0 = time.perf_counter()
                r = call()
                r["wall_ms"] = 1e3 * (time.perf_counter() - t0)
                if rep >= 2 and (best is None or r["device_ms"] + r["host_ms"] < best["device_ms"] + best["host_ms"]):
                    best = r
            return best
        gv = pick(lambda: ctx.image_visibility(*vis))
        ga = pick(lambda: ctx.shared_point_angles(*ang))
    rv, rv_ms = best_of(a.reps, lambda: ref.image_visibility(*vis))
    ra, ra_ms = best_of(a.reps, lambda: ref.shared_point_angles(*ang))
    fields = ("kernel_ms", "copy_ms", "device_ms", "alloc_ms", "host_ms", "wall_ms", "num_batches")
    out["visibility"] = dict({f: gv[f] for f in fields}, end_to_end_ms=gv["device_ms"] + gv["host_ms"], reference_ms=rv_ms,
                             equals_reference=bool(k.vis_same(gv, rv)))
    out["angles"] = dict({f: ga[f] for f in fields}, end_to_end_ms=ga["device_ms"] + ga["host_ms"], reference_ms=ra_ms,
                         equals_reference_bit_for_bit=bool(k.angle_same(ga, ra)))
    # the three methods through Python against the sequential reference scene (which keeps its own model: no conversion)
    rs = k.ref_scene(st)
    ranked, find_ms = best_of(a.reps, lambda: mp.find_next_images(opts))
    want, ref_find_ms = best_of(a.reps, lambda: rs.find_next_images(**opts))
    t0 = time.perf_counter()
    ok = mp.register_next_image(opts, ranked[0])
    reg_ms = 1e3 * (time.perf_counter() - t0)
    reg_stats = pc.last_run_stats()
    t0 = time.perf_counter()
    ref_ok = rs.register_next_image(want[0], **opts)
    ref_reg_ms = 1e3 * (time.perf_counter() - t0)
    bundle, bundle_ms = best_of(a.reps, lambda: mp.find_local_bundle(opts, ranked[0]))
    bundle_stats = pc.last_run_stats()
    ref_bundle, ref_bundle_ms = best_of(a.reps, lambda: rs.find_local_bundle(want[0], **opts))
    out["methods"] = {
        "find_next_images": {"python_ms": find_ms, "reference_ms": ref_find_ms, "equal": ranked == want, "num_ranked": len(ranked)},
        "register_next_image": {"python_ms": reg_ms, "reference_ms": ref_reg_ms, "equal": ok == ref_ok and ranked[0] == want[0], "registered": bool(ok),
                                "once": True, "num_pairs": reg_stats["num_pairs"], "device_ms": reg_stats["device_ms"], "kernel_ms": reg_stats["kernel_ms"]},
        "find_local_bundle": {"python_ms": bundle_ms, "reference_ms": ref_bundle_ms, "equal": bundle == ref_bundle, "bundle": bundle,
                              "num_pairs": bundle_stats["num_pairs"], "device_ms": bundle_stats["device_ms"], "kernel_ms": bundle_stats["kernel_ms"]},
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
