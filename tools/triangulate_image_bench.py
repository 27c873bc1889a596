"""Throughput of the observation triangulator (amc_triangulate_observations, Context.triangulate_observations; DESIGN.md
section 17.8).

Workload: a seeded synthetic scene generated here: --images cameras (default 300) 0.2 apart along a path with one shared
SIMPLE_RADIAL camera and --points planted points (default 100,000), each seen by 4 to 12 neighbouring cameras: --images x
a few thousand points2D.  Every observation is one item, as triangulate_image makes one of every point2D: its candidates
are the point's other observations (the direct correspondences of a graph from the planted tracks) and itself last.
0.5 px noise; 10 % of the candidates are wrong matches (a pixel moved by 30 px); the observations of 30 % of the points
already carry the point, so that their items continue instead of creating.  Reports, for the best of --reps repetitions
after untimed warm-up calls: items/s and observations/s end to end (the C call: host + device time) and by the kernels
alone, kernel / copy / device / allocation / host ms and their shares, the kernel time of the items of 4, 8 and 12
candidates alone (what a wave of equal items costs per item), and the single-threaded CPU reference
(tests/triangulator_ref) on the first --ref-items items with a bit-for-bit comparison.  Prints one JSON line; --out writes
it too.

    python tools/triangulate_image_bench.py [--reps 3] [--out profiles/triangulator/triangulate_image_bench.json]
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


def path_scene(nimg, npts, seed=0, noise=0.5, wrong=0.10, with_point=0.30):
    """Context.triangulate_observations's positional arguments, and the items' lengths"""
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
    # the observations, point by point
    ooff = np.concatenate([[0], np.cumsum(L)])
    op = np.repeat(np.arange(npts), L)
    oi = (np.arange(int(ooff[-1])) - np.repeat(ooff[:-1], L) + np.repeat(first, L)).astype(np.uint32)
    xy = np.zeros((oi.size, 2))
    order = np.argsort(oi, kind="stable")
    cuts = np.searchsorted(oi[order], np.arange(nimg + 1))
    for i in range(nimg):
        sel = order[cuts[i]:cuts[i + 1]]
        if sel.size:
            xy[sel] = ba_scipy.project(2, prm, ba_cases.rotate(q[i], X[op[sel]]) + t[i])
    xy += noise * rng.standard_normal(xy.shape)
    has_pt = rng.random(npts) < with_point
    # the items: observation o of point j -> the other observations of j in order, then o
    nitems = oi.size
    IL = np.repeat(L, L)  # the items' lengths
    ioff = np.concatenate([[0], np.cumsum(IL)]).astype(np.uint64)
    base = np.repeat(ooff[:-1][op], IL)  # the first observation of the item's point, per candidate
    k = np.arange(int(ioff[-1])) - np.repeat(ioff[:-1].astype(np.int64), IL)  # position within the item
    own = np.repeat(np.arange(nitems) - ooff[:-1][op], IL)  # the reference's position within its point
    IL_c = np.repeat(IL, IL)
    pos = np.where(k == IL_c - 1, own, np.where(k < own, k, k + 1))
    cand = base + pos
    cxy = xy[cand].copy()
    bad = (rng.random(cand.size) < wrong) & (k != IL_c - 1)
    ang = rng.uniform(0, 2 * np.pi, int(bad.sum()))
    cxy[bad] += 30.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    chas = (has_pt[op[cand]] & (k != IL_c - 1)).astype(np.uint8)
    cX = np.where(chas[:, None] != 0, X[op[cand]], 0.0)
    return ([2], [prm], np.zeros(nimg, np.uint32), q, t, ioff, oi[cand], cxy, chas, cX), IL


def subset(args, items):
    """the flat problem of the given items"""
    off = args[5].astype(np.int64)
    lens = (off[1:] - off[:-1])[items]
    cand = np.concatenate([np.arange(off[i], off[i + 1]) for i in items]) if len(items) else np.zeros(0, np.int64)
    return args[:5] + (np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), args[6][cand], args[7][cand], args[8][cand], args[9][cand])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=300)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-items", type=int, default=20000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import triangulator_cases as tc
    import triangulator_ref_lib as ref

    from pycolmap_amd import _capi

    args, IL = path_scene(a.images, a.points)
    nitems, ncand = len(IL), len(args[6])
    head = subset(args, np.arange(min(a.ref_items, nitems)))
    by_length = {}
    best = None
    with _capi.Context(0) as ctx:
        ctx.triangulate_observations(*tc.case_call("items_64")[0])  # warm-up: the library, then the timed shape
        ctx.triangulate_observations(*args)
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = ctx.triangulate_observations(*args)
            r["wall_ms"] = 1e3 * (time.perf_counter() - t0)
            if best is None or r["device_ms"] + r["host_ms"] < best["device_ms"] + best["host_ms"]:
                best = r
        got_head = ctx.triangulate_observations(*head)
        for n in (4, 8, 12):
            items = np.flatnonzero(IL == n)[:65536]
            sub = subset(args, items)
            ctx.triangulate_observations(*sub)
            k = min(ctx.triangulate_observations(*sub)["kernel_ms"] for _ in range(a.reps))
            by_length[str(n)] = {"items": int(items.size), "kernel_ms": k, "kernel_ns_per_item": 1e6 * k / max(items.size, 1)}
    t0 = time.perf_counter()
    want_head = ref.triangulate_observations(*head)
    ref_ms = 1e3 * (time.perf_counter() - t0)
    call_ms = best["device_ms"] + best["host_ms"]
    ref_items = len(head[5]) - 1
    out = {
        "workload": {"images": a.images, "planted_points": a.points, "points2D_per_image": nitems / a.images, "items": nitems,
                     "observations": ncand, "mean_item_length": ncand / nitems, "longest_item": int(IL.max())},
        "num_created": best["num_created"], "num_continued": best["num_continued"], "num_batches": best["num_batches"],
        "kernel_ms": best["kernel_ms"], "copy_ms": best["copy_ms"], "device_ms": best["device_ms"],
        "alloc_ms": best["alloc_ms"], "host_ms": best["host_ms"], "wall_ms": best["wall_ms"],
        "kernel_share": best["kernel_ms"] / call_ms, "copy_share": best["copy_ms"] / call_ms, "host_share": best["host_ms"] / call_ms,
        "items_per_s_end_to_end": nitems / (1e-3 * call_ms), "observations_per_s_end_to_end": ncand / (1e-3 * call_ms),
        "items_per_s_kernels": nitems / (1e-3 * best["kernel_ms"]), "observations_per_s_kernels": ncand / (1e-3 * best["kernel_ms"]),
        "kernel_by_item_length": by_length,
        "cpu_reference_items": ref_items, "cpu_reference_ms": ref_ms, "cpu_reference_items_per_s": ref_items / (1e-3 * ref_ms),
        "gpu_equals_reference_bit_for_bit_on_those": tc.same(got_head, want_head),
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
