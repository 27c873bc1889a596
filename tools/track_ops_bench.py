"""Throughput of track completion and track merging (amc_complete_tracks, amc_merge_tracks and the four functions on top;
DESIGN.md section 18.7).

Flat workload: 17.8's scene, generated here: --images cameras (default 300) 0.2 apart along a path with one shared
SIMPLE_RADIAL camera and --points planted points (default 100,000), each seen by 4 to 12 neighbouring cameras, 0.5 px
noise.  30 % of the observations beyond a track's second are detached: each point with detached observations is one
completion item whose candidates they are (the closure of a graph from the planted tracks), 10 % of them moved by 30 px.
5 % of the points are duplicated: the track is cut in two halves 1e-3 apart, a component of two points whose
observations all correspond across the halves; both are roots.  Reports, for the best of --reps repetitions after two
untimed calls: kernel / copy / device / host ms and the end-to-end time of each C call, and the single-threaded CPU
reference (tests/tracks_ref) on the same input with a bit-for-bit comparison.

Model workload: a scene of tests/triangulator_cases.py (--model-images, --model-points) triangulated by the library,
then 30 % detached and 5 % duplicated (tests/tracks_cases.perturbed), through complete_all_tracks and merge_all_tracks
(with one wrong match per image pair; without, when they chain a component past the bound of 18.4 H4):
end-to-end wall time, last_run_stats(), the ratio of candidates tested to candidates visited (what the superset closure
costs) and the distribution of the components' sizes.  Prints one JSON line; --out writes it too.

    python tools/track_ops_bench.py [--reps 3] [--out profiles/tracks/track_ops_bench.json]
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


def path_scene(nimg, npts, seed=0, noise=0.5, detach=0.30, wrong=0.10, duplicate=0.05):
    """the positional arguments of Context.complete_tracks and of Context.merge_tracks"""
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
    ooff = np.concatenate([[0], np.cumsum(L)])
    op = np.repeat(np.arange(npts), L)
    within = np.arange(int(ooff[-1])) - np.repeat(ooff[:-1], L)
    oi = (within + np.repeat(first, L)).astype(np.uint32)
    xy = np.zeros((oi.size, 2))
    order = np.argsort(oi, kind="stable")
    cuts = np.searchsorted(oi[order], np.arange(nimg + 1))
    for i in range(nimg):
        sel = order[cuts[i]:cuts[i + 1]]
        if sel.size:
            xy[sel] = ba_scipy.project(2, prm, ba_cases.rotate(q[i], X[op[sel]]) + t[i])
    xy += noise * rng.standard_normal(xy.shape)
    cams = ([2], [prm], np.zeros(nimg, np.uint32), q, t)
    # completion: the detached observations of every point
    detached = (within >= 2) & (rng.random(oi.size) < detach)
    per_point = np.bincount(op[detached], minlength=npts)
    items = np.flatnonzero(per_point)
    cxy = xy[detached].copy()
    bad = rng.random(cxy.shape[0]) < wrong
    ang = rng.uniform(0, 2 * np.pi, int(bad.sum()))
    cxy[bad] += 30.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    complete = cams + (X[items], np.concatenate([[0], np.cumsum(per_point[items])]).astype(np.uint64), oi[detached], cxy)
    # merging: the duplicated points, each a component of two halves
    dup = np.flatnonzero(rng.random(npts) < duplicate)
    half = L[dup] // 2
    pts = np.repeat(X[dup], 2, axis=0) + rng.normal(0, 1e-3, (2 * dup.size, 3))
    lens = np.stack([half, L[dup] - half], axis=1).reshape(-1)
    obs = np.concatenate([np.arange(ooff[j], ooff[j + 1]) for j in dup]) if dup.size else np.zeros(0, np.int64)
    poo = np.concatenate([[0], np.cumsum(lens)])
    # an observation of one half corresponds to every observation of the other half
    ncorr = np.repeat(np.stack([L[dup] - half, half], axis=1).reshape(-1), lens)
    oco = np.concatenate([[0], np.cumsum(ncorr)])
    other_first = np.repeat(np.stack([poo[1:-1:2], poo[:-1:2]], axis=1).reshape(-1), lens)
    corr = np.repeat(other_first, ncorr) + (np.arange(int(oco[-1])) - np.repeat(oco[:-1], ncorr))
    merge = cams + (2 * np.arange(dup.size + 1, dtype=np.uint64), 2 * np.arange(dup.size + 1, dtype=np.uint64),
                    np.arange(2 * dup.size, dtype=np.uint32), pts, poo.astype(np.uint64), oi[obs], xy[obs], oco.astype(np.uint64),
                    corr.astype(np.uint32))
    return complete, merge


def timed(fn, args, reps):
    fn(*args)
    fn(*args)
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn(*args)
        r["wall_ms"] = 1e3 * (time.perf_counter() - t0)
        if best is None or r["device_ms"] + r["host_ms"] < best["device_ms"] + best["host_ms"]:
            best = r
    return best


def times(r):
    call = r["device_ms"] + r["host_ms"]
    return {"kernel_ms": r["kernel_ms"], "copy_ms": r["copy_ms"], "device_ms": r["device_ms"], "alloc_ms": r["alloc_ms"],
            "host_ms": r["host_ms"], "end_to_end_ms": call, "wall_ms": r["wall_ms"], "num_batches": r["num_batches"]}


def model_workload(nimg, npts, reps, wrong):
    """`wrong` wrong matches per image pair chain points into larger components (18.4 H4 refuses one above 4096)"""
    import pycolmap_amd as pc
    import tracks_cases as k
    import triangulator_cases as tc
    sc = tc.scene(seed=11, nimg=nimg, npts=npts, models=(2,), noise=0.5, views=(4, 12), wrong=wrong)
    r, g = tc.reconstruction(sc)
    t = pc.IncrementalTriangulator(g, r)
    for iid in sc["images"]:
        t.triangulate_image({}, iid)
    st = k.perturbed(k.make_state(sc, k.recon_points(r), k.recon_point2D_ids(r)), seed=12, detach=0.30, duplicate=0.05)
    out = {"images": nimg, "planted_points": npts, "wrong_matches_per_image_pair": wrong, "points3D": len(st["points"]),
           "observations": int(sum(len(p[3]) for p in st["points"].values()))}
    best = {}
    sizes = []

    def keep_sizes(d):  # the hook sees the flat merge problem the host layer made (the reference solves this one)
        poo = np.asarray(d["point_obs_offsets"]).reshape(-1).astype(np.int64)
        cpo = np.asarray(d["comp_point_offsets"]).reshape(-1).astype(np.int64)
        sizes[:] = (poo[cpo[1:]] - poo[cpo[:-1]]).tolist()
        return k.merge_solver(d)
    for rep in range(reps + 2):
        r, _, t = k.reconstruction(st)
        for name, fn in (("complete_all_tracks", pc.complete_all_tracks), ("merge_all_tracks", pc.merge_all_tracks)):
            t0 = time.perf_counter()
            n = fn(t, {})
            wall = 1e3 * (time.perf_counter() - t0)
            s = dict(pc.last_run_stats(), wall_ms=wall, returned=int(n))
            if rep >= 2 and (name not in best or wall < best[name]["wall_ms"]):
                best[name] = s
    r, _, t = k.reconstruction(st)
    pc.complete_all_tracks(t, {})
    pc._pycolmap._merge_tracks_with(t, {}, None, keep_sizes)
    out.update(best)
    c = best["complete_all_tracks"]
    out["candidates_tested_per_visited"] = c["num_candidates_tested"] / max(c["num_candidates_visited"], 1)
    sz = np.array(sizes, np.int64)
    out["component_observations"] = {"components": int(sz.size), "min": int(sz.min()) if sz.size else 0,
                                     "median": float(np.median(sz)) if sz.size else 0.0,
                                     "p90": float(np.percentile(sz, 90)) if sz.size else 0.0, "max": int(sz.max()) if sz.size else 0,
                                     "histogram_le_4_8_16_64_256_1024_4096": [int((sz <= b).sum()) for b in (4, 8, 16, 64, 256, 1024, 4096)]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=300)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--model-images", type=int, default=40)
    ap.add_argument("--model-points", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import tracks_cases as k
    import tracks_ref_lib as ref

    from pycolmap_amd import _capi

    complete, merge = path_scene(a.images, a.points)
    with _capi.Context(0) as ctx:
        gc = timed(ctx.complete_tracks, complete, a.reps)
        gm = timed(ctx.merge_tracks, merge, a.reps)
    t0 = time.perf_counter()
    wc = ref.complete_tracks(*complete)
    ref_c = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    wm = ref.merge_tracks(*merge)
    ref_m = 1e3 * (time.perf_counter() - t0)
    ncand, nitems = len(complete[7]), len(complete[5])
    ncomp, nobs = len(merge[5]) - 1, len(merge[10])
    out = {
        "workload": {"images": a.images, "planted_points": a.points, "completion_items": nitems, "completion_candidates": ncand,
                     "merge_components": ncomp, "merge_points": 2 * ncomp, "merge_observations": nobs, "merge_correspondences": len(merge[13])},
        "complete_tracks": dict(times(gc), num_passed=gc["num_passed"], candidates_per_s_end_to_end=ncand / (1e-3 * (gc["device_ms"] + gc["host_ms"])),
                                candidates_per_s_kernel=ncand / (1e-3 * gc["kernel_ms"]), cpu_reference_ms=ref_c,
                                cpu_reference_candidates_per_s=ncand / (1e-3 * ref_c), gpu_equals_reference_bit_for_bit=k.same("c/", gc, wc)),
        "merge_tracks": dict(times(gm), num_merges=gm["num_merges"], num_pairs_tried=gm["num_pairs_tried"],
                             components_per_s_end_to_end=ncomp / (1e-3 * (gm["device_ms"] + gm["host_ms"])),
                             components_per_s_kernel=ncomp / (1e-3 * gm["kernel_ms"]), cpu_reference_ms=ref_m,
                             cpu_reference_components_per_s=ncomp / (1e-3 * ref_m), gpu_equals_reference_bit_for_bit=k.same("m/", gm, wm)),
    }
    for wrong in (1, 0):  # with wrong matches first; a component above the bound is reported and the clean graph measured
        try:
            out["model"] = model_workload(a.model_images, a.model_points, a.reps, wrong)
            break
        except ValueError as e:
            out["model_refused_with_wrong_matches"] = str(e)
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
