"""Throughput of the point filter (amc_filter_points3d, Context.filter_points3d).

Workload: a seeded synthetic model generated here: --images cameras (default 1,000) 0.2 apart along a path with one
shared SIMPLE_RADIAL camera, --points points (default 1,000,000), each seen by the cameras next to the one it sits in
front of.  Track lengths are skewed: 2 + a geometric number (p = 0.35, cut at 10) for all but --long-fraction (default
0.001) of the points, whose lengths are uniform in 100 .. 400.  0.5 px noise, 5 % of the observations moved by 30 px.
Reports, for the best of --reps repetitions of filter_points3d(4.0, 1.5): observations/s end to end (the C call: host +
device time) and by the kernels alone, kernel / copy / device / allocation / host ms (the copies and the kernels by
HIP event spans of their own, launch gaps included; no kernel trace), the Python call's wall time, the single-threaded CPU
reference (tests/filter_ref) on the same input with a bit-for-bit comparison, and the time to stream the call's input
and output bytes once at the HBM rate (6.3 TB/s achievable of 8.0 TB/s).  Prints one JSON line; --out writes it too.

    python tools/filter_points_bench.py [--reps 3] [--out profiles/filter_points/filter_points_bench.json]
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

HBM_ACHIEVABLE_GBS = 6300.0  # MI355X HBM3E: 8.0 TB/s by the sheet, 6.3 TB/s measured with a copy


def path_model(nimg, npts, long_fraction, seed=0, noise=0.5, outliers=0.05):
    """Context.filter_points3d's positional arguments"""
    import ba_cases
    import ba_scipy
    rng = np.random.default_rng(seed)
    prm = np.array([800.0, 500.0, 400.0, 0.05])
    q = np.array([ba_cases.quat_plus([0, 0, 0, 1.0], rng.uniform(-0.03, 0.03, 3)) for _ in range(nimg)])
    centre = np.stack([0.2 * np.arange(nimg), np.zeros(nimg), np.zeros(nimg)], axis=1)
    t = np.array([-ba_cases.rotate(q[i], centre[i]) for i in range(nimg)])
    L = 2 + np.minimum(rng.geometric(0.35, npts) - 1, 8)
    long = rng.random(npts) < long_fraction
    L[long] = rng.integers(100, 401, int(long.sum()))
    L = np.minimum(L, nimg)
    c = rng.integers(0, nimg, npts)
    first = np.clip(c - L // 2, 0, nimg - L)
    off = np.concatenate([[0], np.cumsum(L)]).astype(np.uint64)
    op = np.repeat(np.arange(npts), L)
    oi = (np.arange(int(off[-1])) - np.repeat(off[:-1].astype(np.int64), L) + np.repeat(first, L)).astype(np.uint32)
    X = np.stack([0.2 * c + rng.uniform(-1.0, 1.0, npts), rng.uniform(-1.0, 1.0, npts), rng.uniform(5.0, 7.0, npts)], axis=1)
    xy = np.zeros((oi.size, 2))
    order = np.argsort(oi, kind="stable")
    cuts = np.searchsorted(oi[order], np.arange(nimg + 1))
    for i in range(nimg):
        sel = order[cuts[i]:cuts[i + 1]]
        if sel.size:
            xy[sel] = ba_scipy.project(2, prm, ba_cases.rotate(q[i], X[op[sel]]) + t[i])
    xy += noise * rng.standard_normal(xy.shape)
    bad = rng.random(oi.size) < outliers
    ang = rng.uniform(0, 2 * np.pi, int(bad.sum()))
    xy[bad] += 30.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    return ([2], [prm], np.zeros(nimg, np.uint32), q, t, X, off, oi, xy), L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--long-fraction", type=float, default=0.001)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import filter_cases as fc
    import filter_ref_lib as ref

    from pycolmap_amd import _capi

    args, L = path_model(a.images, a.points, a.long_fraction)
    nobs, npts, nimg = len(args[7]), a.points, a.images
    # what one call reads and writes once: per observation image index, point index, pixel, squared error, mark; per point
    # position, offset, verdict, error; per image pose, camera index, centre
    bytes_once = nobs * (4 + 4 + 16 + 8 + 1) + npts * (24 + 4 + 1 + 8) + nimg * (32 + 24 + 4 + 24)
    best = None
    with _capi.Context(0) as ctx:
        ctx.filter_points3d(*fc.case_call("points_64")[0])  # warm-up: the library, then both timed shapes
        ctx.filter_points3d(*args, max_reproj_error=4.0, min_tri_angle=1.5)
        ctx.filter_points3d(*args, errors_only=True)
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = ctx.filter_points3d(*args, max_reproj_error=4.0, min_tri_angle=1.5)
            r["wall_ms"] = 1e3 * (time.perf_counter() - t0)
            if best is None or r["device_ms"] + r["host_ms"] < best["device_ms"] + best["host_ms"]:
                best = r
        errs = ctx.filter_points3d(*args, errors_only=True)
    t0 = time.perf_counter()
    want = ref.filter_points3d(*args, max_reproj_error=4.0, min_tri_angle=1.5)
    ref_ms = 1e3 * (time.perf_counter() - t0)
    call_ms = best["device_ms"] + best["host_ms"]
    verdicts = np.bincount(best["point_verdict"], minlength=5)
    out = {
        "workload": {"images": nimg, "points": npts, "observations": nobs, "mean_track_length": nobs / npts,
                     "tracks_of_64_or_more": int((L >= fc.WAVE_CLASS_MIN).sum()), "longest_track": int(L.max()),
                     "max_reproj_error": 4.0, "min_tri_angle": 1.5},
        "num_filtered": best["num_filtered"], "verdicts": {n: int(v) for n, v in zip(_capi.FILTER_VERDICTS, verdicts)},
        "num_batches": best["num_batches"],
        "kernel_ms": best["kernel_ms"], "copy_ms": best["copy_ms"], "device_ms": best["device_ms"],
        "alloc_ms": best["alloc_ms"], "host_ms": best["host_ms"], "wall_ms": best["wall_ms"],
        "observations_per_s_end_to_end": nobs / (1e-3 * call_ms), "observations_per_s_kernels": nobs / (1e-3 * best["kernel_ms"]),
        "errors_only_kernel_ms": errs["kernel_ms"],
        "pair_pass_share_of_kernel_ms_upper_bound": max(0.0, 1.0 - errs["kernel_ms"] / best["kernel_ms"]),
        "cpu_reference_ms": ref_ms, "cpu_reference_over_call": ref_ms / call_ms,
        "cpu_reference_over_kernels": ref_ms / best["kernel_ms"],
        "gpu_equals_reference_bit_for_bit": fc.same_bits(best, want),
        "bytes_once": bytes_once, "hbm_achievable_gbs": HBM_ACHIEVABLE_GBS,
        "stream_once_ms": 1e3 * bytes_once / (HBM_ACHIEVABLE_GBS * 1e9),
        "kernel_ms_over_stream_once_ms": best["kernel_ms"] / (1e3 * bytes_once / (HBM_ACHIEVABLE_GBS * 1e9)),
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
