"""Throughput of track triangulation (amc_triangulate_tracks).

Workload: a seeded synthetic scene (pycolmap_amd.synth.triangulation_scene): 200 cameras on a sphere around a point
cloud, --tracks tracks (default 10^6) of 2-50 observations skewed short, 0.5 px noise, 10 % outliers, max_error a 4 px
angle at f = 1000.  Reports tracks/s of kernel time and of device time (uploads and downloads included), tracks/s end
to end through _capi.Context (the Python call, host-side argument checks and sorting included), the single-call latency
of pycolmap.estimate_triangulation, and the single-threaded CPU reference (tests/tri_ref) on a subset, for scale; the
subset is also checked bit for bit against the GPU.  Prints one JSON line; --out writes it to a file as well.

    python tools/triangulation_bench.py [--tracks 1000000] [--reps 3] [--out profiles/tri/triangulation_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-tracks", type=int, default=20_000)
    ap.add_argument("--single-calls", type=int, default=200)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import pycolmap
    import tri_ref_lib as ref
    from pycolmap_amd import _capi, synth

    F = 1000.0
    opts = dict(max_error=4.0 / F)
    t0 = time.perf_counter()
    sc = synth.triangulation_scene(np.random.default_rng(2026), a.tracks, num_cameras=200, max_len=50, mean_len=5.0,
                                   noise_px=0.5, outlier_frac=0.1, f=F)
    gen_s = time.perf_counter() - t0
    lens = np.diff(sc["offsets"].astype(np.int64))
    args = (sc["poses"], sc["offsets"], sc["obs_pose"], sc["obs_xy"])
    out = {"workload": {"tracks": a.tracks, "observations": int(lens.sum()), "cameras": 200, "mean_len": float(lens.mean()),
                        "max_len": int(lens.max()), "noise_px": 0.5, "outlier_frac": 0.1, "max_error_rad": opts["max_error"],
                        "generation_s": round(gen_s, 2)}}
    with _capi.Context(0) as ctx:
        ctx.triangulate_tracks(*args, **opts)  # warm-up (module load, first allocation)
        walls, devs, kers = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            xyz, ok, mask, st = ctx.triangulate_tracks(*args, **opts)
            walls.append(time.perf_counter() - t0)
            devs.append(st["device_ms"])
            kers.append(st["kernel_ms"])
        w, d, k = float(np.median(walls)), float(np.median(devs)), float(np.median(kers))
        out["gpu"] = {"kernel_ms": round(k, 3), "device_ms": round(d, 3), "end_to_end_ms": round(1e3 * w, 3),
                      "tracks_per_s_kernel": round(a.tracks / (k * 1e-3)), "tracks_per_s_device": round(a.tracks / (d * 1e-3)),
                      "tracks_per_s_end_to_end": round(a.tracks / w), "num_batches": st["num_batches"],
                      "success_rate": float(ok.mean()), "mean_trials": float(st["num_trials"].mean()),
                      "reps": a.reps, "device_ms_all": [round(x, 3) for x in devs]}
        # the CPU reference on the first cpu_tracks tracks, and the GPU on the same subset bit for bit
        nt = min(a.cpu_tracks, a.tracks)
        m = int(sc["offsets"][nt])
        sub = (sc["poses"], sc["offsets"][:nt + 1], sc["obs_pose"][:m], sc["obs_xy"][:m])
        t0 = time.perf_counter()
        rxyz, rok, rmask, rst = ref.triangulate(*sub, **opts)
        cpu_s = time.perf_counter() - t0
        exact = (np.array_equal(rxyz.view(np.uint64), xyz[:nt].view(np.uint64)) and np.array_equal(rok, ok[:nt])
                 and np.array_equal(rmask, mask[:m]) and np.array_equal(rst["num_trials"], st["num_trials"][:nt]))
        out["cpu_reference"] = {"tracks": nt, "seconds": round(cpu_s, 3), "tracks_per_s": round(nt / cpu_s),
                                "threads": 1, "gpu_bit_exact_on_subset": bool(exact)}
    # single-call latency through the pycolmap binding (tracks of the scene with 4-6 observations)
    off = sc["offsets"].astype(np.int64)
    picks = np.flatnonzero((lens >= 4) & (lens <= 6))[:a.single_calls]
    o = pycolmap.EstimateTriangulationOptions(ransac={"max_error": opts["max_error"]})
    calls = []
    for t in picks:
        sl = slice(off[t], off[t + 1])
        pts = [pycolmap.PointData(xy * F + 500.0, xy) for xy in sc["obs_xy"][sl]]
        ims = [pycolmap.Image(cam_from_world=pycolmap.Rigid3d(sc["poses"][p])) for p in sc["obs_pose"][sl]]
        cams = [pycolmap.Camera(model="SIMPLE_PINHOLE", width=1000, height=1000, params=[F, 500.0, 500.0])] * len(pts)
        t0 = time.perf_counter()
        pycolmap.estimate_triangulation(pts, ims, cams, opions=o)
        calls.append(time.perf_counter() - t0)
    calls = np.array(calls[1:]) * 1e6
    out["single_call_us"] = {"calls": int(calls.size), "median": round(float(np.median(calls)), 1),
                             "p90": round(float(np.percentile(calls, 90)), 1)}
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
