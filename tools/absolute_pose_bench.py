"""Absolute pose throughput and latency on one GPU.

    python tools/absolute_pose_bench.py [--queries 10000] [--points 1000] [--outliers 0.4] [--out FILE]

Reports the batch rate through Context.estimate_absolute_poses (end to end, kernel and device time), the median and p90
latency of one pycolmap_amd.absolute_pose_estimation call at --points correspondences, and the single-threaded CPU
reference's rate on a few of the same queries.  Prints one JSON line."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

from pycolmap_amd import _capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--outliers", type=float, default=0.4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--latency-calls", type=int, default=30)
    ap.add_argument("--cpu-queries", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sc = synth.localisation_scene(np.random.default_rng(0), a.queries, num_points=a.points, outlier_frac=a.outliers)
    args = (sc["offsets"], sc["camera_models"], sc["camera_params"], sc["points2D"], sc["points3D"])
    ctx = _capi.Context(0)
    ctx.estimate_absolute_poses(sc["offsets"][:2], sc["camera_models"][:1], sc["camera_params"][:1],
                                sc["points2D"][:a.points], sc["points3D"][:a.points])  # warm-up
    wall, kern, dev = [], [], []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        r = ctx.estimate_absolute_poses(*args)
        wall.append(time.perf_counter() - t0)
        kern.append(r["kernel_ms"])
        dev.append(r["device_ms"])
    ok = r["success"]
    dq = np.abs(np.abs((r["qvec"][ok] * sc["qvec"][ok]).sum(1)) - 1.0)

    import pycolmap_amd as pycolmap
    one = synth.localisation_scene(np.random.default_rng(1), a.latency_calls + 3, num_points=a.points,
                                   outlier_frac=a.outliers)
    off = one["offsets"].astype(np.int64)
    cam = pycolmap.Camera(model="SIMPLE_PINHOLE", width=1600, height=1200, params=one["camera_params"][0])
    lat = []
    for i in range(a.latency_calls + 3):
        sl = slice(off[i], off[i + 1])
        t0 = time.perf_counter()
        pycolmap.absolute_pose_estimation(one["points2D"][sl], one["points3D"][sl], cam)
        lat.append(time.perf_counter() - t0)
    lat = np.array(lat[3:]) * 1e3

    import abspose_ref_lib as ref
    n = a.cpu_queries
    t0 = time.perf_counter()
    ref.estimate(sc["offsets"][:n + 1], sc["camera_models"][:n], sc["camera_params"][:n],
                 sc["points2D"][:int(sc["offsets"][n])], sc["points3D"][:int(sc["offsets"][n])])
    cpu_rate = n / (time.perf_counter() - t0)

    res = dict(workload=f"{a.queries} queries x {a.points} correspondences, {a.outliers:.0%} outliers, SIMPLE_PINHOLE",
               queries_per_s=a.queries / float(np.median(wall)), wall_ms=1e3 * float(np.median(wall)),
               kernel_ms=float(np.median(kern)), device_ms=float(np.median(dev)), num_batches=r["num_batches"],
               success_rate=float(ok.mean()), max_quat_err=float(dq.max()) if dq.size else None,
               single_call_ms_median=float(np.median(lat)), single_call_ms_p90=float(np.percentile(lat, 90)),
               cpu_reference_queries_per_s=cpu_rate)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
