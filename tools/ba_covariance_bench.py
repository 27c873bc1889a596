"""Timing of the bundle-adjustment covariance (amc_ba_covariance, Context.ba_covariance).

Workload: tools/bundle_adjustment_bench.py's scene: --images cameras (default 300) along a path,
--points points (default 100,000) each seen by 5 neighbouring cameras, one shared SIMPLE_RADIAL camera, COLMAP's gauge:
about 1,800 columns.  Reports, for the best of --reps calls: kernel time by phase (evaluation, formation, factor, inverse,
points), copies (device minus kernel), host and wall time, the achieved FP64 rate of the factor and inverse phases (m^3 / 3
operations for the Cholesky factor, m^3 / 3 for the triangular inverse and m^3 / 3 for Z^T Z, a multiply and an add counted
as two) beside the chip's vector FP64 peak, and the single-threaded CPU reference (tests/bacov_ref) on the same problem
with a bit-for-bit check (--no-reference leaves it out).  Prints one JSON line; --out writes it to a file as well.

    python tools/ba_covariance_bench.py [--reps 3] [--out profiles/bundle_adjustment_covariance/ba_covariance_bench.json]

--local runs the local leg instead: the same kind of scene as a Reconstruction (--local-images, --local-points), a
BundleAdjustmentConfig of --local-config neighbouring images in the middle of the path, BundleAdjuster.solve and then
estimate_ba_covariance on it.

    python tools/ba_covariance_bench.py --local [--out profiles/bundle_adjustment_covariance/local_bench.json]
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

# AMD's product specification of the MI355X: 78.6 TFLOPS of vector FP64 with fused multiply-add.  The kernels may not
# fuse (the order of 24.4 is a multiply and then an add), so half of it is the most they can reach.
FP64_VECTOR_PEAK_TFLOPS = 78.6


def _ba_bench():
    spec = importlib.util.spec_from_file_location("bundle_adjustment_bench", ROOT / "tools" / "bundle_adjustment_bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _best(call, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = call()
        r["wall_ms"] = 1e3 * (time.perf_counter() - t0)
        if best is None or r["device_ms"] < best["device_ms"]:
            best = r
    return best


def _rates(m, phases):
    third = m ** 3 / 3.0
    out = {"factor_gflops": 1e-6 * third / phases["factor"] if phases["factor"] else None,
           "inverse_gflops": 1e-6 * 2.0 * third / phases["inverse"] if phases["inverse"] else None,
           "fp64_vector_peak_gflops": 1e3 * FP64_VECTOR_PEAK_TFLOPS,
           "fp64_vector_peak_without_fma_gflops": 0.5e3 * FP64_VECTOR_PEAK_TFLOPS}
    return out


def global_leg(a):
    import bacov_cases
    import bacov_ref_lib as ref

    from pycolmap_amd import _capi
    args = _ba_bench().path_scene(a.images, a.points)
    small = bacov_cases.by_name("columns_65")["problem"]
    with _capi.Context(0) as ctx:
        ctx.ba_covariance(*small)  # warm-up
        best = _best(lambda: ctx.ba_covariance(*args), a.reps)
    m = best["num_columns"]
    out = {"workload": {"images": a.images, "points": a.points, "observations": len(args[8]), "columns": m},
           "success": best["success"], "min_pivot_ratio": best["min_pivot_ratio"],
           "phase_ms": best["phase_ms"], "kernel_ms": best["kernel_ms"], "copy_ms": best["copy_ms"],
           "device_ms": best["device_ms"], "host_ms": best["host_ms"], "wall_ms": best["wall_ms"],
           **_rates(m, best["phase_ms"])}
    if not a.no_reference:
        ref.load()
        t0 = time.perf_counter()
        want = ref.ba_covariance(*args)
        out["cpu_reference_ms"] = 1e3 * (time.perf_counter() - t0)
        out["gpu_equals_reference_bit_for_bit"] = bacov_cases.digest(best) == bacov_cases.digest(want)
    return out


def local_leg(a):
    import ba_cases
    import pycolmap_amd as pc
    args = _ba_bench().path_scene(a.local_images, a.local_points, seed=2)
    sc = dict(models=[2], camera_params=args[1], image_cameras=args[3], qvec=args[4], tvec=args[5], xyz=args[7],
              obs_image=args[8], obs_point=args[9], obs_xy=args[10])
    rec = ba_cases.reconstruction(sc)
    cfg = pc.BundleAdjustmentConfig()
    first = a.local_images // 2 - a.local_config // 2
    for i in range(first, first + a.local_config):
        cfg.add_image(i + 1)
    o = pc.BundleAdjustmentOptions()
    o.solver_options.max_num_iterations = a.iterations
    adj = pc.BundleAdjuster(o, cfg)
    assert adj.solve(rec)
    options = pc.BACovarianceOptions()
    pc.estimate_ba_covariance(options, rec, adj)  # warm-up

    def call():
        cov = pc.estimate_ba_covariance(options, rec, adj)
        assert cov is not None
        return dict(cov.summary)
    best = _best(call, a.reps)
    return {"workload": {"model_images": a.local_images, "model_points": a.local_points, "config_images": a.local_config,
                         "columns": best["num_columns"], "pose_blocks": best["num_pose_blocks"],
                         "camera_blocks": best["num_camera_blocks"], "point_blocks": best["num_point_blocks"]},
            "min_pivot_ratio": best["min_pivot_ratio"], "phase_ms": best["phase_ms"], "kernel_ms": best["kernel_ms"],
            "copy_ms": best["copy_ms"], "device_ms": best["device_ms"], "host_ms": best["host_ms"],
            "total_ms": best["total_ms"], "wall_ms": best["wall_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=300)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-reference", action="store_true", help="leave out the single-threaded CPU reference")
    ap.add_argument("--local", action="store_true", help="the local leg: estimate_ba_covariance after a local solve")
    ap.add_argument("--local-images", type=int, default=300)
    ap.add_argument("--local-points", type=int, default=30000)
    ap.add_argument("--local-config", type=int, default=5)
    a = ap.parse_args()
    line = json.dumps(local_leg(a) if a.local else global_leg(a))
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
