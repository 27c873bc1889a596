"""Throughput of bundle adjustment (amc_bundle_adjust, Context.bundle_adjust).

Workload: a seeded synthetic scene of the BAL "Ladybug" class generated here: --images cameras (default 300) along a
path, --points points (default 100,000) each seen by 5 neighbouring cameras (about 5 x 10^5 observations), one shared
SIMPLE_RADIAL camera, 0.5 px noise, COLMAP's constant masks (first pose, second pose's x translation), --iterations LM
iterations (default 5).  Reports, for the best of --reps repetitions: kernel ms and device ms per LM iteration,
observations/s (observations x LM iterations / device time), PCG iterations, and the bytes/s the Schur products stream
by the byte count of DESIGN.md 15.10 against the HBM peak, taking the whole kernel time as an upper bound on the
products' time (so the figure is a lower bound).  For scale: the single-threaded CPU reference (tests/ba_ref) and scipy's
least_squares on a reduced scene (--small-points), and a bit-for-bit check of the GPU against the reference on that
scene.  Prints one JSON line; --out writes it to a file as well.

    python tools/bundle_adjustment_bench.py [--reps 3] [--out profiles/bundle_adjustment/bundle_adjustment_bench.json]

--local runs the local leg instead: the same kind of scene as a Reconstruction (--local-images,
--local-points), a BundleAdjustmentConfig of --local-config neighbouring images in the middle of the path, and
BundleAdjuster.solve on it: the points those images share with the rest of the model are constant.  Reports kernel, copy
(device minus kernel) and host milliseconds of the best of --reps solves, the share of the host time that the set-up
(model conversion, check and flattening, timed on its own through BundleAdjuster._problem) takes, and the single-threaded
CPU reference (tests/ba_config_ref) on the same flat problem with a bit-for-bit check.

    python tools/bundle_adjustment_bench.py --local [--out profiles/bundle_adjustment_config/local_bench.json]
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

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E
SEEN_BY = 5


def path_scene(nimg, npts, seed=0, noise=0.5):
    """Cameras 0.2 apart along x, looking down z with small rotations; point j sits in front of camera c_j and is seen by
    the SEEN_BY cameras around it.  Returns Context.bundle_adjust's positional arguments."""
    import ba_cases
    import ba_scipy
    rng = np.random.default_rng(seed)
    prm = np.array([800.0, 500.0, 400.0, 0.05])
    q_true = np.array([ba_cases.quat_plus([0, 0, 0, 1.0], rng.uniform(-0.03, 0.03, 3) if i else np.zeros(3))
                       for i in range(nimg)])
    centre = np.stack([0.2 * np.arange(nimg), np.zeros(nimg), np.zeros(nimg)], axis=1)
    t_true = np.array([-ba_cases.rotate(q_true[i], centre[i]) for i in range(nimg)])
    c = rng.integers(SEEN_BY // 2, nimg - SEEN_BY // 2, npts)
    X_true = np.stack([0.2 * c + rng.uniform(-1.2, 1.2, npts), rng.uniform(-1.0, 1.0, npts), rng.uniform(5.0, 7.0, npts)],
                      axis=1)
    oi = (c[:, None] + np.arange(-(SEEN_BY // 2), SEEN_BY // 2 + 1)[None, :]).reshape(-1)
    op = np.repeat(np.arange(npts), SEEN_BY)
    xy = np.zeros((oi.size, 2))
    for i in range(nimg):
        sel = np.flatnonzero(oi == i)
        if sel.size:
            xy[sel] = ba_scipy.project(2, prm, ba_cases.rotate(q_true[i], X_true[op[sel]]) + t_true[i])
    xy += noise * rng.standard_normal(xy.shape)
    q0 = np.array([ba_cases.quat_plus(q_true[i], rng.uniform(-0.003, 0.003, 3) if i else np.zeros(3)) for i in range(nimg)])
    t0 = t_true + np.where(np.arange(nimg)[:, None] > 0, rng.uniform(-0.02, 0.02, (nimg, 3)), 0.0)
    t0[1, 0] = t_true[1, 0]
    X0 = X_true + rng.uniform(-0.03, 0.03, X_true.shape)
    cc = np.ones((1, 12), np.uint8)
    cc[0, [0, 3]] = 0  # refine_focal_length, refine_extra_params
    pc = np.zeros((nimg, 6), np.uint8)
    pc[0, :] = 1
    pc[1, 3] = 1
    return ([2], [prm * np.array([1.01, 1.0, 1.0, 1.1])], cc, np.zeros(nimg, np.uint32), q0, t0, pc, X0,
            oi.astype(np.uint32), op.astype(np.uint32), xy)


def local_leg(a):
    """BundleAdjuster.solve on a few neighbouring images of a large model"""
    import copy

    import ba_cases
    import ba_config_cases as cc
    import ba_config_ref_lib as cref
    import pycolmap_amd as pc
    args = path_scene(a.local_images, a.local_points, seed=2)
    sc = dict(models=[2], camera_params=args[1], image_cameras=args[3], qvec=args[4], tvec=args[5], xyz=args[7],
              obs_image=args[8], obs_point=args[9], obs_xy=args[10])
    t0 = time.perf_counter()
    rec = ba_cases.reconstruction(sc)
    build_ms = 1e3 * (time.perf_counter() - t0)
    cfg = pc.BundleAdjustmentConfig()
    first = a.local_images // 2 - a.local_config // 2
    for i in range(first, first + a.local_config):
        cfg.add_image(i + 1)
    o = pc.BundleAdjustmentOptions()
    o.solver_options.max_num_iterations = a.iterations
    adj = pc.BundleAdjuster(o, cfg)
    t0 = time.perf_counter()
    d = adj._problem(rec)
    setup_ms = 1e3 * (time.perf_counter() - t0)
    pm = np.asarray(d["point_const"]).reshape(-1)
    best = None
    pc.BundleAdjuster(o, cfg).solve(copy.deepcopy(rec))  # warm-up
    for _ in range(a.reps):
        r = copy.deepcopy(rec)
        t0 = time.perf_counter()
        assert adj.solve(r)
        st = dict(adj.summary)
        st["wall_ms"] = 1e3 * (time.perf_counter() - t0)
        if best is None or st["device_ms"] + st["host_ms"] < best[0]["device_ms"] + best[0]["host_ms"]:
            best = (st, r)
    st, solved = best
    t0 = time.perf_counter()
    want = cref.bundle_adjust(*cc.flat_args(d), options=dict(max_num_iterations=a.iterations), point_const=pm)
    ref_ms = 1e3 * (time.perf_counter() - t0)
    by_ref = copy.deepcopy(rec)
    assert pc.BundleAdjuster(o, cfg)._solve_with(by_ref, lambda _d: want)
    return {
        "workload": {"model_images": a.local_images, "model_points": a.local_points, "model_observations": len(args[8]),
                     "config_images": a.local_config, "problem_images": st["num_images"], "problem_points": st["num_points"],
                     "constant_points": st["num_constant_points"], "problem_observations": st["num_observations"],
                     "variable_parameters": st["num_variable_parameters"],
                     "lm_iterations": st["num_successful_steps"] + st["num_unsuccessful_steps"]},
        "initial_cost": st["initial_cost"], "final_cost": st["final_cost"], "termination": st["termination"],
        "pcg_iterations": st["num_pcg_iterations"],
        "kernel_ms": st["kernel_ms"], "copy_ms": st["device_ms"] - st["kernel_ms"], "host_ms": st["host_ms"],
        "wall_ms": st["wall_ms"], "setup_ms": setup_ms, "setup_share_of_host": setup_ms / st["host_ms"] if st["host_ms"] else None,
        "reconstruction_build_ms": build_ms,
        "cpu_reference_ms": ref_ms, "cpu_reference_cost": want["final_cost"],
        "gpu_equals_reference_bit_for_bit": cc.model_bits(solved) == cc.model_bits(by_ref),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=300)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--small-images", type=int, default=12)
    ap.add_argument("--small-points", type=int, default=400)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--local", action="store_true", help="the local leg: BundleAdjuster.solve on a few images of a large model")
    ap.add_argument("--local-images", type=int, default=300)
    ap.add_argument("--local-points", type=int, default=30000)
    ap.add_argument("--local-config", type=int, default=5)
    a = ap.parse_args()
    if a.local:
        line = json.dumps(local_leg(a))
        print(line)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(line + "\n")
        return

    import ba_cases
    import ba_ref_lib as ref
    import ba_scipy

    from pycolmap_amd import _capi

    args = path_scene(a.images, a.points)
    small = path_scene(a.small_images, a.small_points, seed=1)
    options = dict(max_num_iterations=a.iterations)
    nobs = len(args[8])
    kc = 4
    bytes_per_product = nobs * (2 * 8 * (12 + 2 * kc + 6) + 60)  # 15.10
    best = None
    with _capi.Context(0) as ctx:
        ctx.bundle_adjust(*small, options=options)  # warm-up
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = ctx.bundle_adjust(*args, options=options)
            r["wall_ms"] = 1e3 * (time.perf_counter() - t0)
            if best is None or r["device_ms"] < best["device_ms"]:
                best = r
        g_small = ctx.bundle_adjust(*small, options=options)
    t0 = time.perf_counter()
    r_small = ref.bundle_adjust(*small, options=options)
    ref_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    scipy_cost, _ = ba_scipy.Problem(*small).solve(1e-10)
    scipy_ms = 1e3 * (time.perf_counter() - t0)
    steps = best["num_successful_steps"] + best["num_unsuccessful_steps"]
    out = {
        "workload": {"images": a.images, "points": a.points, "observations": nobs, "lm_iterations": steps,
                     "variable_parameters": best["num_variable_parameters"]},
        "initial_cost": best["initial_cost"], "final_cost": best["final_cost"], "termination": best["termination"],
        "pcg_iterations": best["num_pcg_iterations"],
        "kernel_ms_per_lm_iteration": best["kernel_ms"] / max(steps, 1),
        "device_ms_per_lm_iteration": best["device_ms"] / max(steps, 1),
        "host_ms": best["host_ms"], "wall_ms": best["wall_ms"],
        "observations_per_s": nobs * steps / (1e-3 * best["device_ms"]),
        "schur_product_gbs_lower_bound": 1e-9 * bytes_per_product * best["num_pcg_iterations"] / (1e-3 * best["kernel_ms"]),
        "hbm_peak_gbs": HBM_PEAK_GBS,
        "small_scene": {"images": a.small_images, "points": a.small_points, "observations": len(small[8]),
                        "gpu_device_ms": g_small["device_ms"], "cpu_reference_ms": ref_ms, "scipy_ms": scipy_ms,
                        "scipy_cost_at_convergence": scipy_cost, "reference_cost": r_small["final_cost"],
                        "gpu_equals_reference_bit_for_bit": ba_cases.digest(g_small) == ba_cases.digest(r_small)},
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
